"""CPU: the row-band chains of the clip scheduler (pnp_generator_set_band_split; csrc/generator.hip) run on the host under
AddressSanitizer + UBSan (tests/host/band_stub.cpp over the unchanged tests/host/sched_stub.cpp harness): which convs the scheduler
splits, with which boundary rows and events, where it joins, and that every condition of the rule in include/pnpvcve.h switches it
off.  The expected rows come from pnp_band_plan, which tests/test_band_plan.py checks against the safety argument."""
import ctypes
import json
import os
import shutil
import subprocess

import pytest

from pnp_vcve_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def docs(tmp_path_factory):
    cxx = shutil.which('g++') or shutil.which('clang++') or '/opt/rocm/lib/llvm/bin/clang++'
    exe = str(tmp_path_factory.mktemp('band') / 'band_stub')
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-DPNP_HOST_STUB',
           '-Dmain=sched_stub_main', '-Wno-attributes', '-x', 'c++', os.path.join(ROOT, 'tests', 'host', 'band_stub.cpp'), '-o', exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert 'AddressSanitizer' not in r.stderr and 'runtime error' not in r.stderr and 'LeakSanitizer' not in r.stderr, r.stderr[-4000:]
    out = {}
    for ln in r.stdout.splitlines():
        if ln.startswith('{'):
            d = json.loads(ln)
            out[d['name']] = d
    assert len(out) == 19
    for name, d in out.items():
        assert d['pack_rc'] == 0 and d['forward_rc'] == 0 and d['errors'] == [], (name, d['errors'])
        assert d['live_events_after_destroy'] == 0 and d['live_streams_after_destroy'] == 0, name
        assert d['default_band'] == 1
    return out


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_native.LIB_PATH):
        from pnp_vcve_amd import build_native
        build_native.build()
    return _native.lib()


def plan(lib, rows, nconv, a0=0):
    b = (ctypes.c_int * nconv)()
    return list(b) if lib.pnp_band_plan(rows, nconv, a0, b) else None


def chains(d):
    """the branch runs of the recorded convs: [(indices of the chain's convs, index of the join's position)] -- an input conv (source 0
    the RGB frame), the 16 block halves behind it, and conv_hr (64 -> 64 at the frame's size, NHWC output) behind a forward branch"""
    n = len(d['row'])
    out, i = [], 0
    while i < n:
        if d['c0'][i] == 4 and d['mode'][i] == 0:
            idx = list(range(i, i + 17))
            assert all(d['mode'][k] == 0 and d['c0'][k] == 64 and d['nsrc'][k] == 1 for k in idx[1:]), i
            j = i + 17
            if j < n and d['mode'][j] == 0 and d['c0'][j] == 64 and d['nsrc'][j] == 1 and d['conv_h'][j] == d['conv_h'][i]:
                idx.append(j)
                j += 1
            out.append(idx)
            i = j
        else:
            assert d['row'][i] == -1, (d['name'], i)            # heads, conv_last: never split
            i += 1
    return out


def expect_rows(lib, d, idx, a0=0):
    """the scheduler's rule: a first conv that is not on the tile kernels runs whole and the numbering starts behind it"""
    tile = [d['tile'][k] for k in idx]
    assert all(tile[1:]), d['name']
    lead = 0 if tile[0] else 1
    p = plan(lib, d['rows'], len(idx) - lead, a0)
    return [-1] * len(idx) if p is None else [-1] * lead + p


def check_split_everywhere(lib, d, a0=0):
    cs = chains(d)
    nsplit = 0
    for idx in cs:
        want = expect_rows(lib, d, idx, a0)
        assert [d['row'][k] for k in idx] == want, (d['name'], idx[0])
        split = [k for k in idx if d['row'][k] >= 0]
        if split:
            nsplit += 1
            assert len({d['ready'][k] for k in split}) == len(split) and min(d['ready'][k] for k in split) > 0     # one event per conv
            assert len({d['side'][k] for k in split}) == 1 and d['side'][split[0]] > 0
    assert all(s == 0 for s in d['conv_stream'])                  # every conv is issued on the caller's stream (part B: the launcher's)
    # one join per split chain: the caller's stream waits for an event recorded on the side stream
    side = {s for s in d['side'] if s > 0}
    assert len(d['join_on']) == nsplit and (nsplit == 0 or set(d['join_on']) == side)
    return cs, nsplit


def test_720p_chains_rows_events_and_joins(docs, lib):
    d = docs['p720_t3']
    cs, nsplit = check_split_everywhere(lib, d)
    # t = 3: backward frames 2, 1, 0 (frame 2's input conv is the frame alone: the direct kernel, 16 convs split), forward 0, 1, 2 with conv_hr
    assert [len(c) for c in cs] == [17, 17, 17, 18, 18, 18] and nsplit == 6
    assert [d['row'][k] for k in cs[0]] == [-1] + list(range(30, 14, -1))
    assert [d['row'][k] for k in cs[1]] == list(range(30, 13, -1))
    assert [d['row'][k] for k in cs[3]] == list(range(31, 13, -1))
    # the stream and the events are made once (18 `ready` events + the join event), the second forward makes none
    assert d['streams_created_after_forward'] == [1, 1] and d['band_events_created_after_forward'] == [19, 19]


def test_other_first_boundaries(docs, lib):
    check_split_everywhere(lib, docs['p720_t3_a38'], 38)
    d = docs['p720_t3_a38']
    assert [d['row'][k] for k in chains(d)[3]] == list(range(38, 20, -1))
    d = docs['p720_t3_a45']                                       # leaves chain B empty: one launch per conv, nothing created
    assert set(d['row']) == {-1} and d['join_on'] == [] and d['streams_created_after_forward'] == [0]


def test_every_condition_of_the_rule_switches_the_split_off(docs):
    for name in ('p720_t3_off', 'p720_n2_ctx2', 'p720_t2_f16', 'p720_t2_x3', 'p720_t2_direct', 'small_wino2_t3', 'small_units_t3',
                 'rows16_t3'):
        d = docs[name]
        assert set(d['row']) == {-1}, name
        # no stream or event of the split is ever made (two contexts: the two side streams of the batch-level fork)
        assert d['streams_created_after_forward'] == [2 if name == 'p720_n2_ctx2' else 0], name
        assert [w for w in d['join_on'] if name != 'p720_n2_ctx2'] == []


def test_split_variants(docs, lib):
    # two clips one after another in ONE context: still one clip in flight
    cs, nsplit = check_split_everywhere(lib, docs['p720_n2_ctx1'])
    assert nsplit == len(cs) == 2 * 4
    # channel-last blocks (branches + residual in the back half), the bounded-memory schedule with its recomputed branch runs
    cs, nsplit = check_split_everywhere(lib, docs['p720_t2_channel_last'])
    assert nsplit == len(cs) == 4
    cs, nsplit = check_split_everywhere(lib, docs['p720_t9_bounded'])
    assert nsplit == len(cs) > 2 * 9
    # x4 heads: conv_hr runs at 4h x 4w behind the pixel-shuffle convs, outside the chain; both sweeps' chains are 17 convs
    d = docs['vsr_rows19_t2']
    cs, nsplit = check_split_everywhere(lib, d)
    assert [len(c) for c in cs] == [17] * 4 and nsplit == 4


def test_the_row_threshold_per_chain(docs, lib):
    # 19 rows: every chain fits (forward: 18 .. 1); 18 rows: the 18-conv forward chains do not, the backward ones do;
    # 17 rows: only the 16-conv chain behind a direct input conv; 16 rows: none
    for name, want in (('rows19_t3', [1, 1, 1, 1, 1, 1]), ('rows18_t3', [1, 1, 1, 0, 0, 0]), ('rows17_t3', [1, 0, 0, 0, 0, 0])):
        d = docs[name]
        cs, nsplit = check_split_everywhere(lib, d)
        assert [1 if any(d['row'][k] >= 0 for k in c) else 0 for c in cs] == want, name
        assert nsplit == sum(want)
    d = docs['rows19_t3']
    assert [d['row'][k] for k in chains(d)[3]] == list(range(18, 0, -1))


def test_profiling_keeps_the_split_and_counts_a_conv_once(docs, lib):
    d = docs['p720_t3_profiled']
    check_split_everywhere(lib, d)
    # 2 sweeps x 3 frames x 16 block halves + 3 conv_hr launches, every one of them split and counted once; the stub's events are
    # 1 ms apart and only the caller's stream is timed: 1 ms per conv
    nblock_split = sum(1 for r, c0 in zip(d['row'], d['c0']) if r >= 0 and c0 == 64)
    assert d['block_launches'] == 2 * 3 * 16 + 3 and nblock_split == d['block_launches']
    assert d['block_ms'] == pytest.approx(d['block_launches'])

"""CPU: the fold table of the Winograd front halves (csrc/fold_table.h) and its place in the clip schedule, on the host under
AddressSanitizer + UBSan (tests/host/fold_table_stub.cpp over the unchanged tests/host/sched_stub.cpp harness).

* The table itself: csrc/fold_table.h's own host loop -- the record rule and the index function the kernel uses -- run as a stand-alone
  program on exact-size heap blocks, against a numpy restatement of the rule, record for record (plane, factor bits).
* The schedule: every gated front half on the tile kernels carries a table; the launch that wrote it last, in issue order, read that
  conv's own partition planes, lies in the workspace of the conv's context, and was issued on the run's stream in front of the run's
  input conv; nothing else carries one (quadrant-unit kernels, direct and fp16 paths, PNP_OPT_PAR_SKIP off)."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENARIOS = 14
BLOCKS = 8           # BAE blocks per branch run in the default generator: one gated front half each


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    cxx = shutil.which('g++') or shutil.which('clang++') or '/opt/rocm/lib/llvm/bin/clang++'
    out = str(tmp_path_factory.mktemp('fold') / 'fold_table_stub')
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-DPNP_HOST_STUB',
           '-Dmain=sched_stub_main', '-Wno-attributes', '-x', 'c++', os.path.join(ROOT, 'tests', 'host', 'fold_table_stub.cpp'), '-o', out]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-4000:]
    return out


ENV = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')


def clean(r):
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert 'AddressSanitizer' not in r.stderr and 'runtime error' not in r.stderr and 'LeakSanitizer' not in r.stderr, r.stderr[-4000:]


# ------------------------------------------------------------------------------------------------------------ the table
def blocks_to_planes(blk, h, w):
    """(3, ceil(h/8), ceil(w/8)) values per 8x8 block -> (3, h, w) planes (the frame cuts the last row / column of blocks)"""
    return np.ascontiguousarray(np.repeat(np.repeat(blk, 8, 1), 8, 2)[:, :h, :w].astype(np.float32))


def maps(h, w):
    rng = np.random.RandomState(1000 * h + w)
    bh, bw = (h + 7) // 8, (w + 7) // 8
    cls = rng.randint(0, 4, (bh, bw))                                  # 3: no record
    unit = np.float32(1.0) / np.float32(255.0)
    one_hot = np.stack([(cls == j) * unit for j in range(3)])
    val = rng.randint(1, 255, (bh, bw)).astype(np.float32) / np.float32(255.0) * np.where(rng.rand(bh, bw) < 0.5, -1, 1)
    constants = np.stack([(cls == j) * val for j in range(3)])         # one plane per quadrant, its value differs from quadrant to quadrant
    two = one_hot.copy()
    two[2, 0, 0], two[1, 0, 0] = unit, 3 * unit                        # the first quadrant carries two live planes
    two[0, -1, -1], two[2, -1, -1] = unit, unit                        # ... and so does the last (cut by both edges on the ragged frames)
    return {'one_hot': blocks_to_planes(one_hot, h, w), 'zero': np.zeros((3, h, w), np.float32),
            'constants': blocks_to_planes(constants, h, w), 'two_live': blocks_to_planes(two, h, w)}


def table_numpy(par):
    """the rule of csrc/fold_table.h restated: per 8x8 quadrant of the frame rounded up to 16x16 tiles, tile-major, the lowest plane
    that is nonzero at the quadrant's first pixel and 0.25f * its value there; -1 and 0 if none is or the quadrant lies outside"""
    _, h, w = par.shape
    ty, tx = (h + 15) // 16, (w + 15) // 16
    out = np.zeros((ty * tx * 4, 2), np.int32)
    out[:, 0] = -1
    for qy in range(2 * ty):
        for qx in range(2 * tx):
            if 8 * qy < h and 8 * qx < w:
                v = par[:, 8 * qy, 8 * qx]
                nz = np.flatnonzero(v != 0)
                if len(nz):
                    i = ((qy // 2) * tx + qx // 2) * 4 + (qy % 2) * 2 + qx % 2
                    out[i] = (nz[0], (np.float32(0.25) * v[nz[0]]).view(np.int32))
    return out


def gate_numpy(par):
    """bit 3 of the frame's partition word restated: every 8x8 quadrant, on its pixels inside the frame, is all zero or has exactly one
    live plane that is constant there"""
    _, h, w = par.shape
    for y in range(0, h, 8):
        for x in range(0, w, 8):
            q = par[:, y:y + 8, x:x + 8].reshape(3, -1)
            live = [j for j in range(3) if (q[j] != 0).any()]
            if len(live) > 1 or (len(live) == 1 and (q[live[0]] != q[live[0], 0]).any()):
                return False
    return True


@pytest.mark.parametrize('hw', [(64, 64), (48, 80), (100, 132), (148, 216)])
def test_host_table_equals_the_numpy_restatement(exe, tmp_path, hw):
    h, w = hw
    for kind, par in maps(h, w).items():
        fi, fo = tmp_path / f'{kind}.f32', tmp_path / f'{kind}.i32'
        par.tofile(fi)
        clean(subprocess.run([exe, 'table', str(h), str(w), str(fi), str(fo)], capture_output=True, text=True, timeout=120, env=ENV))
        got = np.fromfile(fo, np.int32).reshape(-1, 2)
        want = table_numpy(par)
        assert got.shape == want.shape and np.array_equal(got, want), (hw, kind, np.flatnonzero((got != want).any(1))[:8])
        # what the maps are for: only the map with two live planes in a quadrant fails the gate; its records are still what the rule gives
        assert gate_numpy(par) == (kind != 'two_live'), (hw, kind)
        live = int((want[:, 0] >= 0).sum())
        assert (live == 0) == (kind == 'zero')
        if kind == 'constants':
            assert len(np.unique(want[want[:, 0] >= 0, 1])) > live // 2            # the factors do differ from quadrant to quadrant
        if kind == 'one_hot':
            assert set(np.unique(want[want[:, 0] >= 0, 1])) == {int((np.float32(0.25) * (np.float32(1.0) / np.float32(255.0))).view(np.int32))}
    # the quadrants beyond a ragged frame are there and empty: 100 rows = 13 rows of quadrants in 7 tile rows
    if hw == (100, 132):
        want = table_numpy(maps(h, w)['one_hot'])
        tx = (w + 15) // 16
        below = [((13 // 2) * tx + t) * 4 + 2 + q for t in range(tx) for q in range(2)]
        assert (want[below, 0] == -1).all() and (want[below, 1] == 0).all()


# ------------------------------------------------------------------------------------------------------------ the schedule
@pytest.fixture(scope='module')
def docs(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=ENV)
    clean(r)
    out = {}
    for ln in r.stdout.splitlines():
        if ln.startswith('{'):
            d = json.loads(ln)
            out[d['name']] = d
    assert len(out) == SCENARIOS
    for name, d in out.items():
        assert d['pack_rc'] == 0 and d['forward_rc'] == 0 and d['errors'] == [], (name, d['errors'])
    return out


@pytest.mark.parametrize('name,runs', [('plain_wino2_t3', 6), ('plain_ragged_t3', 6), ('channel_last_t3', 6), ('p720_t2', 4), ('sparse_t3', 6),
                                       ('two_contexts_n2', 12), ('one_context_n2', 12), ('p720_two_contexts_n3', 12)])
def test_every_run_makes_its_frames_table_in_front_of_its_front_halves(docs, name, runs):
    """plain and two-context schedules: one launch per branch run (a backward and a forward run per frame and clip), read by that
    run's front halves and by nothing else; written inside the workspace, on the stream the run's input conv follows on"""
    d = docs[name]
    assert d['launches'] == runs and d['readers'] == BLOCKS * runs
    assert d['readers_of_launch'] == [BLOCKS] * runs
    assert d['launch_in_workspace'] == [1] * runs and d['input_conv_follows_on_the_same_stream'] == [1] * runs
    assert d['gated_tile_convs_without_table'] == 0 and d['tables_without_gate'] == 0 and d['tables_on_other_kernels'] == 0


def test_two_contexts_write_their_own_tables_on_their_own_streams(docs):
    d = docs['two_contexts_n2']
    assert len(set(d['launch_stream'])) == 2 and all(d['launch_stream'].count(s) == 6 for s in set(d['launch_stream']))
    assert len(set(docs['one_context_n2']['launch_stream'])) == 1


@pytest.mark.parametrize('name', ['bounded_t9', 'bounded_sparse_t9'])
def test_bounded_schedule_makes_the_table_again_for_every_recomputed_run(docs, name):
    """the recompute schedule runs some backward branches twice: each run, recomputed or not, has its own launch in front of it (with a
    sparse_val map: behind the frame's pass into the one-frame buffer, which the launcher's read check sees)"""
    d = docs[name]
    assert d['launches'] > 2 * 9 and d['readers'] == BLOCKS * d['launches']
    assert d['readers_of_launch'] == [BLOCKS] * d['launches'] and d['input_conv_follows_on_the_same_stream'] == [1] * d['launches']
    assert d['gated_tile_convs_without_table'] == 0


@pytest.mark.parametrize('name', ['units_128_t3', 'no_skip_t3', 'direct_t3', 'f16_t3'])
def test_no_table_where_no_kernel_reads_one(docs, name):
    """quadrant-unit kernels of small frames, PNP_OPT_PAR_SKIP off (no gate), the direct kernels, the fp16 path"""
    d = docs[name]
    assert d['launches'] == 0 and d['readers'] == 0 and d['tables_on_other_kernels'] == 0

"""CPU: the bounded-memory forward's C ABI (pnp_generator_set_max_resident / _get_max_resident / _min_resident), its workspace
sizing, and its schedule run on the host under AddressSanitizer + UBSan (tests/host/long_clip_stub.cpp over the unchanged
tests/host/sched_stub.cpp harness)."""
import ctypes
import json
import math
import os
import re
import shutil
import subprocess

import pytest

from pnp_vcve_amd import _native, synthetic as syn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('pnp_generator_set_max_resident', 'pnp_generator_get_max_resident', 'pnp_generator_min_resident')


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_native.LIB_PATH):
        from pnp_vcve_amd import build_native
        build_native.build()
    return _native.lib()


def _gen(lib, prec=0, **over):
    cfg = dict(syn.DEFAULT_GENERATOR_CFG)
    cfg.update(over)
    c = _native.GeneratorCfg(mid_channels=64, num_blocks=cfg['num_blocks'], num_experts=cfg['num_experts'],
                             with_cat=int(cfg['with_cat']), use_base_qp=int(cfg['use_base_qp']),
                             expert_softmax=int(cfg['expert_softmax']), with_bias=int(cfg['with_bias']), with_se=int(cfg['with_se']),
                             one_layer=int(cfg['one_layer']), channel_first=int(cfg['channel_first']),
                             align_key=int(cfg['align_key']), vsr=int(cfg['vsr']), deform=0, sparse_val=int(cfg['sparse_val']),
                             num_group=1, flow_inter=0, blocktype=0)
    h = ctypes.c_void_p()
    assert lib.pnp_generator_create(ctypes.byref(c), ctypes.byref(h)) == 0
    assert lib.pnp_generator_set_precision(h, prec) == 0
    return h


def test_new_symbols_are_declared_exported_and_bound(lib):
    hdr = open(os.path.join(ROOT, 'include', 'pnpvcve.h')).read()
    declared = set(re.findall(r'\b(pnp_[a-z0-9_]+)\s*\(', hdr))
    for name in NEW:
        assert name in declared and name in _native.SIGNATURES and hasattr(lib, name), name
    assert lib.pnp_abi_version() == 5


def _spatial_slope(lib, g, k, sizes=((64, 64), (128, 192))):
    """-> (bytes per pixel per frame, non-spatial bytes per frame) of the workspace, with k maps (0 = unbounded).  256 frames apart,
    every region's 256-byte rounding cancels; the per-tile partition flags (4 B per 8x16 tile and frame) are taken out."""
    assert lib.pnp_generator_set_max_resident(g, k) == 0
    t0 = max(k, 1) + 1 if k else 1
    slopes = []
    for h, w in sizes:
        d = lib.pnp_generator_workspace_bytes(g, t0 + 256, h, w) - lib.pnp_generator_workspace_bytes(g, t0, h, w)
        assert d % 256 == 0
        slopes.append(d // 256 - 4 * ((w + 15) // 16) * ((h + 7) // 8))
    (h0, w0), (h1, w1) = sizes
    per_px = (slopes[1] - slopes[0]) / (h1 * w1 - h0 * w0)
    return per_px, slopes[0] - per_px * h0 * w0


@pytest.mark.parametrize('prec,sparse,per_px', [(0, False, 272), (1, False, 400), (2, False, 272), (0, True, 284)])
def test_unset_bound_keeps_the_per_frame_workspace(lib, prec, sparse, per_px):
    """k unset: 16 B/px RGB0 + 256 B/px feature slot (+ 128 B/px fp16 mirror, + 12 B/px sparse_val map) per frame, plus the
    per-frame expert mixtures -- today's sizing, unchanged"""
    g = _gen(lib, prec, sparse_val=sparse)
    try:
        assert lib.pnp_generator_get_max_resident(g) == 0
        sp, nonsp = _spatial_slope(lib, g, 0)
        assert sp == per_px
        assert nonsp > 2e6            # the expert mixtures: 2 x 8 blocks x one 147 KB image per frame, at least
    finally:
        lib.pnp_generator_destroy(g)


@pytest.mark.parametrize('prec,sparse', [(0, False), (1, False), (2, False), (0, True)])
def test_bounded_workspace_grows_by_the_rgb_frame_only(lib, prec, sparse):
    g = _gen(lib, prec, sparse_val=sparse)
    try:
        _, nonsp_unbounded = _spatial_slope(lib, g, 0)
        k = lib.pnp_generator_min_resident(g, 1000)
        sp, nonsp = _spatial_slope(lib, g, k)
        assert sp <= 16 and nonsp == nonsp_unbounded, (sp, nonsp, nonsp_unbounded)
        # t = 1000 at 720p: under 20 % of the unbounded workspace
        assert lib.pnp_generator_set_max_resident(g, 0) == 0
        unb = lib.pnp_generator_workspace_bytes(g, 1000, 720, 1280)
        assert lib.pnp_generator_set_max_resident(g, k) == 0
        bnd = lib.pnp_generator_workspace_bytes(g, 1000, 720, 1280)
        assert 0 < bnd < 0.2 * unb, (bnd, unb, bnd / unb)
        # k >= t: the unbounded sizing
        assert lib.pnp_generator_set_max_resident(g, 1000) == 0
        assert lib.pnp_generator_workspace_bytes(g, 1000, 720, 1280) == unb
    finally:
        lib.pnp_generator_destroy(g)


@pytest.mark.parametrize('with_cat', [True, False])
def test_min_resident_is_monotone_and_within_the_scheme_bound(lib, with_cat):
    g = _gen(lib, with_cat=with_cat, align_key=with_cat)
    try:
        prev = 0
        for t in list(range(1, 400)) + [1000, 1200, 3000]:
            m = lib.pnp_generator_min_resident(g, t)
            assert prev <= m <= t and m <= 2 * math.sqrt(2 * t) + 3, (t, m)
            prev = m
        assert lib.pnp_generator_min_resident(g, 0) == -1
    finally:
        lib.pnp_generator_destroy(g)


def test_bound_below_the_minimum_is_reported(lib):
    g = _gen(lib)
    try:
        assert lib.pnp_generator_set_max_resident(g, -1) == 1001
        m = lib.pnp_generator_min_resident(g, 100)
        assert lib.pnp_generator_set_max_resident(g, m - 1) == 0 and lib.pnp_generator_get_max_resident(g) == m - 1
        assert lib.pnp_generator_workspace_bytes(g, 100, 64, 64) == -1
        assert lib.pnp_generator_workspace_bytes(g, 5, 64, 64) > 0            # k >= t: unbounded
        # the forward refuses it before touching any buffer
        rc = lib.pnp_generator_forward(g, None, None, None, None, None, None, None, None, None, None, 1 << 40, 1, 100, 64, 64, None)
        assert rc == 1001
        assert lib.pnp_generator_set_max_resident(g, m) == 0
        assert lib.pnp_generator_workspace_bytes(g, 100, 64, 64) > 0
    finally:
        lib.pnp_generator_destroy(g)


def test_python_attribute_and_helper(lib):
    from pnp_vcve_amd.generator import IconVSR_restore_wo_refill_mv_ipb_fast_domain_dynamic_with_par as Gen
    m = Gen(**syn.DEFAULT_GENERATOR_CFG)
    assert m.max_resident_features is None
    m.max_resident_features = 12
    assert m.max_resident_features == 12 and m.min_resident_features(23) == 12
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError):
            m.max_resident_features = bad
    m.max_resident_features = 11
    with pytest.raises(ValueError, match='minimum 12'):
        m._check_resident(23)
    m._check_resident(11)                  # k >= t: unbounded, always fine
    m.max_resident_features = None
    assert m.max_resident_features is None
    m._check_resident(23)


# ------------------------------------------------------------------ the schedule under the sanitizers
@pytest.fixture(scope='module')
def stub_run(tmp_path_factory):
    cxx = shutil.which('g++') or shutil.which('clang++') or '/opt/rocm/lib/llvm/bin/clang++'
    exe = str(tmp_path_factory.mktemp('long_clip') / 'long_clip_stub')
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-DPNP_HOST_STUB',
           '-Dmain=sched_stub_main', '-Wno-attributes', '-x', 'c++', os.path.join(ROOT, 'tests', 'host', 'long_clip_stub.cpp'), '-o', exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=env)
    docs = {}
    for ln in r.stdout.splitlines():
        if ln.startswith('{'):
            d = json.loads(ln)
            docs[d['name']] = d
    return r, docs


def test_bounded_schedule_is_clean_under_asan_and_ubsan(stub_run):
    r, docs = stub_run
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert 'AddressSanitizer' not in r.stderr and 'runtime error' not in r.stderr and 'LeakSanitizer' not in r.stderr, r.stderr[-4000:]
    assert len(docs) == 23
    for name, d in docs.items():
        assert d['errors'] == [], (name, d['errors'])
        assert d['create_rc'] == d['set_rc'] == d['pack_rc'] == d['forward_rc'] == d['unbounded_forward_rc'] == 0, name


def test_bounded_schedule_reads_the_same_logical_frames(stub_run):
    """every branch run of the bounded schedule -- recomputed ones included -- aligns the same key frame, reads the same neighbour and
    own backward feature (tagged by the run that wrote them) as the unbounded run of that frame; forward runs and heads in the same
    order; branch runs = 2t + recomputed frames (t - R, R the resident head the plan picked)"""
    _, docs = stub_run
    for name, d in docs.items():
        t, n, k = d['t'], d['n'], d['k']
        assert d['mismatches'] == 0 and d['forward_order_equal'] == 1, name
        assert d['head_reads'] == d['unbounded_head_reads'] and d['head_reads'] >= n * t, name
        recomputed = (t - d['plan_r']) if k < t else 0
        assert d['unbounded_input_convs'] == 2 * n * t
        assert d['input_convs'] == n * (2 * t + recomputed), (name, d['input_convs'], recomputed)
        if k < t:
            assert recomputed > 0 and d['context_bytes'] < d['unbounded_context_bytes'], name
        else:
            assert d['context_bytes'] == d['unbounded_context_bytes'] and d['steps'] == d['unbounded_steps'], name
        # each backward frame runs once in the checkpoint pass and at most once more (its segment's recompute)
        per = {}
        for s in d['steps']:
            per[(s[0], s[1], s[2])] = per.get((s[0], s[1], s[2]), 0) + 1
        assert all(v == 1 for (b, sw, f), v in per.items() if sw == 1)
        assert all(v in (1, 2) for (b, sw, f), v in per.items() if sw == 0)
        assert len(per) == 2 * n * t


def test_the_bounds_the_issue_names_are_covered(stub_run):
    _, docs = stub_run
    ks = {d['k'] for n, d in docs.items() if n.startswith('ibbbp_t23')}
    m = docs['ibbbp_t23_kmin']['k']
    assert ks == {m, m + 3, 22, 23}

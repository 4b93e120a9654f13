"""CPU: the row-band plan (pnp_band_plan, include/pnpvcve_debug.h; csrc/generator.hip band_plan) as a pure function, and the switch's
C ABI (pnp_generator_set_band_split / _get_band_split).

A chain of nconv 3x3 convs runs as chain A (tile rows [0, a_n) of conv n, the caller's stream) and chain B (rows [a_n, rows), a side
stream), a_n = a_0 - n; B's conv n is ordered behind A's conv n - 1 by an event, nothing else orders the two.  The checks restate the
safety argument on explicit pixel-row sets: a 3x3 conv's output rows [p, q) read input rows [p - 1, q + 1) of the frame."""
import ctypes
import os
import re

import pytest

from pnp_vcve_amd import _native, synthetic as syn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# a branch: input conv + 16 block halves (+ conv_hr behind a forward branch); one conv less when the input conv runs on the direct kernel
CHAINS = (18, 17, 16)
HEIGHTS = (720, 1080, 2160)


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_native.LIB_PATH):
        from pnp_vcve_amd import build_native
        build_native.build()
    return _native.lib()


def plan(lib, rows, nconv, a0=0):
    b = (ctypes.c_int * nconv)(*([-7] * nconv))
    ok = lib.pnp_band_plan(rows, nconv, a0, b)
    assert ok in (0, 1)
    if not ok:
        assert list(b) == [-7] * nconv           # untouched
        return None
    return list(b)


def writes(h, lo, hi):
    """pixel rows of tile rows [lo, hi) of a frame h pixels high"""
    return set(range(16 * lo, min(16 * hi, h)))


def reads(h, lo, hi):
    w = writes(h, lo, hi)
    return {r for r in range(min(w) - 1, max(w) + 2) if 0 <= r < h}


def check_chain(h, bounds):
    rows = (h + 15) // 16
    n = len(bounds)
    A = [(0, a) for a in bounds]
    B = [(a, rows) for a in bounds]
    for k, a in enumerate(bounds):
        assert 1 <= a <= rows - 1, (h, k, a)                        # both regions non-empty
        assert writes(h, *A[k]) and writes(h, *B[k])
        assert writes(h, *A[k]) | writes(h, *B[k]) == set(range(h)) and not (writes(h, *A[k]) & writes(h, *B[k]))
        if k == 0:
            continue
        assert a == bounds[k - 1] - 1
        # A reads only what A's previous conv wrote: chain A never waits for chain B
        assert reads(h, *A[k]) <= writes(h, *A[k - 1])
        # B reads what A's and B's previous convs wrote (A's through the event in front of A's conv k)
        assert reads(h, *B[k]) <= writes(h, *A[k - 1]) | writes(h, *B[k - 1])
        assert reads(h, *B[k]) & writes(h, *A[k - 1])                # ... and it does need that event
    # unordered pairs: B's conv k against A's conv m, m > k (whatever buffers the convs ping-pong between)
    for k in range(n):
        for m in range(k + 1, n):
            assert not (writes(h, *A[m]) & reads(h, *B[k])), (h, k, m)
            assert not (writes(h, *A[m]) & writes(h, *B[k])), (h, k, m)
            assert not (reads(h, *A[m]) & writes(h, *B[k])), (h, k, m)


@pytest.mark.parametrize('h', HEIGHTS)
@pytest.mark.parametrize('nconv', CHAINS)
def test_the_centred_plan_keeps_both_regions_and_the_read_write_inequalities(lib, h, nconv):
    rows = (h + 15) // 16
    b = plan(lib, rows, nconv)
    assert b is not None and b[0] == (rows + nconv - 1) // 2
    check_chain(h, b)
    # centred: the two chains get the same number of tile rows, to within one row per conv
    assert abs(sum(b) - sum(rows - a for a in b)) <= nconv
    if h == 720 and nconv == 18:
        assert b[0] == 31 and b[-1] == 14


@pytest.mark.parametrize('nconv', CHAINS)
def test_the_row_threshold(lib, nconv):
    """both regions non-empty over the whole chain needs a_0 <= rows - 1 and a_0 - (nconv - 1) >= 1: rows >= nconv + 1"""
    for rows in range(1, nconv + 1):
        assert plan(lib, rows, nconv) is None, rows
        for a0 in range(1, rows + 2):
            assert plan(lib, rows, nconv, a0) is None, (rows, a0)
    for rows in (nconv + 1, nconv + 2):
        for ragged in (0, 4, 12):                                    # the last tile row cut by the frame's edge
            b = plan(lib, rows, nconv)
            assert b is not None
            check_chain(16 * rows - ragged, b)
    # the frames the small-frame paths serve anyway
    for h in (64, 128, 180, 256):
        assert plan(lib, (h + 15) // 16, nconv) is None


@pytest.mark.parametrize('h', HEIGHTS)
def test_an_explicit_first_boundary(lib, h):
    rows = (h + 15) // 16
    for nconv in CHAINS:
        for a0 in range(1, rows + 2):
            b = plan(lib, rows, nconv, a0)
            if a0 - (nconv - 1) < 1 or a0 > rows - 1:
                assert b is None, (rows, nconv, a0)
            else:
                assert b[0] == a0
                check_chain(h, b)


def test_bad_arguments(lib):
    b = (ctypes.c_int * 4)()
    assert lib.pnp_band_plan(45, 4, 0, None) == 0
    assert lib.pnp_band_plan(45, 0, 0, b) == 0 and lib.pnp_band_plan(0, 4, 0, b) == 0 and lib.pnp_band_plan(45, 4, -1, b) == 0
    assert lib.pnp_band_plan(45, 1, 0, b) == 1 and b[0] == 22


def test_switch_abi_and_python_attribute(lib):
    hdr = open(os.path.join(ROOT, 'include', 'pnpvcve.h')).read()
    declared = set(re.findall(r'\b(pnp_[a-z0-9_]+)\s*\(', hdr))
    for name in ('pnp_generator_set_band_split', 'pnp_generator_get_band_split'):
        assert name in declared and name in _native.SIGNATURES and hasattr(lib, name), name
    assert lib.pnp_abi_version() == 5
    from pnp_vcve_amd.generator import IconVSR_restore_wo_refill_mv_ipb_fast_domain_dynamic_with_par as Gen
    m = Gen(**syn.DEFAULT_GENERATOR_CFG)
    assert m.band_split == 1                                         # the default
    m.band_split = 0
    assert m.band_split == 0 and lib.pnp_generator_get_band_split(m._handle) == 0
    m.band_split = True
    assert m.band_split == 1
    m.band_split = 38
    assert m.band_split == 38
    for bad in (-1, 2.5, None, '1'):
        with pytest.raises(ValueError):
            m.band_split = bad
    assert lib.pnp_generator_set_band_split(m._handle, -1) == 1001 and m.band_split == 38
    assert lib.pnp_generator_set_band_split(None, 1) == 1001 and lib.pnp_generator_get_band_split(None) == -1

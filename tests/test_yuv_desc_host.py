"""CPU: the one internal descriptor and the one constants struct of the 4:2:0 boundary (csrc/yuv.h), by a stand-alone host program
under AddressSanitizer + UBSan (tests/host/yuv_desc.cpp).

* yuv_planes_ok / yuv_planes_fast, written once in terms of the sample's size, accept and refuse exactly what the four predicates
  they replaced did (restated in the program as the reference), on every tuple of a grid around every rule;
* every field of yuv_coef(standard, depth, container), as its 32-bit pattern, is the constant tests/yuv_ref.py (8 bit) and
  tests/yuv16_ref.py (10, 12 bit) restate: the bits of the 8-bit boundary did not move when it took the container's fields on."""
import json
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import yuv16_ref
import yuv_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOATS = ('cy', 'crv', 'cbu', 'cgu', 'cgv', 'kr', 'kg', 'kb', 'sy', 'sc', 'ipb', 'ipr')


@pytest.fixture(scope='module')
def docs(tmp_path_factory):
    cxx = shutil.which('g++') or shutil.which('clang++') or '/opt/rocm/lib/llvm/bin/clang++'
    exe = str(tmp_path_factory.mktemp('yuv_desc') / 'yuv_desc')
    cmd = [cxx, '-std=c++17', '-O2', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-DPNP_HOST_STUB', '-pthread',
           '-Wno-attributes', '-x', 'c++', os.path.join(ROOT, 'tests', 'host', 'yuv_desc.cpp'), '-o', exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=env)
    assert 'AddressSanitizer' not in r.stderr and 'runtime error' not in r.stderr and 'LeakSanitizer' not in r.stderr, r.stderr[-4000:]
    out = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith('{')]
    return r.returncode, out


def test_the_unified_predicates_agree_with_the_four_they_replaced_on_the_whole_grid(docs):
    rc, out = docs
    g = out[0]
    print(g)
    assert g['wrong8'] == 0, g['first8']
    assert g['wrong16'] == 0, g['first16']
    # w x c_step x (y, cb) addresses x cr - cb x (y, c) pitches x (y, c) strides, and depth x container for 16 bit
    assert g['tuples8'] == 4 * 4 * 10 * 10 * 8 * 11 * 11 * 9 * 9 and g['tuples16'] == g['tuples8'] * 4 * 3
    # no predicate is constant on the grid (the counts are the reference's too: every tuple agrees)
    for name, total in (('ok8', g['tuples8']), ('fast8', g['tuples8']), ('ok16', g['tuples16']), ('fast16', g['tuples16'])):
        assert 0 < g[name] < total, name
    assert out[-1] == {'refusals': 1} and rc == 0


def _bits(x):
    return struct.unpack('<I', struct.pack('<f', float(x)))[0]


def test_every_constant_is_the_numpy_restatements_bit_for_bit(docs):
    _, out = docs
    rows = {(d['standard'], d['depth'], d['msb']): d for d in out if 'depth' in d}
    assert sorted(rows) == sorted([(s, 8, 0) for s in range(4)] + [(s, d, m) for s in range(4) for d in (10, 12) for m in (0, 1)])
    for (std, depth, msb), d in rows.items():
        if depth == 8:
            k = yuv_ref.constants(std)
            mid, top = 128, 255
            assert (d['cmid'], d['vmax'], d['shift'], d['vmask']) == (128, _bits(255.0), 0, 255)
        else:
            k = yuv16_ref.constants(std, depth)
            mid, top = k['mid'], k['top']
        for f in FLOATS:
            assert isinstance(k[f], np.float32) and d[f] == _bits(k[f]), (std, depth, f)
        assert d['yoff'] == k['yoff'] and d['cmid'] == mid and d['vmax'] == _bits(top) and d['vmask'] == top, (std, depth)
        assert d['shift'] == ((16 - depth) if msb else 0), (std, depth, msb)

"""CPU: the per-frame Winograd images are made one branch run ahead, off the row-band chains, into two alternating buffers
(csrc/generator.hip: branch_images).  The scheduler runs on the host under AddressSanitizer + UBSan against the recording launchers
of tests/host/sched_stub.cpp; tests/host/wino_prefetch_stub.cpp adds the order of the image launches among the convs and checks, per
schedule, that every image is written before the conv that reads it -- by the launch made for that conv's run, issued before the run's
input conv -- that no image is rewritten while a run that reads it is open, and that a buffer's earlier readers have been joined."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'host', 'wino_prefetch_stub.cpp')


@pytest.fixture(scope='module')
def docs(tmp_path_factory):
    cxx = shutil.which('g++') or shutil.which('clang++') or '/opt/rocm/lib/llvm/bin/clang++'
    exe = str(tmp_path_factory.mktemp('prefetch') / 'wino_prefetch_stub')
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-DPNP_HOST_STUB',
           '-Wno-attributes', '-x', 'c++', SRC, '-o', exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert 'AddressSanitizer' not in r.stderr and 'runtime error' not in r.stderr and 'LeakSanitizer' not in r.stderr, r.stderr[-4000:]
    out = {}
    for ln in r.stdout.splitlines():
        if ln.startswith('{'):
            d = json.loads(ln)
            out[d['name']] = d
    assert r.returncode == 0, [(d['name'], d['errors']) for d in out.values()]
    return out


# name -> (branch runs, images per run)
CASES = {'plain_p720_t3': (6, 8), 'plain_two_layer_t4': (8, 16), 'bounded_t12': (None, 8), 'two_contexts_n2_t3': (12, 8)}


@pytest.mark.parametrize('name', sorted(CASES))
def test_images_are_written_before_their_run_and_never_under_an_open_one(docs, name):
    d = docs[name]
    runs, per_run = CASES[name]
    assert d['pack_rc'] == 0 and d['forward_rc'] == 0 and d['bound_rc'] == 0 and d['errors'] == [], d['errors']
    assert d['image_launches'] == d['runs'] and d['image_reads'] == per_run * d['runs']      # one launch per run, every block conv reads one
    if runs is not None:
        assert d['runs'] == runs                                   # a backward and a forward run per frame
    else:
        assert d['runs'] > 2 * 12                                  # the bounded schedule recomputes backward runs
    a, b = d['launches_into_buffer']
    assert a + b == d['runs'] and abs(a - b) <= (2 if name.startswith('two_contexts') else 1)      # the buffers alternate from run to run


def test_the_chained_schedule_is_the_one_with_side_streams(docs):
    """720p runs as row-band chains (every conv of a run carries a band split), the small frames as quadrant units without them: the
    join check of the stub has something to bite on in the first and is vacuous in the others"""
    assert docs['plain_p720_t3']['side_stream_convs'] >= 6 * 16
    assert all(docs[n]['side_stream_convs'] == 0 for n in CASES if n != 'plain_p720_t3')

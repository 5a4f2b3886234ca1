"""Host check of the per-axis rule of the reconstruction modes (tnmf_amd/csrc/modes.h) and of its Python twin.

modes.h is plain host+device C++: tests/native/modes_check.cpp runs it on the CPU, under ASan + UBSan, for every mode, atom
lengths 1..6 and every activation length 1..8 the limits admit, and proves there that pad and fold are adjoint and that
axis_images / axis_whole say the same as pad_src / pad_dup.  Here its printed tables are held against numpy's own padding --
which covers the two edges where the limits bite, 'circular' with S = a - 1 and 'reflect' with S = a -- and
``_Backend.axis_images`` against the table of images, on numpy arrays and on torch tensors.  No GPU, no oracle needed.
"""
import os
import subprocess

import numpy as np
import pytest
import torch

from tnmf_amd.backends._Backend import axis_images

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ('valid', 'full', 'circular', 'reflect')   # include/tnmf_hip.h: TNMF_MODE_VALID .. TNMF_MODE_REFLECT = 0 .. 3


@pytest.fixture(scope='module')
def tables(tmp_path_factory):
    """(src, img) as modes_check.cpp prints them: src[(mode, a, S)] = the activation copied to every padded position (-1: a
    zero), img[(mode, a, S)][u] = the padded positions of the images of shift u."""
    exe = str(tmp_path_factory.mktemp('modes') / 'modes_check')
    src = os.path.join(ROOT, 'tests', 'native', 'modes_check.cpp')
    subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-I', os.path.join(ROOT, 'tnmf_amd', 'csrc'), '-I', os.path.join(ROOT, 'include'), src, '-o', exe],
                   check=True)
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    out = subprocess.run([exe], check=False, capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith('OK')
    src, img = {}, {}
    for line in out.stdout.splitlines():
        head, _, values = line.partition(':')
        head, values = head.split(), [int(v) for v in values.split()]
        if head and head[0] == 'src':
            src[(MODES[int(head[1])], int(head[2]), int(head[3]))] = values
        elif head and head[0] == 'img':
            img.setdefault((MODES[int(head[1])], int(head[2]), int(head[3])), {})[int(head[4])] = values
    return src, img


def admitted(mode, a, S):
    """The limits, restated: 'circular' wraps at most once, 'reflect' does not repeat the edge, 'valid' needs a sample."""
    return {'valid': S >= a, 'full': True, 'circular': a - 1 <= S, 'reflect': a - 1 < S}[mode]


def test_every_admitted_axis_is_covered(tables):
    src, img = tables
    want = {(mode, a, S) for mode in MODES for a in range(1, 7) for S in range(1, 9) if admitted(mode, a, S)}
    assert set(img) == want
    assert set(src) == {key for key in want if key[0] != 'valid'}
    assert all(sorted(img[key]) == list(range(key[2])) for key in want)
    assert ('circular', 6, 5) in want and ('circular', 6, 4) not in want   # S = a - 1: admitted, the smallest
    assert ('reflect', 6, 6) in want and ('reflect', 6, 5) not in want     # S = a: the smallest admitted


def test_pad_src_is_numpys_padding(tables):
    src, _ = tables
    for (mode, a, S), row in src.items():
        x = np.arange(S)
        if mode == 'full':   # zeros on both sides (here -1: tells a zero from activation 0)
            want = np.pad(x, (a - 1, a - 1), mode='constant', constant_values=-1)
        else:
            want = np.pad(x, (a - 1, 0), mode='wrap' if mode == 'circular' else 'reflect')
        assert row == want.tolist(), (mode, a, S)


@pytest.mark.parametrize('kind', ['numpy', 'torch'])
def test_python_axis_images_matches_the_header(tables, kind):
    _, img = tables
    for (mode, a, S), per_shift in img.items():
        u = np.arange(S, dtype=np.int64) if kind == 'numpy' else torch.arange(S, dtype=torch.int64)
        first, second, has_second = axis_images(mode, u, a, S)
        assert (has_second is None) == (mode in ('valid', 'full')) and (second is None) == (has_second is None)
        assert type(first) is type(u) and (second is None or type(second) is type(u))
        for i in range(S):
            got = [int(first[i])] + ([int(second[i])] if has_second is not None and bool(has_second[i]) else [])
            assert got == per_shift[i], (mode, a, S, i)

"""
The activation correlogram without a GPU: ``activation_correlogram_numpy`` against the definition evaluated one term at a
time (tests/correlogram_reference.py), the front end -- ``activation_correlogram``, ``atom_cooccurrence`` -- over the oracle
backend in every reconstruction mode and with transforms, and the host mirror of the kernel's tiling
(tests/correlogram_dispatch.py): its constants are the kernel's and its cases cross every edge it names.
"""
import os
import re

import numpy as np
import pytest

import correlogram_dispatch as cd
import correlogram_reference as cref
from conftest import ROOT
from test_atom_gains_cpu import _AtomStub, model
from tnmf_amd.correlogram_host import activation_correlogram_numpy, cooccurrence
from tnmf_amd.TransformInvariantNMF import TransformInvariantNMF

MODES = ('valid', 'full', 'circular', 'reflect')


def sparse(shape, seed, dtype=np.float64):
    rng = np.random.default_rng(seed)
    return (rng.random(shape) * (rng.random(shape) > 0.4)).astype(dtype)


# -- 1. the host fallback is the definition -------------------------------------------------------------------------------------
@pytest.mark.parametrize('S,L', [((7,), (3,)), ((5,), (9,)), ((4, 6), (2, 3)), ((3, 5), (4, 1)), ((1, 6), (2, 2)), ((4, 5), (0, 0))])
@pytest.mark.parametrize('per_sample', [False, True])
def test_numpy_is_the_brute_force_sum(S, L, per_sample):
    H = sparse((3, 4) + S, 1)
    want = cref.brute(H, L, per_sample)
    got = activation_correlogram_numpy(H, L, per_sample)
    assert got.dtype == np.float64 and got.shape == ((3,) if per_sample else ()) + (4, 4) + tuple(2 * x + 1 for x in L)
    ratio = cref.within_bar(got, want, S, L, 1 if per_sample else 3)
    print(f'largest error / bar: {ratio:.3f}')
    assert ratio <= 1.


@pytest.mark.parametrize('S,L', [((9,), (12,)), ((4, 6), (5, 7))])
def test_symmetry_zeros_and_the_sum_over_samples(S, L):
    H = sparse((3, 5) + S, 2, np.float32)
    C = activation_correlogram_numpy(H, L, True)
    flip = tuple(slice(None, None, -1) for _ in S)
    np.testing.assert_array_equal(C, C.transpose(0, 2, 1, *range(3, C.ndim))[(slice(None),) * 3 + flip])   # C[p,q,D] == C[q,p,-D]
    for k, (s, x) in enumerate(zip(S, L)):   # zeros where |D_k| >= S_k
        lag = np.abs(np.arange(-x, x + 1))
        assert np.all(np.compress(lag >= s, C, axis=3 + k) == 0) and np.any(np.compress(lag < s, C, axis=3 + k) != 0)
    total = activation_correlogram_numpy(H, L)
    assert cref.within_bar(C.sum(axis=0), total, S, L, 3) <= 1.
    centre = (Ellipsis,) + L
    diag = np.einsum('pp->p', total[centre])
    assert np.all(total ** 2 <= np.multiply.outer(diag, diag).reshape(5, 5, *(1,) * len(S)) * (1 + 1e-12))   # Cauchy-Schwarz


# -- 2. the front end over the oracle backend -----------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('transforms', [None, 'rot90'])
def test_front_end_shapes_default_lag_and_values(mode, transforms):
    nmf = model((3, 1, 9, 9), 2, (3, 3), mode, transforms=transforms)
    T = 1 if transforms is None else 4
    P = 2 * T
    H = nmf.H.reshape((3, P) + nmf.H.shape[-2:])
    C = nmf.activation_correlogram()
    assert C.dtype == np.float64 and C.shape == (P, P, 5, 5)          # the default: atom_shape - 1 per axis
    np.testing.assert_array_equal(C, activation_correlogram_numpy(H, (2, 2)))
    np.testing.assert_array_equal(nmf.activation_correlogram(1), activation_correlogram_numpy(H, (1, 1)))
    per = nmf.activation_correlogram((0, 3), per_sample=True)
    assert per.shape == (3, P, P, 1, 7)
    np.testing.assert_array_equal(per, activation_correlogram_numpy(H, (0, 3), True))
    score, lag = nmf.atom_cooccurrence()
    assert score.shape == (P, P) and lag.shape == (P, P, 2) and lag.dtype == np.int64
    assert np.all((score >= 0) & (score <= 1)) and np.all(np.abs(lag) <= 2)
    want = cooccurrence(C)
    np.testing.assert_array_equal(score, want[0])
    np.testing.assert_array_equal(lag, want[1])


def test_front_end_on_one_shift_axis():
    nmf = model((2, 2, 20), 3, (5,))
    C = nmf.activation_correlogram()
    assert C.shape == (3, 3, 9)
    np.testing.assert_array_equal(C, activation_correlogram_numpy(nmf.H, (4,)))
    assert nmf.activation_correlogram([30]).shape == (3, 3, 61)


def test_per_sample_comes_in_the_order_of_H_under_a_shuffle():
    nmf = model((5, 1, 9, 8), 2, (3, 3))
    plain = nmf.activation_correlogram(per_sample=True)
    nmf._shuffle_idx = np.array([3, 0, 4, 1, 2])
    try:
        np.testing.assert_array_equal(nmf.activation_correlogram(per_sample=True), plain[np.argsort(nmf._shuffle_idx)])
        H = nmf.H
        np.testing.assert_array_equal(nmf.activation_correlogram(per_sample=True), activation_correlogram_numpy(H, (2, 2), True))
    finally:
        nmf._shuffle_idx = None


def test_a_backend_hook_is_used_and_its_refusal_falls_back():
    nmf = model((2, 1, 9, 8), 2, (3, 3))
    calls = []

    def hook(H, max_lag, per_sample=False):
        calls.append((tuple(max_lag), per_sample))
        if max_lag[0] > 2:
            raise NotImplementedError('beyond the limit')
        return np.full((2, 2, 2, 5, 5) if per_sample else (2, 2, 5, 5), 7.)
    nmf._backend.activation_correlogram = hook
    assert np.all(nmf.activation_correlogram() == 7.) and np.all(nmf.activation_correlogram(per_sample=True) == 7.)
    np.testing.assert_array_equal(nmf.activation_correlogram(3), activation_correlogram_numpy(nmf.H, (3, 3)))
    assert calls == [((2, 2), False), ((2, 2), True), ((3, 3), False)]


@pytest.mark.parametrize('bad', [-1, 1.5, True, 'all', (1,), (1, 2, 3), (1, -2), (1, 2.), [None, 1], np.array([1, 1])])
def test_bad_max_lag_raises_ValueError(bad):
    nmf = model((2, 1, 9, 8), 2, (3, 3))
    with pytest.raises(ValueError, match='max_lag must be'):
        nmf.activation_correlogram(bad)
    with pytest.raises(ValueError, match='max_lag must be'):
        nmf.atom_cooccurrence(bad)


@pytest.mark.parametrize('bad', [1, 0, None, 'yes'])
def test_bad_per_sample_raises_ValueError(bad):
    nmf = model((2, 1, 9, 8), 2, (3, 3))
    with pytest.raises(ValueError, match='per_sample must be a bool'):
        nmf.activation_correlogram(per_sample=bad)


def test_an_unfitted_model_raises_RuntimeError():
    nmf = TransformInvariantNMF(n_atoms=2, atom_shape=(3, 4), backend=_AtomStub())
    for call in (nmf.activation_correlogram, nmf.atom_cooccurrence):
        with pytest.raises(RuntimeError, match='needs a fitted model: call fit first'):
            call()


# -- 3. atom_cooccurrence on planted activations ----------------------------------------------------------------------------------
def planted():
    """[2, 4, 40, 50]: plane 1 is plane 0 moved by (2, -3), plane 2 fires every 7th column, plane 3 is dead."""
    rng = np.random.default_rng(5)
    H = np.zeros((2, 4, 40, 50))
    at = rng.integers([0, 0, 6, 8], [2, 1, 32, 40], size=(30, 4))
    for n, _, y, x in at:
        h = 0.5 + rng.random()
        H[n, 0, y, x] += h
        H[n, 1, y + 2, x - 3] += h
    H[:, 2, 10:30:3, 1::7] = 1. + rng.random((2, 7, 7))
    return H


def test_cooccurrence_finds_the_partner_the_rhythm_and_the_dead_plane():
    nmf = model((2, 1, 38, 48), 4, (3, 3))
    nmf._H = planted()
    score, lag = nmf.atom_cooccurrence(max_lag=(4, 15))
    assert score[0, 1] > 0.99 and tuple(lag[0, 1]) == (2, -3)
    assert score[1, 0] > 0.99 and tuple(lag[1, 0]) == (-2, 3)
    assert lag[2, 2, 0] == 0 and lag[2, 2, 1] != 0 and lag[2, 2, 1] % 7 == 0 and score[2, 2] > 0.5
    assert np.all(score[3] == 0) and np.all(score[:, 3] == 0)
    assert np.all((score >= 0) & (score <= 1))


def test_cooccurrence_ties_go_to_the_first_lag_and_lag_0_is_left_out_on_the_diagonal():
    C = np.zeros((2, 2, 3, 5))
    C[0, 0, 1, 2], C[1, 1, 1, 2] = 4., 9.          # the energies at D = 0
    C[0, 1, 0, 3] = C[0, 1, 2, 1] = 3.             # two equal maxima: (-1, 1) comes first in C order
    C[1, 0, 2, 1] = C[1, 0, 0, 3] = 3.
    C[0, 0, 1, 0] = C[0, 0, 1, 4] = 1.             # the diagonal: D = 0 (4.) does not compete
    score, lag = cooccurrence(C)
    assert score[0, 1] == 0.5 and tuple(lag[0, 1]) == (-1, 1) and tuple(lag[1, 0]) == (-1, 1)
    assert score[0, 0] == 0.25 and tuple(lag[0, 0]) == (0, -2)
    assert score[1, 1] == 0. and tuple(lag[1, 1]) == (-1, -2)      # nothing but zeros: the first lag
    only0 = cooccurrence(np.ones((2, 2, 1)))
    assert np.array_equal(only0[0], [[0., 1.], [1., 0.]]) and np.all(only0[1] == 0)


# -- 4. the host mirror of the kernel's tiling --------------------------------------------------------------------------------------
def _flat(name):
    return re.sub(r'\s+', ' ', open(os.path.join(ROOT, 'tnmf_amd', 'csrc', name)).read())


def test_the_constants_are_the_kernels():
    h, hip = _flat('correlogram.h'), _flat('correlogram.hip')
    for name, value in (('kCorrThreads', cd.THREADS), ('kCorrBlock', cd.BLOCK), ('kCorrChunk', cd.CHUNK),
                        ('kCorrTile1Float', cd.TILE1['f32']), ('kCorrTile1Double', cd.TILE1['f64']), ('kCorrTileX', cd.TILE_X),
                        ('kCorrTileYFloat', cd.TILE_Y['f32']), ('kCorrTileYDouble', cd.TILE_Y['f64']), ('kCorrPad', cd.PAD),
                        ('kCorrMaxLag1', cd.MAX_LAG[1]), ('kCorrMaxLag2', cd.MAX_LAG[2]),
                        ('kCorrTargetGroups', cd.TARGET_GROUPS)):
        assert f'constexpr int {name} = {value};' in h, name
    assert f'constexpr size_t kCorrPartialCap = (size_t){cd.PARTIAL_CAP >> 20} << 20;' in h
    for line in ('p.Lye = std::min(p.Ly, Sy - 1);', 'p.Lxe = std::min(p.Lx, Sx - 1);',
                 'p.TY = ndim == 1 ? 1 : dtype == 0 ? kCorrTileYFloat : kCorrTileYDouble;',
                 'p.TX = ndim == 2 ? kCorrTileX : dtype == 0 ? kCorrTile1Float : kCorrTile1Double;',
                 'p.nb = cdiv(P, kCorrBlock);', 'p.pairs = p.nb * p.nb;', 'p.c0 = cdiv(p.Lxe + 1, kCorrChunk);',
                 'p.cr = cdiv(2 * p.Lxe + 1, kCorrChunk);', 'p.chunks = p.c0 + p.Lye * p.cr;',
                 'p.nh = p.Lxe + 1 + p.Lye * (2 * p.Lxe + 1);',
                 'const long long want = (kCorrTargetGroups + units - 1) / units;',
                 'p.ipg = std::max<long long>(1, (p.seglen + strips - 1) / strips);', 'p.strips = (int)((p.seglen + p.ipg - 1) / p.ipg);',
                 'p.lds = (size_t)p.TY * kCorrBlock * (2 * p.TX + kCorrChunk + 2 * kCorrPad) * esize(dtype);',
                 'dx0 = -p.Lxe + (c - p.c0) % p.cr * kCorrChunk;',
                 '__builtin_amdgcn_mfma_f64_16x16x4f64(a, (double)brow[4 * gx + kWaves * j], acc[j], 0, 0, 0);'):
        assert line in hip, line
    assert 'atomic' not in hip.replace('No atomics', '')   # the sums are ordered
    from tnmf_amd.backends.HIP import HIP_Backend
    assert HIP_Backend.CORRELOGRAM_MAX_LAG == cd.MAX_LAG


def test_the_plan():
    p = cd.plan(256, 32, (267, 267), (11, 11), False, 'f32')   # config 3, the default lags
    assert (p['nb'], p['pairs'], p['chunks'], p['nh']) == (2, 4, 12, 12 + 11 * 23) and p['nh'] == 265
    assert (p['tiles'], p['strips'], p['ipg']) == (67 * 5, 43, 1995) and p['groups'] == 43 * 48
    assert p['partial_bytes'] == 43 * 4 * 265 * 2048 and p['lds'] == 43008 <= 64 * 1024
    p = cd.plan(256, 32, (267, 267), (3, 3), False, 'f32')
    assert (p['chunks'], p['nh']) == (4, 25)
    for dt in ('f32', 'f64'):
        for S, L in (((1500,), (1023,)), ((40, 40), (31, 31))):
            p = cd.plan(2, 3, S, L, False, dt)
            assert p['lds'] <= 64 * 1024
            lags = cd.lags_computed(p)                     # every lag >= 0 in C order, once, in the order of the partial sums
            want = [(0, dx) for dx in range(p['Lxe'] + 1)]
            want += [(dy, dx) for dy in range(1, p['Lye'] + 1) for dx in range(-p['Lxe'], p['Lxe'] + 1)]
            assert lags == want and len(lags) == p['nh']
    p = cd.plan(1, 2, (1500,), (1023,), False, 'f32')
    assert (p['c0'], p['chunks'], p['tiles']) == (32, 32, 6)


def test_the_matrix_reaches_every_branch_in_both_precisions():
    for dt in ('f32', 'f64'):
        got = set()
        for name, (N, P, S, L) in cd.MATRIX.items():
            for per_sample in (False, True):
                p = cd.plan(N, P, S, L, per_sample, dt)
                assert p['lds'] <= 64 * 1024 and p['groups'] <= 40000 and p['partial_bytes'] <= 128 << 20, name
                got |= cd.reached(N, P, S, L, per_sample, dt)
        assert got == set(cd.BRANCHES), (dt, set(cd.BRANCHES) ^ got)
    r = lambda name, per, dt: cd.reached(*cd.MATRIX[name], per, dt)   # noqa: E731
    assert {'lag-clamped-x', 'lag-extent-minus-1'} <= r('1d-70-lag-200', False, 'f32') and 'lag-0-only' in r('1d-70-lag-0', False, 'f32')
    assert {'row0-several-chunks', 'chunk-full', 'several-tiles'} <= r('1d-1500-lag-1023', False, 'f64')
    assert {'row-several-chunks', 'lag-clamped-y', 'window-left-of-plane'} <= r('2d-19x37-lag-31-31', True, 'f32')
    assert {'blocks-several', 'last-block-ragged', 'lag-0-skipped-below-diagonal'} <= r('2d-planes-33', False, 'f32')
    assert {'blocks-1', 'last-block-full'} <= r('2d-planes-16', False, 'f32') and 'last-block-full' in r('2d-planes-48', False, 'f64')
    for dt in ('f32', 'f64'):
        assert {'strip-several-items', 'strip-ragged', 'strip-straddles-samples'} <= r('strips-several-items', False, dt)
        assert {'strip-several-items', 'per-sample'} <= r('strips-several-items', True, dt)
    assert 'x-below-tile' in r('1d-255', False, 'f32') and 'x-below-tile' in r('1d-127', False, 'f64')
    assert 'x-above-tile' in r('1d-257', False, 'f32') and 'x-above-tile' in r('1d-129', False, 'f64')
    assert 'y-below-tile' in r('2d-3x63', False, 'f32') and 'y-below-tile' in r('2d-1x63', False, 'f64')
    assert 'y-above-tile' in r('2d-5x65', False, 'f32') and 'y-above-tile' in r('2d-5x65', False, 'f64')

"""
Detections on CPU: the front end's ``detections()`` over an oracle-backed backend without ``find_peaks`` (the host
fallback), against the brute-force reference tests/peaks_reference.py -- exact comparisons throughout.
"""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

import peaks_reference as pref
from conftest import ROOT
from oracle import tnmf_oracle as orc
from oracle_backend import OracleBackend
from tnmf_amd import _lib, sharding, transforms as tr
from tnmf_amd.backends._Backend import sliceNone
from tnmf_amd.TransformInvariantNMF import Detections, TransformInvariantNMF, find_peaks_numpy


class _Stub(OracleBackend):
    """The oracle's primitives in any reconstruction mode, with the few hooks a transformed model needs to take an H half
    step.  No ``find_peaks``: ``detections()`` searches on the host."""

    supports_transforms = True

    def __init__(self, mode='valid'):
        super().__init__(impl='contract')
        self._reconstruction_mode = mode

    def _initialize_matrices(self, V, atom_shape, n_atoms, W=None, axes_W_normalization=None, transforms=None):
        T = 1 if transforms is None else tr.size(transforms)
        self._V_local, self._shard = V, (0, V.shape[0])
        H = np.empty((V.shape[0], n_atoms * T) + self._transform_shape, dtype=V.dtype)
        for i, h in sharding.reference_init_stream(V.shape[0], H.shape[1:], self._shard, V.dtype):
            H[i] = h
        if W is None:
            W = sharding.reference_init_W(n_atoms, self.n_channels, self.atom_shape, V.dtype)
        return W, H

    def reconstruct(self, W, H):
        return orc.reconstruct(W, H, self.impl, self._reconstruction_mode)

    def reconstruction_gradient_H(self, V, W, H, s=sliceNone):
        return orc.gradient_H(self._V_local, W, H, s, self.impl, self._reconstruction_mode)

    def reconstruction_gradient_W(self, V, W, H, s=sliceNone):
        return orc.gradient_W(self._V_local, W, H, s, self.impl, self._reconstruction_mode)

    def reconstruction_energy(self, V, W, H, beta=2., eps=1e-9):
        return orc.energy(self._V_local, W, H, self.impl, self._reconstruction_mode)

    def expand_W(self, W, transforms, W_eff=None):
        e = tr.expand(W, transforms)
        if W_eff is None:
            return e
        W_eff[...] = e
        return W_eff

    def fused_update_H(self, V, W, H, s=sliceNone, sparsity=0., eps=1e-9, beta=2., **_):
        neg, pos = self.reconstruction_gradient_H(V, W, H, s)
        orc.multiplicative_update(H[s], neg, pos, eps, sparsity)


def fitted(shape_V, n_atoms, atom_shape, mode='valid', dtype=np.float64, seed=0, **kw):
    """A model after a 1-iteration fit (W not updated for a transformed model: the stub has no W step for those)."""
    V = np.random.default_rng(seed).random(shape_V).astype(dtype)
    np.random.seed(42)
    nmf = TransformInvariantNMF(n_atoms=n_atoms, atom_shape=atom_shape, backend=_Stub(mode), **kw)
    nmf.fit(V, n_iterations=1, update_W='transforms' not in kw)
    return nmf


def set_H(nmf, H):
    assert nmf._H.shape == H.shape
    nmf._H[...] = H


def expect(nmf, threshold, radius, group=1, max_per_sample=None):
    be = nmf._backend
    return pref.detections(nmf.H, threshold, radius, group, nmf.atom_shape, be._reconstruction_mode,
                           nmf.n_transforms, max_per_sample)


def tie_rich(shape, seed, dtype=np.float64):
    """Integer-valued entries 0..5, about 70 % zeros: ties and plateaus are common."""
    rng = np.random.default_rng(seed)
    return np.where(rng.random(shape) < 0.7, 0, rng.integers(1, 6, shape)).astype(dtype)


# -- 1. semantics -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def model_1d():
    return fitted((2, 1, 30), 3, (5,))       # H [2, 3, 34]


@pytest.fixture(scope='module')
def model_2d():
    return fitted((2, 1, 10, 12), 3, (3, 4), dtype=np.float32)   # H [2, 3, 12, 15]


def test_a_plateau_wider_than_the_window_has_one_winner(model_1d):
    nmf = model_1d
    H = np.zeros(nmf._H.shape)
    H[0, 1, 10:21] = 2.          # 11 equal entries, window 2 * 2 + 1 = 5
    H[1, 2, 5:9] = 1.
    H[1, 2, 30] = 1.             # the same value outside the other plateau's reach
    set_H(nmf, H)
    det = nmf.detections(threshold=0., min_distance=2)
    assert isinstance(det, Detections) and len(det) == 3
    np.testing.assert_array_equal(det.sample, [0, 1, 1])
    np.testing.assert_array_equal(det.atom, [1, 2, 2])
    np.testing.assert_array_equal(det.shift, [[10], [5], [30]])     # the lowest index of each plateau
    np.testing.assert_array_equal(det.transform, [0, 0, 0])
    pref.assert_equal(det, expect(nmf, 0., (2,)))


def test_threshold_is_strict_and_nan_is_nothing(model_1d):
    nmf = model_1d
    H = np.zeros(nmf._H.shape)
    H[0, 0, 3], H[0, 0, 20] = 1.5, 1.5000000000000002
    H[1, 1, 7], H[1, 1, 8], H[1, 1, 9] = 3., np.nan, 2.             # NaN neither detected nor suppressing
    H[1, 1, 25] = np.inf
    set_H(nmf, H)
    det = nmf.detections(threshold=1.5, min_distance=0)
    np.testing.assert_array_equal(det.shift[:, 0], [20, 7, 9, 25])
    pref.assert_equal(det, expect(nmf, 1.5, (0,)))
    det = nmf.detections(threshold=1.5, min_distance=1)             # (3. at 7 does not reach 9; the NaN at 8 does nothing)
    np.testing.assert_array_equal(det.shift[:, 0], [20, 7, 9, 25])
    det = nmf.detections(threshold=1.5, min_distance=2)
    np.testing.assert_array_equal(det.shift[:, 0], [20, 7, 25])
    pref.assert_equal(det, expect(nmf, 1.5, (2,)))


def test_float32_threshold_is_compared_exactly(model_2d):
    nmf = model_2d
    H = np.zeros(nmf._H.shape, dtype=np.float32)
    t32 = np.float32(0.1)                                           # float32(0.1) > 0.1 > its float32 predecessor
    H[0, 0, 2, 2], H[0, 0, 8, 8] = t32, np.nextafter(t32, np.float32(0))
    set_H(nmf, H)
    det = nmf.detections(threshold=0.1, min_distance=0)
    np.testing.assert_array_equal(det.shift, [[2, 2]])
    assert det.strength.dtype == np.float32
    pref.assert_equal(det, expect(nmf, 0.1, (0, 0)))
    assert len(nmf.detections(threshold=float(t32), min_distance=0)) == 0


@pytest.mark.parametrize('radius', [(0, 0), (1, 2), (2, 0), (100, 100), (0, 100)], ids=str)
@pytest.mark.parametrize('threshold', [0., 2.])
def test_tie_rich_planes_equal_the_reference(model_2d, radius, threshold):
    nmf = model_2d
    set_H(nmf, tie_rich(nmf._H.shape, 5, np.float32))
    want = expect(nmf, threshold, radius)
    assert 0 < len(want['sample']) < nmf._H.size
    pref.assert_equal(nmf.detections(threshold=threshold, min_distance=radius), want)
    if radius == (0, 0):   # a pure threshold
        assert len(want['sample']) == int(np.sum(nmf.H > threshold))
    if radius == (100, 100):   # the whole plane: one winner each
        assert len(want['sample']) == 2 * 3


def test_suppress_all_picks_one_atom_per_location(model_2d):
    nmf = model_2d
    H = tie_rich(nmf._H.shape, 6, np.float32)
    set_H(nmf, H)
    det = nmf.detections(threshold=0., min_distance=0, suppress='all')
    pref.assert_equal(det, expect(nmf, 0., (0, 0), group=3))
    # radius 0: per location the strongest atom, the lowest atom index on a tie
    n, y, x = np.nonzero(H.max(axis=1) > 0)
    winners = sorted(zip(n, np.argmax(H, axis=1)[n, y, x], y, x))
    assert [tuple(r) for r in np.column_stack([det.sample, det.atom, det.shift])] == winners
    det = nmf.detections(threshold=0., min_distance=(1, 1), suppress='all')
    pref.assert_equal(det, expect(nmf, 0., (1, 1), group=3))


def test_default_min_distance_is_the_inhibition_range(model_2d):
    nmf = model_2d
    set_H(nmf, tie_rich(nmf._H.shape, 7, np.float32))
    assert nmf._inhibition_range == (2, 3)
    pref.assert_equal(nmf.detections(), expect(nmf, 0., (2, 3)))
    pref.assert_equal(nmf.detections(min_distance=1), expect(nmf, 0., (1, 1)))


def test_max_per_sample_with_ties(model_1d):
    nmf = model_1d
    H = np.zeros(nmf._H.shape)
    H[0, 2, 4], H[0, 0, 30], H[0, 1, 12], H[0, 0, 2] = 3., 3., 3., 5.     # three tied for the second place
    H[1, 1, 1], H[1, 0, 9] = 1., 2.
    set_H(nmf, H)
    det = nmf.detections(min_distance=0, max_per_sample=3)
    # sample 0: 5. and, of the tied 3., the two of lower flat index (atom 0 shift 30, atom 1 shift 12); C order
    np.testing.assert_array_equal(det.sample, [0, 0, 0, 1, 1])
    np.testing.assert_array_equal(det.atom, [0, 0, 1, 0, 1])
    np.testing.assert_array_equal(det.shift[:, 0], [2, 30, 12, 9, 1])
    np.testing.assert_array_equal(det.strength, [5., 3., 3., 2., 1.])
    for k in (0, 1, 2, 3, 10):
        pref.assert_equal(nmf.detections(min_distance=0, max_per_sample=k), expect(nmf, 0., (0,), max_per_sample=k))
    set_H(nmf, tie_rich(nmf._H.shape, 8))
    pref.assert_equal(nmf.detections(min_distance=1, max_per_sample=4), expect(nmf, 0., (1,), max_per_sample=4))


def test_fallback_on_three_shift_axes_and_groups():
    H = tie_rich((2, 4, 4, 5, 6), 9)
    for radius, group in itertools.product([(0, 0, 0), (1, 2, 1), (9, 9, 9)], [1, 2, 4]):
        idx, val = find_peaks_numpy(H, 0., radius, group)
        want_idx, want_val = pref.find_peaks(H, 0., radius, group)
        np.testing.assert_array_equal(idx, want_idx)
        assert val.tobytes() == want_val.tobytes() and 0 < len(idx) < H.size


# -- 2. origin: where the detected occurrence lies in the sample ------------------------------------------------------------
def placed(W_atom, origin, D, mode):
    """[C, *D]: the atom (not flipped) with its first pixel at `origin` -- clipped at the sample border ('valid', 'full'),
    wrapped around it ('circular'), and for 'reflect' once more at the mirrored origin -o on every axis with
    1 <= o <= A - 1 (the activation's mirror image in the left pad)."""
    A = W_atom.shape[1:]
    per_axis = []
    for o, a, d in zip(origin, A, D):
        o = int(o)
        if mode == 'circular':
            per_axis.append([o, o - d])
        elif mode == 'reflect' and 1 <= o <= a - 1:
            per_axis.append([o, -o])
        else:
            per_axis.append([o])
    R = np.zeros((W_atom.shape[0],) + tuple(D))
    for at in itertools.product(*per_axis):
        for j in itertools.product(*[range(a) for a in A]):
            pos = tuple(o + jj for o, jj in zip(at, j))
            if all(0 <= p < d for p, d in zip(pos, D)):
                R[(slice(None),) + pos] += W_atom[(slice(None),) + j]
    return R


@pytest.mark.parametrize('mode', ['valid', 'full', 'circular', 'reflect'])
@pytest.mark.parametrize('D, A', [((9,), (3,)), ((8, 9), (3, 4))], ids=['1d', '2d'])
def test_origin_is_where_the_reconstruction_puts_the_atom(mode, D, A):
    nmf = fitted((2, 2) + D, 3, A, mode=mode)
    S = nmf._H.shape[2:]
    per_axis = [sorted({0, 1, s // 2, s - 2, s - 1}) for s in S]      # borders, next to them, interior
    shifts = list(itertools.product(*per_axis)) if len(S) == 1 else \
        [tuple(ax[i] for ax in per_axis) for i in range(5)] + [(per_axis[0][0], per_axis[1][-1]),
                                                               (per_axis[0][-1], per_axis[1][1]),
                                                               (per_axis[0][2], per_axis[1][0])]
    for u in shifts:
        H = np.zeros(nmf._H.shape)
        H[(1, 2) + u] = 1.
        set_H(nmf, H)
        det = nmf.detections()
        assert len(det) == 1 and det.sample[0] == 1 and det.atom[0] == 2 and tuple(det.shift[0]) == u
        R = nmf._backend.reconstruct(nmf._W, nmf._H)
        want = placed(nmf.W[2], det.origin[0], D, mode)
        assert np.array_equal(R[1] > 0, want > 0), (mode, u, det.origin[0])
        np.testing.assert_allclose(R[1], want, rtol=1e-12, atol=0)
        assert not R[0].any()
        np.testing.assert_array_equal(det.origin[0], np.array(u) - (np.array(A) - 1 if mode == 'valid' else 0))


# -- 3. sample order ------------------------------------------------------------------------------------------------------
def test_samples_are_numbered_in_the_order_of_V_under_a_shuffle():
    nmf = fitted((5, 1, 20), 2, (4,))
    set_H(nmf, tie_rich(nmf._H.shape, 11))
    plain = nmf.detections(min_distance=1)
    internal = nmf._H.copy()
    nmf._shuffle_idx = np.array([3, 0, 4, 1, 2])
    assert np.array_equal(nmf.H[3], internal[0])                    # internal sample 0 is sample 3 of V
    det = nmf.detections(min_distance=1)
    pref.assert_equal(det, expect(nmf, 0., (1,)))
    np.testing.assert_array_equal(det.shift[det.sample == 3], plain.shift[plain.sample == 0])
    pref.assert_equal(nmf.detections(min_distance=1, max_per_sample=2), expect(nmf, 0., (1,), max_per_sample=2))


# -- 4. transforms ----------------------------------------------------------------------------------------------------------
def test_rot90_planes_split_into_atom_and_transform():
    nmf = fitted((2, 1, 9, 9), 2, (3, 3), transforms='rot90')
    assert nmf._H.shape == (2, 8, 11, 11) and nmf.H.shape == (2, 2, 4, 11, 11)
    H = np.zeros(nmf._H.shape)
    H[0, 1 * 4 + 2, 5, 5] = 2.       # atom 1, orientation 2
    H[0, 1 * 4 + 3, 5, 6] = 3.       # the same atom, another orientation, next to it
    H[0, 0 * 4 + 1, 5, 5] = 9.       # another atom at the same place
    H[1, 0 * 4 + 0, 0, 10] = 1.
    set_H(nmf, H)
    det = nmf.detections(min_distance=1)
    np.testing.assert_array_equal(np.stack([det.sample, det.atom, det.transform], 1),
                                  [[0, 0, 1], [0, 1, 2], [0, 1, 3], [1, 0, 0]])
    pref.assert_equal(det, expect(nmf, 0., (1, 1)))
    det = nmf.detections(min_distance=1, suppress='transforms')       # the orientations of atom 1 compete
    np.testing.assert_array_equal(np.stack([det.sample, det.atom, det.transform], 1), [[0, 0, 1], [0, 1, 3], [1, 0, 0]])
    pref.assert_equal(det, expect(nmf, 0., (1, 1), group=4))
    det = nmf.detections(min_distance=1, suppress='all')
    np.testing.assert_array_equal(np.stack([det.sample, det.atom, det.transform], 1), [[0, 0, 1], [1, 0, 0]])
    pref.assert_equal(det, expect(nmf, 0., (1, 1), group=8))
    set_H(nmf, tie_rich(nmf._H.shape, 12))
    for suppress, group in (('atom', 1), ('transforms', 4), ('all', 8)):
        pref.assert_equal(nmf.detections(threshold=1., suppress=suppress), expect(nmf, 1., (2, 2), group=group))


# -- 5. refusals ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kw', [dict(threshold=-1e-9), dict(threshold=float('nan')), dict(threshold=float('inf')),
                                dict(threshold='0'), dict(threshold=True), dict(threshold=None),
                                dict(min_distance=-1), dict(min_distance=(1,)), dict(min_distance=(1, 2, 3)),
                                dict(min_distance=(1, -2)), dict(min_distance=1.5), dict(min_distance=(1., 2.)),
                                dict(min_distance='2'), dict(min_distance=True),
                                dict(suppress='atoms'), dict(suppress=None), dict(suppress='transforms'),
                                dict(max_per_sample=-1), dict(max_per_sample=2.5)], ids=str)
def test_bad_arguments_raise_value_error(model_2d, kw):
    with pytest.raises(ValueError):
        model_2d.detections(**kw)


def test_detections_before_a_fit_raise_runtime_error():
    nmf = TransformInvariantNMF(n_atoms=2, atom_shape=(3,), backend=_Stub())
    with pytest.raises(RuntimeError):
        nmf.detections()


# -- 6. the ABI -------------------------------------------------------------------------------------------------------------
def test_find_peaks_is_declared_exported_and_typed():
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'tnmf_hip.h')).read(), flags=re.S)
    assert re.search(r'\bint tnmf_hip_find_peaks\s*\(', header)
    assert 'tnmf_hip_find_peaks' in _lib.EXPORTS and _lib.ABI_VERSION == 8
    lib = _lib.load()
    fn = lib.tnmf_hip_find_peaks
    vp = ctypes.c_void_p
    assert fn.restype is ctypes.c_int
    assert list(fn.argtypes) == [vp, ctypes.POINTER(_lib.Geom), vp, ctypes.c_double, ctypes.POINTER(ctypes.c_int),
                                 ctypes.c_int, vp, vp, ctypes.c_size_t, vp, vp]
    # argument errors are answered without a device: no context
    g = _lib.make_geom(1, 1, 1, (4,), (1,), 0)
    assert fn(None, ctypes.byref(g), None, 0., (ctypes.c_int * 3)(0, 0, 0), 1, None, None, 0, None, None) == -1

"""
separate() / dominant_source() on the CPU: the host fallback (tnmf_amd/sources_host.py) directly and through the front end
on an oracle backend without the hooks, against the float64 reference (tests/sources_reference.py).  Float64 throughout; the
bounds are relative 1e-10 of the reference, and the properties (masks in [0, 1], the sum over a partition) carry the same.
"""
import os
import re

import numpy as np
import pytest

import sources_reference as sref
from conftest import ROOT
from test_atom_gains_cpu import _AtomStub, model, weights_of
from test_events_cpu import fitted
from tnmf_amd import _lib
from tnmf_amd.atoms_host import pad_activations_numpy
from tnmf_amd.backends._Backend import shift_shape
from tnmf_amd.sources_host import dominant_numpy, separate_numpy, source_tables
from tnmf_amd.TransformInvariantNMF import TransformInvariantNMF

MODES = ['valid', 'full', 'circular', 'reflect']
RTOL = 1e-10
EPS = 1e-9


def close(got, want):
    return np.all(np.abs(got - want) <= RTOL * np.abs(want))


def random_operands(shape_V, P, A, mode, seed=7):
    rng = np.random.default_rng(seed)
    N, D = shape_V[0], shape_V[2:]
    W = rng.random((P, shape_V[1]) + A)
    H = rng.random((N, P) + shift_shape(mode, D, A)) * (rng.random((N, P) + (1,) * len(A)) > 0.2)
    return W, H, rng.random(shape_V)


def reference_of(nmf, sets):
    """The reference on the model's own (W_eff, H): sets of ATOMS -> sets of planes."""
    T = nmf.n_transforms
    planes = [[m * T + t for m in atoms for t in range(T)] for atoms in sets]
    W, H = nmf._backend.to_ndarray(nmf._W_dict), nmf._backend.to_ndarray(nmf._H)
    return sref.outputs(W, pad_activations_numpy(H, nmf.atom_shape, nmf._mode), nmf._V, planes, nmf.eps)


# -- 1. the fallback against the reference ---------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('shape_V, A', [((2, 3, 19), (4,)), ((2, 2, 8, 9), (3, 4))], ids=['1d', '2d'])
def test_the_fallback_equals_the_reference_in_the_four_modes(shape_V, A, mode):
    W, H, V = random_operands(shape_V, 5, A, mode)
    sets = [[3, 0], [1], [4]]   # (plane 2 is in no source)
    order, start = source_tables(sets)
    want = sref.outputs(W, pad_activations_numpy(H, A, mode), V, sets, EPS)
    for output in ('contribution', 'mask', 'masked'):
        got = separate_numpy(W, H, mode, V, order, start, output, EPS)
        assert got.shape == (shape_V[0], 3) + shape_V[1:] and got.dtype == np.float64
        assert close(got, want[output]), output
    label, share = dominant_numpy(W, H, mode, shape_V[2:], order, start, EPS)
    assert label.dtype == np.int32 and label.shape == share.shape == (shape_V[0],) + shape_V[2:]
    np.testing.assert_array_equal(label, want['label'])
    assert close(share, want['share'])


def test_ties_go_to_the_lowest_index_and_unexplained_pixels_get_minus_one():
    W = np.ones((3, 1, 2))
    H = np.zeros((1, 3, 7))   # 'valid': six pixels
    H[0, 0, 1] = H[0, 1, 1] = 2.   # sources 0 and 1 tie at pixels 0 and 1
    H[0, 2, 4] = 1.                # source 2 alone at pixels 3 and 4; pixels 2 and 5 are explained by nobody
    order, start = source_tables([[0], [1], [2]])
    label, share = dominant_numpy(W, H, 'valid', (6,), order, start, 0.)
    np.testing.assert_array_equal(label[0], [0, 0, -1, 2, 2, -1])
    np.testing.assert_array_equal(share[0], [.5, .5, 0., 1., 1., 0.])
    assert np.all(separate_numpy(W, H, 'valid', np.ones((1, 1, 6)), order, start, 'mask', 0.)[0, :, 0, 2] == 0.)


# -- 2. properties, through the front end ------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
def test_over_a_partition_the_sources_add_up(mode):
    nmf = model((2, 3, 8, 9), 4, (3, 3), mode)
    sets = [[2], [0, 3], [1]]
    V, R = nmf.V, nmf.R
    masked, contribution = nmf.separate(sets), nmf.separate(sets, output='contribution')
    assert masked.shape == (2, 3, 3, 8, 9) and masked.dtype == V.dtype
    assert close(contribution.sum(axis=1), R)
    assert close(masked.sum(axis=1), V * R / (R + nmf.eps))
    mask = nmf.separate(sets, output='mask')
    assert np.all(mask >= 0.) and np.all(mask <= 1.) and np.all(masked >= 0.) and np.all(masked <= V[:, None])
    np.testing.assert_array_equal(masked, V[:, None] * mask)


def test_every_output_equals_the_reference_through_the_front_end():
    nmf = model((2, 2, 9, 10), 3, (3, 4), 'reflect')
    sets = [[1], [2, 0]]
    want = reference_of(nmf, sets)
    for output in ('contribution', 'mask', 'masked'):
        assert close(nmf.separate(sets, output=output), want[output]), output
    label, share = nmf.dominant_source(sets)
    assert label.dtype == np.int32 and share.dtype == nmf.V.dtype
    np.testing.assert_array_equal(label, want['label'])
    assert close(share, want['share'])


def test_no_sources_means_every_atom_on_its_own():
    nmf = model((2, 1, 9, 10), 3, (3, 4))
    np.testing.assert_array_equal(nmf.separate(), nmf.separate([[0], [1], [2]]))
    np.testing.assert_array_equal(nmf.separate(output='mask'), nmf.separate([[0], [1], [2]], output='mask'))
    for got, want in zip(nmf.dominant_source(), nmf.dominant_source([[0], [1], [2]])):
        np.testing.assert_array_equal(got, want)
    for m in range(3):
        assert close(nmf.separate(output='contribution')[:, m], nmf.R_partial(m))


def test_unlisted_atoms_enter_the_denominator_only():
    nmf = model((2, 2, 8, 9), 3, (3, 3), 'circular')
    full, part = nmf.separate([[0], [1], [2]], output='mask'), nmf.separate([[2], [0]], output='mask')
    assert part.shape[1] == 2
    assert close(part[:, 0], full[:, 2]) and close(part[:, 1], full[:, 0])
    assert np.all(part.sum(axis=1) < 1.)   # (atom 1 explains something everywhere: the data is positive)


def test_with_rot90_an_atoms_source_holds_its_four_planes():
    nmf = model((2, 1, 8, 8), 2, (3, 3), 'valid', None, 'rot90')
    assert nmf.n_transforms == 4
    order, start = nmf._source_tables([[1], [0]])
    np.testing.assert_array_equal(order, [4, 5, 6, 7, 0, 1, 2, 3])
    np.testing.assert_array_equal(start, [0, 4, 8])
    got = nmf.separate([[1], [0]], output='contribution')
    for g, m in enumerate((1, 0)):
        assert close(got[:, g], nmf.R_partial(m))
    want = reference_of(nmf, [[1], [0]])
    assert close(nmf.separate([[1], [0]]), want['masked'])
    np.testing.assert_array_equal(nmf.dominant_source([[1], [0]])[0], want['label'])


@pytest.mark.parametrize('kind', ['mask', 'real'])
def test_weights_play_no_part_and_hidden_entries_are_masked_to_zero(kind):
    shape_V = (2, 2, 8, 9)
    G = weights_of(shape_V, kind)
    nmf = model(shape_V, 2, (3, 3), 'valid', G)
    want = reference_of(nmf, [[0], [1]])
    want['masked'] = np.where(G > 0, nmf._V, 0.)[:, None] * want['mask']   # (entries of weight 0 are not data)
    assert close(nmf.separate(), want['masked']) and close(nmf.separate(output='contribution'), want['contribution'])
    if kind == 'mask':
        hidden = np.broadcast_to((G == 0)[:, None], (2, 2) + shape_V[1:])
        assert hidden.any() and np.all(nmf.separate()[hidden] == 0.)
        assert np.all(nmf.separate(output='contribution')[hidden] > 0.)   # (the model's imputation)


def test_samples_come_in_the_order_of_V_under_a_shuffle():
    nmf = model((5, 1, 9, 8), 2, (3, 3))
    plain, (label, share) = nmf.separate(), nmf.dominant_source()
    nmf._shuffle_idx = np.array([3, 0, 4, 1, 2])
    try:
        order = np.argsort(nmf._shuffle_idx)
        np.testing.assert_array_equal(nmf.separate(), plain[order])
        np.testing.assert_array_equal(nmf.dominant_source()[0], label[order])
        np.testing.assert_array_equal(nmf.dominant_source()[1], share[order])
    finally:
        nmf._shuffle_idx = None


# -- 3. refusals ------------------------------------------------------------------------------------------------------------
def test_every_bad_argument_is_a_value_error_and_leaves_the_model_as_it_was():
    nmf = model((2, 1, 9, 10), 3, (3, 4))
    before = [np.array(x) for x in (nmf.W, nmf.H, nmf.V)]
    bad_sources = ([[0, 1], [1, 2]],   # overlapping
                   [[0, 0]],           # one atom twice in a set
                   [[0], []],          # an empty set
                   [],                 # no set at all
                   [[0], [3]], [[-1]],  # out of range
                   [[0.0]], [[True]], [['0']],   # not an int
                   [0, 1], 5, 'ab')    # not a sequence of sequences
    for bad in bad_sources:
        with pytest.raises(ValueError, match='sources must be'):
            nmf.separate(bad)
        with pytest.raises(ValueError, match='sources must be'):
            nmf.dominant_source(bad)
    for bad in ('dominant', 'Masked', None, 2):
        with pytest.raises(ValueError, match='output must be'):
            nmf.separate(output=bad)
    assert nmf.separate([(np.int64(2),), np.array([0])]).shape == (2, 2, 1, 9, 10)
    for was, now in zip(before, (nmf.W, nmf.H, nmf.V)):
        np.testing.assert_array_equal(was, now)
    with pytest.raises(RuntimeError):
        TransformInvariantNMF(n_atoms=2, atom_shape=(3, 4), backend=_AtomStub()).separate()


def test_volumes_are_refused():
    nmf = fitted((1, 1, 5, 5, 5), 1, (2, 2, 2))
    with pytest.raises(NotImplementedError, match='separate: 1 or 2 shift axes only'):
        nmf.separate()
    with pytest.raises(NotImplementedError, match='separate: 1 or 2 shift axes only'):
        nmf.dominant_source()


def test_a_backend_whose_hook_declines_falls_back_to_the_host():
    class Declines(_AtomStub):
        supports_sources = True

        def source_parts(self, *a, **k):
            raise NotImplementedError

        def dominant_parts(self, *a, **k):
            raise NotImplementedError

    np.random.seed(42)
    nmf = TransformInvariantNMF(n_atoms=2, atom_shape=(3, 3), backend=Declines())
    nmf.fit(np.random.default_rng(0).random((2, 1, 8, 8)) + 0.05, n_iterations=1, update_W=False)
    want = reference_of(nmf, [[0], [1]])
    assert close(nmf.separate(), want['masked'])
    np.testing.assert_array_equal(nmf.dominant_source()[0], want['label'])


# -- 4. the ABI -------------------------------------------------------------------------------------------------------------
def test_the_entry_point_is_declared_exported_and_built():
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'tnmf_hip.h')).read(), flags=re.S)
    assert re.search(r'\bint tnmf_hip_atom_sources\s*\(', header) and 'tnmf_hip_atom_sources' in _lib.EXPORTS
    for name, code in _lib.SOURCE_OUTPUTS.items():
        assert re.search(rf'#define TNMF_SOURCES_{name.upper()} {code}\b', header)
    makefile = open(os.path.join(ROOT, 'tnmf_amd', 'csrc', 'Makefile')).read()
    assert re.search(r'^SRCS\s*:=.*\bsources\.hip\b', makefile, flags=re.M)
    assert re.search(r'^HDRS\s*:=.*\batom_walk\.h\b.*\bsources\.h\b', makefile, flags=re.M)
    assert _lib.ABI_VERSION == 8
    import ctypes
    lib = _lib.load()
    vp, ci, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    assert list(lib.tnmf_hip_atom_sources.argtypes) == [vp, ctypes.POINTER(_lib.Geom), ci, vp, ci, vp, ci, cd] + [vp] * 7
    g = _lib.make_geom(1, 1, 1, (4,), (2,), 0)   # an argument error is answered without a device: no context
    assert lib.tnmf_hip_atom_sources(None, ctypes.byref(g), 1, None, 1, None, 0, 0., *([None] * 7)) == -1

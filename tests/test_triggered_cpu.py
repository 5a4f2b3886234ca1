"""
The triggered sums without a GPU: ``triggered_sums_numpy`` against the definition evaluated one term at a time and against
exact int64 sums (tests/triggered_reference.py), margin 0 against the oracle's W gradient in every reconstruction mode, the
tap gains against the brute-force drop of the objective, and the front end -- ``activation_triggered_sums``,
``activation_triggered_average``, ``atom_tap_gains``, ``atom_window_gains`` -- over the oracle backend.
"""
import numpy as np
import pytest

import triggered_reference as tref
from oracle import tnmf_oracle as orc
from test_atom_gains_cpu import _AtomStub, model
from tnmf_amd.atoms_host import pad_activations_numpy
from tnmf_amd.backends._Backend import shift_shape
from tnmf_amd.triggered_host import extend_atoms, tap_gains_from_sums, triggered_sums_numpy, window_gains
from tnmf_amd.TransformInvariantNMF import TransformInvariantNMF

MODES = ('valid', 'full', 'circular', 'reflect')
SHAPES = [((13,), (4,)), ((9, 11), (3, 4))]


def margins(D):
    return [(0,) * len(D), (2, 3)[:len(D)], tuple(d + 2 for d in D)]


def operands(D, A, seed, N=3, P=2, F=2, integer=False):
    rng = np.random.default_rng(seed)
    S = tuple(d + a - 1 for d, a in zip(D, A))
    if integer:
        return (rng.integers(0, 8, (N, P) + S) * (rng.random((N, P) + S) > 0.7)).astype(np.float64), \
            rng.integers(-7, 8, (N, F) + D).astype(np.float64)
    return rng.random((N, P) + S) * (rng.random((N, P) + S) > 0.4), rng.standard_normal((N, F) + D)


# -- 1. the host fallback is the definition -------------------------------------------------------------------------------------
@pytest.mark.parametrize('D,A', SHAPES)
@pytest.mark.parametrize('power', [1, 2])
@pytest.mark.parametrize('per_sample', [False, True])
def test_numpy_is_the_brute_force_sum(D, A, power, per_sample):
    Hp, Y = operands(D, A, 1)
    for m in margins(D):
        want = tref.brute(Hp, Y, A, m, power, per_sample)
        T = tref.brute(Hp, np.abs(Y), A, m, power, per_sample)
        got = triggered_sums_numpy(Hp, Y, A, m, power, per_sample)
        assert got.dtype == np.float64 and got.shape == ((3,) if per_sample else ()) + (2, 2) + tref.window(A, m)
        ratio = tref.within_bar(got, want, T, D, A, m, 1 if per_sample else 3)
        print(f'margin {m}: largest error / bar: {ratio:.3f}')
        assert ratio <= 1.
        assert np.all(got[np.broadcast_to(tref.terms(D, A, m, 1) == 0, got.shape)] == 0)   # no term: an exact 0


@pytest.mark.parametrize('D,A', SHAPES)
@pytest.mark.parametrize('power', [1, 2])
def test_numpy_and_brute_force_are_exact_on_integers(D, A, power):
    Hp, Y = operands(D, A, 2, integer=True)
    for m in margins(D):
        want = tref.exact_int64(Hp, Y, A, m, power, True)
        np.testing.assert_array_equal(triggered_sums_numpy(Hp, Y, A, m, power, True), want)
        np.testing.assert_array_equal(tref.brute(Hp, Y, A, m, power, True), want)
        np.testing.assert_array_equal(triggered_sums_numpy(Hp, Y, A, m, power), want.sum(axis=0))


def test_the_number_of_terms_is_counted_term_by_term():
    for D, A in SHAPES:
        for m in margins(D):
            ones_h, ones_y = np.ones((1, 1) + tuple(d + a - 1 for d, a in zip(D, A))), np.ones((1, 1) + D)
            np.testing.assert_array_equal(tref.brute(ones_h, ones_y, A, m)[0, 0], tref.terms(D, A, m, 1))


# -- 2. margin 0 is the reference's W gradient ----------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('D,A', SHAPES)
def test_margin_0_is_the_oracles_W_gradient(mode, D, A):
    rng = np.random.default_rng(3)
    N, P, C = 3, 2, 2
    V, W = rng.random((N, C) + D), rng.random((P, C) + A)
    H = rng.random((N, P) + shift_shape(mode, D, A))
    neg, pos = orc.gradient_W(V, W, H, mode=mode)
    Hp = pad_activations_numpy(H, A, mode)
    m = (0,) * len(D)
    for want, Y in ((neg, V), (pos, orc.reconstruct(W, H, mode=mode))):
        got = triggered_sums_numpy(Hp, Y, A, m)
        assert got.shape == want.shape
        ratio = tref.within_bar(got, want, triggered_sums_numpy(Hp, np.abs(Y), A, m), D, A, m, N)
        print(f'largest error / bar: {ratio:.3f}')
        assert ratio <= 1.


# -- 3. the tap gains are the drop of the objective -----------------------------------------------------------------------------
def plane_at(Hp_plane, D, A, m, j):
    """What one unit of tap j of the window adds to the reconstruction: [N, *D], out[y] = Hp[y + (A - 1) + m - j]."""
    out = np.zeros(Hp_plane.shape[:1] + tuple(D))
    for y in np.ndindex(*D):
        q = tuple(yk + (a - 1) + x - jk for yk, a, x, jk in zip(y, A, m, j))
        if all(0 <= qk < s for qk, s in zip(q, Hp_plane.shape[1:])):
            out[(slice(None),) + y] = Hp_plane[(slice(None),) + q]
    return out


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('D,A,m', [((13,), (4,), (3,)), ((9, 11), (3, 4), (2, 3))])
@pytest.mark.parametrize('weighted', [False, True])
def test_tap_gains_are_the_brute_force_drop_of_the_objective(mode, D, A, m, weighted):
    rng = np.random.default_rng(4)
    N, P, C = 2, 2, 2
    W = rng.random((P, C) + A)
    W[(0, 0) + (0,) * len(A)] = 0.01                           # a small tap the data will want below zero
    H = rng.random((N, P) + shift_shape(mode, D, A)) * (rng.random((N, P) + shift_shape(mode, D, A)) > 0.5)
    G = (rng.random((N, C) + D) * (rng.random((N, C) + D) > 0.2)) if weighted else np.ones((N, C) + D)
    Hp = pad_activations_numpy(H, A, mode)
    R = orc.reconstruct(W, H, mode=mode)
    V = R + 0.1 * rng.standard_normal(R.shape)
    V[:, 0] -= 0.5 * plane_at(Hp[:, 0], D, A, m, m)            # (tap 0 of the atom is position m of the window)
    V = np.maximum(V, 0)
    E = triggered_sums_numpy(Hp, G * (V - R), A, m)
    b = triggered_sums_numpy(Hp, G, A, m, power=2)
    W_ext = extend_atoms(W, m)
    gain, step = tap_gains_from_sums(E, b, W_ext)
    assert np.all(gain >= 0) and np.all(W_ext + step >= 0)
    objective = lambda R_: 0.5 * np.sum(G * (V - R_) ** 2)   # noqa: E731
    inside = np.zeros(W_ext.shape[2:], dtype=bool)
    inside[tuple(slice(x, x + a) for x, a in zip(m, A))] = True
    clipped = inside & (step == -W_ext).any(axis=(0, 1))
    assert clipped.any()                                       # a tap inside the window where the clip -W_ext binds
    taps = [tuple(np.argwhere(~inside)[0]), tuple(np.argwhere(~inside)[-1]), tuple(np.argwhere(clipped)[0]),
            tuple(np.argwhere(inside & ~clipped)[0])]
    for j in taps:
        for p in range(P):
            for c in range(C):
                at = (p, c) + j
                R2 = R.copy()
                R2[:, c] += step[at] * plane_at(Hp[:, p], D, A, m, j)
                drop = objective(R) - objective(R2)
                assert abs(drop - gain[at]) <= 1e-10 * max(1., objective(R)), (j, p, c, drop, gain[at])
                if b[at] > 0 and step[at] > -W_ext[at]:        # unclipped: no other step does better
                    for t in (0.9, 1.1):
                        R3 = R.copy()
                        R3[:, c] += t * step[at] * plane_at(Hp[:, p], D, A, m, j)
                        assert objective(R) - objective(R3) <= drop + 1e-12 * max(1., objective(R))
    ins, outs = window_gains(gain, m, P)
    np.testing.assert_allclose(ins + outs, gain.sum(axis=tuple(range(1, gain.ndim))), rtol=1e-12)
    np.testing.assert_allclose(ins, gain[(Ellipsis,) + tuple(slice(x, x + a) for x, a in zip(m, A))].sum(
        axis=tuple(range(1, gain.ndim))), rtol=1e-12)


def test_tap_gains_where_nothing_fires_are_zero():
    gain, step = tap_gains_from_sums(np.array([1., -2., 3.]), np.array([0., 2., 2.]), np.array([0., 0.5, 0.]))
    np.testing.assert_array_equal(step, [0., -0.5, 1.5])
    np.testing.assert_array_equal(gain, [0., 1. - 0.25, 4.5 - 2.25])


# -- 4. the front end over the oracle backend -----------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('transforms', [None, 'rot90'])
def test_front_end_shapes_default_margin_and_values(mode, transforms):
    nmf = model((3, 2, 9, 9), 2, (3, 3), mode, transforms=transforms)
    T = 1 if transforms is None else 4
    P = 2 * T
    H = nmf.H.reshape((3, P) + nmf.H.shape[-2:])
    Hp = pad_activations_numpy(H, (3, 3), mode)
    W_eff = np.asarray(nmf._backend.to_ndarray(nmf._W_dict), dtype=np.float64)
    V, R = nmf._V, orc.reconstruct(W_eff, H, mode=mode)
    before = [np.array(nmf.W, copy=True), np.array(nmf.H, copy=True), V.copy()]
    X = nmf.activation_triggered_sums()
    assert X.dtype == np.float64 and X.shape == (P, 2, 7, 7)          # the default: (a + 1) // 2 per axis
    np.testing.assert_array_equal(X, triggered_sums_numpy(Hp, V - R, (3, 3), (2, 2)))
    np.testing.assert_array_equal(nmf.activation_triggered_sums(0, 'data'), triggered_sums_numpy(Hp, V, (3, 3), (0, 0)))
    neg, pos = orc.gradient_W(V, W_eff, H, mode=mode)
    np.testing.assert_allclose(nmf.activation_triggered_sums(0, 'data'), neg, rtol=1e-12)
    np.testing.assert_allclose(nmf.activation_triggered_sums((0, 0), 'reconstruction'), pos, rtol=1e-12)
    per = nmf.activation_triggered_sums([1, 4], 'reconstruction', per_sample=True)
    assert per.shape == (3, P, 2, 5, 11)
    np.testing.assert_array_equal(per, triggered_sums_numpy(Hp, R, (3, 3), (1, 4), per_sample=True))
    avg = nmf.activation_triggered_average((4, 9))
    mass = triggered_sums_numpy(Hp, np.ones(V.shape), (3, 3), (4, 9))
    assert avg.shape == (P, 2, 11, 21) and np.array_equal(np.isnan(avg), mass == 0) and np.isnan(avg).any()
    with np.errstate(invalid='ignore'):
        np.testing.assert_array_equal(avg[mass > 0], (triggered_sums_numpy(Hp, V, (3, 3), (4, 9)) / mass)[mass > 0])
    gain, step = nmf.atom_tap_gains(1)
    want = tap_gains_from_sums(triggered_sums_numpy(Hp, V - R, (3, 3), (1, 1)),
                               triggered_sums_numpy(Hp, np.ones(V.shape), (3, 3), (1, 1), power=2), extend_atoms(W_eff, (1, 1)))
    np.testing.assert_array_equal(gain, want[0])
    np.testing.assert_array_equal(step, want[1])
    ins, outs = nmf.atom_window_gains(1)
    assert ins.shape == outs.shape == (2,) and np.all(ins >= 0) and np.all(outs >= 0)
    np.testing.assert_array_equal(np.stack([ins, outs]), np.stack(window_gains(gain, (1, 1), 2)))
    for a, b in zip(before, [nmf.W, nmf.H, nmf._V]):                   # W, H and V are not touched
        np.testing.assert_array_equal(a, b)


def test_front_end_on_one_shift_axis_and_with_weights():
    rng = np.random.default_rng(6)
    G = rng.random((2, 2, 20)) * (rng.random((2, 2, 20)) > 0.3)
    nmf = model((2, 2, 20), 3, (5,), 'full', weights=G)
    Hp = pad_activations_numpy(nmf.H, (5,), 'full')
    V = np.where(G > 0, nmf._V, 0)
    R = orc.reconstruct(nmf.W, nmf.H, mode='full')
    X = nmf.activation_triggered_sums()
    assert X.shape == (3, 2, 11)
    np.testing.assert_allclose(X, triggered_sums_numpy(Hp, G * (V - R), (5,), (3,)), rtol=1e-12, atol=1e-13)
    mass = triggered_sums_numpy(Hp, G, (5,), (3,))
    np.testing.assert_allclose(nmf.activation_triggered_average() * mass, triggered_sums_numpy(Hp, G * V, (5,), (3,)),
                               rtol=1e-12, atol=1e-13)
    gain, step = nmf.atom_tap_gains()
    want = tap_gains_from_sums(triggered_sums_numpy(Hp, G * (V - R), (5,), (3,)),
                               triggered_sums_numpy(Hp, G, (5,), (3,), power=2), extend_atoms(nmf.W, (3,)))
    np.testing.assert_allclose(gain, want[0], rtol=1e-9, atol=1e-12)
    assert nmf.activation_triggered_sums([30]).shape == (3, 2, 65)


def test_per_sample_comes_in_the_order_of_V_under_a_shuffle():
    nmf = model((5, 1, 9, 8), 2, (3, 3))
    plain = nmf.activation_triggered_sums(per_sample=True)
    nmf._shuffle_idx = np.array([3, 0, 4, 1, 2])
    try:
        np.testing.assert_array_equal(nmf.activation_triggered_sums(per_sample=True), plain[np.argsort(nmf._shuffle_idx)])
    finally:
        nmf._shuffle_idx = None


def test_a_backend_hook_is_used_and_its_refusal_falls_back():
    nmf = model((2, 1, 9, 8), 2, (3, 3))
    want = nmf.activation_triggered_sums(3)
    calls = []

    def sums(H, Y, margin, power=1, per_sample=False):
        calls.append((tuple(margin), power, per_sample))
        if margin[0] > 2:
            raise NotImplementedError('beyond the limit')
        return np.full((2, 1, 7, 7), 7.)
    backend = nmf._backend
    backend.supports_triggered = True
    backend.triggered_field = lambda V, W, H, source: V - backend.reconstruct(W, H) if source == 'residual' else None
    backend.triggered_sums = sums
    assert np.all(nmf.activation_triggered_sums() == 7.)
    np.testing.assert_array_equal(nmf.activation_triggered_sums(3), want)
    assert calls == [((2, 2), 1, False), ((3, 3), 1, False)]


@pytest.mark.parametrize('bad', [-1, 1.5, True, 'all', (1,), (1, 2, 3), (1, -2), (1, 2.), [None, 1], np.array([1, 1])])
def test_bad_margin_raises_ValueError(bad):
    nmf = model((2, 1, 9, 8), 2, (3, 3))
    for call in (nmf.activation_triggered_sums, nmf.activation_triggered_average, nmf.atom_tap_gains, nmf.atom_window_gains):
        with pytest.raises(ValueError, match='margin must be'):
            call(bad)


def test_bad_source_and_per_sample_raise_ValueError():
    nmf = model((2, 1, 9, 8), 2, (3, 3))
    for bad in ('weights', 'cleaned', None, 1):
        with pytest.raises(ValueError, match='source must be'):
            nmf.activation_triggered_sums(source=bad)
        with pytest.raises(ValueError, match='source must be'):
            nmf.activation_triggered_average(source=bad)
    for bad in (1, 0, None, 'yes'):
        with pytest.raises(ValueError, match='per_sample must be a bool'):
            nmf.activation_triggered_sums(per_sample=bad)


def test_refusals_unfitted_volumes_and_other_objectives():
    nmf = TransformInvariantNMF(n_atoms=2, atom_shape=(3, 4), backend=_AtomStub())
    for call in (nmf.activation_triggered_sums, nmf.activation_triggered_average, nmf.atom_tap_gains, nmf.atom_window_gains):
        with pytest.raises(RuntimeError, match='needs? a fitted model: call fit first'):
            call()
    nmf = model((2, 1, 9, 8), 2, (3, 3))
    nmf.atom_shape = (3, 3, 3)
    try:
        for call in (nmf.activation_triggered_sums, nmf.activation_triggered_average, nmf.atom_tap_gains, nmf.atom_window_gains):
            with pytest.raises(NotImplementedError, match='1 or 2 shift axes only'):
                call()
    finally:
        nmf.atom_shape = (3, 3)
    nmf._beta = 1.
    try:
        assert nmf.activation_triggered_sums().shape == (2, 1, 7, 7)      # a plain correlation: any beta_loss
        for call in (nmf.atom_tap_gains, nmf.atom_window_gains):
            with pytest.raises(NotImplementedError, match='Frobenius objective'):
                call()
    finally:
        nmf._beta = 2.

"""
The product front-end (tnmf_amd.TransformInvariantNMF) driven by the TEST-ONLY oracle backend must reproduce the
reference's known answers: this checks the MU schedules, the inhibition terms, the RNG draw order and fit_stream on
CPU, independently of the kernels.  (The same answers are checked through the real 'hip' backend in test_hip_*.py.)
"""
import numpy as np
import pytest

from oracle_backend import OracleBackend
from test_oracle_pinning import V_1D, racoon_patches_V, racoon_rgb_V
from tnmf_amd.TransformInvariantNMF import MiniBatchAlgorithm, TransformInvariantNMF


def _nmf(hooks=False, **kw):
    return TransformInvariantNMF(backend=OracleBackend(hooks=hooks), **kw)


def test_1d_inhibition_known_answer():
    np.random.seed(42)
    nmf = _nmf(n_atoms=3, atom_shape=(5,))
    nmf.fit(V_1D, inhibition_strength=0.1, n_iterations=10)
    assert np.isclose(nmf._energy_function(), 2.34946)          # tnmf/tests/test_1d.py:18
    assert np.allclose(nmf.W.sum(axis=-1), 1.)


@pytest.mark.parametrize('hooks', [False, True])
def test_2d_rgb_sparsity_known_answer(hooks):
    np.random.seed(42)
    nmf = _nmf(hooks, n_atoms=10, atom_shape=(7, 7))
    nmf.fit(racoon_rgb_V(), sparsity_H=0.1, n_iterations=10)
    assert np.isclose(nmf._energy_function(), 268.14423)        # tnmf/tests/test_backends.py:18
    assert nmf.R.shape == (2, 3, 76, 102) and nmf.R_partial(0).shape == (2, 3, 76, 102)


def test_cross_inhibition_known_answer():
    np.random.seed(42)
    nmf = _nmf(n_atoms=10, atom_shape=(7, 7), inhibition_range=(3, 3))
    nmf.fit(racoon_rgb_V(), n_iterations=25, cross_atom_inhibition_strength=0.5)
    assert np.isclose(nmf._energy_function(), 724.238350)       # tnmf/tests/test_sparsity_inhibition.py:47


@pytest.mark.parametrize('algorithm,hooks,E', [
    (MiniBatchAlgorithm.Cyclic_MU, True, 14434.02658),           # tnmf/tests/test_minibatch.py:20 (fused hooks)
    (MiniBatchAlgorithm.GSG_MU, False, 14223.14454),             # :22
    (MiniBatchAlgorithm.ASAG_MU, False, 4560.03432),             # :23
])
def test_minibatch_known_answers(algorithm, hooks, E):
    np.random.seed(42)
    nmf = _nmf(hooks, n_atoms=10, atom_shape=(7, 7))
    nmf.fit_minibatches(racoon_patches_V(), sparsity_H=0.1, algorithm=algorithm, batch_size=3, n_epochs=5,
                        sag_lambda=0.8)
    assert np.isclose(nmf._energy_function(), E)


def test_stream_known_answer():
    np.random.seed(42)
    nmf = _nmf(n_atoms=10, atom_shape=(7, 7))
    nmf.fit((v for v in racoon_patches_V()), sparsity_H=0.1, algorithm=MiniBatchAlgorithm.Cyclic_MU,
            subsample_size=50, max_subsamples=5, batch_size=3, n_epochs=5, sag_lambda=0.8)
    assert np.isclose(nmf._energy_function(), 629.109136)       # tnmf/tests/test_stream.py:108


def test_progress_callback_stops():
    seen = []
    np.random.seed(0)
    nmf = _nmf(n_atoms=2, atom_shape=(3,))
    nmf.fit(V_1D, n_iterations=50, progress_callback=lambda m, it: seen.append(it) or it < 2)
    assert seen == [0, 1, 2]


def test_unknown_backend_name():
    with pytest.raises(KeyError):
        TransformInvariantNMF(n_atoms=2, atom_shape=(3,), backend='numpy_fft')


@pytest.mark.parametrize('sag_lambda', [0.8, 1.0])
@pytest.mark.parametrize('algorithm', list(MiniBatchAlgorithm))
def test_epochs_as_operation_lists_equal_the_batch_by_batch_schedules(algorithm, sag_lambda):
    """The front end describes a mini-batch epoch as ONE operation list for backends that offer `run_schedule`
    (HIP_Backend -> tnmf_hip_run_schedule): H half steps, gradient blends acc = a * acc + b * g with the coefficients of
    reference TransformInvariantNMF.py:444-455 (first use from the integer 0 included; (1, 1) for sag_lambda == 1), W updates.
    Interpreted step by step with the oracle's primitives, the lists must reproduce the batch-by-batch schedules -- same RNG
    draws, same accumulator side effect (pos += eps) across epochs."""
    rng = np.random.default_rng(3)
    V = rng.random((7, 2, 12, 14))
    kw = dict(algorithm=algorithm, batch_size=2, n_epochs=3, sag_lambda=sag_lambda, sparsity_H=0.05)
    res = {}
    for flavour in ('lists', 'batch_by_batch'):
        np.random.seed(42)
        be = OracleBackend(hooks=True, schedules=flavour == 'lists')
        nmf = TransformInvariantNMF(n_atoms=3, atom_shape=(3, 4), backend=be)
        nmf.fit(V, **kw)
        res[flavour] = (nmf.W, nmf.H)
        if flavour == 'lists':
            assert len(be.schedule_calls) == 3, 'one operation list per epoch'
            per_batch = {'Cyclic_MU': ['H', 'G'], 'ASG_MU': ['H', 'G', 'W'], 'ASAG_MU': ['H', 'G', 'W']}.get(algorithm.name)
            if per_batch:
                assert be.schedule_calls[0][:len(per_batch)] == per_batch
            else:   # GSG / GSAG: H for every batch, then one gradient and one W update
                assert be.schedule_calls[0] == ['H'] * 4 + ['G', 'W']
    np.testing.assert_allclose(res['lists'][0], res['batch_by_batch'][0], rtol=1e-12, atol=0)
    np.testing.assert_allclose(res['lists'][1], res['batch_by_batch'][1], rtol=1e-12, atol=1e-300)


_FH, _FW, _LG = 'fused_update_H', 'fused_update_W', 'local_gradient_W'
_AR, _AW = ('all_reduce_gradient_W',), ('apply_W',)
_H, _GW, _N = 'reconstruction_gradient_H', 'reconstruction_gradient_W', ('normalize',)
# one epoch at batch_size=2, seed 42: N = 4 draws the order (0, 1) of its two batches, N = 6 the order (1, 0, 2) of its three
_STEP_BY_STEP_CALLS = {
    (4, True): {
        'Cyclic_MU': [(_FH, 0, 2), (_LG, 0, 2), (_FH, 2, 4), (_LG, 2, 4), _AR, _AW],
        'ASG_MU': [(_FH, 0, 2), (_FW, 0, 2), (_FH, 2, 4), (_FW, 2, 4)],
        'GSG_MU': [(_FH, 0, 4), (_FW, 2, 4)],
        'ASAG_MU': [(_FH, 0, 2), (_GW, 0, 2), _N, (_FH, 2, 4), (_GW, 2, 4), _N],
        'GSAG_MU': [(_FH, 0, 4), (_GW, 2, 4), _N],
    },
    (4, False): {
        'Cyclic_MU': [(_H, 0, 2), (_GW, 0, 2), (_H, 2, 4), (_GW, 2, 4), _N],
        'ASG_MU': [(_H, 0, 2), (_GW, 0, 2), _N, (_H, 2, 4), (_GW, 2, 4), _N],
        'GSG_MU': [(_H, 0, 4), (_GW, 2, 4), _N],
        'ASAG_MU': [(_H, 0, 2), (_GW, 0, 2), _N, (_H, 2, 4), (_GW, 2, 4), _N],
        'GSAG_MU': [(_H, 0, 4), (_GW, 2, 4), _N],
    },
    (6, True): {
        'Cyclic_MU': [(_FH, 0, 2), (_LG, 0, 2), (_FH, 2, 4), (_LG, 2, 4), (_FH, 4, 6), (_LG, 4, 6), _AR, _AW],
        'ASG_MU': [(_FH, 2, 4), (_FW, 2, 4), (_FH, 0, 2), (_FW, 0, 2), (_FH, 4, 6), (_FW, 4, 6)],
        'GSG_MU': [(_FH, 0, 6), (_FW, 4, 6)],
        'ASAG_MU': [(_FH, 2, 4), (_GW, 2, 4), _N, (_FH, 0, 2), (_GW, 0, 2), _N, (_FH, 4, 6), (_GW, 4, 6), _N],
        'GSAG_MU': [(_FH, 0, 6), (_GW, 4, 6), _N],
    },
    (6, False): {
        'Cyclic_MU': [(_H, 0, 2), (_GW, 0, 2), (_H, 2, 4), (_GW, 2, 4), (_H, 4, 6), (_GW, 4, 6), _N],
        'ASG_MU': [(_H, 2, 4), (_GW, 2, 4), _N, (_H, 0, 2), (_GW, 0, 2), _N, (_H, 4, 6), (_GW, 4, 6), _N],
        'GSG_MU': [(_H, 0, 6), (_GW, 4, 6), _N],
        'ASAG_MU': [(_H, 2, 4), (_GW, 2, 4), _N, (_H, 0, 2), (_GW, 0, 2), _N, (_H, 4, 6), (_GW, 4, 6), _N],
        'GSAG_MU': [(_H, 0, 6), (_GW, 4, 6), _N],
    },
}


@pytest.mark.parametrize('hooks', [True, False])
@pytest.mark.parametrize('n_samples', [4, 6])
@pytest.mark.parametrize('algorithm', list(MiniBatchAlgorithm))
def test_step_by_step_epochs_issue_the_recorded_backend_calls(algorithm, n_samples, hooks):
    """An epoch that does not go out as one operation list (here: a backend without `run_schedule`) is walked step by step:
    the backend must see exactly the calls, on exactly the slices, recorded before the epochs were stated as lists only --
    the launch structure that a batch-by-batch run has on the GPU.  Three batches drawn out of order show the H steps of
    GSG / GSAG joined into one call."""
    be, log = OracleBackend(hooks=hooks), []
    for name in (_FH, _FW, _LG, _AR[0], _AW[0], _H, _GW, _N[0]):
        fn = getattr(be, name, None)
        if fn is None:
            continue

        def logged(*args, _fn=fn, _name=name, **kw):
            s = [(a.start, a.stop) for a in args if isinstance(a, slice)]
            log.append((_name,) + (s[0] if s else ()))
            return _fn(*args, **kw)
        setattr(be, name, logged)
    V = np.random.default_rng(3).random((n_samples, 2, 12, 14))
    np.random.seed(42)
    nmf = TransformInvariantNMF(n_atoms=3, atom_shape=(3, 4), backend=be)
    nmf.fit(V, algorithm=algorithm, batch_size=2, n_epochs=1, sag_lambda=0.8)
    assert log == _STEP_BY_STEP_CALLS[n_samples, hooks][algorithm.name]


def test_tiny_full_batch_iterations_go_out_as_operation_lists():
    """fit_batch of a problem the backend calls tiny: one ('H', all), ('G', all, 0, 1), ('W',) list per iteration."""
    np.random.seed(42)
    be = OracleBackend(hooks=True, schedules=True)
    nmf = TransformInvariantNMF(n_atoms=3, atom_shape=(5,), backend=be)
    nmf.fit(V_1D, n_iterations=4, sparsity_H=0.1)
    assert be.schedule_calls == [['H', 'G', 'W']] * 4
    np.random.seed(42)
    ref = _nmf(n_atoms=3, atom_shape=(5,))
    ref.fit(V_1D, n_iterations=4, sparsity_H=0.1)
    np.testing.assert_allclose(nmf.W, ref.W, rtol=1e-12)
    np.testing.assert_allclose(nmf.H, ref.H, rtol=1e-12)


def test_commuting_h_steps_are_joined_in_the_step_by_step_schedules():
    """GSG / GSAG driven step by step (several ranks, or no schedule support): the H steps of an epoch are issued per
    contiguous run of samples, not per batch -- and only when the batches are plain disjoint slices."""
    from tnmf_amd.TransformInvariantNMF import _joined
    assert _joined([slice(6, 9), slice(0, 3), slice(3, 6)]) == [slice(0, 9)]
    assert _joined([slice(6, 9), slice(0, 3), slice(4, 4)]) == [slice(0, 3), slice(6, 9)]            # a gap, an empty batch
    lap = [slice(0, 4), slice(3, 6)]
    assert _joined(lap) == lap                                                                       # overlapping: as given
    assert _joined([slice(None)]) == [slice(None)]                                                   # batch_size=None
    strided = [slice(0, 6, 2), slice(6, 9)]
    assert _joined(strided) == strided
    # the schedule as a whole still reproduces the reference's known answer (tests/test_minibatch.py:18-25)
    np.random.seed(42)
    nmf = TransformInvariantNMF(n_atoms=10, atom_shape=(7, 7), backend=OracleBackend(hooks=False), use_fused_updates=False)
    nmf.fit_minibatches(racoon_patches_V(), sparsity_H=0.1, algorithm=MiniBatchAlgorithm.GSG_MU, batch_size=3, n_epochs=5,
                        sag_lambda=0.8)
    assert np.isclose(nmf._energy_function(), 14223.14454)

"""
Stopping on the objective (``objective_every`` / ``tol``), checked on the CPU through the TEST-ONLY oracle backend: the
recorded values are those of ``_energy_function()`` before the recording iterations, the fit stops at the iteration
scikit-learn's criterion names, and the front end takes the backend's objective tap where there is one and the generic
route (an energy evaluation before the iteration) where there is not.
"""
import warnings

import numpy as np
import pytest

from convergence_reference import pick_tol, predict, trajectory
from oracle_backend import OracleBackend
from tnmf_amd.TransformInvariantNMF import MiniBatchAlgorithm, TransformInvariantNMF


def _V(seed=3, shape=(5, 2, 12, 14)):
    return np.random.default_rng(seed).random(shape)


def make_plain(hooks):
    return lambda: TransformInvariantNMF(n_atoms=3, atom_shape=(3, 4), backend=OracleBackend(hooks=hooks))


@pytest.mark.parametrize('hooks', [False, True])
def test_fit_stops_where_the_criterion_says(hooks):
    V, n, every = _V(), 60, 5
    E = trajectory(make_plain(hooks), V, n, sparsity_H=0.05)
    tol = pick_tol(E, every, 5)
    n_iter, converged, records = predict(E, every, tol, n)
    assert converged and n_iter == 5 * every + 1, (n_iter, tol)
    np.random.seed(42)
    nmf = make_plain(hooks)()
    seen = []
    nmf.fit(V, n_iterations=n, sparsity_H=0.05, objective_every=every, tol=tol,
            progress_callback=lambda m, i: seen.append(i) or True)
    assert nmf.n_iter_ == n_iter and nmf.converged_ is True
    assert seen == list(range(n_iter)), 'the callback runs every iteration, the last one included'
    hist = nmf.objective_history_
    assert hist.shape == (len(records), 2)
    np.testing.assert_array_equal(hist[:, 0], [r[0] for r in records])
    np.testing.assert_allclose(hist[:, 1], [r[1] for r in records], rtol=1e-12, atol=0)
    # the iteration that met the criterion was completed in full: the state is the twin's after n_iter iterations
    assert np.isclose(nmf.objective(), E[n_iter], rtol=1e-12, atol=0)
    assert nmf.objective() == nmf._energy_function()


def test_tol_alone_records_every_ten_iterations():
    V, n = _V(), 45
    E = trajectory(make_plain(True), V, n)
    tol = pick_tol(E, 10, 3)
    n_iter, converged, records = predict(E, 10, tol, n)
    assert converged and n_iter == 31
    np.random.seed(42)
    nmf = make_plain(True)()
    nmf.fit(V, n_iterations=n, tol=tol)
    assert (nmf.n_iter_, nmf.converged_) == (31, True)
    np.testing.assert_array_equal(nmf.objective_history_[:, 0], [0, 10, 20, 30])
    np.testing.assert_allclose(nmf.objective_history_[:, 1], [r[1] for r in records], rtol=1e-12, atol=0)


def test_not_converged_when_the_count_runs_out():
    V, n, every = _V(), 12, 4
    E = trajectory(make_plain(False), V, n)
    n_iter, converged, records = predict(E, every, 0.0, n)   # (an MU trajectory decreases strictly: tol = 0 is never met)
    assert not converged and n_iter == n
    np.random.seed(42)
    nmf = make_plain(False)()
    nmf.fit(V, n_iterations=n, objective_every=every, tol=0.0)
    assert nmf.n_iter_ == n and nmf.converged_ is False
    np.testing.assert_array_equal(nmf.objective_history_[:, 0], [0, 4, 8])
    np.testing.assert_allclose(nmf.objective_history_[:, 1], [r[1] for r in records], rtol=1e-12, atol=0)


def test_objective_every_without_tol_only_records():
    V = _V()
    E = trajectory(make_plain(True), V, 7)
    np.random.seed(42)
    nmf = make_plain(True)()
    nmf.fit(V, n_iterations=7, objective_every=3)
    assert nmf.n_iter_ == 7 and nmf.converged_ is False
    np.testing.assert_array_equal(nmf.objective_history_[:, 0], [0, 3, 6])
    np.testing.assert_allclose(nmf.objective_history_[:, 1], E[[0, 3, 6]], rtol=1e-12, atol=0)


def test_callback_stop_still_works():
    np.random.seed(42)
    nmf = make_plain(True)()
    nmf.fit(_V(), n_iterations=50, objective_every=2, tol=0.0, progress_callback=lambda m, i: i < 4)
    assert nmf.n_iter_ == 5 and nmf.converged_ is False
    np.testing.assert_array_equal(nmf.objective_history_[:, 0], [0, 2, 4])


@pytest.mark.parametrize('kw', [dict(tol=-1e-3), dict(tol=float('nan')), dict(tol=float('inf')), dict(tol='1e-3'),
                                dict(tol=True), dict(objective_every=0), dict(objective_every=-2),
                                dict(objective_every=2.0), dict(objective_every=True), dict(tol=1e-3, objective_every=0)])
@pytest.mark.parametrize('minibatch', [False, True])
def test_bad_keywords_raise_before_anything_is_initialised(kw, minibatch):
    nmf = make_plain(True)()
    with pytest.raises(ValueError):
        if minibatch:
            nmf.fit(_V(), n_epochs=3, batch_size=2, **kw)
        else:
            nmf.fit(_V(), n_iterations=3, **kw)
    assert nmf._W is None and nmf._H is None


def test_without_the_keywords_nothing_is_recorded():
    np.random.seed(42)
    be = OracleBackend(hooks=True)
    calls = []
    energy = be.reconstruction_energy
    be.reconstruction_energy = lambda *a, **k: calls.append(1) or energy(*a, **k)
    nmf = TransformInvariantNMF(n_atoms=3, atom_shape=(3, 4), backend=be)
    nmf.fit(_V(), n_iterations=6)
    assert nmf.objective_history_.shape == (0, 2) and nmf.n_iter_ == 6 and nmf.converged_ is False
    assert not calls, 'a fit without the keywords evaluates no objective'
    nmf.fit(_V(), n_epochs=2, batch_size=2)
    assert nmf.objective_history_.shape == (0, 2) and nmf.n_iter_ == 2 and nmf.converged_ is False
    assert not calls


@pytest.mark.parametrize('algorithm', list(MiniBatchAlgorithm))
@pytest.mark.parametrize('schedules', [False, True])
def test_minibatch_algorithms_stop_per_epoch(algorithm, schedules):
    V, n, every = _V(shape=(7, 2, 12, 14)), 24, 2

    def make():
        return TransformInvariantNMF(n_atoms=3, atom_shape=(3, 4), backend=OracleBackend(hooks=True, schedules=schedules))
    kw = dict(algorithm=algorithm, batch_size=2, sag_lambda=0.8, sparsity_H=0.05)
    E = trajectory(make, V, n, **kw)
    # (the stochastic schedules do not decrease monotonically: any tolerance the margin rule accepts will do)
    d = [E[(j - 1) * every] - E[j * every] for j in range(1, 6)]
    tol = 0.5 * (sorted(d)[1] + sorted(d)[2]) / E[0]
    n_iter, converged, records = predict(E, every, tol, n)
    assert converged and n_iter < n
    np.random.seed(42)
    nmf = make()
    nmf.fit(V, n_epochs=n, objective_every=every, tol=tol, **kw)
    assert (nmf.n_iter_, nmf.converged_) == (n_iter, True)
    np.testing.assert_array_equal(nmf.objective_history_[:, 0], [r[0] for r in records])
    np.testing.assert_allclose(nmf.objective_history_[:, 1], [r[1] for r in records], rtol=1e-12, atol=0)
    if schedules:
        assert len(nmf._backend.schedule_calls) == n_iter, 'the one-call epochs stay as they are'


def test_fit_stream_forwards_the_keywords():
    V = _V(shape=(6, 2, 12, 14))
    seen = []
    np.random.seed(42)
    twin = make_plain(True)()
    twin.fit(iter(V), subsample_size=3, n_iterations=5,
             progress_callback=lambda m, i: seen.append((i, m._energy_function())) or True)
    np.random.seed(42)
    nmf = make_plain(True)()
    nmf.fit(iter(V), subsample_size=3, n_iterations=5, objective_every=1)
    # every subsample fit stands alone: the read-outs are those of the last one
    assert nmf.n_iter_ == 5 and nmf.objective_history_.shape == (5, 2)
    last = [e for _, e in seen[5:]]
    np.testing.assert_allclose(nmf.objective_history_[1:, 1], last[:4], rtol=1e-12, atol=0)
    with pytest.raises(ValueError):
        nmf.fit(iter(V), subsample_size=3, n_iterations=5, tol=-1.0)


def test_non_finite_objective_ends_the_fit_with_a_warning():
    np.random.seed(42)
    be = OracleBackend(hooks=False)
    energy, calls = be.reconstruction_energy, []
    be.reconstruction_energy = lambda *a, **k: calls.append(1) or (float('nan') if len(calls) == 3 else energy(*a, **k))
    nmf = TransformInvariantNMF(n_atoms=3, atom_shape=(3, 4), backend=be)
    seen = []
    with pytest.warns(RuntimeWarning):
        nmf.fit(_V(), n_iterations=20, objective_every=2, tol=0.0, progress_callback=lambda m, i: seen.append(i) or True)
    assert nmf.n_iter_ == 5 and nmf.converged_ is False and seen == [0, 1, 2, 3, 4]
    assert nmf.objective_history_.shape == (3, 2) and np.isnan(nmf.objective_history_[2, 1])


# -- the tap route and the generic route ----------------------------------------------------------------------------
class TapBackend(OracleBackend):
    """The oracle backend with the objective tap of the hip backend: fused_update_H(..., objective_out=buf) leaves each
    sample's 1/2 ||V - R||^2 at the (W, H) passed in; read_objective sums the buffer."""
    supports_objective_tap = True

    def __init__(self, **kw):
        super().__init__(hooks=True, **kw)
        self.tapped, self.untapped, self.energies = 0, 0, 0
        plain = self.fused_update_H

        def fused_update_H(V, W, H, s=slice(None), objective_out=None, **kwargs):
            if objective_out is None:
                self.untapped += 1
            else:
                self.tapped += 1
                R = self.reconstruct(W, H[s])
                objective_out[s] = 0.5 * ((self._V_local[s] - R) ** 2).reshape(R.shape[0], -1).sum(axis=1)
            plain(V, W, H, s, **kwargs)
        self.fused_update_H = fused_update_H

    def new_objective_buffer(self):
        return np.full(self._shard[1] - self._shard[0], np.nan)

    def read_objective(self, buf):
        return float(sum(buf.tolist()))

    def reconstruction_energy(self, V, W, H):
        self.energies += 1
        return super().reconstruction_energy(V, W, H)


def test_full_batch_takes_the_tap_and_passes_the_keyword_only_when_it_records():
    V, n, every = _V(), 40, 4
    E = trajectory(make_plain(True), V, n, sparsity_H=0.05)
    tol = pick_tol(E, every, 4)
    n_iter, converged, records = predict(E, every, tol, n)
    assert converged
    np.random.seed(42)
    be = TapBackend()
    nmf = TransformInvariantNMF(n_atoms=3, atom_shape=(3, 4), backend=be)
    nmf.fit(V, n_iterations=n, sparsity_H=0.05, objective_every=every, tol=tol)
    assert (nmf.n_iter_, nmf.converged_) == (n_iter, True)
    assert be.tapped == len(records) and be.untapped == n_iter - len(records)
    assert be.energies == 0, 'the tap replaces the energy evaluation'
    np.testing.assert_allclose(nmf.objective_history_[:, 1], [r[1] for r in records], rtol=1e-12, atol=0)


def test_generic_route_without_the_hook_without_an_h_step_and_on_the_one_call_path():
    V, n = _V(), 6
    # a backend without the tap: one energy evaluation per record
    np.random.seed(42)
    be = OracleBackend(hooks=True)
    calls = []
    energy = be.reconstruction_energy
    be.reconstruction_energy = lambda *a, **k: calls.append(1) or energy(*a, **k)
    nmf = TransformInvariantNMF(n_atoms=3, atom_shape=(3, 4), backend=be)
    nmf.fit(V, n_iterations=n, objective_every=2)
    assert len(calls) == 3 and nmf.objective_history_.shape == (3, 2)
    # update_H=False: no H half step to tap
    E = trajectory(lambda: TransformInvariantNMF(n_atoms=3, atom_shape=(3, 4), backend=TapBackend()), V, n, update_H=False)
    np.random.seed(42)
    be = TapBackend()
    nmf = TransformInvariantNMF(n_atoms=3, atom_shape=(3, 4), backend=be)
    nmf.fit(V, n_iterations=n, objective_every=2, update_H=False)
    assert be.tapped == 0 and be.energies == 3
    np.testing.assert_allclose(nmf.objective_history_[:, 1], E[[0, 2, 4]], rtol=1e-12, atol=0)
    # the one-call iteration of a tiny problem keeps its operation list; the objective is evaluated beside it
    E = trajectory(make_plain(True), V, n)
    np.random.seed(42)
    be = TapBackend(schedules=True)
    nmf = TransformInvariantNMF(n_atoms=3, atom_shape=(3, 4), backend=be)
    nmf.fit(V, n_iterations=n, objective_every=2)
    assert be.schedule_calls == [['H', 'G', 'W']] * n and be.tapped == 0 and be.energies == 3
    np.testing.assert_allclose(nmf.objective_history_[:, 1], E[[0, 2, 4]], rtol=1e-12, atol=0)


def test_sample_objective_needs_the_backend_hook():
    np.random.seed(42)
    nmf = make_plain(True)()
    nmf.fit(_V(), n_iterations=2)
    with pytest.raises(NotImplementedError):
        nmf.sample_objective()
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        assert nmf.objective() == nmf._energy_function()

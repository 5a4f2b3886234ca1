"""Shared by tests/test_convergence_cpu.py and tests/test_hip_objective.py: the float64 trajectory of the objective of a
fit (through the product front end on any backend), and from it the iteration at which a fit with ``tol`` has to stop --
with the margin rule that keeps a badly chosen tolerance from flaking: every comparison the prediction makes must be
decided by more than MARGIN * E_0."""
import numpy as np

MARGIN = 1e-6   # every comparison the prediction makes must be decided by more than MARGIN * E_0


def trajectory(make, V, n, seed=42, **fit_kw):
    """E[i], i = 0..n: ``_energy_function()`` of the state that enters iteration (epoch) i of a fit without the keywords --
    E[0] from a twin fit of zero iterations, the others from a twin's callback after iteration i - 1."""
    count = 'n_epochs' if 'algorithm' in fit_kw else 'n_iterations'
    np.random.seed(seed)
    twin = make()
    twin.fit(V, **{count: 0}, **fit_kw)
    E = [twin._energy_function()]
    np.random.seed(seed)
    twin = make()
    twin.fit(V, **{count: n}, progress_callback=lambda m, i: E.append(m._energy_function()) or True, **fit_kw)
    assert len(E) == n + 1
    return np.asarray(E)


def pick_tol(E, every, j_star):
    """A tolerance that the j_star-th record should be the first to meet: halfway (in the decrease) between that record's
    decrease and the smallest earlier one."""
    d = [E[(j - 1) * every] - E[j * every] for j in range(1, j_star + 1)]
    return 0.5 * (d[-1] + min(d[:-1])) / E[0]


def predict(E, every, tol, n):
    """-> (n_iter, converged, records) of a fit of at most n iterations, from the trajectory; asserts the margin rule at
    every comparison made."""
    records = [(i, E[i]) for i in range(0, n, every)]
    for j in range(1, len(records)):
        gap = records[j - 1][1] - records[j][1] - tol * E[0]
        assert abs(gap) > MARGIN * E[0], f'record {j}: decided by {gap / E[0]:.2e} of E_0 only -- pick another tol or seed'
        if gap <= 0:
            return records[j][0] + 1, True, records[:j + 1]
    return n, False, records

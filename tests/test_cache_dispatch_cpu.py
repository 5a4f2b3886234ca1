"""The host model of the spectrum cache (tests/cache_dispatch.py) against itself: its sequences carry every transition, every
wrong model is told apart from the right one, and wherever the model says a spectrum must be computed again because its
operand was written, the answer from the stale spectrum is far from the right one -- so tests/test_hip_cache_matrix.py, which
holds the library to the oracle, cannot miss a stale hit.  No GPU, no torch."""
import numpy as np
import pytest

import beta_reference as bref
import cache_dispatch as cd
import cache_reference as cref
import fft_dispatch as fd
from oracle import tnmf_oracle as orc

FAR = 1e-2      # a stale spectrum moves the step's output by at least this much (relative, max norm)


def test_geometry_classes_land_where_intended():
    assert cd.check_classes()
    assert not fd.use_fft_under_auto(cd.geometry(cd.geo('mixed', 'f', cref.LARGE - 1)), 'f')
    assert fd.use_fft_under_auto(cd.geometry(cd.geo('mixed', 'f', cref.LARGE)), 'f')


def test_every_transition_is_carried_in_every_dtype_it_occurs_in():
    assert cd.missing() == []
    for name, seq in cd.SEQUENCES.items():
        assert set(seq.carries) <= set(cd.TRANSITIONS), name
        assert len(seq.ops) <= 16, name
        assert seq.path in ('fft', 'hybrid') or seq.base == 'auto_crossover', name
    assert not set(cd.NOT_REACHED) & set(cd.TRANSITIONS)
    sole = cd.sole_carriers()
    print(sole)
    # removing a sole carrier leaves exactly its transitions uncarried
    for base, cells in sole.items():
        rest = {n: s for n, s in cd.SEQUENCES.items() if s.base != base}
        assert {t for t, _ in cd.missing(rest)} == set(cells), base


def test_the_model_says_what_the_sequences_claim():
    """A few of the claims of the `carries` texts, read off the model's counters (h_runs, h_hits, v_runs, v_hits)."""
    def counters(name):
        return [s.counters for s in cd.run(cd.SEQUENCES[name])]

    c = counters('explicit_slices[f-mixed-hybrid]')
    assert c[4] == (3, 0, 0, 0) and c[7] == (3, 3, 0, 0)                    # three slices run once, then hit
    steps = cd.run(cd.SEQUENCES['explicit_slices[f-mixed-hybrid]'])
    assert [cd.W_SPEC in s.recomputed for s in steps[2:8]] == [True] + [False] * 5
    assert all(cd.H_COLS not in s.recomputed for s in steps)
    steps = cd.run(cd.SEQUENCES['explicit_slices[d-resident-hybrid]'])
    assert [cd.H_COLS in s.recomputed for s in steps[2:8]] == [True] * 3 + [False] * 3
    c = counters('one_sample_invalid[f-mixed-hybrid]')
    assert c[6][0] == c[5][0] + 1 and c[7][1] == c[6][1] + 1                # one stale sample: the call runs, then hits
    c = counters('fft_update_then_hits[f-mixed-fft]')
    assert c[2][0] == 1 and c[-1][0] == 1                                   # after the first reconstruct nothing runs again
    c = counters('auto_crossover[f-mixed-auto]')
    assert c[1:] == [(1, 0, 0, 0), (1, 0, 0, 0), (1, 1, 0, 0), (1, 1, 0, 0), (2, 1, 0, 0)]
    for name in ('layout_explicit', 'layout_implicit'):
        for v in ('f-mixed-hybrid', 'd-resident-fft', 'f-resident-hybrid'):
            s = cd.run(cd.SEQUENCES[f'{name}[{v}]'])
            assert cd.W_SPEC in s[3].recomputed and cd.W_SPEC in s[4 if name == 'layout_explicit' else 3].recomputed
    # exact equality with a fresh context is claimed until a call consumes the rows k_fft_rows_mu left
    assert all(s.exact for n, q in cd.SEQUENCES.items() if q.path != 'fft' for s in cd.run(q))
    s = cd.run(cd.SEQUENCES['fft_update_then_hits[f-mixed-fft]'])
    assert [x.exact for x in s] == [True, True, True, False, False, False, False]


@pytest.mark.parametrize('defect', sorted(cd.WRONG_MODELS))
def test_every_wrong_model_is_told_apart_by_its_sequence(defect):
    base = cd.WRONG_MODELS[defect]
    variants = [n for n, s in cd.SEQUENCES.items() if s.base == base]
    assert variants and any(cd.disagreements(cd.SEQUENCES[n], defect) for n in variants), (defect, base)


def test_wrong_models_cover_every_group_of_transitions():
    groups = {'locate and bind': ('overrun_is_located', 'adopt_V_as_base', 'foreign_keeps_flags'),
              'H flags': ('sh_survives_t', 'direct_update_keeps_H', 'fft_update_leaves_nothing', 'lateral_keeps_H',
                          'modes_keep_flags', 'mu_update_keeps_flags'),
              'V flags': ('v_survives_volatile',),
              'W': ('w_hit_across_layout', 'W_survives_normalize_W', 'W_survives_apply_W', 'W_survives_run_schedule',
                    'W_survives_group_expand_W', 'W_survives_group_apply_W', 'W_survives_ops_expand_W', 'W_survives_ops_apply_W',
                    'persistent_schedule_keeps_flags', 'set_path_keeps_flags'),
              'workspace': ('growth_keeps_flags', 'reserve_ignores_binding')}
    assert sorted(d for g in groups.values() for d in g) == sorted(cd.WRONG_MODELS)


def test_layout_offsets_of_the_W_spectra_follow_the_resident_sample_count():
    """Otherwise the two layout sequences would prove nothing: a hit at the other layout's offset would read the right bytes."""
    for cls, dtype in (('mixed', 'f'), ('resident', 'd'), ('resident', 'f')):
        for path in ('fft', 'hybrid'):
            small = fd.make_layout(cd.geometry(cd.geo(cls, dtype, 2)), dtype, path)
            large = fd.make_layout(cd.geometry(cd.geo(cls, dtype, cd.NB)), dtype, path, n_call=2)
            assert small.SW != large.SW and small.TWr != large.TWr, (cls, dtype, path)
            # ... and the bytes the small layout keeps them in hold per-sample arrays of the large one
            assert small.TWr < large.SW and small.SW < large.SW


def test_window_buffers_cross_an_allocation_step_in_the_float64_class_only():
    lay = fd.make_layout(cd.geometry(cd.geo('resident', 'd', cd.NB)), 'd', 'fft', n_call=2)
    assert fd.align_up(lay.total_no_window, 1 << 20) < fd.align_up(lay.total, 1 << 20)
    lay = fd.make_layout(cd.geometry(cd.geo('mixed', 'f', cd.NB)), 'f', 'fft', n_call=2)
    assert fd.align_up(lay.total_no_window, 1 << 20) == fd.align_up(lay.total, 1 << 20)


def test_host_steps_equal_the_oracle_and_the_beta_reference():
    seq = cd.SEQUENCES['explicit_slices[d-resident-fft]']
    host = cref.Host(seq)
    g = cd.geo(seq.cls, seq.dtype, cd.NB)
    H = cref.view(host.buf['H'], 0, (8, g.M) + cd.shift(g)).copy()
    V = cref.view(host.buf['V'], 0, (8, g.C) + g.D).copy()
    W = cref.view(host.buf['W'], 0, (g.M, g.C) + g.A).copy()
    s = slice(2, 4)
    neg, pos = orc.gradient_W(V, W, H, s)
    got = host.evaluate(cd.gw_(2))['NP']
    assert cref.relmax(got[0], neg) < 1e-13 and cref.relmax(got[1], pos) < 1e-13
    neg, pos = bref.gradient_W(V, W, H, s, beta=cref.BETA, eps=cref.EPS)
    got = host.evaluate(cd.gw_(2, beta=1))['NP']
    assert cref.relmax(got[0], neg) < 1e-13 and cref.relmax(got[1], pos) < 1e-13
    neg, pos = orc.gradient_H(V, W, H, s)
    got = host.evaluate(cd.gh_(2))
    assert cref.relmax(got['neg'], neg) < 1e-13 and cref.relmax(got['pos'], pos) < 1e-13
    for kw in (dict(), dict(beta=1), dict(lateral=1)):
        want = H.copy()
        bref.update_H(V, W, want, s, beta=cref.BETA if kw.get('beta') else 2., eps=cref.EPS,
                      inhibition=cref.INHIBITION if kw.get('lateral') else 0., cross_inhibition=cref.CROSS if kw.get('lateral') else 0.,
                      kernels=cref.kernels())
        got = host.evaluate(cd.uh_(2, **kw), commit=False)['H']
        assert cref.relmax(got, want[s]) < 1e-13, kw
    Hc = cref.view(host.buf['HC'], 0, (2, g.M) + g.D).copy()
    want = Hc.copy()
    bref.update_H(V[2:4], W, want, slice(None), beta=2., eps=cref.EPS, mode='circular')
    got = host.evaluate(cd.op('update_H', N=2, H=('HC', 0), V=('V', 2), W='W', mode='circular'), commit=False)['H']
    assert cref.relmax(got, want) < 1e-13


@pytest.mark.parametrize('name', sorted(n for n, s in cd.SEQUENCES.items() if s.base != 'auto_crossover'))
def test_a_stale_spectrum_is_far_from_the_right_answer(name):
    """A condition on the inputs of the sequences, not a measurement: wherever the model computes a spectrum again whose
    operand has changed since it was last transformed, the step evaluated in float64 with the OLD operand differs from the
    right output by at least FAR.  (The two layout sequences are not covered here: their stale operand is whatever the
    other layout keeps in those bytes, which only the GPU test sees.)"""
    seq = cd.SEQUENCES[name]
    host = cref.Host(seq)
    seen = 0
    for i, (step, m) in enumerate(zip(seq.ops, cd.run(seq))):
        out, gaps = host.step(step, m)
        for what, gap in gaps.items():
            print(f'{name} step {i} {step[0]}: stale {what}: {gap:.3e}')
            assert gap >= FAR, (name, i, step[0], what, gap)
            seen += 1
        for k, v in out.items():
            assert np.all(np.isfinite(v)), (name, i, k)
    if seq.base in ('W_writers', 'W_foreign_write', 'W_schedule', 'other_V', 'lateral') or (
            seq.base == 'one_sample_invalid' and seq.path == 'hybrid'):
        assert seen > 0, name     # (these sequences write an operand between two calls that transform it)

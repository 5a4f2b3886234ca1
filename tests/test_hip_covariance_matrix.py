"""
The inverse-diagonal kernels, every path of them: k_inverse_diag_rows, k_inverse_diag_lds and k_inverse_diag_tile
(tnmf_amd/csrc/covariance.hip) through the C entry tnmf_hip_events_inverse_diag and through the backend's
``inverse_diag_event_list`` on the lists of covariance_dispatch.MATRIX, which are chosen with the host mirror
tests/covariance_dispatch.py so that together they execute every named branch (tests/test_covariance_dispatch_cpu.py checks
that without a GPU).  The lists are synthetic Gram matrices handed over as CSR triples; the components come from
``event_components`` on the device and must be those of the breadth-first search of tests/errors_reference.py.

The cases of the matrix are EXACT: every component is L L' with dyadic L and a dyadic inverse, every partial sum an integer
(times a power of two) below 2^53, so d equals the integer reference BIT FOR BIT, whatever the order of the sums and with or
without FMA; a singular component gives +inf on its rows and status 1 and leaves the others their bits.  The rows that are not
active, and the entries into them, hold 1e30: one use of them destroys the bits.  The test owns every buffer: d and status are
prefilled with sentinels and have slack behind them, the scratch is prefilled with NaN and has a tail beyond scratch_doubles;
slack and tail must stay as they were.

The component-graph cases and the dense random ones are not exact; they are held to the bar of errors_reference.inverse_diag
with taps = 0, kappa * 4 n^2 * 2^-52, with kappa <= 1e4 checked on the host.
"""
import ctypes
import time

import numpy as np
import pytest
import torch

import covariance_dispatch as cd
from test_events_errors_cpu import check_d
from test_hip_events import p
from test_hip_events_matrix import backend
from tnmf_amd import _lib

pytestmark = pytest.mark.gpu

SLACK = 5                       # elements behind d and status, and doubles behind the scratch
SENTINEL, TAIL = -7., 12345.5


def context():
    """Any initialised backend: the entry takes its lists per call."""
    return backend(1, 1, 1, (8, 8), (2, 2), 'valid', 'f64')


def on_device(c):
    """(csr, active) of a case of the mirror as device tensors (copies: the cases are read-only)."""
    csr = tuple(torch.from_numpy(np.array(a)).cuda() for a in c['csr'])
    return csr, torch.from_numpy(np.array(c['active'])).cuda()


def components_of(be, c, csr, active):
    """event_components on the device, held to the lists of the breadth-first search."""
    comps = be.event_components(csr, active)
    assert np.array_equal(comps['sizes'], c['sizes']) and comps['sizes'].dtype == np.int32
    for key in ('comp_start', 'member', 'local'):
        assert np.array_equal(comps[key].cpu().numpy(), c[key]), key
    assert comps['rounds'] <= 4 * int(np.ceil(np.log2(c['K'])))
    return comps


def entry(be, c, csr, comps, scratch_doubles=None):
    """One call of tnmf_hip_events_inverse_diag into buffers of the test's own -> (d [K], status [n_comp]), with the slack
    behind both and the tail of the scratch checked."""
    K, sizes = c['K'], comps['sizes']
    if scratch_doubles is None:
        scratch_doubles = cd.default_scratch(sizes)
    d = torch.full((K + SLACK,), SENTINEL, dtype=torch.float64, device='cuda')
    status = torch.full((len(sizes) + SLACK,), int(SENTINEL), dtype=torch.int32, device='cuda')
    scratch = torch.full((scratch_doubles + SLACK,), float('nan'), dtype=torch.float64, device='cuda')
    scratch[scratch_doubles:] = TAIL
    code = be._lib.tnmf_hip_events_inverse_diag(
        be._ctx, K, csr[2].numel(), p(csr[0]), p(csr[1]), p(csr[2]), len(sizes), p(comps['comp_start']),
        sizes.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), comps['member'].numel(), p(comps['member']), p(comps['local']),
        p(scratch), scratch_doubles, p(d), p(status), be._stream())
    torch.cuda.synchronize()
    assert code == 0, code
    d, status = d.cpu().numpy(), status.cpu().numpy()
    assert np.all(d[K:] == SENTINEL) and np.all(status[len(sizes):] == int(SENTINEL)), 'nothing is written behind d and status'
    assert np.all(scratch[scratch_doubles:].cpu().numpy() == TAIL), 'nothing is written beyond scratch_doubles'
    assert not np.any(d[:K] == SENTINEL) and not np.any(status[:len(sizes)] == int(SENTINEL)), 'every element is written'
    return d[:K], status[:len(sizes)]


def check_exact(c, d, status, what):
    wrong = np.flatnonzero(~((d == c['d']) | (np.isnan(d) & np.isnan(c['d']))))
    hit = sorted(n for n, rows in c['rows_of'].items() if np.intersect1d(rows, wrong).size)
    assert d.tobytes() == c['d'].tobytes(), (what, len(wrong), hit, d[wrong[:4]].tolist(), c['d'][wrong[:4]].tolist())
    assert np.array_equal(status, c['status']), (what, status.tolist(), c['status'].tolist())


@pytest.mark.parametrize('name', list(cd.MATRIX))
def test_the_case_is_the_integer_reference_bit_for_bit(name):
    """Through the C entry and through the backend, twice each: the whole matrix as one list ('all') and every class on its
    own."""
    c, be = cd.case(name), context()
    csr, active = on_device(c)
    comps = components_of(be, c, csr, active)
    print(f'{name}: K {c["K"]}, {len(c["sizes"])} components, {len(c["csr"][1])} entries, {comps["rounds"]} rounds')
    t = time.perf_counter()
    d, status = entry(be, c, csr, comps)
    took = time.perf_counter() - t
    check_exact(c, d, status, f'{name}, entry')
    again, status2 = entry(be, c, csr, comps)
    assert again.tobytes() == d.tobytes() and np.array_equal(status2, status), 'the same bits again'
    for _ in range(2):
        out = torch.full((c['K'],), SENTINEL, dtype=torch.float64, device='cuda')
        got, info = be.inverse_diag_event_list(csr, active, out=out)
        assert got is out
        check_exact(c, got.cpu().numpy(), info['status'], f'{name}, backend')
        assert (info['n_active'], info['n_components'], info['largest_component'], info['n_singular']) == \
            (int(c['active'].sum()), len(c['sizes']), int(c['sizes'][-1]), int(c['status'].sum()))
    print(f'{name}: one call of the entry with its buffers {took * 1e3:.1f} ms')


@pytest.mark.parametrize('plan', [k for k in cd.PLANS if cd.PLANS[k] is not None])
@pytest.mark.parametrize('name', ['tiles', 'tiles-singular', 'all'])
def test_the_tiles_under_every_planned_scratch_give_the_bits_of_one_batch(name, plan):
    c, be = cd.case(name), context()
    csr, active = on_device(c)
    comps = components_of(be, c, csr, active)
    scratch = cd.PLANS[plan]
    batches = cd.plan_batches(c['sizes'], scratch)
    print(f'{name}, {plan}: {scratch} doubles, batches of {[[int(c["sizes"][i]) for i in b] for b in batches]}')
    assert len(batches) > 1
    if name == 'tiles':
        assert [len(b) for b in batches] == {'three-batches': [1, 1, 1], 'exact-fit': [2, 1]}[plan]
    one, status = entry(be, c, csr, comps)
    check_exact(c, one, status, f'{name}, one batch')
    for _ in range(2):
        d, status = entry(be, c, csr, comps, scratch)
        assert d.tobytes() == one.tobytes() and np.array_equal(status, c['status']), plan
    got, info = be.inverse_diag_event_list(csr, active, scratch_doubles=scratch)
    assert got.cpu().numpy().tobytes() == one.tobytes() and np.array_equal(info['status'], c['status'])


def test_a_scratch_one_double_short_of_the_largest_tile_is_refused_before_anything_is_written():
    c, be = cd.case('tiles'), context()
    csr, active = on_device(c)
    comps = components_of(be, c, csr, active)
    K, sizes = c['K'], comps['sizes']
    d = torch.full((K,), SENTINEL, dtype=torch.float64, device='cuda')
    status = torch.full((len(sizes),), int(SENTINEL), dtype=torch.int32, device='cuda')
    scratch = torch.full((cd.tile_doubles(300),), TAIL, dtype=torch.float64, device='cuda')

    def call(scratch_doubles, sizes=sizes, scratch=scratch):
        want = cd.refusal(K, csr[2].numel(), len(sizes), int(comps['member'].numel()), scratch_doubles, sizes.tolist(),
                          scratch=scratch is not None)
        code = be._lib.tnmf_hip_events_inverse_diag(
            be._ctx, K, csr[2].numel(), p(csr[0]), p(csr[1]), p(csr[2]), len(sizes), p(comps['comp_start']),
            sizes.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), comps['member'].numel(), p(comps['member']),
            p(comps['local']), p(scratch), scratch_doubles, p(d), p(status), be._stream())
        assert code == want, (code, want)
        return code
    assert call(cd.tile_doubles(300) - 1) == _lib.E_GEOM and call(cd.tile_doubles(300), scratch=None) == -1
    assert call(cd.tile_doubles(300), sizes=np.ascontiguousarray(sizes[::-1])) == _lib.E_GEOM
    torch.cuda.synchronize()
    assert np.all(d.cpu().numpy() == SENTINEL) and np.all(status.cpu().numpy() == int(SENTINEL))
    assert np.all(scratch.cpu().numpy() == TAIL)
    assert call(cd.tile_doubles(300)) == 0
    torch.cuda.synchronize()
    assert d.cpu().numpy().tobytes() == c['d'].tobytes() and not status.cpu().numpy().any()


@pytest.mark.parametrize('name', cd.GRAPHS)
def test_the_component_graphs(name):
    """Row orders that are adversarial for min-label propagation, a star, a complete graph, ties of equal size and the list
    without an edge: the lists of the breadth-first search, within 4 ceil(log2 K) rounds; d inside the bar."""
    c, be = cd.graph_case(name), context()
    csr, active = on_device(c)
    comps = components_of(be, c, csr, active)
    _, mirrored = cd.hooking(c)
    print(f'{name}: K {c["K"]}, sizes {sorted(set(c["sizes"].tolist()))}, {comps["rounds"]} rounds on the device, {mirrored} '
          f'in the mirror, at most {4 * int(np.ceil(np.log2(c["K"])))}')
    assert (comps['rounds'] == 0) == (name == 'diagonal-only')
    assert np.array_equal(comps['row_size'].cpu().numpy(), c['ref']['size'])
    d, status = entry(be, c, csr, comps)
    assert not status.any()
    check_d(d, c['ref'], name)
    again, _ = entry(be, c, csr, comps)
    assert again.tobytes() == d.tobytes()
    got, info = be.inverse_diag_event_list(csr, active)
    assert got.cpu().numpy().tobytes() == d.tobytes() and info['rounds'] == comps['rounds']
    if name == 'diagonal-only':
        assert np.array_equal(d, 1. / np.diag(c['dense']))


def test_dense_random_components_inside_the_bar():
    """G = B B' + n I with seeded B, n in (31, 129, 257): a class of 64 threads, the raised LDS limit and a tile, every
    product a rounding; poisoned rows that are not active between them."""
    c, be = cd.graph_case('random-dense'), context()
    csr, active = on_device(c)
    comps = components_of(be, c, csr, active)
    d, status = entry(be, c, csr, comps)
    assert not status.any()
    ref = c['ref']
    check_d(d, ref, 'random dense')
    on = ref['size'] > 0
    ratio = np.abs(d[on] - ref['d'][on]) / ref['d'][on] / ref['bar'][on]
    for n in cd.DENSE_SIZES:
        print(f'random dense, {n} rows: worst error / bar {ratio[ref["size"][on] == n].max():.3g}')
    print(f'random dense: worst error / bar {ratio.max():.3g}')
    again, _ = entry(be, c, csr, comps)
    assert again.tobytes() == d.tobytes()
    got, _ = be.inverse_diag_event_list(csr, active)
    assert got.cpu().numpy().tobytes() == d.tobytes()

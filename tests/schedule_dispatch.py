"""
Host mirror of the schedule executor: what tnmf_hip_run_schedule (api.hip), its persistent kernel k_schedule and the
fused tail k_finalize_blend_apply (generic.hip) and the volume variant vol_api_run_schedule do with an operation list --
validation, the joining of runs of H steps, the choice of route, and per operation the forms, block counts, chunk counts
and fusions it meets -- restated in plain Python so that the tests can choose the smallest cases that reach every cell
(tests/test_hip_schedule_matrix.py) and a CPU test can check that they do (tests/test_schedule_dispatch_cpu.py).

A geometry is (N, C, D, M, A) as in direct_dispatch.py; a dtype is 'f' or 'd'.  An operation is written with integers,
the way the C ABI sees it: ('H', n0, n1), ('G', n0, n1, a, b), ('W',) -- or ('W', n0, n1) for a W update that carries a
range, which nobody reads -- and ('?', n0, n1) for a kind the library does not know.
"""
from collections import namedtuple

import direct_dispatch as dd
from direct_dispatch import (ESIZE, NUM_CU, cdiv, generic_corr_H_chunks, kBlock, kMaxShiftsPerThread, kSmallQ, kSmallTX,
                             kSmallTY, make_tile, reconstruct_is_small, reconstruct_small_lds)
from fft_dispatch import fft_has, use_fft_under_auto

TINY = 1 << 18            # api.hip: const bool tiny = N * M * Hy * Hx <= 1 << 18 (on Hx, not the row stride)
K_OP_SLOTS = 4            # common.h: kOpSlots, the ring of pinned copies of the list
OP_BYTES = 32             # sizeof(tnmf_hip_op): int kind, n0, n1 (+ 4 bytes of padding), double a, b
SLOT_GROWTH = 4096        # api.hip: align_up(need, 4096)
LDS_MAX = 64 * 1024       # generic.hip: generic_schedule_fits, generic_run_schedule
GRID_CAP = 128            # generic.hip: schedule_grid, generic_schedule_chunks
P_CAP = 64                # generic.hip: generic_schedule_chunks
KINDS = {'H': 0, 'G': 1, 'W': 2, '?': 7}
LAMBDA = 0.8

PATHS = ('auto', 'generic', 'mfma', 'fft', 'hybrid', 'split')


# ----------------------------------------------------------------------------------------------------------------------
# validation and joining (api.hip: tnmf_hip_run_schedule; since the fix vol_api_run_schedule validates the same way)
# ----------------------------------------------------------------------------------------------------------------------
def rng_of(op):
    return (op[1], op[2]) if len(op) >= 3 else (0, 0)


def validate(ops, N, pointers=True):
    """The first refusal, in the library's order: TNMF_E_NULL, then per operation an unknown kind (TNMF_E_UNSUPPORTED)
    before a bad range (TNMF_E_GEOM); the W update is exempt from the range check.  None: the list runs."""
    if not pointers:
        return 'E_NULL'
    for op in ops:
        if op[0] not in ('H', 'G', 'W'):
            return 'E_UNSUPPORTED'
        if op[0] == 'W':
            continue
        n0, n1 = rng_of(op)
        if n0 < 0 or n1 < n0 or n1 > N:
            return 'E_GEOM'
    return None


def join(ops):
    """Runs of consecutive H steps: empties dropped; sorted by n0 (stable); joined where the sorted ranges are pairwise
    disjoint -- ranges that touch merged into one, others kept apart; a run with any overlap (duplicates included) left in
    its original order, without its empties.  Everything else passes through."""
    out, i = [], 0
    while i < len(ops):
        if ops[i][0] != 'H':
            out.append(ops[i])
            i += 1
            continue
        j = i
        while j < len(ops) and ops[j][0] == 'H':
            j += 1
        run = [op for op in ops[i:j] if op[2] > op[1]]
        srt = sorted(run, key=lambda op: op[1])
        if all(srt[k][1] >= srt[k - 1][2] for k in range(1, len(srt))):
            for k, op in enumerate(srt):
                if out and out[-1][0] == 'H' and k > 0 and out[-1][2] == op[1]:
                    out[-1] = ('H', out[-1][1], op[2])
                else:
                    out.append(op)
        else:
            out += run
        i = j
    return out


def run_class(run):
    """Edge classes of one run of H steps (two or more of them)."""
    e = set()
    live = [op for op in run if op[2] > op[1]]
    if len(live) < len(run):
        e.add('run_empties')
    srt = sorted(live, key=lambda op: op[1])
    pairs = [(srt[k - 1], srt[k]) for k in range(1, len(srt))]
    if any(b[1] < a[2] for a, b in pairs):
        if any(a[1:3] == b[1:3] for a, b in pairs):
            e.add('run_duplicate')
        if any(a[1:3] != b[1:3] and b[2] <= a[2] for a, b in pairs):
            e.add('run_nested')
        if any(a[1:3] != b[1:3] and b[2] > a[2] for a, b in pairs):
            e.add('run_overlapping')
    elif pairs:
        if live != srt:
            e.add('run_disjoint_shuffled')
        if any(b[1] == a[2] for a, b in pairs):
            e.add('run_touching')
        if any(b[1] > a[2] for a, b in pairs):
            e.add('run_gap')
    return e


def runs_of(ops):
    out, i = [], 0
    while i < len(ops):
        j = i
        while j < len(ops) and ops[j][0] == 'H':
            j += 1
        if j - i >= 2:
            out.append(ops[i:j])
        i = max(j, i + 1)
    return out


# ----------------------------------------------------------------------------------------------------------------------
# the persistent kernel (generic.hip)
# ----------------------------------------------------------------------------------------------------------------------
def schedule_lds(g, T):
    """generic.hip: schedule_lds -- the largest of the three block functions' needs and the W gradient's fold."""
    tR, tW, tH = make_tile(g.Dy, g.Dx), make_tile(g.Hy, g.Hx), make_tile(g.Dy, g.Dx)
    nA, es = g.Ay * g.Ax, ESIZE[T]
    r = ((tR.TY + g.Ay - 1) * (tR.TX + g.Ax - 1) + nA) * es
    w = (2 * (tW.TY + g.Ay - 1) * (tW.TX + g.Ax - 1) + nA) * es
    h = ((tH.TY + g.Ay - 1) * (tH.TX + g.Ax - 1) + 2 * tH.TY * tH.TX) * es
    gs = min(nA, kBlock)
    h = max(h, (kBlock // gs) * nA * 2 * 8)
    return max(r, w, h)


def schedule_small_max(g, T):
    """generic.hip: schedule_small_max -- the largest slice whose reconstruct takes the small-call form (0: none)."""
    tR = make_tile(g.Dy, g.Dx)
    if not reconstruct_is_small(g._replace(N=1), T, tR):
        return 0
    per = g.C * tR.tiles_y * tR.tiles_x
    return 63 // per if per > 0 else 0


def schedule_lds_any(g, T):
    lds, sm = schedule_lds(g, T), schedule_small_max(g, T)
    if sm > 0:
        lds = max(lds, reconstruct_small_lds(g, T, kSmallQ))
    return lds, sm


def generic_schedule_fits(g, T):
    if g.Ay * g.Ax > kBlock * kMaxShiftsPerThread:
        return False
    return schedule_lds_any(g, T)[0] <= LDS_MAX


def fits_why(g, T):
    if g.Ay * g.Ax > kBlock * kMaxShiftsPerThread:
        return 'shifts'
    return None if schedule_lds_any(g, T)[0] <= LDS_MAX else 'lds'


def schedule_grid(num_cu=NUM_CU, per_cu=1):
    """generic.hip: schedule_grid -- min(resident, min(CUs, 128)); the occupancy is the device's answer (one or more
    workgroups of 256 threads and at most 64 KiB per compute unit: the cap decides on an MI355X)."""
    return min(per_cu * num_cu, min(num_cu, GRID_CAP))


def generic_schedule_chunks(g, num_cu=NUM_CU):
    grid = min(num_cu, GRID_CAP)
    return min(max(cdiv(grid, g.M * g.C), 1), P_CAP)


def is_tiny(g):
    return g.N * g.M * g.Hy * g.Hx <= TINY


def route(geometry, T, path, persistent, n_joined):
    """'volume' | 'persistent' | 'per_op'."""
    if len(geometry[4]) == 3:
        return 'volume'
    g = dd.geo(geometry)
    if n_joined > 0 and is_tiny(g) and persistent != 0 and path in ('auto', 'generic') and generic_schedule_fits(g, T):
        return 'persistent'
    return 'per_op'


def same_functions(geometry, T, ops):
    """Whether the list handed over one operation per call runs the same device functions in the same order as the list
    in one call: the joined H steps take the reconstruct form (small call or plain) of each of their pieces."""
    g = dd.geo(geometry)
    sm = schedule_small_max(g, T)
    for run in runs_of(list(ops)):
        live = [op for op in run if op[2] > op[1]]
        for j in join(run):
            for op in live:
                if j[1] <= op[1] and op[2] <= j[2] and ((j[2] - j[1]) <= sm) != ((op[2] - op[1]) <= sm):
                    return False
    return True


def ring(lengths):
    """The ring of pinned slots over consecutive calls of the persistent route: [(slot, waits for an earlier call,
    regrown to bytes or 0)]."""
    cap, used, out = [0] * K_OP_SLOTS, [False] * K_OP_SLOTS, []
    for k, n in enumerate(lengths):
        slot, need = k % K_OP_SLOTS, n * OP_BYTES
        grown = 0
        if cap[slot] < need:
            grown = cap[slot] = cdiv(need, SLOT_GROWTH) * SLOT_GROWTH
        out.append((slot, used[slot], grown))
        used[slot] = True
    return out


# ----------------------------------------------------------------------------------------------------------------------
# the cell of a case
# ----------------------------------------------------------------------------------------------------------------------
Cell = namedtuple('Cell', 'route error last_path edges info')


def ab_form(a, b):
    if a == 0:
        return 'ab_0_1' if b == 1 else 'ab_0_lambda'
    return 'ab_1_1' if (a, b) == (1, 1) else 'ab_mix'


def _sequence_edges(ops, e):
    """The fusions: the executors look one operation ahead of a W gradient."""
    kinds = [op[0] for op in ops]
    for i, k in enumerate(kinds):
        nxt = kinds[i + 1] if i + 1 < len(kinds) else None
        if k == 'G' and nxt == 'W':
            e.add('G_W_fused')
            if i > 0 and kinds[i - 1] == 'G':
                e.add('G_G_W')
        if k == 'G' and nxt != 'W':
            e.add('G_unfused')
        if k == 'W' and i == 0:
            e.add('W_first')
        if k == 'W' and i > 0 and kinds[i - 1] == 'W':
            e.add('W_twice')
        if k == 'W' and (i == 0 or kinds[i - 1] != 'G'):
            e.add('W_alone')


def _slice_edges(op, N, e):
    n0, n1 = rng_of(op)
    if n1 == n0:
        e.add('empty_H' if op[0] == 'H' else 'empty_G_' + ab_form(op[3], op[4]))
        return
    if n0 == 0:
        e.add('slice_first')
    if n1 == N:
        e.add('slice_last')
    if n0 > 0 and n1 < N:
        e.add('slice_interior')


def _family(geometry, n, T, path, prim, padded):
    """Kernel family of one primitive of the per-operation path on a slice of n samples, where the mirrors of the direct
    kernels can name it (paths auto, generic, mfma); None elsewhere."""
    if path not in dd.PATHS:
        return None
    G = (n,) + tuple(geometry[1:])
    return dd.cell(G, T, path, prim, padded).family


def corr_H_on_fft(geometry, n, T, path):
    """api.hip: corr_H_on_fft for a slice of n samples."""
    G = (n,) + tuple(geometry[1:])
    if path == 'fft':
        return True
    if path == 'hybrid':
        return fft_has(G, T)
    return path == 'auto' and use_fft_under_auto(G, T)


def partials_region(geometry, nmax, T, num_cu=NUM_CU):
    """plan_scratch(gmax).P: the chunks the partials region holds (api.hip: the MFMA count is asked as for float32)."""
    g = dd.geo((nmax,) + tuple(geometry[1:]))
    P = generic_corr_H_chunks(g, num_cu)
    if dd.mfma_has_corr_H(g, 'f'):
        P = max(P, dd.plan_corr_H(g, num_cu).P)
    return P


def slice_chunks(geometry, n, T, path, padded, num_cu=NUM_CU):
    """Chunks of the split-K W gradient of one slice on the direct kernels (do_corr_H_partials)."""
    g = dd.geo((n,) + tuple(geometry[1:]))
    if not padded and dd.use_mfma(g, T, path, 'grad_W'):
        return dd.plan_corr_H(g, num_cu).P
    return generic_corr_H_chunks(g, num_cu)


def cell(geometry, dtype, path, persistent, ops, padded=False, r_scratch=True, num_cu=NUM_CU):
    """The route a list takes and the edge classes it meets."""
    N = geometry[0]
    T = dtype
    err = validate(ops, N)
    if err:
        return Cell('refused', err, None, frozenset({'refused_' + err}), None)
    e = set()
    nd = len(geometry[4])
    if nd == 3:
        # vol_api_run_schedule: always per operation, nothing joined, P clamped to the largest slice's
        _sequence_edges(ops, e)
        for op in ops:
            if op[0] != 'W':
                _slice_edges(op, N, e)
            if op[0] == 'G':
                e.add(ab_form(op[3], op[4]))
        for run in runs_of(ops):
            e |= run_class(run)
        e.add('r_scratch' if r_scratch else 'no_r_scratch')
        return Cell('volume', None, 'volume', frozenset(e), None)
    g = dd.geo(geometry)
    joined = join(ops)
    rt = route(geometry, T, path, persistent, len(joined))
    for run in runs_of(ops):
        e |= run_class(run)
    e.add('r_scratch' if r_scratch else 'no_r_scratch')
    if padded:
        e.add('padded_H')
    for op in ops:
        if op[0] == 'G':
            e.add(ab_form(op[3], op[4]))
        if op[0] != 'W':
            _slice_edges(op, N, e)
    _sequence_edges(joined, e)
    info = {'joined': joined}
    if is_tiny(g):
        if g.N * g.M * g.Hy * g.Hx == TINY:
            e.add('tiny_at_2^18')
        if path not in ('auto', 'generic'):
            e.add('tiny_path_' + path)
        elif not generic_schedule_fits(g, T):
            e.add('fits_false_' + fits_why(g, T))
        elif persistent == 0 and joined:
            e.add('tiny_persistent_0')
    elif (g.N * g.M * g.Hy - g.M * g.Hy) * g.Hx <= TINY or g.N * g.M * g.Hy * (g.Hx - 1) <= TINY:
        e.add('just_above_2^18')
    if rt == 'persistent':
        e.add(f'persistent_{persistent}_{T}_{"1d" if g.one_d else "2d"}')
        grid = schedule_grid(num_cu)
        _, small_max = schedule_lds_any(g, T)
        Pa = generic_schedule_chunks(g, num_cu)
        MC = g.M * g.C
        tR, tW = make_tile(g.Dy, g.Dx), make_tile(g.Hy, g.Hx)
        e.add('small_max_0' if small_max == 0 else 'small_max_positive')
        e.add(f'MC_{MC}' if MC <= 2 else ('rows_gt_grid' if MC > grid else 'rows_le_grid'))
        forms, phases = set(), []
        for op in joined:
            if op[0] == 'W':
                continue
            n = op[2] - op[1]
            if n > 0:
                if n <= small_max:
                    forms.add('recon_small')
                    phases.append(n * g.C * cdiv(g.Dy, kSmallTY) * cdiv(g.Dx, kSmallTX))
                else:
                    forms.add('recon_plain')
                    phases.append(n * g.C * tR.tiles_y * tR.tiles_x)
            if op[0] == 'H' and n > 0:
                phases.append(n * g.M * tW.tiles_y * tW.tiles_x)
            if op[0] == 'G':
                items = n * tR.tiles_y * tR.tiles_x
                P = (items if items > 0 else 1) if items < Pa else Pa
                phases.append(P * MC)
                if n > 0:
                    if Pa == P_CAP and P == Pa:
                        e.add('P_at_cap_64')
                    e.add('P_clamped_to_items' if items < Pa else ('P_lt_items' if P < items else 'P_eq_items'))
        e |= forms
        if len(forms) == 2:
            e.add('recon_small_and_plain_in_one_list')
        for nb in phases:
            if 0 < nb < grid:
                e.add('phase_lt_grid')
            if nb > grid and nb % grid:
                e.add('phase_gt_grid_ragged')
        info.update(grid=grid, small_max=small_max, P=Pa, phases=phases)
        return Cell(rt, None, 'generic', frozenset(e), info)
    # ---- the per-operation path
    e.add(f'per_op_{T}')
    nmax = max([1] + [op[2] - op[1] for op in joined if op[0] != 'W'])
    region = partials_region(geometry, nmax, T, num_cu)
    last, fams, info['chunks'] = None, set(), []
    i = 0
    while i < len(joined):
        op = joined[i]
        n = op[2] - op[1] if op[0] != 'W' else 0
        if op[0] == 'H' and n > 0:
            fams.add(_family(geometry, n, T, path, 'reconstruct', padded))
            last = _family(geometry, n, T, path, 'update_H', padded)
            fams.add(last)
        elif op[0] == 'G':
            if n > 0 and not corr_H_on_fft(geometry, n, T, path):
                P = slice_chunks(geometry, n, T, path, padded, num_cu)
                info['chunks'].append((n, P, region))
                fams.add(_family(geometry, n, T, path, 'reconstruct', padded))
                last = _family(geometry, n, T, path, 'grad_W', padded)
                fams.add(last)
                apply_now = i + 1 < len(joined) and joined[i + 1][0] == 'W'
                e.add(f'finalize_{"apply_now" if apply_now else "blend_only"}_{last}')
                if apply_now:
                    i += 1
            else:
                if n > 0:
                    last = 'fft'
                    e.add(f'fft_arm_path_fft_{T}' if path == 'fft' else f'fft_arm_{path}')
                    if i + 1 < len(joined) and joined[i + 1][0] == 'W':
                        e.add('fft_arm_then_separate_W')
                else:
                    e.add('empty_G_on_axpby')
        i += 1
    grads = [(op[2] - op[1]) for op in joined if op[0] == 'G' and op[2] > op[1]]
    if path == 'auto' and T == 'f' and grads:
        on = [corr_H_on_fft(geometry, n, T, path) for n in grads]
        if any(on) and not all(on):
            e.add('fft_arm_auto_next_to_direct')
    # a joined run whose union runs on another family than its pieces
    for run in runs_of(ops):
        j = join(run)
        if len(j) < len([op for op in run if op[2] > op[1]]):
            piece = {_family(geometry, op[2] - op[1], T, path, 'update_H', padded) for op in run if op[2] > op[1]}
            union = {_family(geometry, op[2] - op[1], T, path, 'update_H', padded) for op in j}
            if None not in piece | union and not (union & piece):
                e.add('join_changes_family')
    if 'refused' in fams:
        e.add('kernel_family_refuses')      # (no case of the matrix may: the list would stop half way)
    info['last'] = last
    return Cell(rt, None, last, frozenset(e), info)


# ----------------------------------------------------------------------------------------------------------------------
# the cells the matrix has to reach, by table of the design notes
# ----------------------------------------------------------------------------------------------------------------------
ROUTE_CELLS = tuple(f'persistent_{p}_{T}_{d}' for p in (1, 2) for T in 'fd' for d in ('1d', '2d')) + (
    'tiny_persistent_0', 'tiny_path_mfma', 'tiny_path_split', 'tiny_path_hybrid', 'tiny_path_fft', 'tiny_at_2^18',
    'just_above_2^18', 'fits_false_shifts', 'fits_false_lds', 'volume')
K_SCHEDULE_CELLS = (
    'recon_small_and_plain_in_one_list', 'small_max_0', 'phase_lt_grid', 'phase_gt_grid_ragged', 'rows_gt_grid', 'MC_1', 'MC_2',
    'P_at_cap_64', 'P_clamped_to_items', 'P_lt_items', 'G_W_fused', 'G_G_W', 'G_unfused', 'W_first', 'W_twice', 'W_alone',
    'ab_0_1', 'ab_0_lambda', 'ab_1_1', 'ab_mix', 'nan_acc', 'empty_H', 'empty_G_ab_0_1', 'empty_G_ab_0_lambda',
    'empty_G_ab_1_1', 'empty_G_ab_mix', 'slice_first', 'slice_interior', 'slice_last', 'r_scratch', 'no_r_scratch', 'padded_H')
HOST_CELLS = (
    'finalize_apply_now_generic', 'finalize_blend_only_generic', 'finalize_apply_now_mfma', 'finalize_blend_only_mfma',
    'fft_arm_path_fft_f', 'fft_arm_path_fft_d', 'fft_arm_auto_next_to_direct', 'fft_arm_then_separate_W', 'empty_G_on_axpby',
    'join_changes_family', 'W_alone', 'nan_acc', 'no_r_scratch', 'padded_H',
    'run_disjoint_shuffled', 'run_touching', 'run_gap', 'run_empties', 'run_nested', 'run_duplicate', 'run_overlapping')
VOLUME_CELLS = ('run_disjoint_shuffled', 'run_touching', 'run_gap', 'run_empties', 'run_nested', 'run_duplicate',
                'run_overlapping', 'G_W_fused', 'G_unfused', 'W_alone', 'empty_H', 'empty_G_ab_0_1', 'nan_acc')
RING_CELLS = ('ring_reuse', 'ring_regrow')
REFUSALS = ('unknown_first', 'unknown_last', 'n1_gt_N', 'n0_lt_0', 'n1_lt_n0', 'W_with_nonsense_range', 'n_ops_0')


def required():
    req = {('route', c) for c in ROUTE_CELLS}
    req |= {('persistent', c) for c in K_SCHEDULE_CELLS}
    req |= {('per_op', c) for c in HOST_CELLS}
    req |= {('volume', c) for c in VOLUME_CELLS}
    req |= {('ring', c) for c in RING_CELLS}
    req |= {(kind, c) for kind in ('refusal_2d', 'refusal_volume') for c in REFUSALS}
    return req


# No geometry is out of reach: generic_schedule_fits answers false on tiny problems the per-operation path accepts -- for
# lists of H steps: more than 1024 shifts (a 1-D atom of 1100 taps; the W gradient of such atoms is refused by both
# direct families), and the W gradient's LDS tile of one-row samples under a tall one-column atom in float64 (67584
# bytes) next to a reconstruct and an H update that fit.
UNREACHABLE = {}

# What the matrix leaves out, by name, with the reason.
NOT_COVERED = {
    ('last_path', 'split / hybrid'): 'the family of each primitive under path="split" and path="hybrid" is not restated here '
                                     '(split_dispatch.py and fft_dispatch.py own those rules); the tiny cases on these '
                                     'paths assert the route (not persistent) and the numbers',
    ('route', 'occupancy_below_one_per_CU'): 'a grid smaller than min(CUs, 128) needs a device whose occupancy query answers '
                                             'less than one workgroup per compute unit; the kernel strides by gridDim and '
                                             'the matrix reads the device, but cannot shrink it',
    ('route', 'cooperative_launch_refused'): 'hipLaunchCooperativeKernel refusing an occupancy-sized grid cannot be provoked '
                                             'from a test',
    ('ring', 'hipHostMalloc_fails'): 'TNMF_E_WORKSPACE of the pinned slot needs an exhausted host',
}

# ----------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_hip_schedule_matrix.py
# ----------------------------------------------------------------------------------------------------------------------
Case = namedtuple('Case', 'geometry dtypes path modes ops poison padded r_scratch')


def case(geometry, ops, dtypes='fd', path='auto', modes=(1, 2, 0), poison=False, padded=False, r_scratch=True):
    return Case(geometry, dtypes, path, modes, tuple(ops), poison, padded, r_scratch)


L = LAMBDA
C1 = (10, 3, (60,), 8, (20,))                 # BASELINE config 1's geometry: 1-D, M*C = 24, small_max 0
T2 = (10, 2, (20, 24), 5, (4, 5))             # 2-D tiny: 16 x 16 tiles, small_max 7 of 10 samples; H update of all: 200 blocks
M3 = (4, 1, (12, 40), 3, (3, 5))              # three atoms: no small form
WIDE = (2, 3, (10, 12), 48, (3, 4))           # 48 atoms x 3 channels = 144 rows on at most 128 workgroups
ONE = (6, 1, (40, 70), 1, (3, 3))             # one row: P = 64 (the cap) of 90 items; one sample: 15 items
TILE = (3, 1, (8, 30), 1, (3, 3))             # one row, one tile per sample
TWO = (11, 1, (20, 40), 2, (5, 3))            # two rows: P = cdiv(128, 2) = 64 exactly, of 66 items
AT18 = (4, 1, (61, 61), 16, (4, 4))           # H 64 x 64: 2^18 activations exactly
OVER18 = (4, 1, (61, 62), 16, (4, 4))         # H 64 x 65: one column per row more
SHIFTS = (1, 1, (1100,), 2, (1100,))          # 1100 shifts per atom: generic_schedule_fits false (H steps only)
TALL = (2, 1, (1, 40), 4, (31, 1))            # one-row samples, 31 x 1 atoms, float64: the W gradient's tile is 67584 bytes
BIG = (40, 1, (32, 32), 10, (7, 7))           # not tiny: 577600 activations; whole batch >= 2^19 (FFT arm under auto);
                                              # five samples and more >= 2^16 (split H update under auto), fewer: MFMA
VOL = (10, 2, (3, 4, 5), 3, (2, 2, 3))        # three shift axes

ASAG = (('H', 0, 2), ('G', 0, 2, 0., L), ('W',), ('H', 2, 10), ('G', 2, 10, 1 - L, L), ('W',))
RUNS = (('H', 6, 10), ('H', 0, 2), ('H', 3, 3), ('H', 2, 4), ('G', 1, 2, 0., 1.), ('W',),       # shuffled, touching, gap, empty
        ('H', 0, 6), ('H', 2, 4), ('G', 9, 10, 1., 1.),                                          # nested
        ('H', 1, 3), ('H', 1, 3), ('G', 0, 10, 1 - L, L),                                        # duplicate
        ('H', 0, 5), ('H', 3, 8))                                                                # overlapping


def _runs(N):
    s = N / 10.
    return tuple((op[0], int(round(op[1] * s)), int(round(op[2] * s))) + tuple(op[3:]) if len(op) > 1 else op for op in RUNS)


MATRIX = {
    # ---- routes
    'c1_asag': case(C1, ASAG),
    'c1_fullbatch': case(C1, (('H', 0, 10), ('G', 0, 10, 0., 1.), ('W',)), poison=True),
    't2_asag': case(T2, ASAG, poison=True),                                        # small and plain reconstruct in one list
    't2_runs': case(T2, RUNS, poison=True),
    't2_padded': case(T2, ASAG, poison=True, padded=True),
    't2_no_scratch': case(T2, (('H', 4, 6), ('G', 4, 6, 0., 1.), ('H', 9, 10), ('G', 9, 10, 1., 1.), ('W',)), r_scratch=False),
    't2_tail': case(T2, (('W',), ('W',), ('G', 2, 5, 0., 1.), ('G', 5, 9, 1., 1.), ('W',), ('G', 0, 1, 1 - L, L), ('H', 0, 0)),
                    modes=(1, 0)),
    't2_empties': case(T2, (('G', 3, 3, 1., 1.), ('G', 10, 10, 1 - L, L), ('W',), ('H', 5, 5), ('G', 0, 0, 0., L),
                            ('G', 2, 4, 1., 1.), ('W',), ('G', 7, 7, 0., 1.), ('G', 4, 5, 1., 1.)), modes=(1, 0)),
    't2_mfma': case(T2, ASAG, dtypes='f', path='mfma', modes=(1,)),
    't2_split': case(T2, ASAG, dtypes='f', path='split', modes=(1,)),
    't2_hybrid': case(T2, ASAG, path='hybrid', modes=(1,)),
    't2_fft': case(T2, ASAG, path='fft', modes=(1,), poison=True),
    'm3': case(M3, (('H', 0, 4), ('G', 1, 3, 0., 1.), ('W',)), modes=(1,)),
    'wide': case(WIDE, (('H', 0, 2), ('G', 0, 1, 0., L), ('G', 1, 2, 1., 1.), ('W',), ('W',)), poison=True, modes=(1, 0)),
    'one': case(ONE, (('H', 0, 6), ('G', 0, 6, 0., 1.), ('W',), ('G', 2, 3, 1., 1.), ('W',)), modes=(1,)),
    'tile': case(TILE, (('G', 1, 2, 0., 1.), ('W',), ('H', 1, 2)), modes=(1,)),
    'two': case(TWO, (('H', 0, 11), ('G', 0, 11, 0., L), ('G', 10, 11, 1 - L, L), ('W',)), modes=(1,)),
    'at18': case(AT18, (('H', 0, 4), ('G', 3, 4, 0., 1.), ('W',)), modes=(1,)),
    'over18': case(OVER18, (('H', 0, 4), ('G', 3, 4, 0., 1.), ('W',)), modes=(1,)),
    'shifts': case(SHIFTS, (('H', 0, 1),), dtypes='d', path='generic', modes=(1,)),
    'tall': case(TALL, (('H', 0, 2), ('H', 1, 2)), dtypes='d', path='generic', modes=(1,)),
    # ---- the per-operation path on a problem that is not tiny
    'big_asag': case(BIG, (('H', 0, 3), ('G', 0, 3, 0., L), ('W',), ('H', 37, 40), ('G', 37, 40, 1 - L, L), ('W',),
                           ('G', 5, 8, 1., 1.), ('G', 8, 8, 1., 1.)), poison=True, modes=(1,)),
    'big_generic': case(BIG, (('H', 0, 3), ('G', 0, 3, 0., L), ('W',), ('G', 5, 8, 1., 1.), ('W',), ('W',)), path='generic',
                        modes=(1,)),
    'big_whole': case(BIG, (('H', 0, 40), ('G', 0, 40, 0., 1.), ('W',), ('G', 20, 22, 1 - L, L), ('W',)), dtypes='f', modes=(1,),
                      poison=True),
    'big_fft': case(BIG, (('G', 0, 40, 0., 1.), ('W',), ('G', 39, 40, 1., 1.)), path='fft', modes=(1,), poison=True),
    'big_runs': case(BIG, _runs(40), modes=(1,), poison=True),
    'big_padded': case(BIG, (('H', 4, 7), ('G', 4, 7, 0., 1.), ('W',), ('W',)), modes=(1,), padded=True, poison=True),
    'big_no_scratch': case(BIG, (('H', 4, 7), ('G', 4, 7, 0., 1.), ('H', 39, 40), ('G', 39, 40, 1., 1.), ('W',)), modes=(1,),
                           r_scratch=False),
    'big_join': case(BIG, (('H', 3, 6), ('H', 0, 3), ('G', 0, 6, 0., 1.), ('W',)), dtypes='f', modes=(1,)),    # 3 + 3 samples
    # ---- volumes
    'vol_asag': case(VOL, (('H', 0, 2), ('G', 0, 2, 0., L), ('W',), ('H', 2, 10), ('G', 2, 10, 1 - L, L), ('W',), ('W',)), modes=(1,),
                     poison=True),
    'vol_runs': case(VOL, (('H', 2, 2), ('G', 3, 3, 0., 1.)) + RUNS, modes=(1,), poison=True),
}

RING_LENGTHS = (3, 200, 5, 130, 1, 129)        # six calls back to back on the tiny route (T2)

REFUSED_LISTS = {
    'unknown_first': ((('?', 0, 1), ('H', 0, 2), ('G', 0, 2, 0., 1.), ('W',)), 'E_UNSUPPORTED'),
    'unknown_last': ((('H', 0, 2), ('G', 0, 2, 0., 1.), ('W',), ('?', 0, 1)), 'E_UNSUPPORTED'),
    'n1_gt_N': ((('H', 0, 2), ('G', 0, 99, 0., 1.), ('W',)), 'E_GEOM'),
    'n0_lt_0': ((('H', 0, 2), ('W',), ('H', -1, 2)), 'E_GEOM'),
    'n1_lt_n0': ((('H', 0, 2), ('G', 2, 1, 0., 1.)), 'E_GEOM'),
    'W_with_nonsense_range': ((('H', 0, 2), ('G', 0, 2, 0., 1.), ('W', 7, -3)), None),
    'n_ops_0': ((), None),
}
REFUSAL_GEOMETRIES = {'refusal_2d': T2, 'refusal_volume': VOL}


def cells_of(cid, c):
    """{(table, cell)} a case reaches, over its dtypes and modes."""
    out = set()
    for T in c.dtypes:
        for mode in c.modes:
            cl = cell(c.geometry, T, c.path, mode, list(c.ops), c.padded, c.r_scratch)
            edges = set(cl.edges)
            if c.poison:
                edges.add('nan_acc')
            for x in edges:
                if x in ROUTE_CELLS:
                    out.add(('route', x))
                out.add((cl.route, x))
            if cl.route == 'volume':
                out.add(('route', 'volume'))
    return out


def reached(matrix):
    """{(table, cell): [case ids]} over the matrix, the ring and the refusals (which every matrix carries)."""
    got = {}
    for cid, c in matrix.items():
        for key in cells_of(cid, c):
            got.setdefault(key, []).append(cid)
    plan = ring(RING_LENGTHS)
    if any(waits for _, waits, _ in plan):
        got[('ring', 'ring_reuse')] = ['ring']
    if any(grown > SLOT_GROWTH for _, _, grown in plan):
        got[('ring', 'ring_regrow')] = ['ring']
    for kind, G in REFUSAL_GEOMETRIES.items():
        for name, (ops, err) in REFUSED_LISTS.items():
            if validate(ops, G[0]) == err:
                got[(kind, name)] = ['refusals']
    return got


def missing(matrix):
    got = reached(matrix)
    return sorted(k for k in required() if k not in got and k not in UNREACHABLE)


def sole_carriers(matrix):
    """{case id: [required cells only it carries]}."""
    out = {}
    for key, cids in reached(matrix).items():
        if key in required() and len(cids) == 1 and cids[0] in matrix:
            out.setdefault(cids[0], []).append(key)
    return out


def scratch_fits(matrix, num_cu=NUM_CU):
    """[(case, dtype, slice length, its chunks, the region's)] of every W gradient on the direct kernels of the
    per-operation path: the partials of a slice live where plan_scratch(gmax) put them."""
    out = []
    for cid, c in matrix.items():
        if len(c.geometry[4]) == 3:
            continue
        for T in c.dtypes:
            cl = cell(c.geometry, T, c.path, 0, list(c.ops), c.padded, c.r_scratch, num_cu)
            for n, P, region in cl.info['chunks']:
                out.append((cid, T, n, P, region))
    return out


# ----------------------------------------------------------------------------------------------------------------------
# seeded random lists
# ----------------------------------------------------------------------------------------------------------------------
RANDOM_SEEDS = tuple(range(24))
MAX_CHAIN = 8            # a list's bar is at most eight times that of one fused half step
AB_FORMS = ((0., 1.), (0., LAMBDA), (1., 1.), (1 - LAMBDA, LAMBDA))


def random_list(seed, N):
    """(ops, poison): at most 12 operations; slices drawn from {empty, one sample, ragged, all}, kinds and (a, b) forms at
    random; cut where the longest chain of dependent half steps would pass MAX_CHAIN; the accumulator is poisoned iff the
    first operation that touches it is a W gradient with a == 0."""
    import numpy as np

    from schedule_reference import chains
    rng = np.random.default_rng(1000 + seed)
    ops = []
    for _ in range(int(rng.integers(3, 13))):
        kind = 'HGW'[int(rng.choice(3, p=(0.45, 0.35, 0.2)))]
        if kind == 'W':
            ops.append(('W',))
            continue
        form = int(rng.integers(4))
        if form == 0:
            n0 = n1 = int(rng.integers(0, N + 1))
        elif form == 1:
            n0 = int(rng.integers(0, N))
            n1 = n0 + 1
        elif form == 2:
            n0 = int(rng.integers(0, N - 1))
            n1 = int(rng.integers(n0 + 1, N + 1))
        else:
            n0, n1 = 0, N
        ops.append(('H', n0, n1) if kind == 'H' else ('G', n0, n1) + AB_FORMS[int(rng.integers(4))])
    while ops and max(v for k, v in chains(to_slices(ops), N).items() if k != 'H_per_sample') > MAX_CHAIN:
        ops.pop()
    while True:
        # a W update from an accumulator of zeros (an empty W gradient with a == 0 in front of it, in this run of the
        # list or at the end of the one before) is 0 / 0 in every row: the empty gradient that zeroed it is taken out
        bad = zeroed_before_W(ops)
        if bad is None:
            break
        del ops[bad]
    first = next((op for op in ops if op[0] in 'GW'), None)
    return tuple(ops), bool(first and first[0] == 'G' and first[3] == 0)


def zeroed_before_W(ops):
    """Index of the empty W gradient with a == 0 whose zeros a W update would divide, over two runs of the list."""
    zero = None
    for _ in range(2):
        for i, op in enumerate(ops):
            if op[0] == 'G' and op[2] > op[1]:
                zero = None
            elif op[0] == 'G' and op[3] == 0:
                zero = i
            elif op[0] == 'W' and zero is not None:
                return zero
    return None


def to_slices(ops):
    """The list in the backend's form: ('H', slice) | ('G', slice, a, b) | ('W',)."""
    return [(op[0],) if op[0] == 'W' else (op[0], slice(op[1], op[2])) + tuple(op[3:]) for op in ops]

"""
Host model of what a tnmf_hip_ctx REMEMBERS between calls, apart from the spectrum-cache flags (those: cache_dispatch.py):
the six device buffers ctx->ws, ctx->hw, ctx->qb, ctx->ob, ctx->wimg and ctx->fft.ws, who lays them out how, how they grow
(ensure_buffer of tnmf_amd/csrc/api.hip, ensure_ws of fft.hip, the W images of split_kernels.h), the ring of pinned slots
of tnmf_hip_run_schedule, the objective tap and the path / split / persistent switches -- restated in plain Python so that
a CPU test can check that a list of call sequences carries every transition of that state at 64, 256 and 304 compute units
(tests/test_context_dispatch_cpu.py) and a GPU test can hold the library to "a used context computes the bits a fresh one
computes" call by call at the C ABI (tests/test_hip_context_matrix.py).

A geometry is (N, C, D, M, A) as in direct_dispatch.py; a dtype is 'f' or 'd'.  An operation is Op(kind, family, size, T):
one small representative call of an (entry point, layout) of USES, in a SMALL and a LARGE geometry (the model, not the eye,
checks that LARGE outgrows what SMALL leaves: check_sizes).  The EXTENT of a layout is the bytes the entry point asks
ensure_* for: everything the call may read or write of that buffer lies below it.

Byte counts come from the mirrors that already hold them (schedule_dispatch, volume_dispatch, lateral_dispatch,
atoms_dispatch, atom_gram_dispatch, correlogram_dispatch, sources_dispatch, fft_dispatch, split_dispatch); what api.hip
adds on top (plan_scratch, the two schedule layouts, the beta / objective / modes arithmetic) is restated here and pinned
to the source as text by the CPU test.
"""
import functools
import random
from collections import namedtuple

import atom_gram_dispatch as gd
import atoms_dispatch as ad
import correlogram_dispatch as cod
import direct_dispatch as dd
import fft_dispatch as fd
import lateral_dispatch as ld
import schedule_dispatch as sd
import sources_dispatch as srd
import split_dispatch as spd
import volume_dispatch as vd

E_OK, E_GEOM, E_UNSUPPORTED, E_STRIDE = 0, -2, -5, -6          # include/tnmf_hip.h
MiB = 1 << 20
ESIZE = {'f': 4, 'd': 8}
LONG = {'f': 'f32', 'd': 'f64'}
K_ENERGY_PARTIALS = 2048                                        # generic.h: kEnergyPartials
K_OBJ_CHUNK = 4096                                              # beta.h: kObjChunk
CUS = (64, 256, 304)
BUFFERS = ('ws', 'hw', 'qb', 'ob', 'wimg', 'fft.ws')
PATHS = ('auto', 'generic', 'mfma', 'fft', 'hybrid', 'split')
TAPS = 3                                                        # taps per shift axis of the lateral kernels the ops use
STRENGTHS = ld.USUAL
PREDECESSOR_SCALE = 2. ** 12                                    # predecessors run on other operands, this much larger
OPERAND_MAX = 2.                                                # |V|, |W|, |H| of every operand set stay below this


def align_up(a, b):
    return -(-a // b) * b


def cdiv(a, b):
    return -(-a // b)


def prod(t):
    out = 1
    for x in t:
        out *= x
    return out


# ---- which entry point may touch which buffer, under which layout ----------------------------------------------------------
# (tests/test_context_dispatch_cpu.py scans api.hip for the buffers; the layout names are this file's)
_PLAN, _VOL = 'ws:plan', 'ws:vol'
_FAM_R = ('fft.ws',)                      # do_reconstruct / do_corr_H may hand over to the FFT family
_FAM_H = ('fft.ws', 'wimg')               # do_corr_W: the FFT family or the split kernels
_UPDATE_H = (_PLAN, _VOL, 'hw:E', 'hw:E_neg_pos', 'hw:modes', 'qb:Q', 'ob:objective') + _FAM_H
USES = {
    'tnmf_hip_ctx_reserve': (_PLAN, _VOL, 'fft.ws'),
    'tnmf_hip_reconstruct': _FAM_R,
    'tnmf_hip_grad_H': (_PLAN, _VOL) + _FAM_H,
    'tnmf_hip_grad_W': (_PLAN, _VOL) + _FAM_R,
    'tnmf_hip_energy': (_PLAN, _VOL) + _FAM_R,
    'tnmf_hip_energy_beta': (_PLAN, _VOL) + _FAM_R,
    'tnmf_hip_energy_weighted': (_PLAN, _VOL) + _FAM_R,
    'tnmf_hip_sample_objective': (_PLAN, _VOL, 'ob:objective') + _FAM_R,
    'tnmf_hip_atom_terms': (_PLAN, 'ob:atom_terms') + _FAM_R,
    'tnmf_hip_atom_gram': (_PLAN, 'ob:atom_gram') + _FAM_R,
    'tnmf_hip_atom_sources': ('ob:sources',),
    'tnmf_hip_activation_correlogram': ('ob:correlogram',),
    'tnmf_hip_update_H': _UPDATE_H,
    'tnmf_hip_update_H_ex': _UPDATE_H + ('hw:vol',),
    'tnmf_hip_update_H_beta': _UPDATE_H + ('hw:vol',),
    'tnmf_hip_update_H_weighted': _UPDATE_H + ('hw:vol',),
    'tnmf_hip_grad_W_fused': (_PLAN, _VOL, 'qb:Q') + _FAM_R,
    'tnmf_hip_grad_W_beta': (_PLAN, _VOL, 'qb:Q') + _FAM_R,
    'tnmf_hip_grad_W_weighted': (_PLAN, _VOL, 'qb:Q') + _FAM_R,
    'tnmf_hip_run_schedule': ('ws:sched_persistent', 'ws:sched_ops', 'ws:vol_sched') + _FAM_H,
}
LAYOUTS = {
    'ws:plan': 'plan_scratch: [R | split-K partials | reduction words]',
    'ws:vol': 'vol_scratch: [R | reduction words | partials]',
    'ws:vol_sched': 'vol_scratch(nmax) with the batch gradient behind it',
    'ws:sched_persistent': 'the persistent schedule: [R | partials | op list | counter]',
    'ws:sched_ops': 'the per-operation schedule: plan_scratch(gmax) with the batch gradient behind it',
    'hw:E': 'E alone (fused lateral step)',
    'hw:E_neg_pos': '[E | neg | pos] (unfused lateral fallback)',
    'hw:modes': '[Hp | negp | posp | E] (reconstruction modes)',
    'hw:vol': 'the volume form [G0 | G1 | neg | pos | Hp | negp | posp]',
    'qb:Q': 'the field Q of the beta / weighted steps (also fft.V_volatile)',
    'ob:objective': 'per-block partial sums of the per-sample objective (entry point and tap)',
    'ob:atom_terms': '[partial sums per (sample, tile, atom) | taps]',
    'ob:atom_gram': '[partial sums per (sample, strip, pair) | taps]',
    'ob:sources': '[taps | channel sums of W | plane order | source starts]',
    'ob:correlogram': 'partial sums per (segment, strip, pair, lag)',
    'wimg': 'pre-split W images of the split family',
    'fft.ws': 'the workspace of the FFT family (fft_dispatch.make_layout)',
}


# ---- bytes -----------------------------------------------------------------------------------------------------------------
def plan_scratch(geometry, T, cus):
    """api.hip: plan_scratch -> dict(R, part, red, total)."""
    N, C, D, M, A = geometry
    r = align_up(N * C * prod(D) * ESIZE[T], 256)
    P = sd.partials_region(geometry, N, T, cus) if N > 0 else 0
    part = align_up(P * M * C * prod(A) * 2 * 8, 256)
    red = align_up((K_ENERGY_PARTIALS + 8) * 8, 256)
    return dict(R=r, part=part, red=red, P=P, total=r + part + red)


def sched_persistent_bytes(geometry, T, cus, n_ops, r_scratch=False):
    """api.hip: the persistent arm of tnmf_hip_run_schedule."""
    N, C, D, M, A = geometry
    P = sd.generic_schedule_chunks(dd.geo(geometry), cus)
    r = 0 if r_scratch else align_up(N * C * prod(D) * ESIZE[T], 256)
    p = align_up(P * M * C * prod(A) * 2 * 8, 256)
    o = align_up(n_ops * sd.OP_BYTES, 256)
    return r + p + o + 1024


def sched_ops_bytes(geometry, T, cus, nmax):
    """api.hip: plan_scratch(gmax).total + the gradient of one batch."""
    N, C, D, M, A = geometry
    return plan_scratch((max(nmax, 1), C, D, M, A), T, cus)['total'] + align_up(2 * M * C * prod(A) * ESIZE[T], 256)


def vol_scratch_bytes(geometry, T, cus, extra=0):
    return vd.vol_scratch(vd.vol(geometry), T, cus, extra)['total']


def vol_hw_bytes(geometry, T, mode, lateral):
    """api.hip: vol_api_update_H_ex, lat + 2 * nS + pad."""
    N, C, D, M, A = geometry
    S = [d + a - 1 if mode == 'valid' else (d - a + 1 if mode == 'full' else d) for d, a in zip(D, A)]
    H = [d + a - 1 for d, a in zip(D, A)]
    nS = align_up(N * M * prod(S) * ESIZE[T], 256)
    nP = align_up(N * M * prod(H) * ESIZE[T], 256)
    return (2 * nS if lateral else 0) + 2 * nS + (0 if mode == 'valid' else 3 * nP)


def qb_bytes(geometry, T):
    """api.hip: beta_fields_of."""
    N, C, D, M, A = geometry
    return align_up(N * C * prod(D) * ESIZE[T], 256)


def objective_bytes(geometry):
    """api.hip: sample_objective_of -> 0 when one block takes a sample (the buffer is not touched)."""
    N, C, D, M, A = geometry
    B = cdiv(C * prod(D), K_OBJ_CHUNK) if C * prod(D) else 1
    return align_up(N * B * 8, 256) if B > 1 else 0


def taps_bytes(geometry, T):
    N, C, D, M, A = geometry
    return srd.taps_bytes(C, M, D, A, LONG[T])


def atom_terms_bytes(geometry, T, group=1):
    N, C, D, M, A = geometry
    return align_up(N * ad.plan(C, D, A)['slots'] * (M // group) * 2 * 8, 256) + taps_bytes(geometry, T)


def atom_gram_bytes(geometry, T, group=1):
    N, C, D, M, A = geometry
    p = gd.plan(C, M, D, A, group, LONG[T])
    return align_up(N * p['strips'] * p['pairs'] * p['wg_doubles'] * 8, 256) + taps_bytes(geometry, T)


def sources_bytes(geometry, T, n_sources, emit):
    N, C, D, M, A = geometry
    return srd.work(C, M, D, A, LONG[T], n_sources, emit)['total']


def shift_shape(geometry):
    return tuple(d + a - 1 for d, a in zip(geometry[2], geometry[4]))


CORR_LAG = 1


def correlogram_bytes(geometry, T, per_sample=False):
    N, C, D, M, A = geometry
    S = shift_shape(geometry)
    return align_up(cod.plan(N, M, S, (CORR_LAG,) * len(S), per_sample, LONG[T])['partial_bytes'], 256)


def wimg_bytes(geometry):
    N, C, D, M, A = geometry
    return cdiv(M, 32) * C * spd.SplitCfg(*spd.split_pick(geometry)).wimg


def fft_ws_bytes(geometry, T, path, window):
    lay = fd.make_layout(geometry, T, path)
    return lay.total if window else lay.total_no_window


# ---- the context -----------------------------------------------------------------------------------------------------------
Use = namedtuple('Use', 'buffer layout extent T')


class Context:
    """Capacities, the last user of every buffer, the switches, the ring; `seen` collects the names of TRANSITIONS."""

    def __init__(self, cus, name='ctx'):
        self.cus, self.name = cus, name
        self.cap = dict.fromkeys(BUFFERS, 0)
        self.last = dict.fromkeys(BUFFERS, None)      # Use of the last call that laid the buffer out
        self.grew = 0                                 # allocations after tnmf_hip_ctx_reserve
        self.path, self.split, self.persistent, self.tap = 'auto', 1, 1, False
        self.tapped_last = self.tapped_now = self.tap_was_set = False
        self.ring_cap, self.ring_used, self.ring_next = [0] * sd.K_OP_SLOTS, [False] * sd.K_OP_SLOTS, 0
        self.beta_last = False
        self.refused_last = False
        self.reserved = False
        self.seen = set()

    # api.hip: ensure_buffer; fft.hip: ensure_ws (no slack); split_kernels.h: launch (no rounding)
    def ensure(self, buffer, nbytes, slack=False, rounding=MiB):
        if nbytes <= self.cap[buffer]:
            if nbytes:
                self.seen.add(f'reuse_fits({buffer})')
            return False
        self.seen.add(f'first_allocation({buffer})' if self.cap[buffer] == 0 else f'regrow({buffer})')
        self.cap[buffer] = align_up(nbytes + (nbytes // 8 if slack else 0), rounding)
        self.grew += 1
        return True

    def use(self, buffer, layout, extent, T):
        """One call lays `buffer` out as `layout` over `extent` bytes."""
        if extent == 0:
            return
        self.ensure(buffer, extent, slack=buffer == 'ws', rounding=1 if buffer == 'wimg' else MiB)
        was = self.last[buffer]
        if was is not None:
            if was.layout != layout:
                self.seen.add(f'dirty({buffer}: {was.layout.split(":")[-1]} -> {layout.split(":")[-1]})')
            if was.T != T:
                self.seen.add(f'dtype_flip({buffer})')
            if buffer == 'ob' and self.tapped_last and layout != 'ob:objective':
                self.seen.add('tap_then_ob_user')
        self.last[buffer] = Use(buffer, layout, extent, T)


def ensure_buffer(have, nbytes, slack):
    """api.hip: ensure_buffer -> the capacity after the call."""
    return have if nbytes <= have else align_up(nbytes + (nbytes // 8 if slack else 0), MiB)


def ring_slot(calls):
    """The slot the `calls`-th persistent schedule of a context takes (1-based), and whether it waits for an event."""
    return (calls - 1) % sd.K_OP_SLOTS, calls > sd.K_OP_SLOTS


# ---- the operations --------------------------------------------------------------------------------------------------------
Op = namedtuple('Op', 'kind family size T')
Ctl = namedtuple('Ctl', 'what value')

SMALL, LARGE = 'small', 'large'
GEOMETRY = {
    ('2d', SMALL): (2, 1, (12, 20), 3, (3, 4)),
    ('2d', LARGE): (6, 1, (256, 256), 4, (5, 5)),
    ('1d', SMALL): (2, 1, (40,), 3, (5,)),
    ('1d', LARGE): (6, 1, (70000,), 4, (9,)),
    ('3d', SMALL): (4, 1, (4, 5, 6), 2, (2, 3, 2)),
    ('3d', LARGE): (4, 1, (40, 48, 80), 2, (2, 2, 3)),
    # the persistent schedule wants a tiny problem (2^18 activations at most): the large one is large in its channels
    ('sched', SMALL): (4, 1, (12, 20), 3, (3, 4)),
    ('sched', LARGE): (8, 8, (128, 128), 1, (3, 3)),
    # the forced paths: the smallest shapes the split and the FFT family take
    ('split', SMALL): (2, 1, (12, 20), 3, (3, 4)),
    ('split', LARGE): (2, 1, (12, 20), 40, (3, 4)),
    ('fft', SMALL): (2, 1, (20, 22), 3, (5, 4)),
    ('fft', LARGE): (20, 1, (100, 120), 2, (5, 4)),
}
BETA = 1.
# kind -> (entry point, families, dtypes, paths it may run under)
DIRECT = ('generic', 'auto')
KINDS = {
    'energy': ('tnmf_hip_energy', ('2d', '1d', '3d', 'fft'), 'fd', DIRECT + ('fft', 'hybrid')),
    'grad_W': ('tnmf_hip_grad_W_fused', ('2d', '1d', '3d', 'fft'), 'fd', DIRECT + ('fft', 'hybrid')),
    'update_H': ('tnmf_hip_update_H', ('2d', '1d', '3d', 'split', 'fft'), 'fd', DIRECT + ('split', 'fft', 'hybrid')),
    'reconstruct': ('tnmf_hip_reconstruct', ('fft',), 'fd', ('hybrid', 'fft')),
    'grad_H': ('tnmf_hip_grad_H', ('2d', '3d'), 'fd', ('generic',)),
    'grad_W_unfused': ('tnmf_hip_grad_W', ('2d', '3d'), 'fd', ('generic',)),
    'energy_beta': ('tnmf_hip_energy_beta', ('2d',), 'fd', ('generic',)),
    'energy_weighted': ('tnmf_hip_energy_weighted', ('2d',), 'fd', ('generic',)),
    'update_H_weighted': ('tnmf_hip_update_H_weighted', ('2d',), 'fd', ('generic',)),
    'grad_W_weighted': ('tnmf_hip_grad_W_weighted', ('2d',), 'fd', ('generic',)),
    'lateral': ('tnmf_hip_update_H_ex', ('2d', '3d'), 'fd', ('generic',)),
    'lateral_fallback': ('tnmf_hip_update_H_ex', ('2d',), 'f', ('mfma',)),
    'modes': ('tnmf_hip_update_H_ex', ('2d', '3d'), 'fd', ('generic',)),
    'update_H_beta': ('tnmf_hip_update_H_beta', ('2d',), 'fd', ('generic',)),
    'grad_W_beta': ('tnmf_hip_grad_W_beta', ('2d',), 'fd', ('generic',)),
    'sample_objective': ('tnmf_hip_sample_objective', ('2d', '3d'), 'fd', ('generic',)),
    'atom_terms': ('tnmf_hip_atom_terms', ('2d',), 'fd', ('generic',)),
    'atom_gram': ('tnmf_hip_atom_gram', ('2d',), 'fd', ('generic',)),
    'atom_sources': ('tnmf_hip_atom_sources', ('2d',), 'fd', ('generic', 'auto')),
    'correlogram': ('tnmf_hip_activation_correlogram', ('2d', '1d'), 'fd', ('generic', 'auto')),
    'schedule': ('tnmf_hip_run_schedule', ('sched', '3d'), 'fd', DIRECT),
}
HALF_STEPS = ('update_H', 'lateral', 'lateral_fallback', 'modes', 'update_H_beta', 'update_H_weighted')
# tnmf_hip_ctx_last_path names the family of "the last primitive call": these two run kernels of their own, dispatch to
# no family and leave the name as it was -- history by definition, and no output
NO_DISPATCH = ('atom_sources', 'correlogram')
SCHEDULE_OPS = (('H', 0, 2), ('G', 0, 2, 0., 1.), ('W',), ('H', 2, 4), ('G', 2, 4, 0.2, 0.8), ('W',))
SOURCES = 2          # atom_sources: two sources of the listed planes, 'masked' output


def schedule_list(n_ops, N):
    """SCHEDULE_OPS filled up to n_ops with empty W gradients (1, 1): exact no-ops the joining does not drop."""
    head = SCHEDULE_OPS[:n_ops]
    return tuple(head) + tuple(('G', k % (N + 1), k % (N + 1), 1., 1.) for k in range(n_ops - len(head)))


def geometry_of(op):
    return GEOMETRY[(op.family, op.size)]


def all_ops():
    out = []
    for kind, (_, families, dtypes, _) in KINDS.items():
        for fam in families:
            for size in (SMALL, LARGE):
                for T in dtypes:
                    if fam == 'split' and T == 'd':
                        continue
                    out.append(Op(kind, fam, size, T))
    return tuple(out)


OPS = all_ops()


def allowed(op, path):
    """Whether the model lets `op` run under `path` as a GOOD call (walks and pairs only make good calls; the refusals are
    the `after_refusal` sequences)."""
    if path not in KINDS[op.kind][3]:
        return False
    if op.family == '3d' or op.kind in ('atom_sources', 'correlogram'):
        return True                                   # (volumes and these two never look at the path)
    if path == 'split':
        return op.family == 'split' and op.T == 'f'
    if path in ('fft', 'hybrid'):
        return op.family == 'fft'
    if path == 'mfma':
        return op.kind == 'lateral_fallback'
    if op.family in ('split', 'fft'):
        return path in ('generic', 'auto')
    return True


def lateral_plan(op, ctx, mode, terms):
    case = ld.Case(geometry_of(op), op.T, ctx.path, mode, (TAPS,) * len(geometry_of(op)[4]), STRENGTHS, 'contig', 'parabolic')
    return ld.plan(case, None, terms, ctx.cap['hw'])


def on_fft(geometry, T, path):
    """api.hip: use_fft_hybrid or path fft, for reconstruct and the W gradient."""
    if path == 'fft':
        return True
    if path == 'hybrid':
        return fd.fft_has(geometry, T)
    return path == 'auto' and fd.use_fft_under_auto(geometry, T)


def use_split(geometry, T, ctx):
    """api.hip: use_split."""
    if T != 'f' or len(geometry[4]) == 3:
        return False
    if ctx.path == 'split':
        return spd.split_has_corr_W(geometry)
    if ctx.path == 'auto':
        return bool(ctx.split) and spd.use_split_under_auto(geometry)
    if ctx.path == 'hybrid':
        return bool(ctx.split) and spd.split_has_corr_W(geometry, True)
    return False


def _reconstruct(ctx, geometry, T):
    if geometry[0] > 0 and on_fft(geometry, T, ctx.path):
        ctx.use('fft.ws', 'fft.ws', fft_ws_bytes(geometry, T, ctx.path, False), T)


def _corr_W(ctx, geometry, T):
    if ctx.path == 'fft':
        ctx.use('fft.ws', 'fft.ws', fft_ws_bytes(geometry, T, ctx.path, True), T)
    elif use_split(geometry, T, ctx):
        ctx.use('wimg', 'wimg', wimg_bytes(geometry), T)


def _plan(ctx, geometry, T):
    ctx.use('ws', 'ws:plan', plan_scratch(geometry, T, ctx.cus)['total'], T)


def _tap(ctx, geometry, T):
    """api.hip: tap_objective -- the partial sums of the tapped half step go through ctx->ob (samples of more than one block)."""
    ctx.tapped_now = False
    if ctx.tap:
        ctx.seen.add('tap_set')
        ctx.use('ob', 'ob:objective', objective_bytes(geometry), T)
        ctx.tapped_now = objective_bytes(geometry) > 0


def call(ctx, op, n_ops=None):
    """One good call of `op` on the model -> return code (always E_OK: see allowed())."""
    assert allowed(op, ctx.path), (op, ctx.path)
    geometry, T = geometry_of(op), op.T
    vol = op.family == '3d'
    kind = op.kind
    tapped_before, beta_before = ctx.tapped_last, ctx.beta_last
    if ctx.refused_last:
        ctx.seen.add('after_refusal')
        ctx.refused_last = False
    before = ctx.grew
    ob_before = ctx.last['ob']
    if vol:
        if kind in ('energy', 'grad_W', 'grad_W_unfused', 'grad_H', 'update_H', 'sample_objective'):
            ctx.use('ws', 'ws:vol', vol_scratch_bytes(geometry, T, ctx.cus), T)
        if kind == 'update_H':
            _tap(ctx, geometry, T)
        if kind == 'sample_objective':
            ctx.use('ob', 'ob:objective', objective_bytes(geometry), T)
        if kind in ('lateral', 'modes'):
            ctx.use('hw', 'hw:vol', vol_hw_bytes(geometry, T, 'circular' if kind == 'modes' else 'valid', kind == 'lateral'), T)
            ctx.use('ws', 'ws:vol', vol_scratch_bytes(geometry, T, ctx.cus), T)
            _tap(ctx, geometry, T)
        if kind == 'schedule':
            N, C, D, M, A = geometry
            extra = align_up(2 * M * C * prod(A) * ESIZE[T], 256)
            ctx.use('ws', 'ws:vol_sched', vol_scratch_bytes((2, C, D, M, A), T, ctx.cus, extra), T)
    elif kind == 'reconstruct':
        _reconstruct(ctx, geometry, T)
    elif kind == 'grad_H':
        _plan(ctx, geometry, T)
        _reconstruct(ctx, geometry, T)
        _corr_W(ctx, geometry, T)
    elif kind in ('energy', 'energy_beta', 'energy_weighted', 'grad_W', 'grad_W_unfused', 'grad_W_beta', 'grad_W_weighted'):
        _plan(ctx, geometry, T)
        _reconstruct(ctx, geometry, T)
        if kind in ('grad_W_beta', 'grad_W_weighted'):
            if ctx.cap['qb'] and qb_bytes(geometry, T) > ctx.cap['qb']:
                ctx.seen.add('qb_regrow')
            ctx.use('qb', 'qb:Q', qb_bytes(geometry, T), T)
        if kind in ('grad_W', 'grad_W_unfused') and on_fft(geometry, T, ctx.path):
            ctx.use('fft.ws', 'fft.ws', fft_ws_bytes(geometry, T, ctx.path, False), T)
    elif kind in ('update_H', 'update_H_beta', 'update_H_weighted'):
        _plan(ctx, geometry, T)
        _reconstruct(ctx, geometry, T)
        _tap(ctx, geometry, T)
        if kind != 'update_H':
            if ctx.cap['qb'] and qb_bytes(geometry, T) > ctx.cap['qb']:
                ctx.seen.add('qb_regrow')
            ctx.use('qb', 'qb:Q', qb_bytes(geometry, T), T)
        _corr_W(ctx, geometry, T)
    elif kind in ('lateral', 'lateral_fallback'):
        p = lateral_plan(op, ctx, 'valid', 'both')
        assert p.route == ('epilogue' if kind == 'lateral' else 'fallback'), (op, p.route, p.error, p.why)
        _plan(ctx, geometry, T)
        N, C, D, M, A = geometry
        nE = align_up(N * M * prod(shift_shape(geometry)) * ESIZE[T], 256)
        if p.route == 'epilogue':
            ctx.use('hw', 'hw:E', nE, T)
            _tap(ctx, geometry, T)
        else:
            # E goes in first (ensure_hwork(nE)); the family then refuses the extra term, and the buffer is asked for
            # [E | neg | pos]: when that grows it, E is computed a second time
            ctx.ensure('hw', nE)
            _tap(ctx, geometry, T)
            ctx.seen.add('lateral_fallback_regrow' if ctx.cap['hw'] < 3 * nE else 'lateral_fallback_no_regrow')
            assert (ctx.cap['hw'] < 3 * nE) == p.regrow
            ctx.use('hw', 'hw:E_neg_pos', 3 * nE, T)
        assert ctx.cap['hw'] == p.hw_bytes, (op, ctx.cap['hw'], p.hw_bytes)
    elif kind == 'modes':
        p = lateral_plan(op, ctx, 'circular', 'both')
        assert p.route == 'modes', (op, p)
        _plan(ctx, geometry, T)
        N, C, D, M, A = geometry
        nP = align_up(N * M * prod(shift_shape(geometry)) * ESIZE[T], 256)
        nE = align_up(N * M * prod(D) * ESIZE[T], 256)
        ctx.use('hw', 'hw:modes', 3 * nP + nE, T)
        _tap(ctx, geometry, T)
        assert ctx.cap['hw'] == p.hw_bytes, (op, ctx.cap['hw'], p.hw_bytes)
    elif kind == 'sample_objective':
        _plan(ctx, geometry, T)
        _reconstruct(ctx, geometry, T)
        ctx.use('ob', 'ob:objective', objective_bytes(geometry), T)
    elif kind in ('atom_terms', 'atom_gram'):
        ctx.use('ob', 'ob:' + kind, (atom_terms_bytes if kind == 'atom_terms' else atom_gram_bytes)(geometry, T), T)
        _plan(ctx, geometry, T)
        _reconstruct(ctx, geometry, T)
    elif kind == 'atom_sources':
        ctx.use('ob', 'ob:sources', sources_bytes(geometry, T, SOURCES, 'masked'), T)
    elif kind == 'correlogram':
        ctx.use('ob', 'ob:correlogram', correlogram_bytes(geometry, T), T)
    elif kind == 'schedule':
        n = len(SCHEDULE_OPS) if n_ops is None else n_ops
        joined = len(sd.join(list(schedule_list(n, geometry[0]))))
        route = sd.route(geometry, T, ctx.path, ctx.persistent, joined)
        if route == 'persistent':
            ctx.use('ws', 'ws:sched_persistent', sched_persistent_bytes(geometry, T, ctx.cus, joined), T)
            slot = ctx.ring_next
            ctx.ring_next = (slot + 1) % sd.K_OP_SLOTS
            need = joined * sd.OP_BYTES
            if ctx.ring_used[slot]:
                ctx.seen.add('ring_wrap')
            if ctx.ring_cap[slot] < need:
                if ctx.ring_cap[slot]:
                    ctx.seen.add('ring_slot_regrow')
                ctx.ring_cap[slot] = align_up(need, sd.SLOT_GROWTH)
            ctx.ring_used[slot] = True
        else:
            ctx.use('ws', 'ws:sched_ops', sched_ops_bytes(geometry, T, ctx.cus, 2), T)
            for _ in range(2):
                _reconstruct(ctx, (2,) + tuple(geometry[1:]), T)
                _corr_W(ctx, (2,) + tuple(geometry[1:]), T)
    else:
        raise KeyError(kind)
    half_step = kind in HALF_STEPS
    # what a tapped half step left in ctx->ob waits there until the next user of the buffer
    ctx.tapped_last = ctx.tapped_now if half_step and ctx.tap else (tapped_before and ctx.last['ob'] is ob_before)
    ctx.tapped_now = False
    if half_step and not ctx.tap and ctx.tap_was_set:
        ctx.seen.add('tap_cleared')          # a half step on a context whose tap was set and has been taken away again
        ctx.tap_was_set = False
    is_beta = kind in ('update_H_beta', 'grad_W_beta', 'update_H_weighted', 'grad_W_weighted')    # (the callers of beta_fields_of)
    frobenius = ('update_H', 'grad_W', 'grad_W_unfused', 'grad_H', 'energy', 'lateral', 'modes', 'schedule', 'lateral_fallback')
    if beta_before and kind in frobenius:
        ctx.seen.add('beta_then_frobenius')
    if is_beta or kind in frobenius:
        ctx.beta_last = is_beta
    if ctx.reserved:
        ctx.seen.add('reserved_first' if ctx.grew == before else 'reserved_too_small')
    return E_OK


# ---- refusals by a documented argument check (include/tnmf_hip.h); nothing is written, nothing of the context changes --------
REFUSALS = {
    'correlogram_lag_beyond_limit': ('tnmf_hip_activation_correlogram', E_UNSUPPORTED, 'generic'),
    'atom_terms_group_not_dividing_M': ('tnmf_hip_atom_terms', E_GEOM, 'generic'),
    'atom_terms_of_a_volume': ('tnmf_hip_atom_terms', E_UNSUPPORTED, 'generic'),
    'update_H_mfma_row_padded': ('tnmf_hip_update_H', E_STRIDE, 'mfma'),
}


def control(ctx, c):
    """set_path / set_split / set_persistent / tap / reserve / refuse on the model -> return code."""
    if c.what == 'set_path':
        if c.value != ctx.path:
            ctx.seen.add('path_flip(-> %s)' % c.value)
        ctx.path = c.value
    elif c.what == 'set_split':
        ctx.split = c.value
    elif c.what == 'set_persistent':
        ctx.persistent = c.value
    elif c.what == 'tap':
        ctx.tap = bool(c.value)
        ctx.tap_was_set = ctx.tap_was_set or ctx.tap
    elif c.what == 'reserve':
        # tnmf_hip_ctx_reserve sizes ws only (and the FFT workspace under the paths that take it): a reservation that
        # keeps EVERY buffer from growing is made of calls as well: the large form of every op (the `reserved_first` sequences)
        fam, T = c.value
        g = GEOMETRY[(fam, LARGE)]
        if fam == '3d':
            ctx.use('ws', 'ws:vol', vol_scratch_bytes(g, T, ctx.cus), T)
        else:
            if ctx.path == 'fft' or on_fft(g, T, ctx.path):
                ctx.use('fft.ws', 'fft.ws', fft_ws_bytes(g, T, ctx.path, ctx.path == 'fft'), T)
            _plan(ctx, g, T)
    elif c.what == 'refuse':
        assert REFUSALS[c.value][2] == ctx.path, (c, ctx.path)
        ctx.refused_last = True
        return REFUSALS[c.value][1]
    elif c.what == 'mark_reserved':
        ctx.reserved = True
    else:
        raise KeyError(c.what)
    return E_OK


def step(ctx, item):
    if isinstance(item, Ctl):
        return control(ctx, item)
    if isinstance(item, tuple) and item and item[0] == 'schedule_n':
        return call(ctx, item[1], item[2])
    return call(ctx, item)


def uses_of(op, cus, path=None, persistent=1):
    """{buffer: Use} of `op` on a fresh context."""
    ctx = Context(cus)
    ctx.path, ctx.persistent = path or default_path(op), persistent
    call(ctx, op)
    return {b: u for b, u in ctx.last.items() if u is not None}, ctx


def default_path(op):
    return KINDS[op.kind][3][0] if op.family not in ('split', 'fft') else {'split': 'split', 'fft': 'hybrid'}[op.family]


# ---- the transitions -------------------------------------------------------------------------------------------------------
def layouts_reached(cus=256):
    """{buffer: [layouts some op of OPS gives it]}."""
    out = {}
    for op in OPS:
        for p in KINDS[op.kind][3]:
            if allowed(op, p):
                ctx = Context(cus)
                ctx.path = p
                ctx.persistent = 1
                call(ctx, op)
                for b, u in ctx.last.items():
                    if u is not None and u.layout not in out.setdefault(b, []):
                        out[b].append(u.layout)
    # the per-operation schedule: persistent off
    if 'ws:sched_ops' not in out['ws']:
        out['ws'].append('ws:sched_ops')
    return out


def _pairs_of_layouts():
    out = []
    for b, lays in sorted(layouts_reached().items()):
        for a in lays:
            for c in lays:
                if a != c:
                    out.append(f'dirty({b}: {a.split(":")[-1]} -> {c.split(":")[-1]})')
    return out


NOT_REACHED = {
    'hipMalloc_refused': 'ensure_buffer / ensure_ws / the W images answering TNMF_E_WORKSPACE (failed_bytes): needs a device '
                         'without room for a few MiB; nobody fills a shared device to get there',
    'persistent_refused_falls_through': 'api.hip: generic_run_schedule answers TNMF_E_UNSUPPORTED when the occupancy query or the '
                                        'cooperative launch refuses the grid; on a device that is not otherwise occupied it '
                                        'never does, and occupying it on purpose is provoking',
}


def transitions():
    out = []
    for b in BUFFERS:
        out += [f'first_allocation({b})', f'reuse_fits({b})', f'regrow({b})']
    out += _pairs_of_layouts()
    out += [f'dtype_flip({b})' for b in BUFFERS if b != 'wimg']       # (the split family is float32 only)
    out += ['path_flip(-> %s)' % p for p in PATHS]
    out += ['lateral_fallback_regrow', 'lateral_fallback_no_regrow', 'tap_set', 'tap_cleared', 'tap_then_ob_user',
            'beta_then_frobenius', 'qb_regrow', 'ring_wrap', 'ring_slot_regrow', 'after_refusal', 'reserved_first',
            'two_contexts_interleaved']
    return tuple(out)


TRANSITIONS = transitions()
# outputs that legitimately depend on the context's history: op kind -> the source line that makes it so.  None found.
HISTORY_DEPENDENT = {}


# ---- the sequences ---------------------------------------------------------------------------------------------------------
# A sequence is a tuple of items: Op, Ctl, ('schedule_n', Op, n_ops), or ('other', item) -- the item on the SECOND context of
# the sequence (two_contexts_interleaved).  Every Op but the last of a pair is a predecessor: it runs on other operands.
Sequence = namedtuple('Sequence', 'kind items why')


def _cfg(path, persistent=1, tap=0):
    return (Ctl('set_path', path), Ctl('set_persistent', persistent), Ctl('tap', tap))


@functools.lru_cache(maxsize=None)
def _op_with(buffer, layout, size, T, cus=256):
    """(op, path, persistent) whose fresh call lays `buffer` out as `layout`."""
    for persistent in (1, 0):
        for op in OPS:
            if op.size != size or op.T != T:
                continue
            for p in KINDS[op.kind][3]:
                if not allowed(op, p):
                    continue
                ctx = Context(cus)
                ctx.path, ctx.persistent = p, persistent
                call(ctx, op)
                u = ctx.last[buffer]
                if u is not None and u.layout == layout:
                    return op, p, persistent
    return None


def pair_sequences():
    out = {}
    lays = layouts_reached()
    for b in BUFFERS:
        for i, T in enumerate('fd'):
            if b == 'wimg' and T == 'd':
                continue
            # regrow: the SMALL form, then the LARGE form of the first op whose large extent outgrows what the small one leaves
            found = None
            for op in OPS:
                if found or op.size != SMALL or op.T != T:
                    continue
                for p in KINDS[op.kind][3]:
                    if not allowed(op, p):
                        continue
                    us, ul = uses_of(op, 256, p)[0], uses_of(op._replace(size=LARGE), 256, p)[0]
                    if b in us and b in ul:
                        cap = ensure_buffer(0, us[b].extent, b == 'ws') if b != 'wimg' else us[b].extent
                        if ul[b].extent > cap:
                            found = Sequence('pair', _cfg(p) + (op, op._replace(size=LARGE)),
                                             f'{us[b].layout}: {us[b].extent} bytes leave {cap}, then {ul[b].extent}')
                            break
            if found:
                out[f'regrow({b})[{T}]'] = found
        for a in lays.get(b, []):
            for c in lays.get(b, []):
                if a == c:
                    continue
                for T in 'fd':
                    A, B = _op_with(b, a, LARGE, T), _op_with(b, c, SMALL, T) or _op_with(b, c, LARGE, T)
                    if not A or not B:
                        continue
                    name = f'dirty({b}: {a.split(":")[-1]} -> {c.split(":")[-1]})[{T}]'
                    items = _cfg(A[1], A[2]) + (A[0],) + _cfg(B[1], B[2]) + (B[0],)
                    why = f'{A[0].kind} leaves {a}, {B[0].kind} lays out {c}'
                    if uses_of(A[0], 256, A[1], A[2])[0][b].extent < uses_of(B[0], 256, B[1], B[2])[0][b].extent:
                        # a layout of a few KiB in front of a larger one: the bytes beyond it are written first, by the
                        # largest user the buffer has
                        F = _largest(b, T)
                        items = _cfg(F[1], F[2]) + (F[0],) + items
                        why = f'{F[0].kind} fills the buffer; ' + why
                    out[name] = Sequence('pair', items, why)
    return out


@functools.lru_cache(maxsize=None)
def _largest(buffer, T, cus=256):
    best = None
    for op in OPS:
        if op.size == LARGE and op.T == T:
            for p in KINDS[op.kind][3]:
                if allowed(op, p):
                    u = uses_of(op, cus, p)[0].get(buffer)
                    if u is not None and (best is None or u.extent > best[0]):
                        best = (u.extent, op, p)
    return best[1], best[2], 1


def _o(kind, family='2d', size=SMALL, T='f'):
    op = Op(kind, family, size, T)
    assert op in OPS, op
    return op


def special_sequences():
    out = {}
    for T in 'fd':
        O = lambda kind, family='2d', size=SMALL: _o(kind, family, size, T)   # noqa: E731
        U = 'f' if T == 'd' else 'd'
        # f32 -> f64 -> f32 (or the other way round) of one entry point, on every buffer with two dtypes
        out[f'dtype_flip[{T}]'] = Sequence('special', _cfg('generic') + tuple(
            x for kind, fam in (('grad_W', '2d'), ('modes', '2d'), ('update_H_beta', '2d'), ('atom_gram', '2d'))
            for x in (_o(kind, fam, SMALL, T), _o(kind, fam, SMALL, U), _o(kind, fam, SMALL, T)))
            + _cfg('hybrid') + (_o('grad_W', 'fft', SMALL, T), _o('grad_W', 'fft', SMALL, U), _o('grad_W', 'fft', SMALL, T)),
            'the same entry point in the other element type and back, per buffer')
        out[f'path_flip[{T}]'] = Sequence('special', _cfg('generic') + (O('update_H'),) + (
            (Ctl('set_path', 'split'), _o('update_H', 'split', SMALL, 'f'), _o('update_H', 'split', LARGE, 'f'),
             _o('update_H', 'split', SMALL, 'f')) if T == 'f' else (Ctl('set_path', 'split'),))
            + ((Ctl('set_path', 'mfma'), _o('lateral_fallback', '2d', SMALL, 'f')) if T == 'f' else (Ctl('set_path', 'mfma'),))
            + (Ctl('set_path', 'hybrid'), O('grad_W', 'fft'), O('update_H', 'fft'), Ctl('set_path', 'fft'), O('grad_W', 'fft'),
               O('update_H', 'fft'), O('update_H', 'fft', LARGE), O('grad_W', 'fft'), Ctl('set_path', 'generic'),
               O('update_H', 'fft'), Ctl('set_path', 'auto'), O('update_H'), O('grad_W', 'fft', LARGE), O('energy')),
            'generic -> split (the first W images, then larger ones) -> mfma -> hybrid and fft (the first FFT workspace, then '
            'its window buffers, then a larger one) -> generic -> auto')
        out[f'tap[{T}]'] = Sequence('special', _cfg('generic') + (
            O('update_H', '2d', LARGE), Ctl('tap', 1), O('update_H', '2d', LARGE), O('atom_gram'), O('lateral', '2d', LARGE),
            O('correlogram'), O('modes', '2d', LARGE), O('atom_terms'), O('update_H_beta', '2d', LARGE), O('atom_sources'),
            O('update_H', '3d', LARGE), O('sample_objective', '2d', LARGE), Ctl('tap', 0), O('update_H', '2d', LARGE), O('update_H')),
            'the tap set on a used context, every tapped half step followed by another user of ctx->ob, then cleared')
        out[f'beta_then_frobenius[{T}]'] = Sequence('special', _cfg('generic') + (
            O('update_H_beta'), O('update_H'), O('grad_W_beta'), O('grad_W'), O('update_H_beta', '2d', LARGE), O('energy'),
            O('update_H_beta'), O('grad_W_beta', '2d', LARGE), O('grad_W', '2d', LARGE)),
            'Q (and V_volatile) left behind by a beta step; the field grows once')
        out[f'ring[{T}]'] = Sequence('ring', _cfg('generic') + tuple(
            x for n, other in zip((3, 5, 6, 130, 6, 200, 260, 4),
                                  (O('grad_W'), O('energy', '2d', LARGE), O('energy', '3d'), O('update_H'), O('grad_W', '2d', LARGE),
                                   O('atom_terms'), O('energy'), O('grad_W', '3d')))
            for x in (('schedule_n', O('schedule', 'sched'), n), other)),
            'eight persistent schedules with lists of 3 to 260 operations, other users of ctx->ws between them')
        out[f'ring_per_op[{T}]'] = Sequence('ring', _cfg('generic', 0) + (
            O('schedule', 'sched'), O('energy'), Ctl('set_persistent', 1), O('schedule', 'sched'), O('schedule', 'sched', LARGE),
            Ctl('set_persistent', 0), O('schedule', 'sched'), O('schedule', 'sched', LARGE), O('schedule', '3d'), O('grad_W'),
            Ctl('set_persistent', 2), O('schedule', 'sched')),
            'the per-operation walk, the persistent kernel (plain and cooperative) and the volume walk in turn')
        out[f'lateral_fallback[{T}]'] = Sequence('special', _cfg('mfma') + (
            _o('lateral_fallback', '2d', SMALL, 'f'), _o('lateral_fallback', '2d', LARGE, 'f'), _o('lateral_fallback', '2d', LARGE, 'f'),
            Ctl('set_path', 'generic'), O('modes', '2d', LARGE), Ctl('set_path', 'mfma'), _o('lateral_fallback', '2d', LARGE, 'f')),
            'both sides of `if (ctx->hw_bytes < nE + 2 * nG)`: a fresh buffer (E computed twice), a buffer the call before or '
            'the reconstruction modes left large enough')
        out[f'after_refusal[{T}]'] = Sequence('special', _cfg('generic') + (
            O('correlogram'), Ctl('refuse', 'correlogram_lag_beyond_limit'), O('correlogram'),
            O('atom_terms'), Ctl('refuse', 'atom_terms_group_not_dividing_M'), O('atom_terms'),
            Ctl('refuse', 'atom_terms_of_a_volume'), O('atom_gram'))
            + ((Ctl('set_path', 'mfma'), _o('lateral_fallback', '2d', SMALL, 'f'), Ctl('refuse', 'update_H_mfma_row_padded'),
                _o('lateral_fallback', '2d', SMALL, 'f')) if T == 'f' else ()),
            'a call refused by an argument check between two good ones')
        reserve = tuple(op for op in OPS if op.size == LARGE and op.T == T and allowed(op, 'generic')
                        and op.family in ('2d', '1d', '3d', 'sched'))
        out[f'reserved_first[{T}]'] = Sequence('special', _cfg('generic') + tuple(
            Ctl('reserve', (fam, T)) for fam in ('2d', '1d', '3d')) + reserve + (Ctl('mark_reserved', 1),) + tuple(
            op._replace(size=SMALL) for op in reserve) + reserve[:6],
            'tnmf_hip_ctx_reserve for the large problems and one call of each large op; after that nothing grows')
        out[f'two_contexts[{T}]'] = Sequence('special', _cfg('generic') + tuple(('other', c) for c in _cfg('generic')) + (
            O('grad_W', '2d', LARGE), ('other', O('grad_W')), O('grad_W'), ('other', O('atom_gram', '2d', LARGE)), O('atom_gram'),
            ('other', O('modes', '2d', LARGE)), O('modes'), ('other', ('schedule_n', O('schedule', 'sched'), 6)),
            ('schedule_n', O('schedule', 'sched'), 6), ('other', O('update_H_beta')), O('update_H_beta', '2d', LARGE),
            ('other', O('energy', '3d', LARGE)), O('energy', '3d')),
            'two contexts of one device take turns')
    return out


WALK_SEEDS = tuple(range(16))
WALK_LENGTH = 40


def _any_op_with(buffer, layout, size, T):
    return _op_with(buffer, layout, size, T) or _op_with(buffer, layout, size, 'f' if T == 'd' else 'd') or \
        _op_with(buffer, layout, LARGE, T) or _op_with(buffer, layout, LARGE, 'f')


def walk(seed):
    """About WALK_LENGTH calls over all of OPS with the switches thrown in between, none of them refused.  Every pair of
    layouts is dealt to two of the walks, which meet their pairs in a shuffled order with drawn sizes; between two pairs
    come drawn calls (the KIND first, so that the few ops of the work buffers meet as often as the many of ctx->ws) and
    drawn switches: the orders nobody thought of."""
    rng = random.Random(1000 + seed)
    T = 'fd'[seed % 2]
    n = len(WALK_SEEDS)
    pairs = [t for k, t in enumerate(t for t in TRANSITIONS if t.startswith('dirty(')) if seed in (k % n, (k * 7 + 3) % n)]
    rng.shuffle(pairs)
    state = {'path': 'generic'}
    items = list(_cfg('generic'))
    paths = ('generic',) * 5 + ('auto', 'hybrid', 'fft') + (('split', 'mfma') if T == 'f' else ())

    def drawn():
        r = rng.random()
        if r < 0.15:
            state['path'] = rng.choice(paths)
            return [Ctl('set_path', state['path'])]
        if r < 0.22:
            return [Ctl('set_persistent', rng.choice((0, 1, 2)))]
        if r < 0.26:
            return [Ctl('set_split', rng.choice((0, 1)))]
        if r < 0.34:
            return [Ctl('tap', rng.choice((0, 1)))]
        mixed = rng.random() < 0.15                     # now and then the other element type
        ok = [op for op in OPS if allowed(op, state['path']) and ((op.T == T) != mixed or op.kind == 'lateral_fallback')]
        kind = rng.choice(sorted({op.kind for op in ok}))
        ok = [op for op in ok if op.kind == kind]
        fam = rng.choice(sorted({op.family for op in ok}))
        ok = [op for op in ok if op.family == fam]
        small = [op for op in ok if op.size == SMALL]
        return [rng.choice(small if small and rng.random() < 0.6 else ok)]

    for t in pairs:
        buffer, rest = t[len('dirty('):-1].split(': ')
        a, b = (x if buffer in ('wimg', 'fft.ws') else f'{buffer}:{x}' for x in rest.split(' -> '))
        A = _any_op_with(buffer, a, rng.choice((SMALL, LARGE)), T)
        B = _any_op_with(buffer, b, rng.choice((SMALL, LARGE)), T)
        items += [Ctl('set_path', A[1]), Ctl('set_persistent', A[2]), A[0], Ctl('set_path', B[1]), Ctl('set_persistent', B[2]), B[0]]
        state['path'] = B[1]
        for _ in range(rng.choice((0, 1, 2, 3))):
            items += drawn()
    while sum(isinstance(x, Op) for x in items) < WALK_LENGTH:
        items += drawn()
    return Sequence('walk', tuple(items), f'seed {seed}')


def _sequences():
    out = dict(pair_sequences())
    out.update(special_sequences())
    out.update({f'walk[{s}]': walk(s) for s in WALK_SEEDS})
    return out


SEQUENCES = _sequences()


def run(seq, cus=256):
    """The model's account of a sequence -> ([(return code, transitions seen so far)] per item, the two contexts)."""
    ctxs = {False: Context(cus, 'first'), True: Context(cus, 'second')}
    out, turns = [], []
    for item in seq.items:
        other = isinstance(item, tuple) and item and item[0] == 'other'
        ctx = ctxs[other]
        rc = step(ctx, item[1] if other else item)
        if not isinstance(item[1] if other else item, Ctl):
            turns.append(other)
        if len(set(turns)) == 2 and any(a != b for a, b in zip(turns, turns[1:])):
            ctxs[False].seen.add('two_contexts_interleaved')
        out.append((rc, frozenset(ctxs[False].seen | ctxs[True].seen)))
    return out, ctxs


def reached(seq, cus=256):
    return set(run(seq, cus)[0][-1][1]) & set(TRANSITIONS)


def reached_by(sequences=None, cus=256):
    sequences = SEQUENCES if sequences is None else sequences
    got = {}
    for name, seq in sequences.items():
        for t in reached(seq, cus):
            got.setdefault(t, []).append(name)
    return got


def missing(sequences=None, cus=256):
    got = reached_by(sequences, cus)
    return sorted(t for t in TRANSITIONS if t not in got)


def base_of(name):
    return name.split('[')[0]


def sole_carriers(sequences=None, cus=256):
    """{base name of a sequence: [transitions only its variants carry]}."""
    out = {}
    for t, names in reached_by(sequences, cus).items():
        bases = {base_of(n) for n in names}
        if len(bases) == 1:
            out.setdefault(bases.pop(), []).append(t)
    return out


SMALL_FFT_WS = 3 * MiB      # the smallest workspace of the FFT family (transform length 32 on both axes): 1.2 MiB, float64 2.4


def check_sizes(cus):
    """SMALL fits in 1 MiB in every buffer; LARGE needs more than the capacity SMALL leaves wherever the same op lays the
    buffer out in both sizes -- or the pair is listed in SAME_STEP with its reason; nothing beyond the tens of MiB.
    -> [(op, buffer, small extent, capacity, large extent)]."""
    rows = []
    for op in OPS:
        if op.size != SMALL:
            continue
        for p in KINDS[op.kind][3]:
            if not allowed(op, p):
                continue
            us, _ = uses_of(op, cus, p)
            ul, _ = uses_of(op._replace(size=LARGE), cus, p)
            for b, u in us.items():
                assert u.extent <= (SMALL_FFT_WS if b == 'fft.ws' else MiB), (op, b, u.extent)
                cap = ensure_buffer(0, u.extent, b == 'ws') if b != 'wimg' else u.extent
                assert ul[b].extent < 64 * MiB, (op, b, ul[b].extent)
                assert ul[b].extent > cap or (op.kind, op.family, b) in SAME_STEP, (op, p, b, u.extent, cap, ul[b].extent)
                rows.append((op, p, b, u.extent, cap, ul[b].extent))
    return rows


# (kind, family, buffer): why the LARGE form does not outgrow what SMALL leaves, at any size a test should run.  The buffer's
# own `regrow` is carried by another op (ob: the correlogram; ws: every other family; wimg: the split family's own pair).
_OBJ = 'N * cdiv(L, 4096) doubles: a MiB needs 5 * 10^8 sample elements'
_SPLIT = 'the large form of the split family is large in its atoms (the W images), not in its samples'
SAME_STEP = {
    ('atom_sources', '2d', 'ob'): 'taps and two tables of M and S + 2 ints: a MiB of taps is a dictionary of 10^5 atom rows',
    ('atom_terms', '2d', 'ob'): '16 bytes per (sample, tile of 1024 pixels, atom): a MiB is 65536 of them, with a float64 '
                                'reference of all parts behind every one',
    ('atom_gram', '2d', 'ob'): '2176 bytes per (sample, strip of 16 tiles, pair of atom blocks): a MiB needs 33 atoms on 100 '
                               'tiles, and the float64 reference holds every part of every atom',
    ('sample_objective', '2d', 'ob'): _OBJ, ('sample_objective', '3d', 'ob'): _OBJ,
    ('update_H', '2d', 'ob'): _OBJ, ('update_H', '1d', 'ob'): _OBJ, ('update_H', '3d', 'ob'): _OBJ, ('update_H', 'fft', 'ob'): _OBJ,
    ('update_H_beta', '2d', 'ob'): _OBJ, ('lateral', '2d', 'ob'): _OBJ, ('lateral', '3d', 'ob'): _OBJ, ('modes', '2d', 'ob'): _OBJ,
    ('modes', '3d', 'ob'): _OBJ, ('lateral_fallback', '2d', 'ob'): _OBJ,
    ('update_H', 'split', 'ws'): _SPLIT,
    ('update_H', 'fft', 'wimg'): 'cdiv(M, 32) * C images: three atoms or four, one image',
}

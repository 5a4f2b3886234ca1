"""
Host model of the FFT family's spectrum cache: FftState (tnmf_amd/csrc/common.h) and every place of fft.hip / api.hip that
changes it, restated in plain Python, so that a CPU test can check that a list of short call sequences carries every
transition (tests/test_cache_dispatch_cpu.py) and a GPU test can hold the library to the model call by call at the C ABI
(tests/test_hip_cache_matrix.py).  A change to which call leaves which spectra behind starts HERE: change the model, and the
two tests name every consequence.

The model is the contract of include/tnmf_hip.h (tnmf_hip_ctx_set_cache ... tnmf_hip_ctx_cache_counters), not a transcript
of the code: where the two differ the library is wrong (see the two `layout_*` sequences).

A pointer is (buffer name, byte offset).  Two buffers are separate allocations: a pointer into one is never a whole number
of samples into a binding of the other *within the binding's sample count* (the binding's own buffer covers that range).

Sizes and offsets of the workspace come from fft_dispatch.make_layout; nothing about them is restated here.
"""
from collections import namedtuple

import fft_dispatch as fd

E_OK, E_UNSUPPORTED = 0, -5                               # include/tnmf_hip.h:37-43
PATHS = ('auto', 'generic', 'mfma', 'fft', 'hybrid', 'split')   # TNMF_PATH_* in enum order
ESIZE = {'f': 4, 'd': 8}
H_ROWS, H_COLS, V_ROWS, V_COLS, W_SPEC = 'rows of H', 'columns of H', 'rows of V', 'columns of V', 'W spectra'

# (hs: row stride of H in elements, 0 = the shift width)
Geo = namedtuple('Geo', 'N C D M A hs')


def geometry(g):
    return (g.N, g.C, g.D, g.M, g.A)


def shift(g):
    return tuple(d + a - 1 for d, a in zip(g.D, g.A))


def stride(g):
    return g.hs or shift(g)[-1]


def h_bytes(g, dtype):
    """bytes of one sample of H (fft.hip:366)."""
    return g.M * shift(g)[0] * stride(g) * ESIZE[dtype]


def v_bytes(g, dtype):
    return g.C * g.D[0] * g.D[1] * ESIZE[dtype]


def same_shape(a, b):
    """fft.hip:337-339: everything but N."""
    return (a.M, a.C, a.D, a.A, stride(a)) == (b.M, b.C, b.D, b.A, stride(b))


Slot = namedtuple('Slot', 'n0 cached v_cached')
NOWHERE = Slot(0, False, False)


class State:
    """FftState (common.h:27-57), the path of the context (common.h:62) and the field Q's buffer (common.h:72)."""

    def __init__(self, path, defect=None):
        self.path = path
        self.defect = defect            # a WRONG_MODELS name: the right model with that one defect
        self.enabled = False
        self.bound = self.explicit = False
        self.H_base = self.V_base = None
        self.geo = None
        self.dtype = None
        self.T_ok, self.SH_ok, self.V_ok, self.SV_ok = [], [], [], []
        self.W_ok = False
        self.W_owner = self.W_geo = self.W_dtype = None
        self.W_key = None               # what names the layout the W spectra were written under: (array, byte offset)
        self.V_volatile = None
        self.qb_bytes = 0
        self.qb_gen = 0                 # ctx->qb is a new allocation every time it grows
        self.ws_bytes = 0
        self.counters = [0, 0, 0, 0]    # h_runs, h_hits, v_runs, v_hits
        # not in FftState: the row spectra of these samples were left by k_fft_rows_mu (fft_update_H), and whether a
        # call has consumed such spectra (the cached context then need not equal a fresh one to the bit any more)
        self.T_mu = []
        self.mu_consumed = False
        # ... nor this: which binding's sample slots the last transform of samples went through (generation, first slot)
        self.bind_gen = 0
        self.v_slot = None
        # the transitions (names of TRANSITIONS, and a few halves of them) the calls so far went through
        self.seen = set()
        self.after_unbind = False
        self.W_dropped_by = None        # the entry point that last took W_ok down

    def any_flag(self):
        return self.W_ok or any(self.T_ok) or any(self.V_ok)

    def has(self, defect):
        return self.defect == defect


# ---- fft.hip ----------------------------------------------------------------------------------------------------------
def clear_flags(st, by=None):
    """fft.hip:158-164."""
    if st.W_ok:
        st.W_dropped_by = by
    st.W_ok = False
    for v in (st.T_ok, st.SH_ok, st.V_ok, st.SV_ok, st.T_mu):
        v[:] = [0] * len(v)


def ensure_ws(st, nbytes):
    """fft.hip:166-201 (an allocation is never refused at test size: NOT_REACHED)."""
    if nbytes <= st.ws_bytes:
        return
    if st.any_flag():
        st.seen.add('growth_clears_flags')
    st.ws_bytes = fd.align_up(nbytes, 1 << 20)
    if not st.has('growth_keeps_flags'):
        clear_flags(st)


def bind(st, g, dtype, H, V, explicit):
    """fft.hip:341-353."""
    st.bound, st.explicit = True, explicit
    st.bind_gen += 1
    st.after_unbind = False
    st.H_base, st.V_base, st.geo, st.dtype = H, V, g, dtype
    n = max(g.N, 0)
    st.T_ok, st.SH_ok, st.V_ok, st.SV_ok, st.T_mu = [0] * n, [0] * n, [0] * n, [0] * n, [0] * n


def unbind(st):
    """fft.hip:545-553."""
    st.bound = st.explicit = False
    st.H_base = st.V_base = None
    st.T_ok, st.SH_ok, st.V_ok, st.SV_ok, st.T_mu = [], [], [], [], []


def _delta(p, base):
    """Byte distance of two pointers; None when they belong to separate allocations (see the module's docstring)."""
    if p is None or base is None or p[0] != base[0]:
        return None
    return p[1] - base[1]


def locate(st, g, dtype, H, V):
    """fft.hip:362-389."""
    if st.enabled and st.bound and g.N > 0:
        if dtype != st.dtype:
            st.seen.add('dtype_differs')
        else:
            differs = [f for f, a, b in zip(('M', 'C', 'D', 'A', 'h_row_stride'), (st.geo.M, st.geo.C, st.geo.D, st.geo.A, stride(st.geo)),
                                            (g.M, g.C, g.D, g.A, stride(g))) if a != b]
            if len(differs) == 1:
                st.seen.add('shape_differs_' + differs[0])
    if not st.enabled or not st.bound or dtype != st.dtype or not same_shape(st.geo, g) or g.N <= 0:
        return NOWHERE
    hb, vb = h_bytes(g, dtype), v_bytes(g, dtype)
    n0 = -1
    if H is not None:
        d = _delta(H, st.H_base)
        if d is not None and d < 0:
            st.seen.add('H_before_base')
        elif d is not None and d % hb:
            st.seen.add('H_not_whole_samples_in')
        if d is None or d < 0 or d % hb:
            return NOWHERE
        n0 = d // hb
    elif V is not None and st.V_base is not None:
        d = _delta(V, st.V_base)
        if d is not None and d < 0:
            st.seen.add('V_before_base')
        elif d is not None and d % vb:
            st.seen.add('V_misaligned')
        if d is None or d < 0 or d % vb:
            return NOWHERE
        n0 = d // vb
        st.seen.add('located_by_V')
    if 0 <= n0 < st.geo.N < n0 + g.N:
        st.seen.add('slice_overruns_binding')
    if n0 < 0 or (n0 + g.N > st.geo.N and not st.has('overrun_is_located')):
        return NOWHERE
    if st.explicit and g.N < st.geo.N and n0 + g.N <= st.geo.N:
        st.seen.add('explicit_slice_first' if n0 == 0 else 'explicit_slice_last' if n0 + g.N == st.geo.N else 'explicit_slice_interior')
    v_cached = False
    if V is not None:
        if st.V_base is None:           # :381-385: a binding taken without V adopts the samples
            if n0 > 0:
                st.seen.add('adopt_V_at_n0_gt_0')
            st.V_base = V if st.has('adopt_V_as_base') else (V[0], V[1] - n0 * vb)
            st.V_ok[:] = [0] * len(st.V_ok)
            st.SV_ok[:] = [0] * len(st.SV_ok)
        v_cached = _delta(V, st.V_base) == n0 * vb
    return Slot(n0, True, v_cached)


def all_ok(v, n0, n):
    return all(i < len(v) and v[i] for i in range(n0, n0 + n))


def set_ok(v, n0, n, val):
    for i in range(n0, min(n0 + n, len(v))):
        v[i] = val


Call = namedtuple('Call', 'sl lay')


def prepare(st, g, dtype, H, V, window=False):
    """fft.hip:407-436."""
    if V is not None and V == st.V_volatile:
        V = None
    if not st.enabled:
        st.seen.add('cache_off_nothing_tracked')
    sl = locate(st, g, dtype, H, V)
    if not sl.cached:
        if st.enabled and not st.explicit and (H is not None or V is not None):
            if st.bound:
                st.seen.add('foreign_under_implicit_bind')
            if st.after_unbind:
                st.seen.add('unbind_then_implicit')
            st.seen.add('implicit_bind_H_and_V' if H is not None and V is not None else
                        'implicit_bind_H_only' if H is not None else 'implicit_bind_V_only')
            bind(st, g, dtype, H, V, False)
            sl = Slot(0, H is not None, V is not None)
        else:
            if st.enabled and st.explicit:
                st.seen.add('foreign_under_explicit_bind')
            if not st.has('foreign_keeps_flags'):
                clear_flags(st)
    full = st.geo if (sl.cached or sl.v_cached) else g
    lay = fd.make_layout(geometry(full._replace(M=g.M, C=g.C, D=g.D, A=g.A)), dtype, st.path, n_call=g.N)
    ensure_ws(st, lay.total if window else lay.total_no_window)
    return Call(sl, lay)


def spectra_V(st, g, c, full, rec, volatile=False):
    """fft.hip:464-489."""
    n0 = c.sl.n0
    track = c.sl.v_cached and st.enabled
    hit = track and all_ok(st.V_ok, n0, g.N)
    st.counters[3 if hit else 2] += 1
    st.v_slot = (st.bind_gen, n0) if (c.sl.cached or c.sl.v_cached) else None
    if hit:
        st.seen.add('V_rows_hit')
        if full and not all_ok(st.SV_ok, n0, g.N):
            st.seen.add('V_cols_on_first_demand')
    if not track and c.sl.cached and st.enabled:
        if any(st.V_ok[n0:n0 + g.N]):
            st.seen.add('V_volatile_never_cached' if volatile else 'H_slice_with_other_V')
    if not track and c.sl.cached and not st.has('v_survives_volatile'):
        set_ok(st.V_ok, n0, g.N, 0)
        set_ok(st.SV_ok, n0, g.N, 0)
    if not hit:
        rec.add(V_ROWS)
        if track:
            set_ok(st.SV_ok, n0, g.N, 0)
            set_ok(st.V_ok, n0, g.N, 1)
    if full and not (hit and all_ok(st.SV_ok, n0, g.N)):
        rec.add(V_COLS)
        if track:
            set_ok(st.SV_ok, n0, g.N, 1)


def drop_H(st, n0, n):
    """T_ok and SH_ok go together (the full spectra are only as good as the rows they came from: fft.hip:525)."""
    if any(st.SH_ok[n0:n0 + n]):
        st.seen.add('SH_cleared_with_T')
    set_ok(st.T_ok, n0, n, 0)
    set_ok(st.T_mu, n0, n, 0)
    if not st.has('sh_survives_t'):
        set_ok(st.SH_ok, n0, n, 0)


def rows_of_H(st, g, c, rec):
    """fft.hip:492-516."""
    n0 = c.sl.n0
    track = c.sl.cached and st.enabled
    if track and all_ok(st.T_ok, n0, g.N):
        st.counters[1] += 1
        st.seen.add('H_hit')
        if any(st.T_mu[n0:n0 + g.N]):
            st.mu_consumed = True
            st.seen.add('fft_update_H_leaves_T')
        return
    if track and any(st.T_ok[n0:n0 + g.N]):
        st.seen.add('H_run_one_sample_invalid')
    st.counters[0] += 1
    rec.add(H_ROWS)
    if track:
        drop_H(st, n0, g.N)
        set_ok(st.T_ok, n0, g.N, 1)


def spectra_of_H(st, g, c, rec):
    """fft.hip:519-527."""
    rows_of_H(st, g, c, rec)
    track = c.sl.cached and st.enabled
    if track and all_ok(st.SH_ok, c.sl.n0, g.N):
        return
    rec.add(H_COLS)
    if track:
        st.seen.add('SH_only_when_resident')
        set_ok(st.SH_ok, c.sl.n0, g.N, 1)


def fft_invalidate_H(st, g, dtype, H, why='hybrid_update'):
    """fft.hip:555-565."""
    if st.has('direct_update_keeps_H'):
        return
    sl = locate(st, g, dtype, H, None)
    if sl.cached:
        if any(st.T_ok[sl.n0:sl.n0 + g.N]):
            st.seen.add(why + '_slice')
        drop_H(st, sl.n0, g.N)
    else:
        if any(st.T_ok):
            st.seen.add(why + '_all')
        drop_H(st, 0, len(st.T_ok))


def fft_invalidate_W(st, writer):
    """fft.hip:569."""
    if not st.has('W_survives_' + writer):
        if st.W_ok:
            st.W_dropped_by = writer
        st.W_ok = False


def mixed(g, dtype):
    return fd.mixed_has_reconstruct(geometry(g), dtype), fd.mixed_has_grad_W(geometry(g), dtype)


def fft_reconstruct(st, g, dtype, W, H, rec):
    """fft.hip:588-648."""
    c = prepare(st, g, dtype, H, None)
    rows_of_H(st, g, c, rec)
    mix = mixed(g, dtype)[0]
    key = ('TWr', c.lay.TWr) if mix else ('SW', c.lay.SW)
    same_layout = st.W_key == key or st.has('w_hit_across_layout')
    w_hit = (st.enabled and st.W_ok and st.W_owner == W and st.W_dtype == dtype and same_shape(st.W_geo, g)
             and (c.sl.cached or st.W_geo.N == g.N) and same_layout)
    if w_hit and st.explicit and c.sl.cached:
        st.seen.add('W_hit_across_slices')
    if not w_hit and st.enabled:
        if st.W_ok and st.W_owner != W:
            st.seen.add('W_miss_other_pointer')
        if st.W_ok and st.W_dtype != dtype:
            st.seen.add('W_miss_other_dtype')
        if st.W_ok and st.W_owner == W and st.W_dtype == dtype and same_shape(st.W_geo, g) and st.W_key != key:
            st.seen.add('W_hit_must_not_survive_layout_' + ('explicit' if st.explicit else 'implicit'))
        if not st.W_ok and st.W_owner == W and st.W_dropped_by:
            st.seen.add('W_miss_after_' + st.W_dropped_by)
    if not w_hit:
        rec.add(W_SPEC)
        st.W_dropped_by = None
        st.W_ok, st.W_owner, st.W_geo, st.W_dtype, st.W_key = st.enabled, W, g, dtype, key
    if not mix:
        # The library has a third branch here (fft.hip:622-628: contract inside the column kernel when the layout is not
        # resident).  make_layout makes the layout resident whenever one of the mixed forms is missing (:131), so a call the
        # mixed reconstruct does not take always finds it resident: the branch cannot be reached in the product build, and
        # the assert keeps this model from diverging silently if that rule changes.
        assert c.lay.resident, (g, dtype)
        spectra_of_H(st, g, c, rec)


def fft_grad_H(st, g, dtype, V, rec):
    """fft.hip:678-703 (the flipped spectra of W are made anew by every call: not cached, not listed)."""
    c = prepare(st, g, dtype, None, V, True)
    spectra_V(st, g, c, True, rec, V == st.V_volatile)


def fft_update_H(st, g, dtype, V, H, rec):
    """fft.hip:705-738."""
    c = prepare(st, g, dtype, H, V, True)
    spectra_V(st, g, c, True, rec, V == st.V_volatile)
    if c.sl.cached and st.enabled:
        drop_H(st, c.sl.n0, g.N)
        if not st.has('fft_update_leaves_nothing'):
            set_ok(st.T_ok, c.sl.n0, g.N, 1)    # :736: k_fft_rows_mu left the row spectra of the new H behind
            set_ok(st.T_mu, c.sl.n0, g.N, 1)


def fft_grad_W(st, g, dtype, V, H, rec):
    """fft.hip:787-890."""
    c = prepare(st, g, dtype, H, V)
    rows_of_H(st, g, c, rec)
    mix = mixed(g, dtype)[1]
    spectra_V(st, g, c, not mix, rec, V == st.V_volatile)
    if not mix:
        spectra_of_H(st, g, c, rec)


def fft_reserve(st, g, dtype, window):
    """fft.hip:571-578."""
    inside = st.bound and st.dtype == dtype and same_shape(st.geo, g) and st.geo.N >= g.N
    if st.has('reserve_ignores_binding'):
        inside = False
    lay = fd.make_layout(geometry(st.geo if inside else g), dtype, st.path, n_call=g.N)
    need = lay.total if window else lay.total_no_window
    own = fd.make_layout(geometry(g), dtype, st.path)
    if inside and need > st.ws_bytes and fd.align_up(need, 1 << 20) > fd.align_up(own.total if window else own.total_no_window, 1 << 20):
        st.seen.add('reserve_inside_binding_sizes_for_binding')
    if need <= st.ws_bytes and st.any_flag():
        st.seen.add('reserve_without_growth_keeps')
    ensure_ws(st, need)


# ---- api.hip: what takes the family -----------------------------------------------------------------------------------
def on_fft(st, g, dtype):
    """api.hip:232, :293: reconstruct and the W gradient."""
    if st.path == 'fft':
        return True
    if st.path == 'hybrid':
        return fd.fft_has(geometry(g), dtype)
    takes = st.path == 'auto' and fd.use_fft_under_auto(geometry(g), dtype)
    if st.path == 'auto' and dtype == 'f' and fd.fft_has(geometry(g), dtype):
        st.seen.add('auto_takes' if takes else 'auto_leaves')
    return takes


def do_reconstruct(st, g, dtype, W, H, rec):
    """api.hip:229-245."""
    if g.N > 0 and on_fft(st, g, dtype):
        fft_reconstruct(st, g, dtype, W, H, rec)


def beta_fields_of(st, g, dtype):
    """api.hip:318-326: Q goes into ctx->qb, which grows with the call; -> the pointer that stands for the samples."""
    need = fd.align_up(g.N * v_bytes(g, dtype), 256)
    if need > st.qb_bytes:
        if st.qb_bytes:
            st.seen.add('qb_growth_moves_V_volatile')
        st.qb_bytes, st.qb_gen = need, st.qb_gen + 1
    st.V_volatile = ('qb%d' % st.qb_gen, 0)
    return st.V_volatile


# ---- the entry points: each returns (return code, the set of spectra the call computes) --------------------------------
def set_cache(st, enable):
    """api.hip:691-696."""
    st.enabled = bool(enable)
    clear_flags(st)
    return E_OK, set()


def ctx_bind(st, g, dtype, H, V, volume=False):
    """api.hip:698-713: H == NULL, geom == NULL (g None) and a volume geometry drop the binding."""
    if g is None or H is None or volume:
        if st.bound:
            st.seen.add('bind_null_geom' if g is None else 'bind_volume' if volume else 'bind_null_H')
        unbind(st)
        st.after_unbind = True
    else:
        bind(st, g, dtype, H, V, True)
    return E_OK, set()


def invalidate(st):
    """api.hip:724-728."""
    clear_flags(st, 'foreign_write_and_invalidate')
    return E_OK, set()


def set_path(st, path):
    """api.hip:668-674."""
    if path not in PATHS:
        st.seen.add('set_path_refused')
        return E_UNSUPPORTED, set()
    if st.any_flag():
        st.seen.add('set_path_same_keeps' if path == st.path else 'set_path_other_drops')
    if path != st.path and not st.has('set_path_keeps_flags'):
        clear_flags(st)
    st.path = path
    return E_OK, set()


def reserve(st, g, dtype):
    """api.hip:651-666."""
    if g.N > 0 and st.path == 'fft':
        fft_reserve(st, g, dtype, True)
    if g.N > 0 and st.path != 'fft' and on_fft(st, g, dtype):
        fft_reserve(st, g, dtype, False)
    return E_OK, set()


def reconstruct(st, g, dtype, W, H):
    """api.hip:741-747."""
    rec = set()
    do_reconstruct(st, g, dtype, W, H, rec)
    return E_OK, rec


def energy(st, g, dtype, V, W, H):
    """api.hip:807-833."""
    return reconstruct(st, g, dtype, W, H)


def grad_H(st, g, dtype, V, W, H, r_given):
    """api.hip:749-764, :250-276."""
    rec = set()
    if not r_given:
        do_reconstruct(st, g, dtype, W, H, rec)
    if st.path == 'fft':
        fft_grad_H(st, g, dtype, V, rec)
    return E_OK, rec


def update_H(st, g, dtype, V, W, H, r_is_valid=False, mode='valid', lateral=False, beta=False):
    """api.hip:1045-1120 (tnmf_hip_update_H, _update_H_ex, _update_H_beta, _update_H_weighted).  beta: the fields (Q, P)
    stand for (V, R), which is the case for beta != 2 and for every weighted step (:1083)."""
    rec = set()
    if mode != 'valid':
        # :1100-1119: a 'valid' step on the padded copy, which sits at one address (ctx->hw) with new contents every call
        Hp = ('hw', 0)
        if st.any_flag():
            st.seen.add('modes_invalidate_before_and_after')
        if not st.has('modes_keep_flags'):
            clear_flags(st)                                   # :1111
        do_reconstruct(st, g, dtype, W, Hp, rec)
        if beta:
            V = beta_fields_of(st, g, dtype)
        if st.path == 'fft':
            fft_grad_H(st, g, dtype, V, rec)
        if not st.has('modes_keep_flags'):
            clear_flags(st)                                   # :1118
        return E_OK, rec
    if not r_is_valid:
        do_reconstruct(st, g, dtype, W, H, rec)               # :1081
    if beta:
        V = beta_fields_of(st, g, dtype)                      # :1083
    if st.path == 'fft':
        if lateral:
            # the family has no epilogue for the lateral terms (:253): unfused gradient, then one update kernel
            fft_grad_H(st, g, dtype, V, rec)                  # :1095
            if not st.has('lateral_keeps_H'):
                fft_invalidate_H(st, g, dtype, H, 'lateral_fallback')   # :1096
        else:
            fft_update_H(st, g, dtype, V, H, rec)             # :258
    else:
        fft_invalidate_H(st, g, dtype, H)                     # :259: the direct kernels are about to change H
    return E_OK, rec


def grad_W(st, g, dtype, V, W, H, r_is_valid=False, beta=False):
    """api.hip:1172-1207 (tnmf_hip_grad_W_fused, _grad_W_beta)."""
    rec = set()
    if not r_is_valid:
        do_reconstruct(st, g, dtype, W, H, rec)
    if beta and g.N > 0:
        V = beta_fields_of(st, g, dtype)
    if g.N > 0 and on_fft(st, g, dtype):
        fft_grad_W(st, g, dtype, V, H, rec)
    return E_OK, rec


def mu_update(st):
    """api.hip:783-791: arr may be (part of) the activations whose row spectra are cached."""
    if not st.has('mu_update_keeps_flags'):
        clear_flags(st, 'mu_update')
    return E_OK, set()


def write_W(st, writer):
    """normalize_W (api.hip:801), apply_W (:1413), group_apply_W / ops_apply_W and group_expand_W / ops_expand_W (the
    expanded dictionary is written at an address the family may have seen): fft_invalidate_W."""
    fft_invalidate_W(st, writer)
    return E_OK, set()


W_WRITERS = ('normalize_W', 'apply_W', 'group_expand_W', 'group_apply_W', 'ops_expand_W', 'ops_apply_W')


def run_schedule(st, g, dtype, V, W, H, ops):
    """api.hip:1329-1380 under path 'fft' / 'hybrid' (the persistent kernel of :1287-1328 takes 'auto' / 'generic' only):
    the list walked operation by operation.  ops: ('update_H' | 'grad_W' | 'apply_W', n0, n1)."""
    rec = set()
    hb, vb = h_bytes(g, dtype), v_bytes(g, dtype)
    if ops and st.path in ('auto', 'generic') and g.N * g.M * shift(g)[0] * shift(g)[1] <= 1 << 18:
        # :1286-1318: a tiny resident problem is walked by the persistent kernel (or, refused, by the direct kernels below):
        # H and W change under the family's caches, whatever they hold of another problem
        if st.any_flag():
            st.seen.add('run_schedule_persistent_invalidates')
        if not st.has('persistent_schedule_keeps_flags'):
            clear_flags(st, 'run_schedule')
    for kind, n0, n1 in ops:
        gs = g._replace(N=n1 - n0)
        Hb, Vb = (H[0], H[1] + n0 * hb), (V[0], V[1] + n0 * vb)
        if kind == 'update_H' and gs.N > 0:
            rec |= update_H(st, gs, dtype, Vb, W, Hb)[1]
        elif kind == 'grad_W':
            rec |= grad_W(st, gs, dtype, Vb, W, Hb)[1]
        elif kind == 'apply_W':
            fft_invalidate_W(st, 'run_schedule')                # :1372
    return E_OK, rec


# ---- the transitions --------------------------------------------------------------------------------------------------
TRANSITIONS = (
    # locate and bind
    'cache_off_nothing_tracked',            # fft.hip:364, :413
    'implicit_bind_H_and_V',                # fft.hip:413-417
    'implicit_bind_H_only',                 # fft.hip:417 (reconstruct)
    'implicit_bind_V_only',                 # fft.hip:417 (grad_H with R given)
    'explicit_slice_first',                 # fft.hip:371
    'explicit_slice_interior',
    'explicit_slice_last',
    'slice_overruns_binding',               # fft.hip:377
    'H_before_base',                        # fft.hip:370
    'H_not_whole_samples_in',               # fft.hip:370
    'dtype_differs',                        # fft.hip:364
    'shape_differs_M',                      # fft.hip:338
    'shape_differs_C',
    'shape_differs_D',
    'shape_differs_A',
    'shape_differs_h_row_stride',
    'located_by_V',                         # fft.hip:372-375
    'V_before_base',                        # fft.hip:374
    'V_misaligned',                         # fft.hip:374
    'adopt_V_at_n0_gt_0',                   # fft.hip:381-385
    'H_slice_with_other_V',                 # fft.hip:386, :470-475
    'foreign_under_explicit_bind',          # fft.hip:419
    'foreign_under_implicit_bind',          # fft.hip:416
    'unbind_then_implicit',                 # api.hip:700-702, fft.hip:545
    'bind_null_geom',                       # api.hip:700
    'bind_null_H',                          # api.hip:700
    'bind_volume',                          # api.hip:704-707
    # H flags
    'H_hit',                                # fft.hip:495-498
    'H_run_one_sample_invalid',             # fft.hip:495
    'SH_only_when_resident',                # fft.hip:604-621
    'SH_cleared_with_T',                    # fft.hip:502, :560, :716
    'fft_update_H_leaves_T',                # fft.hip:736
    'hybrid_update_invalidates_slice',      # api.hip:259, fft.hip:558-560
    'hybrid_update_not_located_invalidates_all',   # fft.hip:561-564
    'lateral_fallback_invalidates',         # api.hip:1096
    'modes_invalidate_before_and_after',    # api.hip:1111, :1118
    # V flags
    'V_rows_hit',                           # fft.hip:468
    'V_cols_on_first_demand',               # fft.hip:484-487
    'V_volatile_never_cached',              # fft.hip:410, :470-475
    'qb_growth_moves_V_volatile',           # api.hip:321-322
    # W
    'W_hit_across_slices',                  # fft.hip:596-597
    'W_miss_other_pointer',
    'W_miss_other_dtype',
    'W_miss_after_mu_update',               # api.hip:789
    'W_miss_after_normalize_W',             # api.hip:801
    'W_miss_after_apply_W',                 # api.hip:1413
    'W_miss_after_run_schedule',            # api.hip:1372
    'W_miss_after_group_expand_W',          # group.hip:168
    'W_miss_after_group_apply_W',           # group.hip:206
    'W_miss_after_ops_expand_W',            # atom_ops.hip:332
    'W_miss_after_ops_apply_W',             # atom_ops.hip:371
    'run_schedule_persistent_invalidates',  # api.hip:1318
    'W_miss_after_foreign_write_and_invalidate',   # include/tnmf_hip.h: the caller's promise
    'W_hit_must_not_survive_layout_explicit',      # fft.hip:596-597: a foreign problem under an explicit binding
    'W_hit_must_not_survive_layout_implicit',      # fft.hip:596-597: an implicit re-binding to another sample count
    'set_path_same_keeps',                  # api.hip:671
    'set_path_other_drops',                 # api.hip:671
    'set_path_refused',                     # api.hip:670
    # workspace
    'growth_clears_flags',                  # fft.hip:190, :199
    'reserve_without_growth_keeps',         # fft.hip:168
    'reserve_inside_binding_sizes_for_binding',    # fft.hip:575-577
    'auto_crossover',                       # api.hip:158-161
)

NOT_REACHED = {
    'hipMalloc_refused': 'fft.hip:171-195: needs a device without room for a few MiB; allocation failures are not provoked',
    'run_schedule_fused_blend_apply': 'api.hip:1362, the second fft_invalidate_W of run_schedule: taken on the per-operation '
                                      'walk when the W gradient of a slice runs on the direct kernels, which under fft and '
                                      'hybrid never happens at these shapes (the family takes every W gradient) and under '
                                      'auto needs a resident problem of more than 2^18 activations (146 samples) whose '
                                      'slices stay under 2^19: a W-gradient oracle over hundreds of samples per test',
}

# ---- the sequences ----------------------------------------------------------------------------------------------------
D0, A0, M0, NB = (20, 22), (5, 4), 3, 6      # transform length 32 on both axes; a binding of 6 samples, slices of 2
CLASSES = ('mixed', 'resident')


def channels(cls, dtype):
    """mixed: float32, one channel (TWr kept, no SH).  resident: float64, or float32 with two channels (SW and SH kept)."""
    assert (cls, dtype) != ('mixed', 'd')
    return 2 if (cls, dtype) == ('resident', 'f') else 1


def geo(cls, dtype, N, **other):
    return Geo(N, channels(cls, dtype), D0, M0, A0, 0)._replace(**other)


def check_classes():
    """Each class lands where it is meant to: the family takes it on both paths, and the layout is (not) resident."""
    for cls, dtype in (('mixed', 'f'), ('resident', 'd'), ('resident', 'f')):
        for N in (2, 3, NB):
            g = geometry(geo(cls, dtype, N))
            for path in ('fft', 'hybrid'):
                assert fd.family(g, dtype, path, 'reconstruct') == 'fft' and fd.family(g, dtype, path, 'grad_W') == 'fft'
                assert fd.family(g, dtype, path, 'update_H') == ('fft' if path == 'fft' else 'direct')
                lay = fd.make_layout(g, dtype, path)
                assert (lay.Ly, lay.Lx) == (32, 32) and lay.resident == (cls == 'resident'), (cls, dtype, path, lay)
    return True


# An operation is (entry point, {arguments}).  Pointers are (buffer, sample[, extra elements]) in units of the sequence's
# own geometry; `shape` replaces fields of the geometry for one call; `dtype` its element type.
#   buffers: H, V (8 samples: the binding takes 6 of them), G, U (a foreign problem's activations and samples: 3 samples),
#            W, W2 (dictionaries), R (reconstruction scratch), NP (neg | pos of the W gradient)
def op(name, **kw):
    return (name, kw)


def rec_(n0, N=2, W='W', H='H', **kw):
    return op('reconstruct', N=N, H=(H, n0), W=W, **kw)


def gw_(n0, N=2, W='W', H='H', V='V', v0=None, **kw):
    return op('grad_W', N=N, H=(H, n0), V=(V, n0 if v0 is None else v0), W=W, **kw)


def uh_(n0, N=2, W='W', H='H', V='V', v0=None, **kw):
    return op('update_H', N=N, H=(H, n0), V=(V, n0 if v0 is None else v0), W=W, **kw)


def gh_(n0, N=2, W='W', H='H', V='V', **kw):
    return op('grad_H', N=N, H=(H, n0), V=(V, n0), W=W, **kw)


ON = op('set_cache', enable=1)
BIND = op('bind', N=NB, H=('H', 0), V=('V', 0))
BIND_NO_V = op('bind', N=NB, H=('H', 0), V=None)
BINDL = op('bind', N=292, H=('HL', 0), V=None)      # the large buffer: 292 samples (cache_reference.LARGE)
HALVE = lambda buf, n0, n=1: op('mu_update', arr=(buf, n0), n=n)     # noqa: E731  arr <- arr / 2 through tnmf_hip_mu_update

ANY = (('f', 'mixed'), ('d', 'resident'))
ALL = ANY + (('f', 'resident'),)
BOTH = ('fft', 'hybrid')

# name -> (variants (dtype, class), paths, operations, {transition: why this sequence carries it})
_BASE = {
    'cache_off': (ANY, BOTH, [rec_(0), rec_(0), gw_(0), gw_(0)], {
        'cache_off_nothing_tracked': 'every call runs both transforms again, nothing is bound'}),
    'implicit_full_iteration': (ALL, BOTH, [ON, uh_(0, NB), gw_(0, NB), uh_(0, NB), gw_(0, NB)], {
        'H_hit': 'the W half step reuses the rows the reconstruct made (hybrid) or the update left (fft)',
        'V_rows_hit': 'V is transformed once',
        'fft_update_H_leaves_T': 'under fft the second reconstruct hits the rows k_fft_rows_mu left',
        'hybrid_update_invalidates_slice': 'under hybrid the direct update drops the rows of the whole call',
        'implicit_bind_H_only': 'the reconstruct inside update_H binds H alone; the update itself adopts V'}),
    'implicit_H_only_then_V_only': (ANY, ('fft',), [ON, rec_(0, NB), rec_(0, NB), gh_(0, NB, r_given=1), gh_(0, NB, r_given=1),
                                                  rec_(0, NB)], {
        'implicit_bind_H_only': 'reconstruct binds H alone and hits on the second call',
        'implicit_bind_V_only': 'grad_H with R given has no H: it re-binds by V alone, the second call hits',
        'located_by_V': 'the second grad_H is located through V_base',
        'foreign_under_implicit_bind': 'the binding by V has no H_base: the last reconstruct re-binds and runs'}),
    'explicit_slices': (ALL, BOTH, [ON, BIND, rec_(0), rec_(2), rec_(4), rec_(0), rec_(2), rec_(4), gw_(2), gw_(2),
                                    op('energy', N=2, H=('H', 2), V=('V', 2), W='W')], {
        'explicit_slice_first': 'n0 = 0', 'explicit_slice_interior': 'n0 = 2', 'explicit_slice_last': 'n0 = 4',
        'W_hit_across_slices': 'the spectra of W are made by the first slice only',
        'H_hit': 'the second round hits per slice, and so does the energy of a slice',
        'SH_only_when_resident': 'columns of H are recomputed set only in the resident class'}),
    'one_sample_invalid': (ANY, BOTH, [ON, BIND, rec_(0, 4), HALVE('G', 0), rec_(0, 4), uh_(1, 1), rec_(0, 4), rec_(0, 4)], {
        'H_run_one_sample_invalid': 'hybrid: the direct update of sample 1 alone makes the call on 0..3 run again',
        'hybrid_update_invalidates_slice': 'samples 0, 2, 3 keep their flags (the model), the call still runs',
        'SH_cleared_with_T': 'resident: the columns of sample 1 go with its rows',
        'W_miss_after_mu_update': 'mu_update on another buffer still drops everything: W is made again'}),
    'pointer_games': (ANY, ('hybrid',), [ON, op('bind', N=NB, H=('H', 1), V=('V', 1)), rec_(1), rec_(1),
                                         rec_(0), rec_(1), rec_(6), rec_(1), op('reconstruct', N=2, H=('H', 1, 8), W='W'), rec_(1),
                                         rec_(1)], {
        'H_before_base': 'H[0:2] lies one sample before the binding at H[1:7]: foreign, flags cleared',
        'slice_overruns_binding': 'H[6:8] starts inside and ends outside',
        'H_not_whole_samples_in': 'eight elements into sample 1',
        'foreign_under_explicit_bind': 'each of the three clears the flags and keeps the binding: the next slice runs, '
                                       'the one after hits'}),
    'shape_fields': (ANY, ('hybrid',), [ON, BIND, rec_(0), rec_(0, shape=dict(M=2)), rec_(0), rec_(0, shape=dict(C=3)), rec_(0),
                                        rec_(0, shape=dict(D=(19, 22))), rec_(0), rec_(0, shape=dict(A=(4, 4))), rec_(0),
                                        rec_(0, shape=dict(hs=26)), rec_(0), rec_(0)], {
        'shape_differs_M': 'M = 2', 'shape_differs_C': 'C = 3', 'shape_differs_D': 'Dy = 19', 'shape_differs_A': 'Ay = 4',
        'shape_differs_h_row_stride': 'rows of 26 elements'}),
    'dtype_differs': (ANY, ('hybrid',), [ON, BIND, rec_(0), rec_(0, H='G', W='W2', dtype='other'), rec_(0), rec_(0)], {
        'dtype_differs': 'a call of the other element type on buffers of its own is foreign'}),
    'dtype_differs_implicit': (ANY, ('hybrid',), [ON, rec_(0), rec_(0, H='G', W='W2', dtype='other'), rec_(0), rec_(0)], {
        'dtype_differs': 'without an explicit binding the call re-binds, and W_ok survives that',
        'W_miss_other_dtype': 'so the W spectra of the first call are refused by their element type (and pointer)'}),
    'V_pointer_games': (ANY, ('fft',), [ON, BIND, gh_(2, r_given=1), gh_(2, r_given=1),
                                        op('grad_H', N=2, H=('H', 2), V=('V', 2, 4), W='W', r_given=1), gh_(2, r_given=1),
                                        op('bind', N=NB, H=('H', 1), V=('V', 1)), gh_(0, r_given=1), gh_(1, r_given=1),
                                        gh_(1, r_given=1)], {
        'located_by_V': 'grad_H with R given is located by its samples',
        'V_misaligned': 'four elements into sample 2: foreign',
        'V_before_base': 'V[0:2] before a binding at V[1:7]',
        'V_rows_hit': 'the repeated call hits'}),
    'V_cols_later': ((('f', 'mixed'),), ('fft',), [ON, BIND, gw_(2), gh_(2, r_given=1), gh_(2, r_given=1)], {
        'V_cols_on_first_demand': 'the mixed W gradient wants the rows of V only; grad_H finds them and makes the columns'}),
    'adopt_V': (ANY, BOTH, [ON, BIND_NO_V, rec_(2), gw_(2), gw_(2), gw_(0), gw_(0), gw_(2)], {
        'adopt_V_at_n0_gt_0': 'the binding has no V; the W gradient of slice 2..3 adopts V - 2 samples as the base, so the '
                              'slice at 0 is tracked too and the slice at 2 still hits'}),
    'other_V': (ANY, BOTH, [ON, BIND, gw_(2), gw_(2), gw_(2, V='U', v0=0), gw_(2), gw_(2)], {
        'H_slice_with_other_V': 'the samples of a foreign problem through the slots of slice 2..3: untracked, and the V '
                                'flags of the slots dropped, so the bound samples run again'}),
    'unbind': (ANY, ('hybrid',), [ON, BIND, rec_(2), op('bind', N=None, H=None, V=None), rec_(2), rec_(2), BIND, rec_(2),
                                  op('bind', N=NB, H=None, V=None), rec_(2), rec_(2), BIND, rec_(2),
                                  op('bind', N=NB, H=('H', 0), V=('V', 0), volume=1), rec_(2), rec_(2)], {
        'unbind_then_implicit': 'after the unbind the slice binds itself implicitly (runs), then hits',
        'bind_null_geom': 'geom == NULL', 'bind_null_H': 'H == NULL', 'bind_volume': 'a volume geometry drops the binding as well'}),
    'foreign_passes_through': (ALL, BOTH, [ON, BIND, gw_(0), rec_(0, 3, H='G'), gw_(0), gw_(0)], {
        'foreign_under_explicit_bind': 'a foreign problem of 3 samples clears H, V and W flags; the binding stays'}),
    'implicit_rebind': (ANY, BOTH, [ON, gw_(0, NB, r_is_valid=1), gw_(0, NB), gw_(0, 3, H='G', V='U'), gw_(0, 3, H='G', V='U'), gw_(0, NB)], {
        'implicit_bind_H_and_V': 'the W gradient with R given is the first call: it binds H and V at once',
        'foreign_under_implicit_bind': 'another problem re-binds; coming back re-binds again and runs'}),
    'fft_update_then_hits': (ALL, ('fft',), [ON, BIND, uh_(2), rec_(2), gw_(2), uh_(2, r_is_valid=1), rec_(2)], {
        'fft_update_H_leaves_T': 'T_ok = 1 after the update: reconstruct and the W gradient hit',
        'SH_cleared_with_T': 'resident: the update drops SH, the reconstruct after it makes the columns again'}),
    'hybrid_update_foreign_H': (ANY, ('hybrid',), [ON, BIND, rec_(0), rec_(2), uh_(0, 2, H='G', V='U', r_is_valid=1), rec_(0),
                                                   rec_(2)], {
        'hybrid_update_not_located_invalidates_all': 'the direct update of activations outside the binding (R given, so '
                                                     'nothing else touches the cache) drops the rows of every sample'}),
    'lateral': (ANY, ('fft',), [ON, BIND, op('reserve', N=2), rec_(2), uh_(2, lateral=1), rec_(2), rec_(2)], {
        'lateral_fallback_invalidates': 'path fft has no epilogue for the lateral terms: unfused gradient, mu_update_extra, '
                                        'and the rows of the slice dropped'}),
    'modes': (ANY, BOTH, [ON, BIND, gw_(2), gw_(2), op('update_H', N=2, H=('HC', 0), V=('V', 2), W='W', mode='circular'),
                          gw_(2), gw_(2)], {
        'modes_invalidate_before_and_after': 'the padded copy at one address: everything dropped before and after'}),
    'volatile_V': (ANY, BOTH, [ON, BIND, gw_(2), gw_(2, beta=1), gw_(2), gw_(2), uh_(2, beta=1), gw_(2),
                               uh_(2, weighted=1), gw_(2)], {
        'V_volatile_never_cached': 'the field Q goes through the slots of slice 2..3: their V flags drop, the next '
                                   'Frobenius call runs; the last H step is the weighted entry point (weights GW)'}),
    'volatile_V_moves': (ANY, ('hybrid',), [ON, BIND, gw_(2, beta=1), gw_(2), gw_(0, 4, beta=1), gw_(0, 4), gw_(0, 4)], {
        'qb_growth_moves_V_volatile': 'four samples need a larger Q: ctx->qb moves and V_volatile with it'}),
    'W_writers': (ALL, BOTH, [ON, BIND, rec_(0), rec_(2, W='W2'), rec_(2), op('normalize_W', W='W'), rec_(2), gw_(2),
                              op('mu_update', raw=('NP', 0, 10)), rec_(2), op('apply_W', W='W'), rec_(2), rec_(4)], {
        'W_miss_other_pointer': 'W2 takes the spectra over, W takes them back',
        'W_miss_after_normalize_W': 'normalize_W',
        'W_miss_after_apply_W': 'apply_W (half an atom of the gradient is halved first, so that the step moves W by more '
                                'than the normalisation takes back; the reconstruct between the two makes the W spectra '
                                'valid again, so that apply_W alone drops them)',
        'W_hit_across_slices': 'the last call hits'}),
    'W_schedule': (ANY, BOTH, [ON, BIND, rec_(0), op('run_schedule', ops=[('update_H', 0, 2), ('grad_W', 0, 2), ('apply_W', 0, 0)]),
                               rec_(0), rec_(2)], {
        'W_miss_after_run_schedule': 'the list\'s APPLY_W writes W'}),
    'W_group_writers': (ANY, BOTH, [ON, BIND, op('group_expand_W', W='W'), rec_(0, W='WE'), op('group_expand_W', W='W2'),
                                    rec_(0, W='WE'), rec_(2, W='WE'), op('group_apply_W', W='W'), rec_(2, W='WE'), rec_(4, W='WE')], {
        'W_miss_after_group_expand_W': 'the flip group: W_eff (here WE: 6 atoms, of which the activations use the first 3) '
                                       'keeps its address and takes the expansion of another dictionary',
        'W_miss_after_group_apply_W': 'fold, update, normalise and expand in one launch write WE again'}),
    'W_ops_writers': (ANY, BOTH, [ON, BIND, op('ops_expand_W', W='W'), rec_(0, W='WE'), op('ops_expand_W', W='W2'),
                                  rec_(0, W='WE'), rec_(2, W='WE'), op('ops_apply_W', W='W'), rec_(2, W='WE'), rec_(4, W='WE')], {
        'W_miss_after_ops_expand_W': 'the same two maps (identity, mirror along x) as an atom-operator handle',
        'W_miss_after_ops_apply_W': 'likewise'}),
    'W_foreign_write': (ALL, BOTH, [ON, BIND, rec_(0), op('host_write', buf='W', what='swap_atoms'), op('invalidate'), rec_(0),
                                    rec_(2)], {
        'W_miss_after_foreign_write_and_invalidate': 'W written by other means; tnmf_hip_ctx_invalidate is sufficient'}),
    'layout_explicit': (ALL, BOTH, [ON, BIND, rec_(0, W='W2'), rec_(0, 2, H='G'), rec_(0)], {
        'W_hit_must_not_survive_layout_explicit': 'the foreign call lays the workspace out for 2 samples and marks W_ok for W; '
                                                  'the slice of the binding reads the layout for 6, where the first call '
                                                  'left the spectra of W2'}),
    'layout_implicit': (ALL, BOTH, [ON, gw_(0, NB), rec_(0, NB), rec_(0, 2, H='G'), rec_(0, 2, H='G')], {
        'W_hit_must_not_survive_layout_implicit': 'problem B re-binds implicitly, W_ok survives, the layout follows 2 samples'}),
    'set_path': (ANY, ('hybrid',), [ON, BIND, gw_(2), op('set_path', path='hybrid'), gw_(2), op('set_path', path='fft'), gw_(2),
                                    op('set_path', path='bogus'), gw_(2)], {
        'set_path_same_keeps': 'hybrid -> hybrid: hits', 'set_path_other_drops': 'hybrid -> fft: runs',
        'set_path_refused': 'an unknown path is refused and changes nothing: hits'}),
    'window_growth': ((('d', 'resident'),), ('fft',), [ON, BIND, gw_(2), gw_(2), gh_(2, r_given=1), gw_(2)], {
        'growth_clears_flags': 'grad_H is the first call that wants the window buffers: 3 -> 4 MiB, every flag dropped'}),
    'large_binding_growth': ((('f', 'mixed'),), ('fft',), [ON, BINDL, rec_(0, H='HL'), rec_(0, H='HL'),
                                                          gh_(0, H='HL', r_given=1), rec_(0, H='HL')], {
        'growth_clears_flags': 'float32: the window buffers of a binding of 292 samples are megabytes; grad_H grows the '
                               'workspace and the rows of the slice run again'}),
    'large_binding_reserve': ((('f', 'mixed'),), ('fft',), [ON, BINDL, op('reserve', N=2), rec_(0, H='HL'),
                                                           gh_(0, H='HL', r_given=1), rec_(0, H='HL'), op('reserve', N=2),
                                                           rec_(0, H='HL')], {
        'reserve_inside_binding_sizes_for_binding': 'float32: reserve for a slice sizes for the 292 samples with the window',
        'reserve_without_growth_keeps': 'the second reserve changes nothing'}),
    'reserve': ((('d', 'resident'), ('f', 'mixed')), ('fft',), [ON, BIND, op('reserve', N=2), gw_(2), gh_(2, r_given=1), gw_(2),
                                                 op('reserve', N=2), gw_(2)], {
        'reserve_inside_binding_sizes_for_binding': 'reserve for a slice sizes for the 6 samples with the window: the '
                                                    'grad_H after it grows nothing and the V rows hit',
        'reserve_without_growth_keeps': 'the second reserve changes nothing'}),
    'auto_crossover': ((('f', 'mixed'),), ('auto',), [ON, rec_(0, 292, H='HL'), rec_(0, 291, H='HL'), rec_(0, 292, H='HL'),
                        op('run_schedule', ops=[('grad_W', 0, 2)]), rec_(0, 292, H='HL')], {
        'run_schedule_persistent_invalidates': 'a tiny resident problem (the 6 samples of H) walked by the persistent kernel '
                                               'under auto: everything the cache holds of the large problem is dropped (the list is one W gradient, '
                                               'so that no H update or W update drops anything on its own account)',
        'auto_crossover': '292 samples of 3 x 24 x 25 activations are the first 2^19: the family takes them, and binds; 291 '
                          'go to the direct kernels and leave the cache alone, so the third call hits'}),
}

Sequence = namedtuple('Sequence', 'dtype path cls ops carries base')


def _expand():
    out = {}
    for name, (variants, paths, ops, carries) in _BASE.items():
        for dtype, cls in variants:
            for path in paths:
                out[f'{name}[{dtype}-{cls}-{path}]'] = Sequence(dtype, path, cls, ops, carries, name)
    return out


SEQUENCES = _expand()

# a wrong model: the right one with one defect -> the sequence (base name) that tells them apart
WRONG_MODELS = {
    # locate and bind
    'overrun_is_located': 'pointer_games',
    'adopt_V_as_base': 'adopt_V',
    'foreign_keeps_flags': 'foreign_passes_through',
    # H flags
    'sh_survives_t': 'fft_update_then_hits',
    'direct_update_keeps_H': 'one_sample_invalid',
    'fft_update_leaves_nothing': 'fft_update_then_hits',
    'lateral_keeps_H': 'lateral',
    'modes_keep_flags': 'modes',
    'mu_update_keeps_flags': 'one_sample_invalid',
    # V flags
    'v_survives_volatile': 'volatile_V',
    # W
    'w_hit_across_layout': 'layout_explicit',
    'W_survives_normalize_W': 'W_writers',
    'W_survives_apply_W': 'W_writers',
    'W_survives_run_schedule': 'W_schedule',
    'W_survives_group_expand_W': 'W_group_writers',
    'W_survives_group_apply_W': 'W_group_writers',
    'W_survives_ops_expand_W': 'W_ops_writers',
    'W_survives_ops_apply_W': 'W_ops_writers',
    'persistent_schedule_keeps_flags': 'auto_crossover',
    'set_path_keeps_flags': 'set_path',
    # workspace
    'growth_keeps_flags': 'window_growth',
    'reserve_ignores_binding': 'reserve',
}


# ---- running a sequence through the model -----------------------------------------------------------------------------
def pointer(seq, p, g_nominal, what):
    """(buffer, sample[, elements]) -> (buffer, byte offset) in units of the sequence's own geometry."""
    if p is None:
        return None
    buf, sample, extra = (tuple(p) + (0,))[:3]
    per = h_bytes(g_nominal, seq.dtype) if what == 'H' else v_bytes(g_nominal, seq.dtype)
    return (buf, sample * per + extra * ESIZE[seq.dtype])


def call_of(seq, kw):
    """geometry, dtype and the pointers of one operation."""
    dtype = seq.dtype
    if kw.get('dtype') == 'other':
        dtype = 'd' if seq.dtype == 'f' else 'f'
    nominal = geo(seq.cls, seq.dtype, kw.get('N') or 0)
    g = nominal._replace(**kw.get('shape', {}))
    H = pointer(seq, kw.get('H'), nominal, 'H')
    V = pointer(seq, kw.get('V'), nominal, 'V')
    W = (kw['W'], 0) if kw.get('W') else None
    return g, dtype, H, V, W


def apply(st, seq, step):
    """One operation on the model -> (return code, recomputed set)."""
    name, kw = step
    g, dtype, H, V, W = call_of(seq, kw)
    if name == 'set_cache':
        return set_cache(st, kw['enable'])
    if name == 'bind':
        return ctx_bind(st, g if kw['N'] is not None else None, dtype, H, V, bool(kw.get('volume')))
    if name == 'invalidate':
        return invalidate(st)
    if name == 'set_path':
        return set_path(st, kw['path'])
    if name == 'reserve':
        return reserve(st, g, dtype)
    if name == 'reconstruct':
        return reconstruct(st, g, dtype, W, H)
    if name == 'energy':
        return energy(st, g, dtype, V, W, H)
    if name == 'grad_H':
        return grad_H(st, g, dtype, V, W, H, bool(kw.get('r_given')))
    if name == 'update_H':
        return update_H(st, g, dtype, V, W, H, bool(kw.get('r_is_valid')), kw.get('mode', 'valid'), bool(kw.get('lateral')),
                        bool(kw.get('beta') or kw.get('weighted')))
    if name == 'grad_W':
        return grad_W(st, g, dtype, V, W, H, bool(kw.get('r_is_valid')), bool(kw.get('beta')))
    if name == 'mu_update':
        return mu_update(st)
    if name in W_WRITERS:
        return write_W(st, name)
    if name == 'run_schedule':
        full = geo(seq.cls, seq.dtype, NB)
        return run_schedule(st, full, dtype, ('V', 0), ('W', 0), ('H', 0), kw['ops'])
    if name == 'host_write':
        return E_OK, set()              # the library is not told: that is what the invalidate after it is for
    raise KeyError(name)


Step = namedtuple('Step', 'rc recomputed counters exact v_slot seen')


def run(seq, defect=None):
    """The model's account of a sequence: per operation the return code, what is computed, the four counters after it,
    and whether the cached context still equals a fresh one to the bit (no spectra of k_fft_rows_mu consumed so far)."""
    st = State(seq.path, defect)
    out = []
    for step in seq.ops:
        st.v_slot = None
        rc, rec = apply(st, seq, step)
        out.append(Step(rc, frozenset(rec), tuple(st.counters), not st.mu_consumed, st.v_slot, frozenset(st.seen)))
    return out


# ---- which sequence carries which transition --------------------------------------------------------------------------
# what the model marks under another name than the transition's
_ALIASES = {'hybrid_update_slice': 'hybrid_update_invalidates_slice', 'hybrid_update_all': 'hybrid_update_not_located_invalidates_all',
            'lateral_fallback_slice': 'lateral_fallback_invalidates', 'lateral_fallback_all': 'lateral_fallback_invalidates'}


def reached(seq):
    """The transitions a sequence carries: the ones the right model goes through while it runs the sequence."""
    seen = set(run(seq)[-1].seen)
    got = {_ALIASES.get(t, t) for t in seen}
    if {'auto_takes', 'auto_leaves'} <= seen:
        got.add('auto_crossover')
    return got & set(TRANSITIONS)


DTYPES_OF = {t: ('f',) if t in ('auto_crossover', 'run_schedule_persistent_invalidates', 'V_cols_on_first_demand') else ('f', 'd')
             for t in TRANSITIONS}
# ('auto' takes the family for float32 only; every float64 consumer of the samples wants their full spectra, so rows that
# hit never wait for columns there)


def reached_by(sequences=None):
    sequences = SEQUENCES if sequences is None else sequences
    got = {}
    for name, seq in sequences.items():
        for t in reached(seq):
            got.setdefault((t, seq.dtype), []).append(name)
    return got


def required():
    return [(t, d) for t in TRANSITIONS for d in DTYPES_OF[t]]


def missing(sequences=None):
    got = reached_by(sequences)
    return sorted(c for c in required() if c not in got)


def sole_carriers(sequences=None):
    """{base sequence: [transitions only its variants carry]}."""
    sequences = SEQUENCES if sequences is None else sequences
    out = {}
    need = set(required())
    for (t, d), names in reached_by(sequences).items():
        if (t, d) not in need:
            continue
        bases = {sequences[n].base for n in names}
        if len(bases) == 1:
            b = bases.pop()
            if t not in out.setdefault(b, []):
                out[b].append(t)
    return out


def disagreements(seq, defect):
    """The steps at which the wrong model differs from the right one in the counters or the recomputed set."""
    right, wrong = run(seq), run(seq, defect)
    return [i for i, (a, b) in enumerate(zip(right, wrong)) if (a.counters, a.recomputed, a.rc) != (b.counters, b.recomputed, b.rc)]

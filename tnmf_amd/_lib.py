"""
ctypes binding of libtnmf_hip.so (C ABI: include/tnmf_hip.h).

There is no CPU fallback: if the shared library is missing or does not export the full ABI, importing a symbol
raises.  Build it with ``python -c "import __graft_entry__ as g; g.build()"`` or ``make -C tnmf_amd/csrc``.
"""
import ctypes
import os
from typing import Optional, Sequence

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'lib', 'libtnmf_hip.so')

ABI_VERSION = 8

# every symbol include/tnmf_hip.h declares
EXPORTS = (
    'tnmf_hip_abi_version', 'tnmf_hip_strerror', 'tnmf_hip_ctx_create', 'tnmf_hip_ctx_destroy',
    'tnmf_hip_ctx_reserve', 'tnmf_hip_ctx_set_path', 'tnmf_hip_ctx_last_path', 'tnmf_hip_reconstruct',
    'tnmf_hip_grad_H', 'tnmf_hip_grad_W', 'tnmf_hip_mu_update', 'tnmf_hip_normalize_W', 'tnmf_hip_energy',
    'tnmf_hip_convolve_multi_1d', 'tnmf_hip_update_H', 'tnmf_hip_grad_W_fused', 'tnmf_hip_apply_W',
    'tnmf_hip_pad_H', 'tnmf_hip_fold_H', 'tnmf_hip_ctx_set_cache', 'tnmf_hip_ctx_invalidate',
    'tnmf_hip_ctx_set_split', 'tnmf_hip_ctx_h_row_stride', 'tnmf_hip_ctx_bind', 'tnmf_hip_ctx_set_persistent',
    'tnmf_hip_ctx_last_schedule_persistent',
    'tnmf_hip_ctx_cache_counters', 'tnmf_hip_sum_parts',
    'tnmf_hip_update_H_ex', 'tnmf_hip_run_schedule', 'tnmf_hip_axpby', 'tnmf_hip_convolve_axis',
    'tnmf_hip_beta_fields', 'tnmf_hip_update_H_beta', 'tnmf_hip_grad_W_beta', 'tnmf_hip_energy_beta',
    'tnmf_hip_weighted_fields', 'tnmf_hip_update_H_weighted', 'tnmf_hip_grad_W_weighted', 'tnmf_hip_energy_weighted',
    'tnmf_hip_group_expand_W', 'tnmf_hip_group_fold_grad_W', 'tnmf_hip_group_apply_W',
    'tnmf_hip_atom_ops_create', 'tnmf_hip_atom_ops_destroy', 'tnmf_hip_ops_expand_W', 'tnmf_hip_ops_fold_grad_W',
    'tnmf_hip_ops_apply_W',
    'tnmf_hip_ctx_set_objective_tap', 'tnmf_hip_sample_objective', 'tnmf_hip_atom_terms',
    'tnmf_hip_atom_gram', 'tnmf_hip_atom_sources', 'tnmf_hip_atom_terms_beta', 'tnmf_hip_atom_gram_beta',
    'tnmf_hip_find_peaks', 'tnmf_hip_activation_correlogram',
    'tnmf_hip_triggered_sums_plan', 'tnmf_hip_triggered_sums',
    'tnmf_hip_events_render', 'tnmf_hip_events_update', 'tnmf_hip_events_grad_W', 'tnmf_hip_events_gain',
    'tnmf_hip_events_norms', 'tnmf_hip_pursuit_score', 'tnmf_hip_pursuit_pick', 'tnmf_hip_events_landscape',
    'tnmf_hip_events_alternatives',
    'tnmf_hip_events_pairs', 'tnmf_hip_events_gram', 'tnmf_hip_events_project', 'tnmf_hip_events_nnls',
    'tnmf_hip_events_inverse_diag',
    'tnmf_hip_events_patches', 'tnmf_hip_patch_moments',
)

MODES = {'valid': 0, 'full': 1, 'circular': 2, 'reflect': 3}

# transform groups (TNMF_GROUP_*): name -> id; tnmf_amd/transforms.py defines them
GROUPS = {'flip': 0, 'mirrors': 1, 'rot90': 2, 'dihedral': 3}

# the cell (= output tile) of tnmf_hip_events_render per number of shift axes: TNMF_EVENTS_CELL_*
EVENT_CELLS = {1: (256,), 2: (16, 16)}
# the events of a plane that tnmf_hip_events_grad_W sums into one slab: TNMF_EVENTS_SEGMENT
EVENT_SEGMENT = 64
# the largest component tnmf_hip_events_inverse_diag factors in LDS: TNMF_EVENTS_INVERSE_LDS
EVENT_INVERSE_LDS = 200
# the signal tnmf_hip_events_patches gathers (TNMF_PATCH_*): name -> id
PATCH_SOURCES = {'data': 0, 'residual': 1, 'cleaned': 2}
# the doubles of C * prod(A) a fold table allows: TNMF_PATCH_STAGE_MAX
PATCH_STAGE_MAX = 2048

# what tnmf_hip_atom_sources writes (TNMF_SOURCES_*): name -> id
SOURCE_OUTPUTS = {'contribution': 0, 'mask': 1, 'masked': 2, 'dominant': 3}

PATHS = {'auto': 0, 'generic': 1, 'mfma': 2, 'fft': 3, 'hybrid': 4, 'split': 5}


class Geom(ctypes.Structure):
    """tnmf_hip_geom"""
    _fields_ = [('ndim', ctypes.c_int), ('N', ctypes.c_int), ('M', ctypes.c_int), ('C', ctypes.c_int),
                ('D', ctypes.c_int * 3), ('A', ctypes.c_int * 3), ('dtype', ctypes.c_int),
                ('h_row_stride', ctypes.c_int)]


class Op(ctypes.Structure):
    """tnmf_hip_op"""
    _fields_ = [('kind', ctypes.c_int), ('n0', ctypes.c_int), ('n1', ctypes.c_int), ('a', ctypes.c_double),
                ('b', ctypes.c_double)]


OP_UPDATE_H, OP_GRAD_W, OP_APPLY_W = 0, 1, 2

E_GEOM = -2
E_UNSUPPORTED = -5
# the largest window A + 2 m of tnmf_hip_triggered_sums per number of shift axes: triggered.h, kTrigMaxWindow1 / 2
TRIGGERED_MAX_WINDOW = {1: 4096, 2: 128}
E_STRIDE = -6   # TNMF_E_STRIDE: the kernel family of this call wants C-contiguous H


class TnmfHipError(RuntimeError):
    def __init__(self, code: int, where: str, text: str):
        super().__init__(f'{where} failed with code {code}: {text}')
        self.code = code


_lib: Optional[ctypes.CDLL] = None


def load() -> ctypes.CDLL:
    """Load the library once; fail loudly when it is absent or incomplete."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f'{LIB_PATH} not found: the HIP extension is not built. The hip backend has no CPU fallback. '
            'Run `make -C tnmf_amd/csrc` (needs hipcc) first.')
    lib = ctypes.CDLL(LIB_PATH)
    missing = [name for name in EXPORTS if not hasattr(lib, name)]
    if missing:
        raise RuntimeError(f'{LIB_PATH} does not export {missing}')
    vp, ci, cd, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_size_t
    gp = ctypes.POINTER(Geom)
    lib.tnmf_hip_abi_version.restype = ci
    lib.tnmf_hip_strerror.restype = ctypes.c_char_p
    lib.tnmf_hip_strerror.argtypes = [ci]
    lib.tnmf_hip_ctx_create.argtypes = [ci, ctypes.POINTER(vp)]
    lib.tnmf_hip_ctx_destroy.argtypes = [vp]
    lib.tnmf_hip_ctx_reserve.argtypes = [vp, gp]
    lib.tnmf_hip_ctx_set_path.argtypes = [vp, ci]
    lib.tnmf_hip_ctx_set_cache.argtypes = [vp, ci]
    lib.tnmf_hip_ctx_set_split.argtypes = [vp, ci]
    lib.tnmf_hip_ctx_set_persistent.argtypes = [vp, ci]
    lib.tnmf_hip_ctx_last_schedule_persistent.argtypes = [vp]
    lib.tnmf_hip_ctx_last_schedule_persistent.restype = ci
    lib.tnmf_hip_ctx_h_row_stride.argtypes = [vp, gp, ctypes.POINTER(ci)]
    lib.tnmf_hip_ctx_invalidate.argtypes = [vp]
    lib.tnmf_hip_ctx_bind.argtypes = [vp, gp, vp, vp]
    lib.tnmf_hip_ctx_cache_counters.argtypes = [vp, ctypes.POINTER(ctypes.c_ulonglong * 4)]
    lib.tnmf_hip_ctx_last_path.restype = ctypes.c_char_p
    lib.tnmf_hip_ctx_last_path.argtypes = [vp]
    lib.tnmf_hip_reconstruct.argtypes = [vp, gp, vp, vp, vp, vp]
    lib.tnmf_hip_grad_H.argtypes = [vp, gp, vp, vp, vp, vp, vp, vp, vp]
    lib.tnmf_hip_grad_W.argtypes = [vp, gp, vp, vp, vp, vp, vp, vp, vp]
    lib.tnmf_hip_mu_update.argtypes = [vp, ci, vp, vp, vp, cd, sz, vp]
    lib.tnmf_hip_normalize_W.argtypes = [vp, gp, vp, vp]
    lib.tnmf_hip_energy.argtypes = [vp, gp, vp, vp, vp, ctypes.POINTER(cd), vp]
    lib.tnmf_hip_convolve_multi_1d.argtypes = [vp, ci, ci, sz, ctypes.POINTER(ci), vp, vp, vp,
                                               ctypes.POINTER(cd), ci, ctypes.POINTER(cd), ci, vp]
    lib.tnmf_hip_convolve_axis.argtypes = [vp, ci, sz, ci, sz, vp, vp, ctypes.POINTER(cd), ci, vp]
    lib.tnmf_hip_update_H.argtypes = [vp, gp, vp, vp, vp, vp, ci, cd, cd, vp]
    lib.tnmf_hip_update_H_ex.argtypes = [vp, gp, ci, vp, vp, vp, vp, cd, cd, cd, cd, ctypes.POINTER(cd), ci,
                                         ctypes.POINTER(cd), ci, ctypes.POINTER(cd), ci, vp]
    lib.tnmf_hip_run_schedule.argtypes = [vp, gp, vp, vp, vp, vp, vp, ctypes.POINTER(Op), ci, cd, cd, vp]
    lib.tnmf_hip_grad_W_fused.argtypes = [vp, gp, vp, vp, vp, vp, ci, vp, vp]
    lib.tnmf_hip_apply_W.argtypes = [vp, gp, vp, vp, cd, vp]
    lib.tnmf_hip_sum_parts.argtypes = [vp, ci, vp, ci, sz, vp, vp]
    lib.tnmf_hip_axpby.argtypes = [vp, ci, vp, vp, cd, cd, sz, vp]
    lib.tnmf_hip_beta_fields.argtypes = [vp, ci, cd, cd, vp, vp, vp, vp, sz, vp]
    lib.tnmf_hip_update_H_beta.argtypes = [vp, gp, ci, vp, vp, vp, vp, cd, cd, cd, cd, ctypes.POINTER(cd), ci,
                                           ctypes.POINTER(cd), ci, ctypes.POINTER(cd), ci, cd, vp]
    lib.tnmf_hip_grad_W_beta.argtypes = [vp, gp, vp, vp, vp, vp, ci, vp, cd, cd, vp]
    lib.tnmf_hip_energy_beta.argtypes = [vp, gp, cd, cd, vp, vp, vp, ctypes.POINTER(cd), vp]
    lib.tnmf_hip_weighted_fields.argtypes = [vp, ci, cd, cd, vp, vp, vp, vp, vp, sz, vp]
    lib.tnmf_hip_update_H_weighted.argtypes = [vp, gp, ci, vp, vp, vp, vp, vp, cd, cd, cd, cd, ctypes.POINTER(cd), ci,
                                               ctypes.POINTER(cd), ci, ctypes.POINTER(cd), ci, cd, vp]
    lib.tnmf_hip_grad_W_weighted.argtypes = [vp, gp, vp, vp, vp, vp, vp, ci, vp, cd, cd, vp]
    lib.tnmf_hip_energy_weighted.argtypes = [vp, gp, cd, cd, vp, vp, vp, vp, ctypes.POINTER(cd), vp]
    lib.tnmf_hip_group_expand_W.argtypes = [vp, gp, ci, vp, vp, vp]
    lib.tnmf_hip_group_fold_grad_W.argtypes = [vp, gp, ci, vp, vp, vp]
    lib.tnmf_hip_group_apply_W.argtypes = [vp, gp, ci, vp, vp, vp, cd, vp]
    pi = ctypes.POINTER(ci)
    lib.tnmf_hip_atom_ops_create.argtypes = [vp, ci, pi, ci, ci, pi, pi, pi, ctypes.POINTER(cd), ctypes.POINTER(vp)]
    lib.tnmf_hip_atom_ops_destroy.argtypes = [vp]
    lib.tnmf_hip_ops_expand_W.argtypes = [vp, gp, vp, vp, vp, vp]
    lib.tnmf_hip_ops_fold_grad_W.argtypes = [vp, gp, vp, vp, vp, vp]
    lib.tnmf_hip_ops_apply_W.argtypes = [vp, gp, vp, vp, vp, vp, cd, vp]
    lib.tnmf_hip_ctx_set_objective_tap.argtypes = [vp, vp]
    lib.tnmf_hip_sample_objective.argtypes = [vp, gp, cd, cd, vp, vp, vp, vp, vp, vp]
    lib.tnmf_hip_atom_terms.argtypes = [vp, gp, ci, vp, vp, vp, vp, vp, vp, vp]
    lib.tnmf_hip_atom_gram.argtypes = [vp, gp, ci, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.tnmf_hip_atom_terms_beta.argtypes = [vp, gp, ci, cd, cd, vp, vp, vp, vp, vp, vp, vp]
    lib.tnmf_hip_atom_gram_beta.argtypes = [vp, gp, ci, cd, cd, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.tnmf_hip_atom_sources.argtypes = [vp, gp, ci, vp, ci, vp, ci, cd, vp, vp, vp, vp, vp, vp, vp]
    lib.tnmf_hip_find_peaks.argtypes = [vp, gp, vp, cd, pi, ci, vp, vp, sz, vp, vp]
    lib.tnmf_hip_activation_correlogram.argtypes = [vp, gp, vp, pi, ci, vp, vp]
    lib.tnmf_hip_triggered_sums_plan.argtypes = [vp, gp, ci, pi, ci, ctypes.POINTER(sz)]
    lib.tnmf_hip_triggered_sums.argtypes = [vp, gp, vp, vp, ci, pi, ci, ci, vp, sz, vp, vp]
    ll = ctypes.c_longlong
    lib.tnmf_hip_events_render.argtypes = [vp, gp, vp, vp, ll, vp, vp, ll, vp, vp]
    lib.tnmf_hip_events_update.argtypes = [vp, gp, ci, vp, vp, vp, ll, vp, vp, cd, cd, vp]
    lib.tnmf_hip_events_grad_W.argtypes = [vp, gp, ci, vp, vp, vp, vp, ll, vp, vp, vp, vp, vp]
    lib.tnmf_hip_events_gain.argtypes = [vp, gp, ci, vp, vp, vp, ll, vp, vp, vp, vp, vp]
    lib.tnmf_hip_events_norms.argtypes = [vp, gp, ci, vp, vp, vp]
    lib.tnmf_hip_pursuit_score.argtypes = [vp, gp, vp, vp, vp, vp, ll, vp]
    lib.tnmf_hip_pursuit_pick.argtypes = [vp, gp, ci, vp, vp, ll, vp, vp, vp, vp, vp, vp, vp]
    lib.tnmf_hip_events_landscape.argtypes = [vp, gp, ci, vp, vp, vp, ll, vp, vp, vp, vp, vp, vp]
    lib.tnmf_hip_events_alternatives.argtypes = [vp, gp, ci, vp, vp, vp, ll, vp, vp, ci, ci, vp, vp, vp, vp]
    lib.tnmf_hip_events_pairs.argtypes = [vp, gp, vp, ll, vp, vp, ll, vp, sz, vp, vp]
    lib.tnmf_hip_events_gram.argtypes = [vp, gp, ci, vp, vp, ll, vp, vp, ll, vp, vp]
    lib.tnmf_hip_events_project.argtypes = [vp, gp, ci, vp, vp, ll, vp, vp, vp]
    lib.tnmf_hip_events_nnls.argtypes = [vp, ll, ll, vp, vp, vp, vp, vp, cd, ci, ci, vp, pi, ctypes.POINTER(cd), pi,
                                         ctypes.POINTER(cd), ci, pi, vp]
    lib.tnmf_hip_events_inverse_diag.argtypes = [vp, ll, ll, vp, vp, vp, ll, vp, pi, ll, vp, vp, vp, ll, vp, vp, vp]
    lib.tnmf_hip_events_patches.argtypes = [vp, gp, ci, ci, vp, vp, vp, ll, vp, vp, vp, vp, vp, ci, vp, vp]
    lib.tnmf_hip_patch_moments.argtypes = [vp, ci, ci, vp, vp, vp, vp, ll, ci, vp, vp, vp, vp, vp]
    lib.tnmf_hip_pad_H.argtypes = [vp, gp, ci, vp, vp, vp]
    lib.tnmf_hip_fold_H.argtypes = [vp, gp, ci, vp, vp, vp]
    for name in EXPORTS:
        fn = getattr(lib, name)
        if fn.restype is ctypes.c_int or name not in ('tnmf_hip_strerror', 'tnmf_hip_ctx_last_path'):
            fn.restype = ci
    if lib.tnmf_hip_abi_version() != ABI_VERSION:
        raise RuntimeError(f'{LIB_PATH}: ABI version {lib.tnmf_hip_abi_version()} != expected {ABI_VERSION}')
    _lib = lib
    return lib


def check(code: int, where: str) -> None:
    if code != 0:
        text = load().tnmf_hip_strerror(code)
        raise TnmfHipError(code, where, text.decode() if text else '?')


def make_geom(n: int, m: int, c: int, sample_shape: Sequence[int], atom_shape: Sequence[int], dtype_code: int,
              h_row_stride: int = 0) -> Geom:
    k = len(atom_shape)
    if k not in (1, 2, 3) or len(sample_shape) != k:
        raise NotImplementedError('the hip backend supports 1, 2 or 3 shift dimensions')
    g = Geom()
    g.ndim, g.N, g.M, g.C, g.dtype = k, int(n), int(m), int(c), int(dtype_code)
    for i in range(k):
        g.D[i] = int(sample_shape[i])
        g.A[i] = int(atom_shape[i])
    g.h_row_stride = int(h_row_stride)   # 0: C-contiguous activations
    return g

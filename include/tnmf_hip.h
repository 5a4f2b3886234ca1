/*
 * tnmf_hip.h -- C ABI of libtnmf_hip.so: the MI355X (gfx950) kernels behind the 'hip' backend of the
 * shift-invariant multiplicative-update loop of emdgroup/tnmf.
 *
 * The reference has no FFI on this path (it is pure Python); the boundary it does have is the Python class
 * tnmf/backends/_Backend.py:13-130.  Each entry point below names the reference method it stands under.  They are
 * bound from Python with ctypes (tnmf_amd/_lib.py); INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to a C-contiguous buffer owned by the caller (e.g. torch.Tensor.data_ptr());
 *     the library never frees or keeps it beyond the call.  `stream` is a hipStream_t passed as void* (NULL = default).
 *   - every function returns int: 0 ok, <0 argument error (TNMF_E_*), >0 a hipError_t.  Nothing throws.
 *   - element type: geom.dtype 0 = float32, 1 = float64.  'valid' reconstruction mode only:
 *       V[N,C,*D]  W[M,C,*A]  H[N,M,*(D+A-1)]  R[N,C,*D];   ndim = 1 or 2 shift axes.
 *   - mini-batch slices are contiguous along the sample axis: the caller offsets V/H/R pointers and passes the slice's N.
 *   - one context = one device.  SURVEY.md 8b sketched a multi-device context (tnmf_hip_ctx_create(device_ids[], n)) and
 *     an in-library tnmf_hip_allreduce_negpos; this library deliberately has neither: the product runs one process per
 *     GPU and the single collective of the path -- the sum of the [neg | pos] buffer of tnmf_hip_grad_W_fused -- is done
 *     by the caller between tnmf_hip_grad_W_fused and tnmf_hip_apply_W (torch.distributed / RCCL in tnmf_amd/backends/HIP.py).
 *   - calls on one ctx are not thread-safe; different ctxs are independent.  All launches are asynchronous on
 *     `stream` except tnmf_hip_energy, which synchronises the stream to return its scalar.
 */
#ifndef TNMF_HIP_H
#define TNMF_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 8 since the beta-divergence entry points; the weighted entry points came later as a purely additive change (no
 * existing signature or return code changed), so the version stayed 8. */
#define TNMF_HIP_ABI_VERSION 8

enum {
    TNMF_OK = 0,
    TNMF_E_NULL = -1,      /* required pointer is NULL */
    TNMF_E_GEOM = -2,      /* bad geometry (ndim, sizes <= 0, atom larger than supported) */
    TNMF_E_DTYPE = -3,     /* dtype not 0/1 */
    TNMF_E_WORKSPACE = -4, /* workspace allocation failed */
    TNMF_E_UNSUPPORTED = -5,
    TNMF_E_STRIDE = -6     /* h_row_stride > shift width, and the kernel family forced for this call wants C-contiguous H */
};

typedef struct tnmf_hip_ctx tnmf_hip_ctx;

typedef struct {
    int ndim;  /* 1, 2 or 3 shift axes (3: volumes, axes z, y, x -- see "Volumes" below) */
    int N;     /* samples in this call (mini-batch slice length) */
    int M;     /* atoms */
    int C;     /* channels */
    int D[3];  /* sample shape; the first ndim entries are used */
    int A[3];  /* atom shape;   the first ndim entries are used */
    int dtype; /* 0 = f32, 1 = f64 */
    /* Row stride of H in elements; 0 (or the shift width D[last] + A[last] - 1) = C-contiguous, as the reference's arrays
     * are.  A larger value describes activations whose rows are padded to whole cache lines: H[n,m,y,x] at
     * ((n*M + m)*Hy + y)*h_row_stride + x, the plane and sample strides following from it.  Supported where H is
     * streamed by the FFT family, the split kernel and the generic kernels -- everything TNMF_PATH_AUTO dispatches to for
     * such activations; only the f32 MFMA kernels want C-contiguous rows (AUTO skips them for padded ones; with
     * TNMF_PATH_MFMA forced the call answers TNMF_E_STRIDE and touches nothing -- the caller then passes a contiguous copy).
     * Outputs shaped like H (neg / pos of tnmf_hip_grad_H) are always C-contiguous. */
    int h_row_stride;
} tnmf_hip_geom;

/* Kernel family selection (tnmf_hip_ctx_set_path): AUTO picks the MFMA kernels where the shape allows and, for float32
 * problems with at least 2^19 activation entries, the HYBRID dispatch described below.  FFT is the
 * frequency-domain formulation (the algorithm of the reference's default backend, tnmf/backends/NumPy_FFT.py:16-40):
 * float32 2-D problems with shift shapes up to 576, float64 up to 288.  In float32 FFT is a W-ONLY path: the dictionary
 * and the energy of a fit stay within 1e-5 of a float64 reference, the activations do not (every gradient entry carries
 * ~1e-7 of the LARGEST entry as absolute transform error, and the H update divides two gradients); callers who need H at
 * float32 grade use AUTO / HYBRID, whose H update runs on the direct kernels. */
enum { TNMF_PATH_AUTO = 0, TNMF_PATH_GENERIC = 1, TNMF_PATH_MFMA = 2, TNMF_PATH_FFT = 3, TNMF_PATH_HYBRID = 4,
       TNMF_PATH_SPLIT = 5 };
/* HYBRID: reconstruct and the W gradient on the FFT family (their float32 transform error is benign: R has no small
 * entries, the W gradient is a sum over all samples), the H gradient / fused H update on the direct kernels (exact
 * summation of the few-tap border entries).  Falls back to AUTO where the FFT family does not cover the shape.
 * The FFT family (under FFT and HYBRID alike) assumes non-negative factors: R and the W gradient are clamped at zero
 * from below, which only removes transform rounding noise (V, W, H >= 0 imply both >= 0) and keeps the denominators
 * of the multiplicative updates non-negative. */

/* SPLIT: the direct kernels, with the H gradient / fused H update on the bf16 matrix cores: every float32 operand is
 * split exactly into three bf16 terms and a product is the sum of the six term products of weight >= 2^-16 -- float32-grade
 * results (error against a float64 reference no larger than the f32 MFMA chain's) at 16/6 of the f32 matrix rate.
 * MFMA keeps every kernel on the exact f32-input MFMA (a k-ordered fmaf chain).  AUTO and HYBRID use the split H update
 * where it covers the shape (float32, 2-D, atoms up to 16 x 16) unless tnmf_hip_ctx_set_split(ctx, 0) turned it off. */
int tnmf_hip_ctx_set_split(tnmf_hip_ctx *ctx, int enable);

/* tnmf_hip_run_schedule walks the operation list of a TINY resident problem inside ONE persistent kernel whose workgroups
 * meet at grid-wide barriers (generic.hip: k_schedule) -- which is only sound while every workgroup of the grid is
 * resident.  The library sizes that grid with an occupancy query of the kernel's real footprint on this device; when not
 * even that fits, or under mode 2 the runtime refuses the cooperative launch, the list is walked operation by operation
 * instead (same arithmetic, more launches).  mode 0: never use the persistent kernel (a caller that shares the GPU with
 * other processes -- CU masks, co-tenants -- should say so); 1 (default): plain launch of the occupancy-sized grid;
 * 2: the same grid through hipLaunchCooperativeKernel.  (The reference has no counterpart: its schedules are Python
 * loops, tnmf/TransformInvariantNMF.py:457-504.) */
int tnmf_hip_ctx_set_persistent(tnmf_hip_ctx *ctx, int mode);
/* 1 when the last tnmf_hip_run_schedule on this ctx ran as one persistent launch, 0 when it walked the list per operation. */
int tnmf_hip_ctx_last_schedule_persistent(const tnmf_hip_ctx *ctx);

int tnmf_hip_abi_version(void);
/* Row stride (elements) this context would like H of `geom` to have: the shift width itself, or -- when the H update runs
 * on the split kernel next to the FFT family -- the shift width rounded up to 32 floats, so that every 32-pixel tile of a
 * row is exactly one 128-byte line (267-float rows make each tile straddle two lines: 1.7x the H traffic, measured). */
int tnmf_hip_ctx_h_row_stride(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, int *stride_out);
const char *tnmf_hip_strerror(int code);

/* One context per device: caches device properties and owns the scratch (R, split-K partials). */
int tnmf_hip_ctx_create(int device_id, tnmf_hip_ctx **out);
int tnmf_hip_ctx_destroy(tnmf_hip_ctx *ctx);
/* Pre-size the scratch for `geom` so that later calls allocate nothing (graph-capture safe).  Also forgets a workspace
 * size the FFT family was refused earlier (such a size is otherwise not attempted again: under TNMF_PATH_AUTO the
 * direct kernels take over silently), so call it again after freeing device memory. */
int tnmf_hip_ctx_reserve(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom);
int tnmf_hip_ctx_set_path(tnmf_hip_ctx *ctx, int path);
/* Name of the kernel family the last primitive call on this ctx dispatched to ("generic", "mfma", "split", "fft"). */
const char *tnmf_hip_ctx_last_path(const tnmf_hip_ctx *ctx);
/* FFT family only: the library may keep the row spectra of the activations H it transformed or updated last, and the
 * spectra of the samples V it transformed last, and reuse them while the same pointers and geometry come back (the
 * reference's NumPy_CachingFFT.py:22-140 caches spectra the same way).  Off by default.  A caller that enables it
 * vouches that H changes only through this library and V not at all, and calls tnmf_hip_ctx_invalidate() after
 * writing either by any other means.  The spectra of the dictionary W are kept likewise, between the entry points that
 * write W (tnmf_hip_mu_update, _normalize_W, _apply_W, the group and atom-operator entry points, _run_schedule): a
 * caller who writes W by other means calls tnmf_hip_ctx_invalidate() as well, and that call is sufficient. */
int tnmf_hip_ctx_set_cache(tnmf_hip_ctx *ctx, int enable);
int tnmf_hip_ctx_invalidate(tnmf_hip_ctx *ctx);
/* The resident problem of a fit: geom->N samples of activations at H (row stride geom->h_row_stride) and of samples at V
 * (may be NULL).  With the cache enabled, a later call whose H pointer is a whole number of samples into this H -- a
 * mini-batch slice, the way the reference's backends receive `H[s]` (tnmf/backends/NumPy.py:77-80,101) -- works on the
 * matching sample range of ONE cache with per-sample validity: a Cyclic-MU epoch transforms every batch once, like a
 * full-batch iteration (the reference's counterpart: per-slice caches, tnmf/backends/NumPy_CachingFFT.py:143-158).
 * (TNMF_PATH_AUTO still picks the kernel family by the size of the slice itself: small batches take the direct kernels,
 * which read row-padded activations through the row stride.)  Without a binding the cache
 * follows the operands of the last call.  H == NULL or geom == NULL drops the binding.  The binding holds no reference:
 * the caller re-binds (or invalidates) when the buffers are replaced. */
int tnmf_hip_ctx_bind(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, const void *H, const void *V);
/* Observability of the cache: out[0] / out[1] = row-transform passes over activations that ran / were skipped because
 * the cache held every sample of the call, out[2] / out[3] the same for the samples V (counted since ctx creation). */
int tnmf_hip_ctx_cache_counters(const tnmf_hip_ctx *ctx, unsigned long long out[4]);

/* ---- primitives: API-parity path --------------------------------------------------------------------------- */

/* Backend.reconstruct (tnmf/backends/_Backend.py:120-122; NumPy.py:122-132):
 *   R[n,c,d] = sum_m sum_a H[n,m,d+a] * W[m,c,A-1-a] */
int tnmf_hip_reconstruct(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, const void *W, const void *H, void *R,
                         void *stream);

/* Backend.reconstruction_gradient_H (_Backend.py:110-118; NumPy.py:93-120):
 *   neg[n,m,u] = sum_c sum_a W[m,c,a] * Vpad[n,c,u+a],  pos = same with R.  R == NULL: R is computed internally. */
int tnmf_hip_grad_H(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, const void *V, const void *R_or_null,
                    const void *W, const void *H, void *neg, void *pos, void *stream);

/* Backend.reconstruction_gradient_W (_Backend.py:100-108; NumPy.py:69-91):
 *   neg[m,c,a] = sum_n sum_d H[n,m,d+A-1-a] * V[n,c,d],  pos = same with R.  Deterministic two-stage reduction. */
int tnmf_hip_grad_W(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, const void *V, const void *R_or_null,
                    const void *W, const void *H, void *neg, void *pos, void *stream);

/* TransformInvariantNMF._multiplicative_update (tnmf/TransformInvariantNMF.py:217-235), elementwise part:
 *   pos += reg (IN PLACE, as the reference does);  arr = (arr * neg) / pos.   dtype 0/1, n_elems elements. */
int tnmf_hip_mu_update(tnmf_hip_ctx *ctx, int dtype, void *arr, const void *neg, void *pos, double reg,
                       size_t n_elems, void *stream);

/* Backend.normalize over the atom axes (_Backend.py:75-77 as called from TransformInvariantNMF.py:237-238):
 *   W[m,c,:] /= sum_a W[m,c,a] */
int tnmf_hip_normalize_W(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, void *W, void *stream);

/* Backend.reconstruction_energy (_Backend.py:127-130): *out_host = 1/2 sum (V - R)^2 in double.  Synchronises. */
int tnmf_hip_energy(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, const void *V, const void *W, const void *H,
                    double *out_host, void *stream);

/* Backend.convolve_multi_1d (_Backend.py:79-81; _NumPyBackend.py:56-64): zero-padded 'same' convolution of
 * arr[rows, *shape] along each shift axis with an odd-length kernel (host pointers kernel0/kernel1, doubles). */
int tnmf_hip_convolve_multi_1d(tnmf_hip_ctx *ctx, int dtype, int ndim, size_t rows, const int *shape,
                               const void *in, void *out, void *tmp, const double *kernel0, int len0,
                               const double *kernel1, int len1, void *stream);

/* One axis of the same convolution, for any number of shift axes: arr viewed as [rows][len][inner], convolved along
 * `len` (zero-padded 'same', odd-length kernel of at most 127 taps, host doubles), out != in.  convolve_multi_1d over k
 * axes is k calls in the reference's order, first shift axis first (_NumPyBackend.py:60-62), ping-ponging two buffers --
 * how the three axes of a volume are done. */
int tnmf_hip_convolve_axis(tnmf_hip_ctx *ctx, int dtype, size_t rows, int len, size_t inner, const void *in, void *out,
                           const double *kernel, int klen, void *stream);

/* ---- Volumes (ndim == 3) -----------------------------------------------------------------------------------------
 * The reference takes any number of shift axes in NumPy (tnmf/backends/NumPy.py:69-132 contracts over all of them) and
 * one to three in PyTorch (tnmf/backends/PyTorch.py:13-17: conv1d / conv2d / conv3d).  With ndim == 3 the entry points
 * tnmf_hip_reconstruct, _grad_H, _grad_W, _grad_W_fused, _update_H, _apply_W, _normalize_W, _energy, _pad_H, _fold_H and
 * _ctx_reserve run direct kernels of their own (float32 and float64, C-contiguous activations: h_row_stride 0 or the
 * shift width), and so do tnmf_hip_update_H_ex and tnmf_hip_run_schedule (one launch chain per list); _mu_update, _axpby,
 * _sum_parts and _convolve_axis do not look at the geometry.  tnmf_hip_ctx_bind is accepted and has nothing to do.  tnmf_hip_ctx_last_path reads "volume". */

/* ---- reconstruction modes other than 'valid' --------------------------------------------------------------------
 * Every mode of the reference is a 'valid' reconstruction of padded activations (padding table:
 * tnmf/backends/_PyTorchBackend.py:42-52, applied in tnmf/backends/PyTorch.py:36-43): 'full' pads A-1 zeros on both
 * sides, 'circular' / 'reflect' pad A-1 wrapped / mirrored elements on the left.  The activation tensor of mode `mode`
 * has shift shape S = D-A+1 ('full') or D ('circular', 'reflect'); the padded one always has D+A-1, which is what all
 * the primitives above take.  The H gradient of a mode is the 'valid' gradient folded back by the adjoint of the pad.
 * TNMF_E_GEOM per shift axis: S < 1; 'circular' with A-1 > S (more than one wrap); 'reflect' with A-1 >= S (a mirror
 * without the edge).  'full' has no further limit: an atom may be as long as the sample. */
enum { TNMF_MODE_VALID = 0, TNMF_MODE_FULL = 1, TNMF_MODE_CIRCULAR = 2, TNMF_MODE_REFLECT = 3 };

/* Hpad[N,M,*(D+A-1)] = pad(H[N,M,*S]) */
int tnmf_hip_pad_H(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, int mode, const void *H, void *Hpad, void *stream);
/* G[N,M,*S] = pad^T(Gpad[N,M,*(D+A-1)]): every padded position's gradient is summed into the activation it copies */
int tnmf_hip_fold_H(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, int mode, const void *Gpad, void *G, void *stream);

/* ---- fused half steps: performance path (same math as the primitives + mu_update) --------------------------- */

/* TransformInvariantNMF._update_H without inhibition (TransformInvariantNMF.py:246-250,271):
 *   R = reconstruct(W,H);  H *= corr(W,V) / (corr(W,R) + eps + sparsity), in place.
 *   R_scratch: device buffer [N,C,*D] or NULL (ctx scratch is used).  r_is_valid != 0: R_scratch already holds
 *   reconstruct(W, H) (the caller ran tnmf_hip_reconstruct itself, e.g. to time the two kernels separately). */
int tnmf_hip_update_H(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, const void *V, const void *W, void *H_inout,
                      void *R_scratch, int r_is_valid, double eps, double sparsity, void *stream);

/* TransformInvariantNMF._update_H in full (TransformInvariantNMF.py:246-271), for every reconstruction mode:
 *   G   = kernel0 (*) kernel1 (*) H  along the shift axes, zeros outside (Backend.convolve_multi_1d, _NumPyBackend.py:56-64)
 *   pos += inhibition * (G - H) + cross_inhibition / (M - 1) * (sum over atoms of G - G)            (:256-269)
 *   H  *= neg / (pos + eps + sparsity)
 * kernel0 / kernel1 / kernel2: HOST pointers to the odd-length 1-D kernels of the shift axes, first axis first (ndim == 1:
 * kernel0 only, ndim == 2: kernel0 and kernel1), ignored when both strengths are 0.  mode == TNMF_MODE_VALID: H as for tnmf_hip_update_H (row stride honoured); the lateral terms are
 * computed by one kernel and enter the epilogue of the fused update (split kernel on row-padded H, generic kernels) or,
 * for the other families, one update kernel behind the unfused gradient.  Other modes: H is C-contiguous with the mode's
 * shift shape; the library pads it (work arrays of its own), runs the 'valid' kernels and applies fold + update in one
 * kernel.  R_scratch: device buffer [N,C,*D] or NULL.  Volumes (ndim == 3): the same step on the volume kernels -- three
 * passes of the 1-D convolution and one kernel for the lateral terms, pad / fold for the padded modes, one update kernel. */
int tnmf_hip_update_H_ex(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, int mode, const void *V, const void *W,
                         void *H_inout, void *R_scratch, double eps, double sparsity, double inhibition,
                         double cross_inhibition, const double *kernel0, int len0, const double *kernel1, int len1,
                         const double *kernel2, int len2, void *stream);

/* Local part of TransformInvariantNMF._update_W (TransformInvariantNMF.py:240-241 / :444-448):
 *   negpos[0] = neg_W, negpos[1] = pos_W as one contiguous [2,M,C,*A] buffer (what the all-reduce carries).
 *   R_scratch / r_is_valid as for tnmf_hip_update_H. */
int tnmf_hip_grad_W_fused(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, const void *V, const void *W, const void *H,
                          void *R_scratch, int r_is_valid, void *negpos, void *stream);

/* ---- mini-batch schedules in one call ---------------------------------------------------------------------------------
 * The stochastic schedules of the reference (ASG / GSG / ASAG / GSAG, TransformInvariantNMF.py:467-504, and Cyclic-MU,
 * :457-465) are chains of small dependent steps -- with batch_size 3, an H half step on 3 samples, a W gradient on the
 * same 3, a W update, 256 times per epoch -- whose cost driven batch by batch from the host is launch latency and
 * interpreter time.  tnmf_hip_run_schedule takes a whole epoch as a list of operations on sample ranges of the resident
 * problem and issues every kernel from one host call:
 *   TNMF_OP_UPDATE_H  H[n0:n1] *= corr(W, V) / (corr(W, R) + eps + sparsity)            (= tnmf_hip_update_H on the slice)
 *   TNMF_OP_GRAD_W    acc = a * acc + b * [neg | pos](V, H)[n0:n1]    (a == 0: acc = b * g; _accumulate_gradient_W,
 *                     :444-455, with (a, b) = (1, 1), (1 - lambda, lambda) or, from the integer start (0, 0), (0, lambda))
 *   TNMF_OP_APPLY_W   W = W * acc_neg / (acc_pos + eps), normalised; acc_pos is left incremented by eps (:232)
 * geom->N = samples of the resident problem (V, H_inout point at sample 0); acc: device buffer [2,M,C,*A] that persists
 * between calls where the schedule says so (ASAG / GSAG).  Single device: with several ranks the gradient must be summed
 * across them between GRAD_W and APPLY_W, which is the caller's collective.
 * A RUN of consecutive TNMF_OP_UPDATE_H operations on pairwise disjoint sample ranges is executed as the H half step of
 * their union (ranges sorted and joined where they touch): such steps commute -- the H update of a sample reads that sample
 * and W only, and W does not change inside the run -- so GSG-MU / GSAG-MU (:474-479, :493-504: H for every shuffled batch, W
 * from the last batch) cost one H half step over all samples per epoch, not one launch chain per batch.
 * The whole list is checked before anything runs, on one, two and three shift axes alike: an unknown kind is
 * TNMF_E_UNSUPPORTED, a range outside [0, N] or with n1 < n0 TNMF_E_GEOM (TNMF_OP_APPLY_W names no samples: its n0, n1 are
 * not read), and a refused list leaves W, H and acc as they were. */
enum { TNMF_OP_UPDATE_H = 0, TNMF_OP_GRAD_W = 1, TNMF_OP_APPLY_W = 2 };
typedef struct {
    int kind;    /* TNMF_OP_* */
    int n0, n1;  /* sample range [n0, n1) of the resident problem (may be empty) */
    double a, b; /* TNMF_OP_GRAD_W */
} tnmf_hip_op;
/* (Frobenius objective only: the beta-divergence steps below are driven step by step.) */
int tnmf_hip_run_schedule(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, const void *V, void *W_inout, void *H_inout,
                          void *R_scratch, void *acc, const tnmf_hip_op *ops, int n_ops, double eps, double sparsity,
                          void *stream);

/* acc = a * acc + b * g over n_elems elements (a == 0: acc = b * g, whatever acc held): the blend of
 * _accumulate_gradient_W (TransformInvariantNMF.py:444-455) for callers that drive the schedules step by step (several
 * ranks: the collective sits between the gradient and this). */
int tnmf_hip_axpby(tnmf_hip_ctx *ctx, int dtype, void *acc, const void *g, double a, double b, size_t n_elems,
                   void *stream);

/* Deterministic cross-rank reduction of the [neg | pos] buffer ("all-gather ... then sum in rank order"):
 *   out[i] = ((parts[0][i] + parts[1][i]) + parts[2][i]) + ...   for the n_parts buffers of n_elems elements that the
 * caller gathered one behind the other (rank order), in the element type.  Every rank that runs it on the same gathered
 * buffer gets the same bits, whatever protocol the collective library would have picked for an all-reduce.  The gather
 * itself is the caller's (torch.distributed.all_gather_into_tensor over RCCL in tnmf_amd/backends/HIP.py). */
int tnmf_hip_sum_parts(tnmf_hip_ctx *ctx, int dtype, const void *parts, int n_parts, size_t n_elems, void *out,
                       void *stream);

/* Rest of _update_W (TransformInvariantNMF.py:232-238,244): W = W * neg / (pos + eps); W /= sum over atom axes.
 * `pos` is left incremented by eps, like the reference's in-place `pos += eps`. */
int tnmf_hip_apply_W(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, void *W_inout, void *negpos, double eps,
                     void *stream);

/* ---- beta-divergence objectives (ABI 8) ----------------------------------------------------------------------------
 * D_beta(V | R): beta = 2 is the Frobenius objective of every entry above, 1 Kullback-Leibler, 0 Itakura-Saito, any other
 * finite beta the general form.  The multiplicative updates (Serizel et al. 2016, the mini-batch algorithms the reference
 * names, tnmf/TransformInvariantNMF.py:135-139) are those of the Frobenius objective with (V, R) replaced by the fields
 *   R~ = max(R, 0) + eps,   Q = V * R~^(beta-2),   P = R~^(beta-1)
 *   H <- H * corr_W(W, Q) / (corr_W(W, P) + eps + sparsity [+ lateral terms]),   W <- W * corr_H(H, Q) / (corr_H(H, P) + eps)
 * so every kernel family, reconstruction mode, row stride and lateral epilogue of the Frobenius steps runs unchanged on
 * (Q, P).  With beta == 2 every entry below IS its Frobenius counterpart (same call, same bits).  With beta != 2:
 *   - volumes (ndim == 3) answer TNMF_E_UNSUPPORTED and non-finite beta likewise, before anything is written;
 *   - Q lives in a work buffer of the context allocated by the first such call (tnmf_hip_ctx_reserve does not size it):
 *     a caller that captures the calls into a graph makes one warm-up call first;
 *   - P overwrites the reconstruction in R_scratch (or the context's scratch);
 *   - the FFT family never takes Q for the samples whose spectra it caches (Q has a fixed address and new contents every
 *     call): the spectra of V are neither reused nor recorded for it, those of H are kept as for the Frobenius steps.
 * tnmf_hip_run_schedule stays Frobenius-only. */

/* Q = V * R~^(beta-2), P = R~^(beta-1) elementwise over n_elems elements of type dtype.  beta 0, 1, 2: divisions and
 * products only (beta 1 writes P = 1); any other beta: pow in the element type.  P may alias R; nothing else may alias. */
int tnmf_hip_beta_fields(tnmf_hip_ctx *ctx, int dtype, double beta, double eps, const void *V, const void *R, void *Q,
                         void *P, size_t n_elems, void *stream);

/* tnmf_hip_update_H_ex for D_beta: reconstruct, fields, then the same correlations and update with (Q, P). */
int tnmf_hip_update_H_beta(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, int mode, const void *V, const void *W,
                           void *H_inout, void *R_scratch, double eps, double sparsity, double inhibition,
                           double cross_inhibition, const double *kernel0, int len0, const double *kernel1, int len1,
                           const double *kernel2, int len2, double beta, void *stream);

/* tnmf_hip_grad_W_fused for D_beta: negpos = [corr_H(H, Q) | corr_H(H, P)] as one [2,M,C,*A] buffer -- the same buffer
 * the collective carries and tnmf_hip_apply_W consumes.  r_is_valid != 0: R_scratch holds reconstruct(W, H) (it is
 * overwritten with P). */
int tnmf_hip_grad_W_beta(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, const void *V, const void *W, const void *H,
                         void *R_scratch, int r_is_valid, void *negpos, double beta, double eps, void *stream);

/* *out_host = sum D_beta(V | max(R, 0) + eps) in double (beta 1: V log(V/R~) - V + R~ with 0 log 0 = 0; beta 0:
 * V/R~ - log(V/R~) - 1), deterministic two-stage reduction.  beta == 2: tnmf_hip_energy.  Synchronises. */
int tnmf_hip_energy_beta(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, double beta, double eps, const void *V,
                         const void *W, const void *H, double *out_host, void *stream);

/* ---- weighted objectives (ABI 8, additive: the version stays 8) ------------------------------------------------------
 * sum G * D_beta(V | R) for an elementwise weight G >= 0 of V's shape and element type (a 0/1 mask of missing or
 * untrusted samples is the common case).  Its multiplicative updates are those above with both fields multiplied by G:
 *   beta != 2:  Q = G * V * R~^(beta-2),   P = G * R~^(beta-1)
 *   beta == 2:  Q = G * V,                 P = G * R          (no clamp, no eps: G == 1 is the Frobenius step)
 * Entries with G == 0 give Q = P = 0 by selection, and add exactly 0 to the energy: V may hold anything there (NaN and
 * inf included).  G is a device pointer laid out like V (mini-batch slices offset it like V).
 *   - G == NULL: each step / energy entry below IS its _beta counterpart (same call, same bits);
 *   - otherwise any finite beta, 2 included, runs reconstruct -> weighted fields -> the correlations on (Q, P), with
 *     everything the beta-divergence block above says about Q, P, R_scratch and the spectrum cache (the spectra of V
 *     are never used for a weighted step);
 *   - volumes (ndim == 3) and non-finite beta answer TNMF_E_UNSUPPORTED before anything is written.
 * tnmf_hip_run_schedule stays unweighted. */

/* G * (Q, P) elementwise over n_elems elements of type dtype (forms above).  G must not be NULL.  P may alias R; nothing
 * else may alias. */
int tnmf_hip_weighted_fields(tnmf_hip_ctx *ctx, int dtype, double beta, double eps, const void *V, const void *G,
                             const void *R, void *Q, void *P, size_t n_elems, void *stream);

/* tnmf_hip_update_H_beta for the weighted objective. */
int tnmf_hip_update_H_weighted(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, int mode, const void *V, const void *G,
                               const void *W, void *H_inout, void *R_scratch, double eps, double sparsity,
                               double inhibition, double cross_inhibition, const double *kernel0, int len0,
                               const double *kernel1, int len1, const double *kernel2, int len2, double beta,
                               void *stream);

/* tnmf_hip_grad_W_beta for the weighted objective (the same [neg | pos] buffer). */
int tnmf_hip_grad_W_weighted(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, const void *V, const void *G, const void *W,
                             const void *H, void *R_scratch, int r_is_valid, void *negpos, double beta, double eps,
                             void *stream);

/* *out_host = sum G * D_beta(V | max(R, 0) + eps), at beta == 2 sum 1/2 G (V - R)^2, in double with the deterministic
 * two-stage reduction of tnmf_hip_energy_beta.  Synchronises. */
int tnmf_hip_energy_weighted(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, double beta, double eps, const void *V,
                             const void *G, const void *W, const void *H, double *out_host, void *stream);

/* ---- per-sample objective and the objective tap (ABI 8, additive: the version stays 8) -------------------------------
 * The objective of one sample n is its share of what the energy entries above return: the sum over the sample's C * D
 * elements of 1/2 (V - R)^2, of D_beta(V | max(R, 0) + eps), or of G times either (G <= 0 selects exactly 0).  It is
 * summed in double by a two-stage reduction of fixed order without atomics; how a sample is cut into blocks depends on
 * C * D alone, so a sample's value does not depend on which other samples share the call.  Every H half step
 * materialises R = reconstruct(W, H as passed in) before it does anything else with it: the tap reads the objective off
 * that R, which makes watching convergence cost one pass over (V, R[, G]) instead of a reconstruction of its own. */

/* While per_sample_dev is not NULL, tnmf_hip_update_H, _update_H_ex, _update_H_beta and _update_H_weighted write
 * per_sample_dev[n], n in [0, geom->N), the objective of sample n of the call at (W, H_inout as passed in) -- of the
 * objective the entry point steps (Frobenius, D_beta, weighted), on 1, 2 or 3 shift axes, in every reconstruction mode,
 * r_is_valid or not -- right after the reconstruction, on the call's stream, without a host copy or a synchronisation.  The
 * step computes what it computes without the tap (the same bits in H_inout).  per_sample_dev: geom->N doubles on the device,
 * which must stay valid until the tap is cleared; NULL clears the tap.  The partial sums live in a work buffer of the
 * context that the first tapped call allocates (tnmf_hip_ctx_reserve does not size it).  tnmf_hip_run_schedule ignores
 * the tap. */
int tnmf_hip_ctx_set_objective_tap(tnmf_hip_ctx *ctx, double *per_sample_dev);

/* per_sample_dev[n] = the objective of sample n at (W, H): a reconstruction of its own into the context's scratch, then
 * the tap's kernel.  Asynchronous on the stream: no host copy, no synchronisation.  G_or_null != NULL: weighted.  The
 * restrictions of tnmf_hip_energy_weighted: non-finite beta answers TNMF_E_UNSUPPORTED, and volumes (ndim == 3) anything
 * but the unweighted Frobenius objective (beta == 2, G_or_null == NULL) likewise; a NULL operand or output answers
 * TNMF_E_NULL -- all before anything is written. */
int tnmf_hip_sample_objective(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, double beta, double eps, const void *V,
                              const void *G_or_null, const void *W, const void *H, double *per_sample_dev, void *stream);

/* ---- atom terms: what each atom explains (ABI 8, additive: the version stays 8) ------------------------------------------
 * With R_m the contribution of atom m in all its orientations -- the planes m * group + t, t < group, of H and W -- and
 * d = V - R:   a[n, m] = sum G R_m[n] d[n],   b[n, m] = sum G R_m[n]^2   (G = 1 without weights), so that
 *   1/2 ||V[n] - (R[n] - R_m[n])||^2 - 1/2 ||V[n] - R[n]||^2 = a[n, m] + b[n, m] / 2     (the weighted norms with G)
 * in the unit of tnmf_hip_events_gain; 1 + a / b is the optimal rescaling of the atom alone.  One pass over H with the
 * arithmetic of a reconstruct: r_m[c, x] = sum_{t < group} sum_a Hpad[n, m group + t, x + a] W[m group + t, c, A-1-a] in
 * the element type (the blocks' planes summed before r is squared), r (G d) and G r^2 accumulated in double, each
 * workgroup's sums combined in a fixed order (partial sums per (sample, tile, atom), then their ordered sum): no
 * floating-point atomics, the same bits from run to run.  Entries of weight <= 0 add exactly 0, whatever V holds there. */

/* a, b of every atom: ab[(n*(M/group) + m)*2 + {0,1}] (double, device), for geom->M planes in blocks of `group`
 * (the T orientations of one atom; group = 1 without transforms).  H: padded activations [N, M, *(D+A-1)], row stride
 * honoured.  W: the M planes (W, or W_eff).  G_or_null: weights of V's shape and dtype.  R_or_null: reconstruct(W, H);
 * NULL: computed into the ctx scratch by the ctx's kernel family.  Every element of ab is written.  Asynchronous on the
 * stream.  The partial sums and a re-ordered copy of W live in a work buffer of the context that the first call allocates
 * (tnmf_hip_ctx_reserve does not size it).
 * TNMF_E_GEOM: group < 1 or M % group != 0.  TNMF_E_UNSUPPORTED: ndim == 3, or an atom whose tile of H (16 + A_y - 1
 * rows of 64 + 4 ceil((A_x + 1) / 4) elements; one shift axis: one row of 1024 + 4 ceil((A + 1) / 4)) exceeds 60 KiB.
 * A refused call writes nothing. */
int tnmf_hip_atom_terms(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, int group, const void *V, const void *G_or_null,
                        const void *R_or_null, const void *W, const void *H, double *ab, void *stream);

/* ---- atom Gram: how atoms overlap (ABI 8, additive: the version stays 8) ------------------------------------------------
 * With R_m and d as under "atom terms":   B[n, m, m'] = sum G R_m[n] R_m'[n]   (G = 1 without weights): diag(B) is b, and
 * with per-atom scale factors s (R(s) = sum s_m R_m) the objective of sample n is the exact quadratic
 *   E(s) = E(1) - a^T (s - 1) + 1/2 (s - 1)^T B (s - 1);      without the atoms of a set S (s_S = 0): + sum_S a + 1/2 sum_SS B.
 * One pass over H: r_m as for the atom terms, one channel at a time, parked in LDS per pixel tile for up to 32 (float) or
 * 16 (double) atoms; the sums over the tile's pixels on the matrix cores (v_mfma_f64_16x16x4_f64), operands G r_m (the
 * product in double) and r_m' converted to double, accumulated in double over a strip of 16 tiles per workgroup; with more
 * atoms every pair of atom blocks is a workgroup of its own (512 threads in two halves with 32 rows, else 256).  Partial
 * sums per (sample, strip, block pair), then their sum in strip order: no floating-point atomics, the same bits from run
 * to run; B[n, m, m'] and B[n, m', m] are the same sum.
 * Entries of weight <= 0 add exactly 0, whatever V holds there. */

/* a[n*(M/group) + m] and B[(n*(M/group) + m)*(M/group) + m'] (double, device), B symmetric and written in full, in the
 * order of H's atoms; per sample.  Operands, `group`, G_or_null, R_or_null, the row stride of H and the work buffer as for
 * tnmf_hip_atom_terms.  Every element of a and B is written.  Asynchronous on the stream.
 * TNMF_E_GEOM: group < 1 or M % group != 0.  TNMF_E_UNSUPPORTED: ndim == 3, or an atom whose tile of H (as for
 * tnmf_hip_atom_terms) does not fit the 160 KiB of LDS next to the parked rows: 16 rows of 1040 elements, the tile's
 * weights and 512 bytes.  A refused call writes nothing. */
int tnmf_hip_atom_gram(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, int group, const void *V, const void *G_or_null,
                       const void *R_or_null, const void *W, const void *H, double *a, double *B, void *stream);

/* ---- atom terms, beta: what each atom explains under a beta-divergence (ABI 8, additive: the version stays 8) -----------
 * With R_m and r = R_m[n] as under "atom terms", x = max(R, 0) + eps, x_m = max(R - r, 0) + eps and D_beta the element
 * divergence of tnmf_hip_energy_beta:
 *   gain[n, m]  = sum G (D_beta(V | x_m) - D_beta(V | x))       what the sample's objective rises by without atom m: exact
 *   a[n, m]     = sum G r (V x^(beta-2) - x^(beta-1))           = <R_m, Q - P> of tnmf_hip_beta_fields: -dE/ds_m at s = 1
 *   b[n, m]     = sum G r^2 c,   c = (beta-1) x^(beta-2) + (2-beta) V x^(beta-3)                        d^2E/ds_m^2 at s = 1
 *   B[n, m, m'] = sum G c r_m r_m'                              diag(B) = b
 * (G = 1 without weights).  E(s) ~ E(1) - a^T (s - 1) + 1/2 (s - 1)^T B (s - 1) in per-atom scale factors is the local
 * second-order model, exact only at beta = 2.  c is negative where V > x (beta-1) / (beta-2) for beta > 2 and where
 * V < x (1-beta) / (2-beta) for beta < 1: the weights G c are signed, b and diag(B) can be negative, and only G <= 0
 * selects an exact zero (whatever V holds there).
 * The walk over H, r in the element type, the partial sums and their order are those of tnmf_hip_atom_terms and
 * tnmf_hip_atom_gram: no floating-point atomics, the same bits from run to run.  The pixel factors G (V x^(beta-2) -
 * x^(beta-1)) and G c are formed in double from the element-type V, R and G (no pow for beta 0 and 1) and rounded once to
 * the element type; r times them and, for B, (G c) r_m times r_m' are accumulated in double.  The gain term of a pixel is
 * evaluated in double, R - r in double, in forms in which nothing cancels where r is small beside R --
 *   beta 1: V log(x / x_m) + (x_m - x)  (x_m - x where V == 0);    beta 0: V (1 / x_m - 1 / x) + log(x_m / x);
 *   else:   [(beta-1) (x_m^beta - x^beta) - beta V (x_m^(beta-1) - x^(beta-1))] / (beta (beta-1)),
 * the logarithm as log1p((x - x_m) / x_m), the differences of powers as x^p expm1(p log(x_m / x)) -- and a pixel with
 * r == 0 or G <= 0 adds an exact 0 without evaluating anything.  Where an atom alone explains a pixel with V > 0 (x_m
 * = eps) the term is of the size V log(R / eps): the objective's own.
 * beta == 2 runs the kernels of tnmf_hip_atom_terms / tnmf_hip_atom_gram (d = V - R: no clamp, no eps): a, b and B are
 * theirs bit for bit, and gain = a + b / 2 in double. */

/* a, b, gain of every atom: abg[(n*(M/group) + m)*3 + {0,1,2}] (double, device).  Operands, `group`, G_or_null, R_or_null
 * (NULL: reconstructed into the ctx scratch by the ctx's kernel family), the row stride of H and the work buffer as for
 * tnmf_hip_atom_terms (three partial sums per (sample, tile, atom) instead of two; at beta == 2 the two of
 * tnmf_hip_atom_terms and its (a, b) behind the taps).  eps: the model's, >= 0.  Every element of abg is written.
 * Asynchronous on the stream.
 * TNMF_E_GEOM: group < 1, M % group != 0, a beta that is not finite, or eps < 0 (or NaN).  TNMF_E_UNSUPPORTED: as
 * tnmf_hip_atom_terms.  A refused call writes nothing. */
int tnmf_hip_atom_terms_beta(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, int group, double beta, double eps, const void *V,
                             const void *G_or_null, const void *R_or_null, const void *W, const void *H, double *abg,
                             void *stream);

/* a[n*(M/group) + m] and B[(n*(M/group) + m)*(M/group) + m'] (double, device) as defined above, B symmetric and written in
 * full.  Everything else as for tnmf_hip_atom_gram, whose plan, partial sums and finalize it shares.
 * TNMF_E_GEOM: group < 1, M % group != 0, a beta that is not finite, or eps < 0 (or NaN).  TNMF_E_UNSUPPORTED: as
 * tnmf_hip_atom_gram.  A refused call writes nothing. */
int tnmf_hip_atom_gram_beta(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, int group, double beta, double eps, const void *V,
                            const void *G_or_null, const void *R_or_null, const void *W, const void *H, double *a, double *B,
                            void *stream);

/* ---- sources: per-source signals by soft masks (ABI 8, additive: the version stays 8) -------------------------------------
 * A source is a set of planes of H and W (an atom in all its orientations, or several atoms).  With r_g[c, x] the sum of
 * what the planes of source g add to R -- r of "atom terms", in the element type -- and total = sum r over EVERY plane, the
 * planes in no source included:
 *   TNMF_SOURCES_CONTRIBUTION  out[n, g, c, x] = r_g
 *   TNMF_SOURCES_MASK          out[n, g, c, x] = r_g / (total + eps)
 *   TNMF_SOURCES_MASKED        out[n, g, c, x] = V * (r_g / (total + eps))        (evaluated in that order)
 *   TNMF_SOURCES_DOMINANT      label[n, x] = the g with the largest sum_c r_g (the lowest g of a tie; -1 where sum_c total
 *                              is 0),  share[n, x] = that sum / (sum_c total + eps)
 * One pass over H on the walk of tnmf_hip_atom_terms, the planes in the order the sources list them; r_g is stored raw when
 * its last plane is in, and after the last plane every thread rewrites its own stores over the total it then holds: the
 * denominator is the pass's own ordered sum of the numerators (source 0 first, the unlisted planes last), so r_g <= total
 * as computed and 0 <= mask <= 1, 0 <= masked <= V (V >= 0) hold without a clamp, whatever reconstruct() would give for R.
 * Where total + eps is 0 the mask, the masked value and the share are 0.  For TNMF_SOURCES_DOMINANT sum_c r_g is the same
 * walk on one channel whose taps are sum_c W, the channels added in channel order.  No atomics: one writer per element, the
 * same bits from run to run. */
#define TNMF_SOURCES_CONTRIBUTION 0
#define TNMF_SOURCES_MASK 1
#define TNMF_SOURCES_MASKED 2
#define TNMF_SOURCES_DOMINANT 3

/* plane_order[source_start[g] .. source_start[g + 1]), g < n_sources, are the planes of source g: n_listed ints and
 * n_sources + 1 ints, in host or device memory (they are read, checked and completed on the host before anything is
 * launched: the call waits for the stream once); the planes of [0, geom->M) that are not listed follow in ascending order
 * as a hidden last group.  H: padded activations [N, M, *(D+A-1)], row stride honoured.  W: the M planes.  V: read for
 * TNMF_SOURCES_MASKED only.  out: [N, n_sources, C, *D] in the element type, every element written (NULL for
 * TNMF_SOURCES_DOMINANT); label (int) and share (element type): [N, *D], every element written (for
 * TNMF_SOURCES_DOMINANT only).  The kernels are asynchronous on the stream.  The work buffer is that of
 * tnmf_hip_atom_terms.
 * TNMF_E_NULL: a pointer the call reads or writes is NULL.  TNMF_E_GEOM: n_sources < 1, emit not one of the four, eps
 * negative or not a number, n_listed outside [n_sources, M], source_start not 0 = s[0] < s[1] < ... < s[n_sources] =
 * n_listed, a plane outside [0, M) or listed twice.  TNMF_E_UNSUPPORTED: ndim == 3, or a tile of H beyond the LDS limit of
 * tnmf_hip_atom_terms.  A refused call writes nothing. */
int tnmf_hip_atom_sources(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, int n_sources, const int *plane_order, int n_listed,
                          const int *source_start, int emit, double eps, const void *V, const void *W, const void *H,
                          void *out, int *label, void *share, void *stream);

/* ---- transform groups: rotation and mirror invariance (ABI 8, additive: the version stays 8) -------------------------
 * A dictionary W[M,C,*A] stands for M * T effective atoms W_eff[m*T + t] = T_t(W[m]), every T_t a permutation of the
 * atom's pixels.  The groups, with t in the order below (numpy, a = W[m, c]):
 *   TNMF_GROUP_FLIP      T = 2   a, a[..., ::-1]                       (1 or 2 shift axes; 2: mirror along x)
 *   TNMF_GROUP_MIRRORS   T = 4   a, a[:, ::-1], a[::-1, :], a[::-1, ::-1]   (2 shift axes)
 *   TNMF_GROUP_ROT90     T = 4   np.rot90(a, k), k = 0..3             (2 shift axes, square atoms)
 *   TNMF_GROUP_DIHEDRAL  T = 8   np.rot90(a, k), k = 0..3, then np.rot90(a[:, ::-1], k), k = 0..3   (likewise)
 * Every other entry point runs the effective problem as it is: H[N, M*T, *shift], W_eff[M*T, C, *A].  The W half step
 * takes the gradient of W_eff (tnmf_hip_grad_W_fused / _beta / _weighted on W_eff), folds it onto W with the adjoint of
 * the expansion, neg[m] = sum_t T_t^-1(neg_eff[m*T + t]) and likewise pos -- BEFORE the collective, which then carries
 * the M-atom buffer -- and updates W as tnmf_hip_apply_W does, then expands W into W_eff again.
 * `geom` describes the dictionary: M atoms (the effective count follows from the group), C, ndim and A; N and D are not
 * read.  Volumes (ndim == 3), unknown groups, groups of two axes on one, and ROT90 / DIHEDRAL on non-square atoms answer
 * TNMF_E_UNSUPPORTED before anything is written.  Every entry that writes W_eff drops the FFT family's cached spectra of
 * the dictionary (W_eff keeps its address and changes its contents), as tnmf_hip_apply_W does.
 * tnmf_hip_run_schedule has no transformed form. */
enum { TNMF_GROUP_FLIP = 0, TNMF_GROUP_MIRRORS = 1, TNMF_GROUP_ROT90 = 2, TNMF_GROUP_DIHEDRAL = 3 };

/* W_eff[M*T,C,*A] = the expansion of W[M,C,*A] (a permutation: exact). */
int tnmf_hip_group_expand_W(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, int group, const void *W, void *W_eff,
                            void *stream);

/* negpos[2,M,C,*A] = the fold of negpos_eff[2,M*T,C,*A]: the T terms of each element summed in ascending t in double,
 * rounded once to the element type (the float64 fold, rounded). */
int tnmf_hip_group_fold_grad_W(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, int group, const void *negpos_eff,
                               void *negpos, void *stream);

/* The single-rank W step after the gradient of W_eff, in one launch: fold, W = W * neg / (pos + eps), W /= its sum over
 * the atom axes, W_eff = the expansion of the new W.  Same bits as tnmf_hip_group_fold_grad_W, tnmf_hip_apply_W and
 * tnmf_hip_group_expand_W in a row; negpos_eff is only read (the folded pos + eps is not kept). */
int tnmf_hip_group_apply_W(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, int group, void *W_inout, void *W_eff_out,
                           const void *negpos_eff, double eps, void *stream);

/* ---- atom operators: arbitrary-angle rotation and scale invariance (ABI 8, additive: the version stays 8) -------------
 * The transform groups above widened to any T non-negative linear maps L_t of an atom's pixels, the same for every
 * channel: W_eff[m*T + t, c] = L_t W[m, c], and the W half step folds with the transpose, neg[m, c] = sum_t
 * L_t^T neg_eff[m*T + t, c] (pos likewise) -- before the collective, as for the groups.  Every other entry point runs the
 * effective problem as it is.  The maps live in a handle made for one context:
 *   tnmf_hip_atom_ops_create takes the entries (t[k], out_px[k], in_px[k], w[k]), k < nnz, of (L_t a)[out] =
 *   sum w * a[in] -- pixels as flat C-order indices of the atom of `ndim` axes `A`, weights host doubles -- and builds two
 *   gather tables on the device: per (t, out pixel) its taps in ascending in pixel, per in pixel its entries in ascending
 *   (t, out pixel).  Refused before anything is allocated: volumes (ndim == 3: TNMF_E_UNSUPPORTED), other ndim, sizes
 *   <= 0, T <= 0, nnz < 0, indices out of range and a triple (t, out, in) given twice (TNMF_E_GEOM), weights that are
 *   not finite or negative (TNMF_E_UNSUPPORTED), NULL arrays (TNMF_E_NULL).  *out is written only on success.
 *   tnmf_hip_atom_ops_destroy frees a handle (NULL: nothing to do); destroy the handles of a context before the context.
 * Every output element is the sum of its products w * x in table order, in double with the multiplies and adds rounded
 * separately, rounded once to the element type: deterministic, and for the tables of a group (weight 1, one tap, t in the
 * group's order) the same bits as the tnmf_hip_group_* entry points.  `geom` describes the dictionary (M atoms, C, ndim,
 * A; N and D are not read); an ndim or A other than the handle's answers TNMF_E_GEOM, a handle of another context and
 * volumes TNMF_E_UNSUPPORTED, a NULL pointer TNMF_E_NULL, all before anything is written.  Every entry that writes W_eff
 * drops the FFT family's cached spectra of the dictionary.  tnmf_hip_run_schedule has no operator form. */
typedef struct tnmf_hip_atom_ops tnmf_hip_atom_ops;

int tnmf_hip_atom_ops_create(tnmf_hip_ctx *ctx, int ndim, const int *A, int T, int nnz, const int *t,
                             const int *out_px, const int *in_px, const double *w, tnmf_hip_atom_ops **out);
int tnmf_hip_atom_ops_destroy(tnmf_hip_atom_ops *ops);

/* W_eff[M*T,C,*A] = the expansion of W[M,C,*A]. */
int tnmf_hip_ops_expand_W(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, const tnmf_hip_atom_ops *ops, const void *W,
                          void *W_eff, void *stream);

/* negpos[2,M,C,*A] = the fold of negpos_eff[2,M*T,C,*A] (the adjoint of the expansion). */
int tnmf_hip_ops_fold_grad_W(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, const tnmf_hip_atom_ops *ops,
                             const void *negpos_eff, void *negpos, void *stream);

/* The single-rank W step after the gradient of W_eff, in one launch of one workgroup per (m, c) row: fold, W = W * neg /
 * (pos + eps), W /= its sum over the atom axes (the reduction of tnmf_hip_apply_W), W_eff = the expansion of the new W
 * (the row staged in LDS: rows of more than 64 KiB answer TNMF_E_GEOM).  Same bits as tnmf_hip_ops_fold_grad_W,
 * tnmf_hip_apply_W and tnmf_hip_ops_expand_W in a row; negpos_eff is only read. */
int tnmf_hip_ops_apply_W(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, const tnmf_hip_atom_ops *ops, void *W_inout,
                         void *W_eff_out, const void *negpos_eff, double eps, void *stream);

/* ---- detections: thresholded, non-maximum-suppressed peaks of H (ABI 8, additive: the version stays 8) ---------------
 * The read-out of a fit.  H is viewed as [N, P, *S]: P = geom->M planes (with transforms the M * T effective atoms) of
 * shift shape S = D + A - 1, rows `h_row_stride` apart (pad columns are neither read nor reported), on 1, 2 or 3 shift
 * axes.  `geom` describes H as it does everywhere; the activations of a reconstruction mode other than 'valid' have
 * another shift shape S (see "reconstruction modes" above): for those the caller passes D = S and A = 1 on every shift
 * axis.  C is not read.  Nothing wraps around in any mode.
 * The entry (n, p, u) with value h is a detection iff h > threshold (strict; threshold >= 0) and no competitor suppresses
 * it.  Its competitors are the other entries (n, q, v) of the same sample with |v_k - u_k| <= radius[k] on every shift
 * axis k, inside the plane, and q in the run of `group` consecutive planes [g * group, (g + 1) * group) that holds p
 * (group 1: its own plane; T: the orientations of its atom; P: every plane).  A competitor suppresses it when its value is
 * larger, or equal with the lower flat C-order index in [N, P, *S] -- one winner per plateau and neighbourhood.  NaN
 * compares false: never a detection, never a suppressor.  radius 0 everywhere with group 1 is a pure threshold; a radius
 * at or beyond the extent of an axis means the whole axis.
 * Output: count_out (one unsigned 64-bit word on the device) is zeroed on the stream, then counts EVERY detection; the
 * detections are appended in no particular order as idx_out[slot] = flat C-order index in [N, P, *S] of the H passed (a
 * mini-batch slice counts from its own first sample), val_out[slot] = the entry's bits in the element type, while
 * slot < capacity.  Nothing is written at or beyond `capacity`; a count above it tells the caller the size to come back
 * with.  Asynchronous like the other entry points: the caller reads count_out.
 * TNMF_E_GEOM: a negative radius, group < 1 or not a divisor of geom->M, sizes <= 0, a row stride below the shift width;
 * TNMF_E_UNSUPPORTED: a threshold that is negative or NaN; TNMF_E_NULL, TNMF_E_DTYPE as usual (idx_out / val_out may be
 * NULL when capacity is 0) -- all before anything is written. */
int tnmf_hip_find_peaks(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, const void *H, double threshold, const int *radius,
                        int group, long long *idx_out, void *val_out, size_t capacity, unsigned long long *count_out,
                        void *stream);

/* ---- activation correlogram: which planes co-occur, and at what offset (ABI 8, additive: the version stays 8) -------------
 * The second-order structure of the activations.  H is viewed as [N, P, *S] exactly as under "detections": P = geom->M
 * planes of shift shape S = D + A - 1 (the caller passes D = S, A = 1 for H as it is in any reconstruction mode), rows
 * `h_row_stride` apart, pad columns never read; C is not read.  1 or 2 shift axes.  For the lags |D_k| <= L_k = max_lag[k]
 *   C[n, p, q, D] = sum_u H[n, p, u] H[n, q, u + D]     over the u with u and u + D inside the plane (nothing wraps),
 * stored at index D_k + L_k of axis k: C_out is [P, P, *(2 L + 1)] doubles on the device, the sum over the samples, or with
 * per_sample != 0 [N, P, P, *(2 L + 1)].  Every element is written; lags at or beyond the extent of an axis are exactly 0.
 * C[p, q, D] and C[q, p, -D] are the same sum and have the same bits.
 * Arithmetic: both operands converted to double, the products and sums on v_mfma_f64_16x16x4_f64 -- for float H every
 * product is exact.  Blocks of 16 planes, every ordered pair of blocks a workgroup of its own, and only the half of the
 * lags that is >= 0 in C order; per (sample, pixel tile) the tile of the first block (one axis: 256 pixels, double 128; two:
 * 4 x 64, double 2 x 64) and the window of the second that it meets under one chunk of lags -- one D_y, up to 32 consecutive D_x --
 * are staged in LDS.  Partial sums per (sample with per_sample, else the whole call; strip of (sample, tile) items; block
 * pair; lag) live in the work buffer of tnmf_hip_atom_terms and are added in strip order by a second kernel that also
 * writes the mirror: no floating-point atomics, the same bits from run to run.
 * Limits: max_lag <= 1023 with one shift axis, <= 63 per axis with two; any P.  Asynchronous on the stream.
 * TNMF_E_UNSUPPORTED: ndim == 3, a lag beyond that limit, more than 2^31 - 1 workgroups.  TNMF_E_GEOM: any other ndim, a
 * negative lag, sizes <= 0 (N < 0), a row stride below the shift width.  TNMF_E_NULL (ctx, geom, max_lag, C_out, and H
 * with N > 0) and TNMF_E_DTYPE as usual -- all before anything is written. */
int tnmf_hip_activation_correlogram(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, const void *H, const int *max_lag,
                                    int per_sample, double *C_out, void *stream);

/* ---- triggered sums: the data around the places where a plane fires (ABI 8, additive: the version stays 8) -----------------
 * The W gradient's own correlation on a window larger than the atom.  geom describes the samples as everywhere (N, M = P
 * planes, D, A, dtype, h_row_stride; C is not read).  H is the PADDED activations [N, P, *(D + A - 1)] (the padding table
 * of "reconstruction modes"), rows `h_row_stride` apart, pad columns never read; Y is [N, n_fields, *D], C-contiguous, of
 * the geometry's dtype: the data, the reconstruction, the residual, the weights.  With a margin m_k >= 0 per shift axis
 *   X[p, f, j] = sum_n sum_q H[n, p, q]^power * Y[n, f, q - (A - 1) - m + j]      0 <= j_k < A_k + 2 m_k, power 1 or 2,
 * over the terms whose index of Y lies inside the sample: X_out is [P, n_fields, *(A + 2 m)] doubles on the device, or
 * with per_sample != 0 [N, P, n_fields, *(A + 2 m)].  Every element is written; an entry with no term is an exact 0, and
 * N = 0 gives zeros for the summed form.  At m = 0 and power 1 this is `neg` (Y = V) and `pos` (Y = R) of the W gradient.
 * 1 or 2 shift axes.
 * Arithmetic: both operands converted to double, the square of power = 2 taken in double (exact for float H), products and
 * sums on v_mfma_f64_16x16x4_f64: 16 planes of H are the rows, 16 consecutive window columns of one (field, window row)
 * the columns -- the B operand is a Toeplitz read of one staged row of Y -- and 4 pixels along x the contraction.  Per
 * (sample, pixel tile) the tile of 16 planes (one axis: 256 pixels, double 128; two: 4 x 64, double 2 x 64) and the patch
 * of Y it meets under one chunk of up to 32 such cells are staged in LDS.  Partial sums per (sample with per_sample, else
 * the whole call; strip of (sample, tile) items; block of 16 planes; cell) are added in strip order by a second kernel: no
 * floating-point atomics, the same bits from run to run.
 * The work buffer is the CALLER's (as the workspace of tnmf_hip_events_grad_W): tnmf_hip_triggered_sums_plan writes the
 * bytes the call with the same geom, n_fields, margin and per_sample needs into *work_bytes (0 with N = 0) and refuses
 * exactly what the call refuses, so a caller learns TNMF_E_UNSUPPORTED before it allocates.  The context's own buffers
 * are not touched.
 * Limits: a window A + 2 m <= 4096 with one shift axis, <= 128 per axis with two; any P, any n_fields.  Asynchronous on
 * the stream.
 * TNMF_E_NULL: ctx, geom, margin, X_out (work_bytes of _plan), work with work_bytes > 0, H or Y with N > 0.  TNMF_E_DTYPE.
 * TNMF_E_GEOM: ndim not 1..3, sizes <= 0 (N < 0), a negative margin, n_fields < 1, power not 1 or 2, a row stride below the
 * shift width.  TNMF_E_UNSUPPORTED: ndim == 3, a window beyond that limit, more than 2^31 - 1 workgroups or outputs.
 * TNMF_E_WORKSPACE: work_bytes below the plan's -- all before anything is written. */
int tnmf_hip_triggered_sums_plan(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, int n_fields, const int *margin,
                                 int per_sample, size_t *work_bytes);
int tnmf_hip_triggered_sums(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, const void *H, const void *Y, int n_fields,
                            const int *margin, int power, int per_sample, void *work, size_t work_bytes,
                            double *X_out, void *stream);

/* ---- events: render, refit and learn from a list of detections (ABI 8, additive: the version stays 8) -----------------------------
 * The H side with the activations held as a list.  An EVENT is (n, p, u, h): local sample n, plane p of the effective
 * dictionary W_eff[P, C, *A] (P = geom->M; with transforms p = atom * T + transform), shift index u in the activations of
 * the reconstruction mode (shift shape S, "reconstruction modes" above), strength h, finite and >= 0.  geom describes the
 * samples as everywhere (N, C, D, A, dtype; h_row_stride is not read): 1 or 2 shift axes, float32 or float64.
 * Every mode is a 'valid' reconstruction of padded activations, so an entry at padded position q adds h * W_eff[p, c, j]
 * to R[n, c, q - (A - 1) + j], 0 <= j < A, wherever that lies inside the sample.  An event stands for its IMAGES in the
 * padded frame [D + A - 1]; per shift axis, with a the atom extent and S the shift extent:
 *   valid      q = u
 *   full       q = u + a - 1
 *   circular   q = u + a - 1, and also q = u - (S - (a - 1)) when u >= S - (a - 1)
 *   reflect    q = u + a - 1, and also q = (a - 1) - u when 1 <= u <= a - 1
 * (the padding table read backwards).  The images of an event are the Cartesian product over the axes: at most 2^ndim.
 *
 * tnmf_hip_events_render: R[N, C, *D] = the sum over all images of strength[event] * W_eff[plane], placed as above.  It
 * is a gather without atomics -- the same list gives the same bits run after run, duplicates add up -- and writes every
 * element of R exactly once, zeros included: R needs no initialisation and is never read.  THE IMAGE LIST is the caller's
 * to build, once per support (only the strengths change between the steps of a refit):
 *   - cells of TNMF_EVENTS_CELL_1D padded positions (ndim == 1), TNMF_EVENTS_CELL_2D x TNMF_EVENTS_CELL_2D (ndim == 2)
 *     tile the padded frame, nc[i] = ceil((D[i] + A[i] - 1) / cell) per axis; the cell of an image at q is q / cell per
 *     axis, its key (n * nc[0] + cell_0) * nc[1] + cell_1 (ndim == 1: n * nc[0] + cell_0);
 *   - images: n_images rows of four ints (plane, q_0, q_1, event) (ndim == 1: (plane, 0, q_0, event)), `event` the index
 *     into `strength` [n_events], sorted by ascending key; the order inside a cell is free and fixes the order of the
 *     additions;
 *   - cell_start: N * nc[0] * nc[1] + 1 ints, cell_start[key] = the first row of that key (the rows of a key end where
 *     the next begins), cell_start[last] = n_images -- a searchsorted of 0 .. number of keys in the sorted keys.
 *   The list lives on the device, so its CONTENTS cannot be refused by an asynchronous call: a row whose plane or event is
 *   out of range is skipped and cell_start is clamped to [0, n_images] -- nothing is read or written out of bounds -- and
 *   a row filed under the wrong key is simply not seen by the tiles it belongs to.  Workspace: none.
 *
 * tnmf_hip_events_update: one multiplicative update of the strengths against V, given R = the render of the same
 * strengths: with neg_e = sum over the images of event e, the channels c and the atom entries j of V[n, c, x] *
 * W_eff[p, c, j] over the in-sample pixels x, and pos_e the same sum with R,
 *   strength[e] <- strength[e] * neg_e / (pos_e + eps + sparsity)
 * -- the dense Frobenius H half step without inhibition (tnmf_hip_update_H_ex) on activations that are zero off the
 * support, read at the support; a strength of 0 stays 0.  It needs the events distinct in (n, p, u).  events: n_events
 * rows of four ints (n, p, u_0, u_1) (ndim == 1: (n, p, 0, u_0)) in the order of `strength`; the images are derived from
 * them by the table above.  The sums are taken in double in a fixed order (deterministic) and the quotient is rounded
 * once to the element type.  It reads R and writes the n_events strengths, nothing else; a row whose sample, plane or
 * shift is out of range is skipped.
 *
 * Both are asynchronous.  Refused before anything is written: TNMF_E_NULL (ctx, geom, an operand the sizes make
 * necessary; `images` / `strength` may be NULL when n_images == 0, and everything of the update when n_events == 0),
 * TNMF_E_DTYPE, TNMF_E_UNSUPPORTED for volumes (ndim == 3), for more than 2^31 - 1 images or events and for an eps or
 * sparsity that is negative or NaN, TNMF_E_GEOM for any other ndim, sizes <= 0, negative counts, an unknown mode and the
 * per-axis limits of the mode ("reconstruction modes" above). */
#define TNMF_EVENTS_CELL_1D 256
#define TNMF_EVENTS_CELL_2D 16

int tnmf_hip_events_render(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, const void *W_eff, const int *images,
                           long long n_images, const int *cell_start, const void *strength, long long n_events, void *R,
                           void *stream);

int tnmf_hip_events_update(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, int mode, const void *W_eff, const int *events,
                           void *strength_inout, long long n_events, const void *V, const void *R, double eps,
                           double sparsity, void *stream);

/* tnmf_hip_events_gain: what each event of a list explains -- the Frobenius energy E = 1/2 ||V - R||^2 of the list without
 * event e minus that of the list, R being the render of the whole list.  With phi_e[c, x] = the sum over the images of e of
 * W_eff[p, c, .] placed at the image, restricted to the pixels inside sample n, and d = V - R,
 *   gain[e] = h_e * a_e + 1/2 * h_e^2 * b_e,   a_e = <phi_e, d>,   b_e = ||phi_e||^2
 * exactly (E is quadratic in h_e): positive where the event lowers the objective, and 1/2 h_e^2 b_e >= 0 at a fixed point
 * of the refit, where a_e = 0.  The images of one event may overlap inside the sample ('reflect' with 1 <= u <= a - 1: the
 * offsets u and -u), so b_e is not the sum of the images' norms: with t over the taps of image i whose pixel px(i, t) lies in
 * the sample,  a_e = sum_i sum_t w_t * d(px(i, t)),  b_e = sum_i sum_t w_t * phi_e(px(i, t)),  phi_e(px) summed over the at
 * most four images that cover px (the tap itself for an event of one image).
 *   mag[e] = sum_i sum_t  h_e * |w_t * d(px)| + 1/2 * h_e^2 * |w_t * phi_e(px)|
 * is the sum of the magnitudes of the terms of gain[e]: the scale of its rounding error (may be NULL: not written).
 * events: the n_events rows of four ints of tnmf_hip_events_update, in the order of `strength` (read, not written);
 * duplicates are allowed, every row is scored against the R it is given.  gain, mag: n_events DOUBLES, whatever the element
 * type; d = (double)V - (double)R and every sum are taken in double in a fixed order, no atomics: the same list gives the
 * same bits run after run.  Every element of both is written -- they need no initialisation -- 0 for a row whose sample,
 * plane or shift is out of range (no sample data is read for it).  It reads W_eff, events, strength, V and R and writes
 * gain and mag, nothing else.  Workspace: none.  Asynchronous.  With n_events == 0 or N == 0 it does nothing.
 * Refused before anything is written, as tnmf_hip_events_update is: TNMF_E_NULL (ctx, geom, and with n_events > 0 and
 * N > 0 every operand but mag), TNMF_E_DTYPE, TNMF_E_UNSUPPORTED for volumes and for more than 2^31 - 1 events,
 * TNMF_E_GEOM for any other ndim, sizes <= 0, a negative count, an unknown mode and the per-axis limits of the mode. */
int tnmf_hip_events_gain(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, int mode, const void *W_eff, const int *events,
                         const void *strength, long long n_events, const void *V, const void *R, double *gain,
                         double *mag /* may be NULL */, void *stream);

/* tnmf_hip_events_grad_W: the W gradient of a list of events -- with the images q of event e = (n, p, u, h_e) per the table
 * above, for every plane p, channel c and atom entry j (0 <= j < A per axis)
 *   neg[p, c, j] = sum over the events e of plane p, over their images q, of  h_e * V[n_e, c, q - (A - 1) + j]
 *   pos[p, c, j] = the same sum with R, the render of the same strengths and the same W_eff
 * -- pixels outside the sample are skipped, duplicate rows add up: the dense Frobenius W gradient (tnmf_hip_grad_W_fused)
 * of activations that are zero off the support, so a multiplicative W step on the list is tnmf_hip_apply_W (or a fold of a
 * transform group first) on this buffer.  negpos_eff: [2, P, C, *A] in the element type, neg first; every element is
 * written, zeros for a plane without events: it needs no initialisation and is never read.  W_eff itself is not an
 * operand (R carries it).  No float atomics: the same list gives the same bits run after run, on any device.
 * THE PLANE LIST is the caller's to build, once per support:
 *   - events: the n_events rows of four ints (n, p, u_0, u_1) of tnmf_hip_events_update, in the order of `strength`;
 *   - by_plane: n_events ints, the indices of the rows sorted by ascending plane with a STABLE sort (rows of one plane keep
 *     their order: it is the order of the additions);
 *   - plane_start: P + 1 ints, plane_start[p] = the first entry of by_plane of plane p, plane_start[P] = n_events -- a
 *     searchsorted of 0 .. P in the sorted planes;
 *   - each plane's run is cut into SEGMENTS of TNMF_EVENTS_SEGMENT entries (the last one shorter), numbered through the
 *     planes in plane order; a segment is summed in list order in double into one slab of 2 * C * prod(A) doubles, and the
 *     slabs of a plane are added in segment order in double and rounded once to the element type.  The segment length is a
 *     constant of this contract, not of the device.
 *   - workspace: (n_events / TNMF_EVENTS_SEGMENT + P) * 2 * C * prod(A) doubles (integer division; an upper bound of the
 *     number of segments), uninitialised, the caller's; no other memory is used, and none of H's size.
 *   As for the image list the CONTENTS cannot be refused: an entry of by_plane outside [0, n_events), a row whose sample or
 *   shift is out of range or whose plane is not the one it is filed under is skipped, plane_start is clamped to
 *   [0, n_events] and a run that ends before it begins is empty -- nothing is read or written out of bounds.
 * Asynchronous.  Refused before anything is written: TNMF_E_NULL (ctx, geom, negpos_eff, and with n_events > 0 and N > 0
 * every other operand), TNMF_E_DTYPE, TNMF_E_UNSUPPORTED for volumes and for more than 2^31 - 1 events, TNMF_E_GEOM as
 * for tnmf_hip_events_update. */
#ifndef TNMF_EVENTS_SEGMENT
#define TNMF_EVENTS_SEGMENT 64
#endif

int tnmf_hip_events_grad_W(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, int mode, const int *events, const int *by_plane,
                           const int *plane_start, const void *strength, long long n_events, const void *V, const void *R,
                           void *workspace, void *negpos_eff, void *stream);

/* ---- pursuit: forward selection of events (ABI 8, additive: the version stays 8) ------------------------------------------
 * The forward half of greedy selection, tnmf_hip_events_gain being the backward one: a round of convolutional matching
 * pursuit scores EVERY possible event (n, p, u) against the residual d = V - R of the list so far.  With phi_{p,u} the
 * occurrence of plane p at shift u exactly as tnmf_hip_events_gain defines it -- all images, clipped to the sample, images
 * that overlap added before they are squared -- a = <phi, d> and b = ||phi||^2, adding the event at its best strength
 * h = a / b lowers E = 1/2 ||V - R||^2 by g = a^2 / (2 b), for a > 0.  The dense map a[N, P, *S] is the H gradient's
 * numerator of the residual (tnmf_hip_grad_H with d in the place of the samples, folded for the mode by tnmf_hip_fold_H): it
 * is not an entry point of its own.  1 or 2 shift axes, float32 and float64, every mode.  All three calls are asynchronous,
 * use no workspace and no float atomics -- the same operands give the same bits run after run -- and write every element of
 * their outputs, which need no initialisation.
 *
 * tnmf_hip_events_norms: b[P, *S] (DOUBLES, C-contiguous, S the shift shape of `mode`) = ||phi_{p,u}||^2, summed in double in
 * a fixed order; 0 where the occurrence has no pixel inside the sample.  A shift whose single image lies wholly inside the
 * sample has the norm of the plane, sum w^2, taken once per plane; every other shift -- clipped, wrapped or mirrored -- goes
 * through the image walk.  geom as for the events (h_row_stride is not read).
 * Refused before anything is written: TNMF_E_NULL (ctx, geom, W_eff, b), TNMF_E_DTYPE, TNMF_E_UNSUPPORTED for volumes, for
 * more than 65535 planes and for a shift shape beyond 2^31 - 1 entries, TNMF_E_GEOM for any other ndim, sizes <= 0, an
 * unknown mode and the per-axis limits of the mode.
 *
 * tnmf_hip_pursuit_score: the gain map of a round.  a and gain_out are [N, P, *S] in the element type, viewed as
 * tnmf_hip_find_peaks views H: P = geom->M planes of shift shape S = D + A - 1 (for a mode other than 'valid' the caller
 * passes D = S and A = 1 on every axis), rows `h_row_stride` apart -- pad columns are neither read nor written.  b is the
 * table of tnmf_hip_events_norms, [P, *S] doubles, C-contiguous.  C is not read.
 *   gain_out = (element type)((double)a * (double)a / (2 * b))   where a > 0 and b > 0 (one rounding of the double quotient),
 *   gain_out = 0   elsewhere -- NaN compares false, so a NaN in a gives 0.
 * Then, on the same stream, the entries at the n_taken flat C-order indices of `taken` (in [N, P, *S], as tnmf_hip_find_peaks
 * reports them: the rows of the list so far) are set to 0, which keeps the rows of the list distinct; an index out of range
 * is skipped.  gain_out may be a itself.  A streaming pass: 16-byte accesses where a, gain_out and the row stride allow.
 * Refused before anything is written: TNMF_E_NULL (ctx, geom, and with N > 0 a, b, gain_out, and taken when n_taken > 0),
 * TNMF_E_DTYPE, TNMF_E_UNSUPPORTED for volumes and for more than 2^31 - 1 rows per sample, TNMF_E_GEOM for any other ndim,
 * sizes <= 0, a negative n_taken and a row stride below the shift width.
 *
 * tnmf_hip_pursuit_pick: the exact score of the candidates a round keeps -- the map only ranks; in float32 its entries carry
 * the rounding of the correlation, which the strengths and the energy bookkeeping must not.  idx: n_picked flat C-order
 * indices in [N, P, *S], S the shift shape of `mode`; R: the render of the list so far (tnmf_hip_events_render).  Per index,
 * with the sums of tnmf_hip_events_gain taken in double in its fixed order (d = (double)V - (double)R),
 *   events_out[i] = the four ints (n, p, u_0, u_1) of tnmf_hip_events_update (ndim == 1: (n, p, 0, u_0)),
 *   a = sum_i sum_t w_t * d(px(i, t)),   b = sum_i sum_t w_t * phi(px(i, t)),
 *   strength_out[i] = max(a, 0) / b rounded once to the element type (0 where b is 0),
 *   gain_out[i] = a > 0 ? a^2 / (2 b) : 0,   mag_out[i] = sum_i sum_t |w_t * d(px(i, t))|   (DOUBLES; mag_out may be NULL)
 * -- mag is the scale of the rounding error of a.  An index out of range gives a row of -1 and 0 for strength, gain and mag
 * (no sample data is read for it).  geom as for the events (h_row_stride is not read).  With n_picked == 0 it does nothing.
 * Refused before anything is written: TNMF_E_NULL (ctx, geom, and with n_picked > 0 idx and every output but mag_out, and with
 * N > 0 W_eff, V and R as well), TNMF_E_DTYPE, TNMF_E_UNSUPPORTED for volumes, for more than 2^31 - 1 indices and for a
 * shift shape beyond 2^31 - 1 entries, TNMF_E_GEOM for any other ndim, sizes <= 0, a negative count, an unknown mode and the
 * per-axis limits of the mode. */
int tnmf_hip_events_norms(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, int mode, const void *W_eff,
                          double *b /* [P, *S] */, void *stream);

int tnmf_hip_pursuit_score(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, const void *a, const double *b, void *gain_out,
                           const long long *taken, long long n_taken, void *stream);

int tnmf_hip_pursuit_pick(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, int mode, const void *W_eff, const long long *idx,
                          long long n_picked, const void *V, const void *R, int *events_out /* int4 rows */,
                          void *strength_out, double *gain_out /* double */, double *mag_out /* double, may be NULL */,
                          void *stream);

/* ---- landscape: every event scored at its neighbouring shifts (ABI 8, additive: the version stays 8) ------------------------
 * What the objective would be if a row of the list sat one shift over, everything else in the list held fixed: the quantity
 * behind sub-pixel positions and behind moving a row.  For event e = (n, p, u, h_e) of a list whose render is R, the residual
 * of the list WITHOUT the row is  d_e = V[n] - R[n] + h_e * phi_e,  phi_e = phi_{p,u} the occurrence as tnmf_hip_events_gain
 * defines it.  For every offset delta in {-1, 0, +1}^ndim, u' = u + delta -- 3 neighbours on one shift axis, 9 on two, the
 * neighbour index being delta_0 + 1 (ndim == 1) or (delta_0 + 1) * 3 + (delta_1 + 1) (ndim == 2) -- with t over the taps of
 * image i of phi' = phi_{p,u'} whose pixel px(i, t) lies in the sample:
 *   a_out[e, delta]   = sum_i sum_t w_t * d_e(px(i, t))
 *   b_out[e, delta]   = sum_i sum_t w_t * phi'(px(i, t))        ( = ||phi'||^2, images that overlap added before squaring)
 *   mag_out[e, delta] = sum_i sum_t |w_t * d_e(px(i, t))|       (the scale of the rounding error of a; may be NULL: not written)
 * -- the sums of tnmf_hip_pursuit_pick with d_e in the place of d.  A neighbour whose u' lies outside the shift shape S of the
 * mode on any axis gets a = b = mag = 0: nothing wraps from one end of the shift range to the other.  Replacing the row by
 * one at u' at its best strength a / b lowers E = 1/2 ||V - R||^2, measured from the list without e, by a^2 / (2 b) where
 * a > 0 and b > 0 (the caller's to form).  At delta = 0:  a - h_e * b = the a_e of tnmf_hip_events_gain, and
 * h_e * a_e + 1/2 * h_e^2 * b = its gain[e].
 * events, strength: those of tnmf_hip_events_gain, read and not written; duplicates are allowed, each row puts back only
 * itself.  Outputs: [n_events, 3^ndim] DOUBLES, C-contiguous, whatever the element type.  d_e(px) = fma(h_e, phi_e(px),
 * (double)V - (double)R) and every sum are taken in double in a fixed order -- tap t of an image in lane t % 64 in ascending
 * t, images in image order, then the butterfly of the wave -- without atomics: the same operands give the same bits run after
 * run, on any device.  Every element of the outputs is written -- they need no initialisation -- zeros for a row whose
 * sample, plane or shift is out of range (no sample data is read for it).  Two paths, chosen per row by its geometry alone
 * and giving the same bits: a row whose own occurrence and all 3^ndim neighbours are single images wholly inside the sample
 * has its (A + 2)-sized patch of d_e staged once in LDS (when C * prod(A + 2) <= 2048 doubles) and b taken once as the
 * plane's sum of squares; every other row walks each neighbour's images.  It reads W_eff, events, strength, V and R and
 * writes the outputs, nothing else.  Workspace: none.  Asynchronous.  With n_events == 0 or N == 0 it does nothing.
 * Refused before anything is written, as tnmf_hip_events_gain is: TNMF_E_NULL (ctx, geom, and with n_events > 0 and N > 0
 * every operand but mag_out), TNMF_E_DTYPE, TNMF_E_UNSUPPORTED for volumes and for more than (2^31 - 1) / 9 events,
 * TNMF_E_GEOM for any other ndim, sizes <= 0, a negative count, an unknown mode and the per-axis limits of the mode. */
int tnmf_hip_events_landscape(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, int mode, const void *W_eff, const int *events,
                              const void *strength, long long n_events, const void *V, const void *R, double *a_out,
                              double *b_out, double *mag_out /* may be NULL */, void *stream);

/* ---- alternatives: every event scored under other planes at its own shift (ABI 8, additive: the version stays 8) ------------
 * The landscape turned by 90 degrees: what the objective would be if a row of the list had another atom or another
 * orientation, everything else in the list held fixed -- the quantity behind re-estimating the label of a row.  For event
 * e = (n, p, u, h_e) of a list whose render is R, d_e = V[n] - R[n] + h_e * phi_e is the residual of the list WITHOUT the row
 * (tnmf_hip_events_landscape).  The candidates are an arithmetic progression of planes through the row's own plane, given
 * by n_alt >= 1 and stride >= 1 with block = n_alt * stride a divisor of P:
 *   first_e = (p / block) * block + p % stride,   p'_j = first_e + j * stride  (j = 0 .. n_alt - 1),   j_own = (p - first_e) / stride
 * -- with plane = atom * T + transform, (n_alt, stride) = (T, 1) are the orientations of the row's atom, (M, T) every atom in
 * the row's orientation, (P, 1) every plane.  For every j, phi' = phi_{p'_j,u}, the occurrence as tnmf_hip_events_gain defines
 * it at the row's own shift (the image geometry is the same for every j: every plane has the atom shape), w' the taps of
 * p'_j, t over the taps of image i whose pixel px(i, t) lies in the sample:
 *   a_out[e, j]   = sum_i sum_t w'_t * d_e(px(i, t))
 *   b_out[e, j]   = sum_i sum_t w'_t * phi'(px(i, t))       ( = ||phi'||^2, images that overlap added before squaring)
 *   mag_out[e, j] = sum_i sum_t |w'_t * d_e(px(i, t))|      (the scale of the rounding error of a; may be NULL: not written)
 * -- the sums of tnmf_hip_events_landscape at delta = 0 taken with the taps of plane p'_j.  Replacing the row by plane p'_j at
 * its best strength a / b lowers E = 1/2 ||V - R||^2, measured from the list without e, by a^2 / (2 b) where a > 0 and b > 0
 * (the caller's to form).  At j_own:  a - h_e * b = the a_e of tnmf_hip_events_gain, and h_e * a_e + 1/2 * h_e^2 * b = its
 * gain[e]; the three sums there are those of tnmf_hip_events_landscape at delta = 0.
 * events, strength: those of tnmf_hip_events_gain, read and not written; duplicates are allowed, each row puts back only
 * itself.  Outputs: [n_events, n_alt] DOUBLES, C-contiguous, whatever the element type.  d_e(px) = fma(h_e, phi_e(px),
 * (double)V - (double)R) and every sum are taken in double in a fixed order -- tap t of an image in lane t % 64 in ascending
 * t, images in image order, then the butterfly of the wave -- without atomics: the same operands give the same bits run after
 * run, on any device.  Every element of the outputs is written -- they need no initialisation -- zeros for a row whose
 * sample, plane or shift is out of range (no sample data is read for it).  Two paths, chosen per row by its geometry alone
 * and giving the same bits: a row whose occurrence is a single image wholly inside the sample has its C * prod(A) patch of
 * d_e staged once in LDS (when that is <= 2048 doubles) -- V and R are read once per row, not n_alt times -- and b taken as
 * the plane's sum of squares in the same lane order; every other row -- clipped, wrapped or mirrored -- walks its images
 * once per batch of candidates.  It reads W_eff, events, strength, V and R and writes the outputs, nothing else.
 * Workspace: none.  Asynchronous.  With n_events == 0 or N == 0 it does nothing.
 * Refused before anything is written, as tnmf_hip_events_landscape is: TNMF_E_NULL (ctx, geom, and with n_events > 0 and
 * N > 0 every operand but mag_out), TNMF_E_DTYPE, TNMF_E_UNSUPPORTED for volumes and for n_events * n_alt > 2^31 - 1,
 * TNMF_E_GEOM for any other ndim, sizes <= 0, a negative count, an unknown mode, the per-axis limits of the mode, n_alt < 1,
 * stride < 1 and a block n_alt * stride that does not divide P. */
int tnmf_hip_events_alternatives(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, int mode, const void *W_eff,
                                 const int *events, const void *strength, long long n_events, const void *V, const void *R,
                                 int n_alt, int stride, double *a_out, double *b_out,
                                 double *mag_out /* may be NULL */, void *stream);

/* ---- events: exact strengths (ABI 8, additive: the version stays 8) -------------------------------------------------------
 * The strengths that MINIMISE the Frobenius objective on a fixed support -- the orthogonal step of orthogonal matching
 * pursuit -- computed on the list alone.  For K distinct events with occurrences phi_e (all images, clipped to the sample,
 * images that overlap added: tnmf_hip_events_gain) the objective is a quadratic in the strengths,
 *   E(h) = 1/2 ||V||^2 - c' h + 1/2 h' G h,     c_i = <phi_i, V>,     G_ij = <phi_i, phi_j>,
 * and G_ij is non-zero only for rows of one sample whose footprints meet: G is sparse.  The samples enter once, through c.
 * c and G are DOUBLES whatever the element type; no entry uses float atomics, each writes every element of its outputs,
 * and the same operands give the same bits run after run.  geom as for the events (h_row_stride is not read), 1 or 2 shift
 * axes, float32 and float64, every mode.
 *
 * tnmf_hip_events_pairs: the candidate pattern of G above the diagonal.  images / cell_start: THE IMAGE LIST of
 * tnmf_hip_events_render, sorted by (sample, cell); events: the n_events rows of tnmf_hip_events_update (read for the sample
 * of a row).  A row pair i < j of the same sample is a candidate when some image of i and some image of j are closer than
 * the atom extent on every shift axis, |q_i - q_j| < A: a SUPERSET of the pairs with G_ij != 0 -- a candidate whose overlap
 * lies wholly outside the sample has the value exactly 0.  The work is proportional to the images in the cells an image
 * can reach.  Output as tnmf_hip_find_peaks': count_out (one unsigned 64-bit word on the device) is zeroed on the stream,
 * then counts EVERY candidate found; they are appended in no particular order as pairs_out[slot] = i * n_events + j while
 * slot < capacity, once per image pair (a row pair may appear up to 16 times: the caller sorts and removes duplicates).
 * Nothing is written at or beyond `capacity`; a count above it is the size to come back with.  A row of the image list whose
 * event is out of range, whose position is negative or beyond the cells, or whose event's sample is out of range is
 * skipped, cell_start is clamped to [0, n_images]: nothing is read or written out of bounds.  Asynchronous.
 * Refused before anything is written: TNMF_E_NULL (ctx, geom, count_out, pairs_out when capacity > 0, the lists when the
 * counts and N are positive), TNMF_E_DTYPE, TNMF_E_UNSUPPORTED for volumes and for more than 2^31 - 1 images, events or
 * stored entries (capacity), TNMF_E_GEOM for any other ndim, sizes <= 0 and negative counts.
 *
 * tnmf_hip_events_gram: val_out[p] = <phi_i, phi_j> for the n_pairs pairs (i, j) = (row_i[p], row_j[p]), i == j included:
 * one wave per pair, the lanes over row i's taps in the order of tnmf_hip_events_gain, phi_j summed over its images at each
 * pixel; on the diagonal it is that entry's b_e.  <phi_i, phi_j> and <phi_j, phi_i> differ in the order of their additions:
 * a caller that wants a bit-symmetric matrix computes i <= j and mirrors.  val_out[p] = 0 for an index outside
 * [0, n_events), a row whose sample, plane or shift is out of range, and rows of two samples.  Asynchronous.
 * Refused before anything is written: TNMF_E_NULL (ctx, geom, and with n_pairs > 0 every operand), TNMF_E_DTYPE,
 * TNMF_E_UNSUPPORTED for volumes and for more than 2^31 - 1 events or pairs, TNMF_E_GEOM as for tnmf_hip_events_gain.
 *
 * tnmf_hip_events_project: c_out[e] = <phi_e, V> = sum_i sum_t w_t * V(px(i, t)) for every row, the walk and the order of
 * tnmf_hip_events_gain; 0 for a row out of range (no sample data is read for it).  Asynchronous.  Refusals as for
 * tnmf_hip_events_gain (every operand with n_events > 0).
 *
 * tnmf_hip_events_nnls: minimise 1/2 h' G h - c' h over h >= 0, in double.  G: CSR on the device -- row_start[n_rows + 1],
 * col[nnz] ascending within a row, val[nnz], the diagonal present, symmetric; c[n_rows]; h_inout[n_rows]: the start on
 * entry (projected onto h >= 0; NaN counts as 0), the last iterate on return.  A row with G_ii <= 0 has no pixel in the
 * sample: its strength is 0 and it takes no part.  The method is projected gradient with step 1 / L, L = max_i sum_j |G_ij|
 * (Gershgorin; exact for non-negative atoms), Nesterov momentum and the gradient restart <y - x+, x+ - x> > 0.
 * The stopping quantity, evaluated AT THE ITERATE RETURNED (not at the momentum point), is
 *   kkt = max_i |pg_i| / max_i |c_i|,   g = G h - c,   pg_i = g_i where h_i > 0,   min(g_i, 0) where h_i = 0;
 * with max |c| = 0 the answer is h = 0 with kkt = 0.  It stops at kkt <= tol or after max_iterations steps;
 * max_iterations = 0 returns the projected start with its kkt.  The host reads ONE double every check_every iterations
 * (iterations 0, check_every, 2 * check_every, ... and max_iterations) and nothing else, so the iteration count it stops
 * at is a multiple of check_every.  This entry is SYNCHRONOUS at those reads; on return h_inout is queued on the stream.
 * HOST outputs: iterations_out, kkt_out (the last kkt read), converged_out (kkt <= tol), history_out [history_capacity, 2]
 * doubles (iteration, kkt) of the checks (may be NULL with capacity 0), n_history_out (may be NULL) the pairs stored.
 * workspace: 7 * n_rows + 8 doubles on the device, uninitialised, the caller's.  Column indices outside [0, n_rows) are
 * skipped and row_start is clamped to [0, nnz]: nothing is read out of bounds.  With n_rows == 0 it does nothing
 * (0 iterations, converged).
 * Refused before anything is written: TNMF_E_NULL (ctx, the three scalar outputs, and with n_rows > 0 every device
 * operand), TNMF_E_GEOM for negative sizes, max_iterations < 0, check_every < 1, TNMF_E_UNSUPPORTED for a tol that is not
 * finite and > 0 and for more than 2^31 - 1 rows or entries. */
int tnmf_hip_events_pairs(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, const int *images, long long n_images,
                          const int *cell_start, const int *events, long long n_events, long long *pairs_out,
                          size_t capacity, unsigned long long *count_out, void *stream);

int tnmf_hip_events_gram(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, int mode, const void *W_eff, const int *events,
                         long long n_events, const int *row_i, const int *row_j, long long n_pairs,
                         double *val_out /* double */, void *stream);

int tnmf_hip_events_project(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, int mode, const void *W_eff, const int *events,
                            long long n_events, const void *V, double *c_out /* double */, void *stream);

int tnmf_hip_events_nnls(tnmf_hip_ctx *ctx, long long n_rows, long long nnz, const int *row_start, const int *col,
                         const double *val, const double *c, double *h_inout, double tol, int max_iterations,
                         int check_every, double *workspace, int *iterations_out /* host */, double *kkt_out /* host */,
                         int *converged_out /* host */, double *history_out /* host, may be NULL */, int history_capacity,
                         int *n_history_out /* host, may be NULL */, void *stream);

/* ---- events: standard errors (ABI 8, additive: the version stays 8) -------------------------------------------------------
 * How well the strengths of a list are determined.  At the solution of tnmf_hip_events_nnls the strengths of the active
 * rows A = {i : h_i > 0} are the least-squares estimate on that support: Cov(h_A) = sigma^2 (G_AA)^-1.  This entry gives
 * the DIAGONAL of (G_AA)^-1, exactly: G is sparse, G_AA is block diagonal over the connected components of its coupling
 * graph (rows couple where their footprints meet), and each component is a small dense problem -- one Cholesky
 * factorisation, the inverse of the factor, d_i = sum_{k >= i} (L^-1)_ki^2.  All in double.
 *
 * tnmf_hip_events_inverse_diag.  On the DEVICE: the CSR triple of tnmf_hip_events_nnls (row_start[n_rows + 1], col[nnz],
 * val[nnz]; columns ascending within a row, the diagonal present, symmetric); comp_start[n_comp + 1], the boundaries of
 * the components in member[n_active]: the active rows grouped by component and ascending inside each; local[n_rows]: a
 * row's position inside its component, -1 for a row that is not active; scratch: scratch_doubles doubles, uninitialised,
 * the caller's.  On the HOST: comp_sizes[n_comp], the sizes comp_start[c + 1] - comp_start[c], from which every launch is
 * planned.  The components are given in ASCENDING SIZE.  Three paths by the size n of a component:
 *   n = 1                               d = 1 / G_ii, elementwise over such components: no workgroup per component;
 *   2 <= n <= TNMF_EVENTS_INVERSE_LDS   one workgroup per component, the packed lower triangle in LDS (column-major, so
 *                                       that the lanes of every inner loop read consecutive doubles); TNMF_EVENTS_INVERSE_LDS
 *                                       = 200 is the largest n with n (n + 1) / 2 + n doubles (the triangle and the original
 *                                       diagonal) inside 160 KB: 20 300 of 20 480;
 *   n > TNMF_EVENTS_INVERSE_LDS         the same steps on a dense n x n tile plus one column, n^2 + n doubles of scratch, one
 *                                       workgroup per component; launched in batches whose tiles fit scratch_doubles.  No
 *                                       component of at most TNMF_EVENTS_INVERSE_LDS rows reads the scratch (it may be NULL).
 * Outputs on the device: d_out[n_rows] = ((G_AA)^-1)_ii for an active row, NaN for any other -- every element is written --
 * and status_out[n_comp] = 0, or 1 for a component that is numerically singular: a pivot of its factorisation
 * <= n * 2^-52 * (that row's original G_ii); its rows get d = +inf, the other components are not affected.  (Two orientations
 * of a symmetric atom at one place are collinear: this happens on legitimate lists.)  An entry of a component's rows whose
 * column is not active or belongs to another component is skipped; indices outside their ranges are skipped and runs are
 * clamped: nothing is read or written out of bounds.  The sums run in a fixed order, there are no atomics: the same
 * operands give the same bits run after run.  Asynchronous.  With n_rows == 0 it does nothing.
 * Refused before anything is written and without touching a device: TNMF_E_NULL for a NULL ctx, a NULL operand that the
 * sizes make necessary and any negative size; TNMF_E_UNSUPPORTED for more than 2^31 - 1 rows or entries; TNMF_E_GEOM for
 * n_active > n_rows, n_comp > n_active, sizes below 1, not ascending or not adding up to n_active, and a largest component
 * above TNMF_EVENTS_INVERSE_LDS whose tile does not fit the scratch. */
#define TNMF_EVENTS_INVERSE_LDS 200

int tnmf_hip_events_inverse_diag(tnmf_hip_ctx *ctx, long long n_rows, long long nnz, const int *row_start, const int *col,
                                 const double *val, long long n_comp, const int *comp_start,
                                 const int *comp_sizes /* host */, long long n_active, const int *member, const int *local,
                                 double *scratch /* may be NULL */, long long scratch_doubles, double *d_out /* double */,
                                 int *status_out, void *stream);

/* ---- patches: the data under each event, and how an atom's occurrences vary (ABI 8, additive: the version stays 8) -----------
 * tnmf_hip_events_grad_W sums the patches of a plane's events into one gradient and keeps the sum alone.  These two entries
 * keep the patches themselves -- the "waveforms" of a spike sorter, the cut-outs of a motif finder -- and their second
 * moments per atom: the spread that says where one atom should be two, as the atom Gram says where two atoms are one.
 *
 * For an event e = (n, p, u, h_e) with the images q_i of the table of "events: render, refit and learn" the signal s is one
 * of three, formed in double, and the PATCH is its gather under the images:
 *   TNMF_PATCH_DATA      s = (double)V[n]
 *   TNMF_PATCH_RESIDUAL  s = (double)V[n] - (double)R[n]                       (R the render of the whole list)
 *   TNMF_PATCH_CLEANED   s = fma(h_e, phi_e, (double)V[n] - (double)R[n])      (the list without the row: the d_e of
 *                                                                              tnmf_hip_events_landscape, phi_e summed over
 *                                                                              the images that cover the pixel, in image order)
 *   x_e[c, j] = sum over the images i, in image order, of s[c, q_i - (A - 1) + j]          (0 <= j < A per axis)
 * -- a pixel outside the sample contributes 0 and is never read.  x_e is the adjoint of placing the plane at shift u: it lives
 * in the frame of W_eff[p], the IMAGE FRAME.  By construction <W_eff[p], x_e> is the a_e of tnmf_hip_events_gain for
 * TNMF_PATCH_RESIDUAL and a_out[e, delta = 0] of tnmf_hip_events_landscape for TNMF_PATCH_CLEANED (up to the order of the
 * additions).  The ATOM FRAME is y_e[c] = L_t^T x_e[c] with p = m * T + t: the fold the W half step applies to its summed
 * gradient, applied to one event, so that <W[m], y_e> = <W_eff[p], x_e>.  For a transform group it is the inverse
 * permutation; without transforms y = x.
 *
 * tnmf_hip_events_patches: out[n_events, C, *A] DOUBLES, whatever the element type, in the order of `events`.  events,
 * strength, V, R: those of tnmf_hip_events_gain, read and not written; duplicates are allowed, each row puts back only itself.
 * THE FOLD TABLE is the caller's to build, once per set of transforms, as plain device arrays (nA = prod(A)):
 *   fold_ptr [T * nA + 1] ints, fold_src [nnz] ints, fold_w [nnz] doubles, with
 *   y[c, i] = sum over k in [fold_ptr[t * nA + i], fold_ptr[t * nA + i + 1]) of fold_w[k] * x[c, fold_src[k]]
 * the products summed in table order in double -- row (t, i) holds the entries (t, out pixel, in pixel = i, weight) of the
 * operators with fold_src the out pixel.  fold_ptr == NULL gives the image frame (fold_src, fold_w and T are then not read
 * beyond the checks below).  A run of the table that ends before it begins is empty, an entry whose source is outside
 * [0, nA) is skipped and a start below 0 is taken as 0; the table's own length is not an operand: fold_ptr must not point
 * beyond the entries the caller allocated.
 * One wave per event; tap t of an image in lane t % 64, images in image order (the walk of tnmf_hip_events_gain).  With a
 * table the wave stages x_e in LDS and gathers y_e from there, otherwise it stores x_e straight.  No atomics: the same
 * operands give the same bits run after run.  Every element of out is written -- it needs no initialisation -- zeros for a
 * row whose sample, plane or shift is out of range (no sample data is read for it).  TNMF_PATCH_DATA of a single-image row
 * is (double)V at the (permuted) pixel to the bit under no table or a table of single entries of weight 1.  It reads its
 * operands and writes out, nothing else.  Workspace: none.  Asynchronous.  With n_events == 0 or N == 0 it does nothing.
 * Refused before anything is written, as tnmf_hip_events_gain is: TNMF_E_NULL (ctx, geom, and with n_events > 0 and N > 0
 * events, V and out; R, W_eff and strength unless source is TNMF_PATCH_DATA; fold_src and fold_w with a fold_ptr),
 * TNMF_E_DTYPE, TNMF_E_UNSUPPORTED for volumes, for more than 2^31 - 1 events and for n_events * C * prod(A) > 2^31 - 1,
 * TNMF_E_GEOM for any other ndim, sizes <= 0, a negative count, an unknown mode, the per-axis limits of the mode, an unknown
 * source, T < 1, geom->M not a multiple of T, and with a table C * prod(A) > TNMF_PATCH_STAGE_MAX doubles (what a wave's
 * share of the workgroup's LDS holds).
 *
 * tnmf_hip_patch_moments: the second moments of the patches of one chunk of a list, per atom.  Y [n_rows, D] DOUBLES, the
 * patches in the atom frame, D = C * prod(A); strength_d [n_rows] DOUBLES in the order of Y; by_atom [n_rows] ints, the rows
 * of Y in a STABLE order of ascending atom; atom_start [n_atoms + 1] ints, atom_start[m] = the first entry of by_atom of atom
 * m (the plane list of tnmf_hip_events_grad_W, by atom).  Outputs, all DOUBLES:
 *   S[m, i, j] = sum_e y_e[i] * y_e[j]      g[m, i] = sum_e h_e * y_e[i]      s2[m] = sum_e h_e^2      count[m] = entries of atom m
 * every sum over the entries of atom m in list order.  With accumulate != 0 the outputs are added to, in double, and the
 * chunk continues the order: S is taken four entries at a time, the fours beginning at the multiples of four of the position
 * in by_atom (entries of a four outside the atom's run, and columns beyond D, are fed as zeros), g and s2 one entry at a
 * time.  So a list cut into chunks at multiples of four of the sorted position gives, chunk after chunk with accumulate, the
 * values of the same list in one call (and every cut gives the same g and s2).  With accumulate == 0 every element of the
 * outputs is written: they need no initialisation, and an atom without entries gets exact zeros.
 * S is a batched symmetric rank-K update on the matrix cores (v_mfma_f64_16x16x4_f64): one wave owns one pair (I <= J) of
 * 16 x 16 blocks of one atom, walks the atom's run, and stores its block and the mirror image -- of a diagonal block the
 * upper triangle and its mirror image -- so S is symmetric to the bit.  The waves of the diagonal blocks take g (and the
 * first of them s2 and count) from the operands they hold.  No split over the entries and no atomics: the same operands give
 * the same bits run after run.  As in the other list entries the CONTENTS cannot be refused: an entry of by_atom outside
 * [0, n_rows) is fed as zeros (it still counts) and atom_start is clamped to [0, n_rows]; a run that ends before it begins
 * is empty.  Workspace: none.  Asynchronous.
 * Refused before anything is written: TNMF_E_NULL (ctx, atom_start, an output; Y, strength_d and by_atom with n_rows > 0),
 * TNMF_E_GEOM for D <= 0, n_atoms <= 0 and n_rows < 0, TNMF_E_UNSUPPORTED for n_atoms * D * D > 2^31 - 1 and for more than
 * 2^31 - 1 rows. */
#define TNMF_PATCH_DATA 0
#define TNMF_PATCH_RESIDUAL 1
#define TNMF_PATCH_CLEANED 2
#define TNMF_PATCH_STAGE_MAX 2048

int tnmf_hip_events_patches(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, int mode, int source, const void *W_eff,
                            const int *events, const void *strength, long long n_events, const void *V, const void *R,
                            const int *fold_ptr /* may be NULL */, const int *fold_src, const double *fold_w, int T,
                            double *out /* double */, void *stream);

int tnmf_hip_patch_moments(tnmf_hip_ctx *ctx, int D, int n_atoms, const double *Y, const double *strength_d,
                           const int *by_atom, const int *atom_start, long long n_rows, int accumulate, double *S,
                           double *g, double *s2, double *count, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TNMF_HIP_H */

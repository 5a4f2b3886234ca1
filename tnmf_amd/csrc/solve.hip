// solve.hip -- the exact strengths of a list of events (include/tnmf_hip.h, "events: exact strengths"): the objective of a
// list is the quadratic E(h) = 1/2 |V|^2 - c'h + 1/2 h'Gh with c_i = <phi_i, V> and G_ij = <phi_i, phi_j>, phi the
// occurrence of event_walk.h.  The samples enter once, through c; everything after that lives on K-vectors and the non-zeros of G.
//
// k_events_pairs: the candidate row pairs i < j.  One wave per image of the list sorted by (sample, cell): an image at padded
// position q meets the images at |q' - q| < A per axis, which lie in the cells (q - (A - 1)) / cell .. (q + (A - 1)) / cell,
// one run of the list per cell row (cell_start); the lanes stride over the run, and the images inside the reach whose event
// is ABOVE the wave's own are appended as i * K + j through one integer atomic per wave and step (the ballot of
// peaks.hip).  The order of the output is not fixed and a row pair appears once per image pair: the caller sorts and
// removes duplicates.  A superset of G's pattern: the overlap of a candidate may lie wholly outside the sample.
//
// k_events_gram: one wave per pair (i, j), the walk of k_events_gain -- the lanes stride over row i's taps (for_each_tap),
// phi_j at each pixel (phi_at), doubles, the butterfly (wave_sum).  On the diagonal it is k_events_gain's b.
//
// k_events_project: c_i = <phi_i, V>, the same walk against the samples.
//
// NNLS: projected gradient with Nesterov momentum and the gradient restart of O'Donoghue and Candes on the CSR matrix, all in
// double.  Per iteration two launches and no host traffic:
//   k_nnls_step   kRowLanes lanes per row.  With beta the momentum coefficient in device memory, y = x + beta (x - x_prev) is
//                 formed on the fly from the two iterates; one pass over the row gives (G y)_i and (G x)_i -- the second sum
//                 costs one more fma per non-zero, on operands already loaded -- so the projected gradient AT THE ITERATE x
//                 comes with the step: x_next_i = max(y_i - ((G y)_i - c_i) / L, 0), the restart term
//                 (y_i - x_next_i) (x_next_i - x_i), and pg_i of g = G x - c.  The block adds the restart terms of its rows in
//                 row order and takes the maximum of their |pg| (LDS, one thread): one entry per block.
//   k_nnls_reduce one workgroup: the sum of the blocks' restart terms and the maximum of |pg| in a fixed order (strided
//                 partial sums, a tree of fixed shape through LDS); thread 0 writes kkt = max |pg| / max |c| and the next
//                 beta with plain stores.
// The host reads kkt every check_every iterations (one double) and nowhere else.  No atomics: the same operands give the
// same bits run after run.
#include <algorithm>
#include <cmath>

#include "event_walk.h"
#include "solve.h"

namespace {

constexpr int kWaves = kEventThreads / 64;
constexpr int kRowLanes = 16;                       // lanes per row of the matrix
constexpr int kRowsPerBlock = kEventThreads / kRowLanes;

__global__ __launch_bounds__(kEventThreads) void k_events_pairs(EventGeo g, const int4 *__restrict__ img, int n_images,
                                                                 const int *__restrict__ cell_start,
                                                                 const int4 *__restrict__ ev, int K,
                                                                 long long *__restrict__ pairs, unsigned long long capacity,
                                                                 unsigned long long *count) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long long a = (long long)blockIdx.x * kWaves + wave; a < n_images; a += (long long)gridDim.x * kWaves) {
        const int4 me = img[a];   // plane, qy, qx, event (wave-uniform)
        if ((unsigned)me.w >= (unsigned)K || me.y < 0 || me.z < 0) continue;
        const int cy = me.y / g.ty, cx = me.z / g.tx;
        if (cy >= g.ncy || cx >= g.ncx) continue;
        const long long n = ev[me.w].x;   // the sample of the image's event: its cells hold the images it can meet
        if ((unsigned long long)n >= (unsigned long long)g.N) continue;
        const int cy0 = max((me.y - (g.Ay - 1)) / g.ty, 0), cy1 = min((me.y + g.Ay - 1) / g.ty, g.ncy - 1);
        const int cx0 = max((me.z - (g.Ax - 1)) / g.tx, 0), cx1 = min((me.z + g.Ax - 1) / g.tx, g.ncx - 1);
        for (int ry = cy0; ry <= cy1; ++ry) {
            const long long row = (n * g.ncy + ry) * g.ncx;
            const int i0 = max(cell_start[row + cx0], 0), i1 = min(cell_start[row + cx1 + 1], n_images);
            for (int base = i0; base < i1; base += 64) {
                const int b = base + lane;
                bool hit = false;
                int other = 0;
                if (b < i1) {
                    const int4 im = img[b];
                    other = im.w;
                    hit = (unsigned)im.w < (unsigned)K && im.w > me.w && abs(im.y - me.y) < g.Ay && abs(im.z - me.z) < g.Ax;
                }
                const unsigned long long m = __ballot(hit);
                if (!m) continue;
                unsigned long long first = 0;
                if (lane == 0) first = atomicAdd(count, (unsigned long long)__popcll(m));
                first = __shfl(first, 0, 64);
                if (hit) {
                    const unsigned long long slot = first + __popcll(m & ((1ull << lane) - 1ull));
                    if (slot < capacity) pairs[slot] = (long long)me.w * K + other;
                }
            }
        }
    }
}

__device__ __forceinline__ bool row_ok(const EventGeo &g, int Sy, int Sx, const int4 &v) {
    return (unsigned)v.x < (unsigned)g.N && (unsigned)v.y < (unsigned)g.P && (unsigned)v.z < (unsigned)Sy &&
           (unsigned)v.w < (unsigned)Sx;
}

template <typename T>
__global__ __launch_bounds__(kEventThreads) void k_events_gram(EventGeo g, int mode, int Sy, int Sx,
                                                                const T *__restrict__ W, const int4 *__restrict__ ev, int K,
                                                                const int *__restrict__ ri, const int *__restrict__ rj,
                                                                long long n_pairs, double *__restrict__ val) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int AA = g.Ay * g.Ax, taps = g.C * AA;
    for (long long p = (long long)blockIdx.x * kWaves + wave; p < n_pairs; p += (long long)gridDim.x * kWaves) {
        const int i = ri[p], j = rj[p];
        bool ok = (unsigned)i < (unsigned)K && (unsigned)j < (unsigned)K;
        int4 vi = make_int4(0, 0, 0, 0), vj = vi;
        if (ok) {
            vi = ev[i], vj = ev[j];
            ok = row_ok(g, Sy, Sx, vi) && row_ok(g, Sy, Sx, vj) && vi.x == vj.x;
        }
        if (!ok) {   // (wave-uniform: outside the contract, or rows of two samples)
            if (lane == 0) val[p] = 0.;
            continue;
        }
        const Occurrence oi(g, mode, Sy, Sx, vi.z, vi.w), oj(g, mode, Sy, Sx, vj.z, vj.w);
        const T *wi = W + (size_t)vi.y * taps, *wj = W + (size_t)vj.y * taps;
        double s = 0.;
        for_each_tap(g, oi, lane, 64, [&](int t, int c, int y, int x) {
            s += (double)wi[t] * phi_at(g, oj, wj, c * AA, y, x);
        });
        s = wave_sum(s);
        if (lane == 0) val[p] = s;
    }
}

template <typename T>
__global__ __launch_bounds__(kEventThreads) void k_events_project(EventGeo g, int mode, int Sy, int Sx,
                                                                   const T *__restrict__ W, const int4 *__restrict__ ev,
                                                                   long long n_events, const T *__restrict__ V,
                                                                   double *__restrict__ c_out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int taps = g.C * g.Ay * g.Ax;
    for (long long e = (long long)blockIdx.x * kWaves + wave; e < n_events; e += (long long)gridDim.x * kWaves) {
        const int4 v = ev[e];
        if (!row_ok(g, Sy, Sx, v)) {   // (wave-uniform: no sample data is read)
            if (lane == 0) c_out[e] = 0.;
            continue;
        }
        const Occurrence o(g, mode, Sy, Sx, v.z, v.w);
        const T *w = W + (size_t)v.y * taps;
        const size_t sample = (size_t)v.x * g.C * g.Dy * g.Dx;
        double s = 0.;
        for_each_tap(g, o, lane, 64, [&](int t, int c, int y, int x) {
            s += (double)w[t] * (double)V[sample + ((size_t)c * g.Dy + y) * g.Dx + x];
        });
        s = wave_sum(s);
        if (lane == 0) c_out[e] = s;
    }
}

// ---- NNLS -------------------------------------------------------------------------------------------------------------
// the workspace: seven K-vectors (r and pg hold one entry per block of the step) and the scalars
struct NnlsWs {
    double *x[3], *r, *pg, *rowabs, *act, *scal;
};
enum { kInvL = 0, kCmax = 1, kBeta = 2, kT = 3, kKkt = 4, kScalars = 8 };

__device__ __forceinline__ double lanes_sum(double v) {   // over the kRowLanes lanes of a row, in every one of them
#pragma unroll
    for (int off = kRowLanes / 2; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// the run of row i, clamped: nothing is read outside [0, nnz)
__device__ __forceinline__ void csr_run(const int *__restrict__ row_start, int i, int nnz, int *a, int *b) {
    *a = min(max(row_start[i], 0), nnz);
    *b = min(max(row_start[i + 1], *a), nnz);
}

// rowabs_i = sum_j |G_ij|; act_i = 1 where G_ii > 0, else 0
__global__ __launch_bounds__(kEventThreads) void k_nnls_rows(int K, int nnz, const int *__restrict__ row_start,
                                                              const int *__restrict__ col, const double *__restrict__ val,
                                                              double *__restrict__ rowabs, double *__restrict__ act) {
    const int sub = threadIdx.x % kRowLanes;
    const int i = blockIdx.x * kRowsPerBlock + threadIdx.x / kRowLanes;   // (uniform over the lanes of a row)
    double s = 0., d = 0.;
    if (i < K) {
        int a, b;
        csr_run(row_start, i, nnz, &a, &b);
        for (int k = a + sub; k < b; k += kRowLanes) {
            const int j = col[k];
            if ((unsigned)j >= (unsigned)K) continue;
            const double v = val[k];
            s += fabs(v);
            if (j == i) d += v;
        }
    }
    s = lanes_sum(s), d = lanes_sum(d);
    if (i < K && sub == 0) rowabs[i] = s, act[i] = d > 0. ? 1. : 0.;
}

// one workgroup: 1 / L with L = max_i rowabs_i, max_i |c_i|, beta = 0, t = 1
__global__ __launch_bounds__(kEventThreads) void k_nnls_scale(int K, const double *__restrict__ rowabs,
                                                               const double *__restrict__ c, double *__restrict__ scal) {
    __shared__ double s_a[kEventThreads], s_b[kEventThreads];
    double L = 0., cm = 0.;
    for (int i = threadIdx.x; i < K; i += kEventThreads) L = fmax(L, rowabs[i]), cm = fmax(cm, fabs(c[i]));
    s_a[threadIdx.x] = L, s_b[threadIdx.x] = cm;
    __syncthreads();
    for (int off = kEventThreads / 2; off >= 1; off >>= 1) {
        if ((int)threadIdx.x < off) {
            s_a[threadIdx.x] = fmax(s_a[threadIdx.x], s_a[threadIdx.x + off]);
            s_b[threadIdx.x] = fmax(s_b[threadIdx.x], s_b[threadIdx.x + off]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        scal[kInvL] = s_a[0] > 0. ? 1. / s_a[0] : 0.;
        scal[kCmax] = s_b[0];
        scal[kBeta] = 0., scal[kT] = 1., scal[kKkt] = 0.;
    }
}

// the start: h projected onto h >= 0 (NaN -> 0), 0 for a row that takes no part and for every row when max |c| = 0
__global__ __launch_bounds__(kEventThreads) void k_nnls_start(int K, const double *__restrict__ h,
                                                               const double *__restrict__ act,
                                                               const double *__restrict__ scal, double *__restrict__ x0,
                                                               double *__restrict__ x1) {
    const int i = blockIdx.x * kEventThreads + threadIdx.x;
    if (i >= K) return;
    const double v = h[i];
    const double x = act[i] > 0. && scal[kCmax] > 0. && v > 0. ? v : 0.;
    x0[i] = x, x1[i] = x;
}

__global__ __launch_bounds__(kEventThreads) void k_nnls_step(int K, int nnz, const int *__restrict__ row_start,
                                                              const int *__restrict__ col, const double *__restrict__ val,
                                                              const double *__restrict__ c, const double *__restrict__ act,
                                                              const double *__restrict__ scal,
                                                              const double *__restrict__ xp, const double *__restrict__ xc,
                                                              double *__restrict__ xn, double *__restrict__ r,
                                                              double *__restrict__ pg) {
    __shared__ double s_r[kRowsPerBlock], s_p[kRowsPerBlock];
    const int sub = threadIdx.x % kRowLanes;
    const int i = blockIdx.x * kRowsPerBlock + threadIdx.x / kRowLanes;
    const double beta = scal[kBeta], invL = scal[kInvL];
    double gy = 0., gx = 0.;
    if (i < K) {
        int a, b;
        csr_run(row_start, i, nnz, &a, &b);
        for (int k = a + sub; k < b; k += kRowLanes) {
            const int j = col[k];
            if ((unsigned)j >= (unsigned)K) continue;
            const double v = val[k], x = xc[j];
            gx = fma(v, x, gx);
            gy = fma(v, fma(beta, x - xp[j], x), gy);
        }
    }
    gy = lanes_sum(gy), gx = lanes_sum(gx);
    double rr = 0., p = 0.;
    if (i < K && sub == 0) {
        double next = 0.;
        if (act[i] > 0.) {
            const double x = xc[i], y = fma(beta, x - xp[i], x);
            next = fmax(y - (gy - c[i]) * invL, 0.);
            rr = (y - next) * (next - x);
            const double gi = gx - c[i];
            p = x > 0. ? fabs(gi) : fmax(-gi, 0.);
        }
        xn[i] = next;
    }
    // the block's share of the two reductions, its rows in row order: one entry per block for k_nnls_reduce
    if (sub == 0) s_r[threadIdx.x / kRowLanes] = rr, s_p[threadIdx.x / kRowLanes] = p;
    __syncthreads();
    if (threadIdx.x == 0) {
        double sum = 0., mx = 0.;
        for (int k = 0; k < kRowsPerBlock; ++k) sum += s_r[k], mx = fmax(mx, s_p[k]);
        r[blockIdx.x] = sum, pg[blockIdx.x] = mx;
    }
}

// one workgroup over the blocks' shares: the restart test, the next momentum coefficient, kkt of the iterate the step
// started from
__global__ __launch_bounds__(kEventThreads) void k_nnls_reduce(int K, const double *__restrict__ r,
                                                                const double *__restrict__ pg, double *__restrict__ scal) {
    __shared__ double s_a[kEventThreads], s_b[kEventThreads];
    double sum = 0., mx = 0.;
    for (int i = threadIdx.x; i < K; i += kEventThreads) sum += r[i], mx = fmax(mx, pg[i]);
    s_a[threadIdx.x] = sum, s_b[threadIdx.x] = mx;
    __syncthreads();
    for (int off = kEventThreads / 2; off >= 1; off >>= 1) {
        if ((int)threadIdx.x < off) {
            s_a[threadIdx.x] += s_a[threadIdx.x + off];
            s_b[threadIdx.x] = fmax(s_b[threadIdx.x], s_b[threadIdx.x + off]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {   // (plain stores of one lane)
        const double t = scal[kT], cm = scal[kCmax];
        double t_next = 1., beta = 0.;
        if (!(s_a[0] > 0.)) {   // no restart: the momentum goes on
            t_next = 0.5 * (1. + sqrt(1. + 4. * t * t));
            beta = (t - 1.) / t_next;
        }
        scal[kT] = t_next, scal[kBeta] = beta;
        scal[kKkt] = cm > 0. ? s_b[0] / cm : 0.;
    }
}

}  // namespace

int events_pairs(tnmf_hip_ctx *ctx, const EventGeo &g, const int *images, long long n_images, const int *cell_start,
                 const int *events, long long n_events, long long *pairs, size_t capacity, unsigned long long *count,
                 hipStream_t s) {
    TNMF_HIP_TRY(hipMemsetAsync(count, 0, sizeof(unsigned long long), s));
    if (n_images <= 0 || n_events <= 0 || g.N <= 0) return TNMF_OK;
    const unsigned grid = events_grid(ctx, (n_images + kWaves - 1) / kWaves);
    hipLaunchKernelGGL(k_events_pairs, dim3(grid), dim3(kEventThreads), 0, s, g, (const int4 *)images, (int)n_images,
                       cell_start, (const int4 *)events, (int)n_events, pairs, (unsigned long long)capacity, count);
    TNMF_LAUNCH_CHECK();
    return TNMF_OK;
}

int events_gram(tnmf_hip_ctx *ctx, const EventFrame &f, int dtype, const void *W, const int *events, long long n_events,
                const int *row_i, const int *row_j, long long n_pairs, double *val, hipStream_t s) {
    if (n_pairs <= 0) return TNMF_OK;
    const unsigned grid = events_grid(ctx, (n_pairs + kWaves - 1) / kWaves);
    with_dtype(dtype, [&](auto zero) {
        using T = decltype(zero);
        hipLaunchKernelGGL(k_events_gram<T>, dim3(grid), dim3(kEventThreads), 0, s, f.g, f.mode, f.Sy, f.Sx, (const T *)W,
                           (const int4 *)events, (int)n_events, row_i, row_j, n_pairs, val);
    });
    TNMF_LAUNCH_CHECK();
    return TNMF_OK;
}

int events_project(tnmf_hip_ctx *ctx, const EventFrame &f, int dtype, const void *W, const int *events, long long n_events,
                   const void *V, double *c, hipStream_t s) {
    if (n_events <= 0) return TNMF_OK;
    const unsigned grid = events_grid(ctx, (n_events + kWaves - 1) / kWaves);
    with_dtype(dtype, [&](auto zero) {
        using T = decltype(zero);
        hipLaunchKernelGGL(k_events_project<T>, dim3(grid), dim3(kEventThreads), 0, s, f.g, f.mode, f.Sy, f.Sx,
                           (const T *)W, (const int4 *)events, n_events, (const T *)V, c);
    });
    TNMF_LAUNCH_CHECK();
    return TNMF_OK;
}

long long events_nnls_workspace(long long n_rows) { return 7 * n_rows + kScalars; }

int events_nnls(tnmf_hip_ctx *ctx, int K, int nnz, const int *row_start, const int *col, const double *val, const double *c,
                double *h, double tol, int max_iterations, int check_every, double *workspace, int *iterations,
                double *kkt_out, int *converged, double *history, int history_capacity, int *n_history, hipStream_t s) {
    (void)ctx;
    NnlsWs w;
    for (int b = 0; b < 3; ++b) w.x[b] = workspace + (size_t)b * K;
    w.r = workspace + (size_t)3 * K, w.pg = workspace + (size_t)4 * K, w.rowabs = workspace + (size_t)5 * K;
    w.act = workspace + (size_t)6 * K, w.scal = workspace + (size_t)7 * K;
    const dim3 rows((unsigned)((K + kRowsPerBlock - 1) / kRowsPerBlock)), flat((unsigned)cdiv(K, kEventThreads));
    const dim3 block(kEventThreads);
    hipLaunchKernelGGL(k_nnls_rows, rows, block, 0, s, K, nnz, row_start, col, val, w.rowabs, w.act);
    TNMF_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_nnls_scale, dim3(1), block, 0, s, K, (const double *)w.rowabs, c, w.scal);
    TNMF_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_nnls_start, flat, block, 0, s, K, (const double *)h, (const double *)w.act,
                       (const double *)w.scal, w.x[0], w.x[1]);
    TNMF_LAUNCH_CHECK();
    int prev = 0, cur = 1, checks = 0, done = 0;
    double kkt = 0.;
    for (int it = 0;; ++it) {
        const int next = 3 - prev - cur;
        hipLaunchKernelGGL(k_nnls_step, rows, block, 0, s, K, nnz, row_start, col, val, c, (const double *)w.act,
                           (const double *)w.scal, (const double *)w.x[prev], (const double *)w.x[cur], w.x[next], w.r,
                           w.pg);
        TNMF_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_nnls_reduce, dim3(1), block, 0, s, (int)rows.x, (const double *)w.r, (const double *)w.pg,
                           w.scal);
        TNMF_LAUNCH_CHECK();
        // (kkt of an iterate comes with the step that leaves it: the check that accepts x[cur] has launched one more step,
        // whose x[next] is not used -- one launch pair in iterations + 1)
        if (it % check_every == 0 || it == max_iterations) {   // the one scalar the host reads
            TNMF_HIP_TRY(hipMemcpyAsync(&kkt, w.scal + kKkt, sizeof(double), hipMemcpyDeviceToHost, s));
            TNMF_HIP_TRY(hipStreamSynchronize(s));
            if (history && checks < history_capacity) history[2 * checks] = it, history[2 * checks + 1] = kkt;
            ++checks;
            if (kkt <= tol || it == max_iterations) {
                done = it;
                break;
            }
        }
        prev = cur, cur = next;
    }
    TNMF_HIP_TRY(hipMemcpyAsync(h, w.x[cur], (size_t)K * sizeof(double), hipMemcpyDeviceToDevice, s));
    *iterations = done, *kkt_out = kkt, *converged = kkt <= tol ? 1 : 0;
    if (n_history) *n_history = std::min(checks, history_capacity);
    return TNMF_OK;
}

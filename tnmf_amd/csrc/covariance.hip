// covariance.hip -- the diagonal of (G_AA)^-1 (include/tnmf_hip.h, "events: standard errors"): G the Gram matrix of a list in
// CSR (solve.hip), A its active rows.  G_AA is block diagonal over the connected components of its coupling graph, so the
// diagonal of the inverse is exact per component: G_cc = L L', (G_cc^-1)_ii = sum_{k >= i} (L^-1)_ki^2.  The caller hands the
// components over as lists (comp_start, member, local), ascending in size; three paths, all in double:
//
// k_inverse_diag_rows   elementwise.  A row that is not active gets NaN; a component of one row gets 1 / G_ii (its diagonal
//                       entry looked up in its CSR run).  A list of isolated rows costs this launch alone.
// k_inverse_diag_lds    one workgroup per component of 2 .. kInverseDiagLds rows, the matrix a PACKED LOWER TRIANGLE in LDS,
//                       COLUMN-major: column j starts at j n - j (j - 1) / 2 and holds rows j .. n - 1.  Every inner loop
//                       below runs the threads over the ROWS i of one column at a time: consecutive lanes touch consecutive
//                       doubles.  For 8-byte LDS accesses that is the conflict-free pattern -- a ds_read_b64 serves 32 lanes
//                       per cycle from 64 four-byte banks, a ds_write_b64 16 lanes from 32: 256 and 128 contiguous bytes --
//                       while a row-major triangle would put the lanes of a column at the strides i + 1, even for every
//                       other row (two-way conflicts and worse).  The second operand of every product is one address for the
//                       whole wave (a broadcast).  Launched per size class (16, 32, 64, 128, kInverseDiagLds rows) with
//                       that class's LDS, so that small components share a compute unit.
// k_inverse_diag_tile   the same code on a dense column-major n x n tile (plus one column) of the caller's scratch, one
//                       workgroup per component of more rows; launched in batches whose tiles fit the scratch.
//
// The steps of a component, the same in both: zero the triangle; scatter the CSR entries of its rows through `local` (one
// wave per row, the lanes over the run; an entry whose column is not active, or lies in another component, is skipped);
// Cholesky in place, left-looking -- column j takes the products of the columns before it, k ascending, then the pivot is
// tested and the column divided; the inverse of the factor in place, column by column from the last: with X = L^-1 the part
// below the diagonal of column j is -X[j+1:, j+1:] L[j+1:, j] / l_jj, which needs the columns of X to its right and column j
// of L alone, both still in place; then d_i = sum_{k >= i} X_ki^2, one wave per column, the lanes over k, the butterfly of
// wave_sum.  Every sum runs in a fixed order and nothing is accumulated by atomics: the same operands give the same bits.
//
// A pivot <= n * 2^-52 * (the ORIGINAL G_jj of that row) marks the component numerically singular: its rows get +inf and its
// status 1, the others are not touched.
#include <algorithm>
#include <cmath>
#include <limits>

#include "covariance.h"
#include "event_walk.h"

namespace {

constexpr double kEps = 2.220446049250313e-16;   // 2^-52

// the packed lower triangle, column-major
struct Packed {
    double *a;
    int n;
    __device__ __forceinline__ double &at(int i, int j) const { return a[j * n - j * (j - 1) / 2 + (i - j)]; }
    __device__ __forceinline__ int size() const { return n * (n + 1) / 2; }
};

// a dense column-major tile (only its lower triangle is used)
struct Dense {
    double *a;
    int n;
    __device__ __forceinline__ double &at(int i, int j) const { return a[(size_t)j * n + i]; }
    __device__ __forceinline__ int size() const { return n * n; }
};

// the run of row i, clamped: nothing is read outside [0, nnz)
__device__ __forceinline__ void csr_run(const int *__restrict__ row_start, int i, int nnz, int *a, int *b) {
    *a = min(max(row_start[i], 0), nnz);
    *b = min(max(row_start[i + 1], *a), nnz);
}

// the members of component c, clamped to the list: *n = 0 for a run that is not inside [0, n_active]
__device__ __forceinline__ void comp_run(const int *__restrict__ comp_start, int c, int n_active, int *first, int *n) {
    const int a = comp_start[c], b = comp_start[c + 1];
    const bool ok = a >= 0 && b >= a && b <= n_active;
    *first = ok ? a : 0, *n = ok ? b - a : 0;
}

__global__ __launch_bounds__(kEventThreads) void k_inverse_diag_rows(int K, int nnz, const int *__restrict__ row_start,
                                                                      const int *__restrict__ col,
                                                                      const double *__restrict__ val, int n_single,
                                                                      const int *__restrict__ comp_start, int n_active,
                                                                      const int *__restrict__ member,
                                                                      const int *__restrict__ local,
                                                                      double *__restrict__ d, int *__restrict__ status) {
    const int t = blockIdx.x * kEventThreads + threadIdx.x;
    if (t < K && local[t] < 0) d[t] = std::numeric_limits<double>::quiet_NaN();
    if (t >= n_single) return;
    // the singles come first, so component t is member t; any other run is not of this path (its own launch writes it)
    if (t >= n_active || comp_start[t] != t || comp_start[t + 1] != t + 1) return;
    const int i = member[t];
    if ((unsigned)i >= (unsigned)K) return;
    int a, b;
    csr_run(row_start, i, nnz, &a, &b);
    double g = 0.;
    for (int k = a; k < b; ++k)
        if (col[k] == i) g = val[k];
    const bool ok = g > 0.;   // (the bar n * 2^-52 * G_ii of a pivot that IS G_ii)
    d[i] = ok ? 1. / g : std::numeric_limits<double>::infinity();
    status[t] = ok ? 0 : 1;
}

// One workgroup, one component: mem its n rows (ascending), m the zero-initialisable storage, diag0 n doubles, tmp n doubles
// (kLds: not used, a thread owns at most one row).
template <bool kLds, typename M>
__device__ __forceinline__ void inverse_diag_component(const M m, const int n, double *diag0, double *tmp, int K, int nnz,
                                                       const int *__restrict__ row_start, const int *__restrict__ col,
                                                       const double *__restrict__ val, const int *__restrict__ mem,
                                                       const int *__restrict__ local, double *__restrict__ d,
                                                       int *__restrict__ status_c) {
    const int tid = threadIdx.x, nt = blockDim.x;
    const int lane = tid & 63, wave = tid >> 6, n_waves = nt >> 6;
    for (int e = tid; e < m.size(); e += nt) m.a[e] = 0.;
    __syncthreads();
    // the entries of the component's rows, below and on the diagonal
    for (int r = wave; r < n; r += n_waves) {
        const int i = mem[r];
        if ((unsigned)i >= (unsigned)K) continue;   // (wave-uniform)
        int a, b;
        csr_run(row_start, i, nnz, &a, &b);
        for (int k = a + lane; k < b; k += 64) {
            const int j = col[k];
            if ((unsigned)j >= (unsigned)K) continue;
            const int lj = local[j];
            if (lj < 0 || lj > r || mem[lj] != j) continue;   // not active, above the diagonal, or of another component
            m.at(r, lj) = val[k];
        }
    }
    __syncthreads();
    for (int i = tid; i < n; i += nt) diag0[i] = m.at(i, i);
    __syncthreads();
    // Cholesky, left-looking
    bool singular = false;
    for (int j = 0; j < n; ++j) {
        for (int i = j + tid; i < n; i += nt) {
            double s = m.at(i, j);
#pragma unroll 8
            for (int k = 0; k < j; ++k) s = fma(-m.at(i, k), m.at(j, k), s);   // (the loads ahead, the sum in order)
            m.at(i, j) = s;
        }
        __syncthreads();
        const double pivot = m.at(j, j);   // (the same value in every thread: the branch is uniform)
        if (!(pivot > (double)n * kEps * diag0[j])) {
            singular = true;
            break;
        }
        const double l = sqrt(pivot);
        __syncthreads();                   // (every thread has read the pivot)
        for (int i = j + tid; i < n; i += nt) m.at(i, j) = i == j ? l : m.at(i, j) / l;
        __syncthreads();
    }
    if (singular) {
        for (int i = tid; i < n; i += nt) {
            const int row = mem[i];
            if ((unsigned)row < (unsigned)K) d[row] = std::numeric_limits<double>::infinity();
        }
        if (tid == 0) *status_c = 1;
        return;
    }
    // X = L^-1 in place, from the last column
    for (int j = n - 1; j >= 0; --j) {
        const double x = 1. / m.at(j, j);
        double keep = 0.;
        for (int i = j + 1 + tid; i < n; i += nt) {
            double s = 0.;
#pragma unroll 8
            for (int k = j + 1; k <= i; ++k) s = fma(m.at(i, k), m.at(k, j), s);
            if (kLds) keep = -s * x;
            else tmp[i] = -s * x;
        }
        __syncthreads();                   // (column j of L has been read)
        for (int i = j + 1 + tid; i < n; i += nt) m.at(i, j) = kLds ? keep : tmp[i];
        if (tid == 0) m.at(j, j) = x;
        __syncthreads();
    }
    for (int i = wave; i < n; i += n_waves) {
        double s = 0.;
        for (int k = i + lane; k < n; k += 64) {
            const double v = m.at(k, i);
            s = fma(v, v, s);
        }
        s = wave_sum(s);
        const int row = mem[i];
        if (lane == 0 && (unsigned)row < (unsigned)K) d[row] = s;
    }
    if (tid == 0) *status_c = 0;
}

// components c0 .. c0 + gridDim.x - 1, each of 2 .. n_cap rows (another size: not of this launch)
__global__ __launch_bounds__(kEventThreads) void k_inverse_diag_lds(int K, int nnz, const int *__restrict__ row_start,
                                                                     const int *__restrict__ col,
                                                                     const double *__restrict__ val, int c0, int n_cap,
                                                                     const int *__restrict__ comp_start, int n_active,
                                                                     const int *__restrict__ member,
                                                                     const int *__restrict__ local, double *__restrict__ d,
                                                                     int *__restrict__ status) {
    extern __shared__ double s_inverse_diag[];
    const int c = c0 + blockIdx.x;
    int first, n;
    comp_run(comp_start, c, n_active, &first, &n);
    if (n < 2 || n > n_cap || n > (int)blockDim.x) return;   // (uniform over the workgroup)
    const Packed m{s_inverse_diag, n};
    inverse_diag_component<true>(m, n, s_inverse_diag + m.size(), nullptr, K, nnz, row_start, col, val, member + first, local,
                                 d, status + c);
}

// components c0 .. c0 + gridDim.x - 1 of more than kInverseDiagLds rows; their tiles follow each other in the scratch
__global__ __launch_bounds__(kEventThreads) void k_inverse_diag_tile(int K, int nnz, const int *__restrict__ row_start,
                                                                      const int *__restrict__ col,
                                                                      const double *__restrict__ val, int c0,
                                                                      const int *__restrict__ comp_start, int n_active,
                                                                      const int *__restrict__ member,
                                                                      const int *__restrict__ local, double *scratch,
                                                                      long long scratch_doubles, double *__restrict__ d,
                                                                      int *__restrict__ status) {
    const int c = c0 + blockIdx.x;
    int first, n;
    long long at = 0;
    for (int b = c0; b < c; ++b) {   // (the sizes of the batch before this one; a batch is short)
        comp_run(comp_start, b, n_active, &first, &n);
        at += (long long)n * n + n;
    }
    comp_run(comp_start, c, n_active, &first, &n);
    if (n <= kInverseDiagLds || at + (long long)n * n + n > scratch_doubles) return;   // (uniform over the workgroup)
    double *tile = scratch + at;
    const Dense m{tile, n};
    // (the column after the tile is the original diagonal while the matrix is factored and the new column while the factor is
    // inverted: the two are never live together)
    inverse_diag_component<false>(m, n, tile + (size_t)n * n, tile + (size_t)n * n, K, nnz, row_start, col, val,
                                  member + first, local, d, status + c);
}

}  // namespace

int events_inverse_diag(tnmf_hip_ctx *ctx, int K, int nnz, const int *row_start, const int *col, const double *val,
                        int n_comp, const int *comp_start, const int *sizes, int n_active, const int *member,
                        const int *local, double *scratch, long long scratch_doubles, double *d, int *status,
                        hipStream_t s) {
    (void)ctx;
    if (K <= 0) return TNMF_OK;
    // the sizes ascend (checked by the caller): the classes are runs, their ends found by bisection
    const auto end_of = [&](int cap) { return (int)(std::upper_bound(sizes, sizes + n_comp, cap) - sizes); };
    const int n_single = end_of(1);
    hipLaunchKernelGGL(k_inverse_diag_rows, dim3((unsigned)cdiv(K, kEventThreads)), dim3(kEventThreads), 0, s, K, nnz,
                       row_start, col, val, n_single, comp_start, n_active, member, local, d, status);
    TNMF_LAUNCH_CHECK();
    // the LDS path, a launch per size class: the class's LDS, a wave per workgroup up to 64 rows
    int c0 = n_single;
    for (const int cap : {16, 32, 64, 128, kInverseDiagLds}) {
        const int c1 = end_of(cap);
        if (c1 == c0) continue;
        const size_t lds = (size_t)cap * (cap + 3) / 2 * sizeof(double);
        if (lds > 64 * 1024)
            TNMF_HIP_TRY(hipFuncSetAttribute((const void *)k_inverse_diag_lds, hipFuncAttributeMaxDynamicSharedMemorySize,
                                             160 * 1024));
        hipLaunchKernelGGL(k_inverse_diag_lds, dim3((unsigned)(c1 - c0)), dim3(cap <= 64 ? 64 : kEventThreads), lds, s, K,
                           nnz, row_start, col, val, c0, cap, comp_start, n_active, member, local, d, status);
        TNMF_LAUNCH_CHECK();
        c0 = c1;
    }
    // the tiles in the scratch, in batches that fit it; a launch waits for the one before it on the stream
    while (c0 < n_comp) {
        int c1 = c0;
        long long used = 0;
        while (c1 < n_comp && used + events_inverse_diag_tile(sizes[c1]) <= scratch_doubles)
            used += events_inverse_diag_tile(sizes[c1++]);
        if (c1 == c0) return TNMF_E_GEOM;   // (refused by the caller before anything was launched)
        hipLaunchKernelGGL(k_inverse_diag_tile, dim3((unsigned)(c1 - c0)), dim3(kEventThreads), 0, s, K, nnz, row_start, col,
                           val, c0, comp_start, n_active, member, local, scratch, scratch_doubles, d, status);
        TNMF_LAUNCH_CHECK();
        c0 = c1;
    }
    return TNMF_OK;
}

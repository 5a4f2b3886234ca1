// rows_copy_probe.hip -- what a two-array copy in the access shape of the forward row transform of H reaches on this box:
// config 3 (8192 planes x 267 rows; source rows at a 1152-byte pitch with 1068 bytes valid, destination rows of 1152 bytes
// with 1088 written), 16 bytes per lane, no LDS, no arithmetic.  A workgroup of 256 threads moves tiles of 32 rows (the 16
// row pairs of a transform tile): 32 x 67 pieces in, 32 x 68 pieces out, nine of each per thread at the most.
//   grid forms: one workgroup per tile | persistent workgroups (PER_CU per CU) walking consecutive tiles, the next
//               tile's loads issued before the current tile's stores
//   hints:      plain | non-temporal loads | non-temporal loads and stores | non-temporal stores
// Rates count the DRAM lines touched, as the kernel's figures do: 1152 bytes read and 1088 written per row.
// Build: hipcc -O3 --offload-arch=gfx950 rows_copy_probe.hip -o rows_copy_probe
#include <hip/hip_runtime.h>
#include <cstdio>
typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int NT = 256, ROWS_T = 32, LP = 67, SP = 68, PITCH4 = 72;   // pieces of 16 bytes
constexpr int NL = (ROWS_T * LP + NT - 1) / NT, NS = (ROWS_T * SP + NT - 1) / NT;
static_assert(NL == NS, "one register per piece on both sides");

template <int HINT>
__device__ __forceinline__ void load_tile(f4 (&v)[NL], const f4 *src, long row0, long rows, int tid) {
#pragma unroll
    for (int i = 0; i < NL; ++i) {
        const int idx = tid + i * NT, r = idx / LP, c = idx - r * LP;
        v[i] = f4{0, 0, 0, 0};
        if (idx < ROWS_T * LP && row0 + r < rows) {
            const f4 *p = src + (row0 + r) * PITCH4 + c;
            v[i] = (HINT == 1 || HINT == 2) ? __builtin_nontemporal_load(p) : *p;
        }
    }
}

template <int HINT>
__device__ __forceinline__ void store_tile(const f4 (&v)[NL], f4 *dst, long row0, long rows, int tid) {
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const int idx = tid + i * NT, r = idx / SP, c = idx - r * SP;
        if (idx < ROWS_T * SP && row0 + r < rows) {
            f4 *p = dst + (row0 + r) * PITCH4 + c;
            if (HINT >= 2) __builtin_nontemporal_store(v[i], p);
            else *p = v[i];
        }
    }
}

template <int HINT>
__global__ __launch_bounds__(NT) void k_copy_tiles(const f4 *src, f4 *dst, long rows) {
    f4 v[NL];
    const long row0 = (long)blockIdx.x * ROWS_T;
    load_tile<HINT>(v, src, row0, rows, threadIdx.x);
    store_tile<HINT>(v, dst, row0, rows, threadIdx.x);
}

template <int HINT>
__global__ __launch_bounds__(NT) void k_copy_walk(const f4 *src, f4 *dst, long rows, long tiles) {
    const long per = (tiles + gridDim.x - 1) / gridDim.x;
    long t = blockIdx.x * per;
    const long t1 = t + per < tiles ? t + per : tiles;
    if (t >= t1) return;
    f4 v[NL], w[NL];
    load_tile<HINT>(v, src, t * ROWS_T, rows, threadIdx.x);
    for (; t < t1; ++t) {
        if (t + 1 < t1) load_tile<HINT>(w, src, (t + 1) * ROWS_T, rows, threadIdx.x);
        store_tile<HINT>(v, dst, t * ROWS_T, rows, threadIdx.x);
#pragma unroll
        for (int i = 0; i < NL; ++i) v[i] = w[i];
    }
}

template <typename F>
void timed(const char *what, long rows, F launch) {
    hipEvent_t a, b;
    (void)hipEventCreate(&a);
    (void)hipEventCreate(&b);
    launch();
    (void)hipDeviceSynchronize();
    (void)hipEventRecord(a);
    for (int r = 0; r < 10; ++r) launch();
    (void)hipEventRecord(b);
    (void)hipEventSynchronize(b);
    float ms;
    (void)hipEventElapsedTime(&ms, a, b);
    ms /= 10;
    const hipError_t e = hipGetLastError();
    printf("%-58s %.4f ms  %.2f TB/s%s\n", what, ms, rows * (1152.0 + 1088.0) / ms / 1e9, e == hipSuccess ? "" : "  FAILED");
}

template <int HINT>
void run(const char *hint, const f4 *src, f4 *dst, long rows) {
    const long tiles = (rows + ROWS_T - 1) / ROWS_T;
    char what[96];
    snprintf(what, sizeof what, "%s, one workgroup per tile (%ld)", hint, tiles);
    timed(what, rows, [&] { k_copy_tiles<HINT><<<(unsigned)tiles, NT>>>(src, dst, rows); });
    for (int per_cu : {2, 4, 8}) {
        snprintf(what, sizeof what, "%s, walking, %d workgroups per CU", hint, per_cu);
        timed(what, rows, [&] { k_copy_walk<HINT><<<256 * per_cu, NT>>>(src, dst, rows, tiles); });
    }
}

int main() {
    const long rows = 8192L * 267;
    f4 *src, *dst;
    if (hipMalloc(&src, rows * PITCH4 * 16) != hipSuccess || hipMalloc(&dst, rows * PITCH4 * 16) != hipSuccess) return 1;
    (void)hipMemset(src, 0, rows * PITCH4 * 16);
    (void)hipMemset(dst, 0, rows * PITCH4 * 16);
    printf("%ld rows: %.3f GB read, %.3f GB written (whole 128-byte lines)\n", rows, rows * 1152e-9, rows * 1088e-9);
    run<0>("plain", src, dst, rows);
    run<1>("non-temporal loads", src, dst, rows);
    run<2>("non-temporal loads and stores", src, dst, rows);
    run<3>("non-temporal stores", src, dst, rows);
    return hipDeviceSynchronize() == hipSuccess ? 0 : 1;
}

// Host check of tnmf_amd/csrc/modes.h, the per-axis rule of the reconstruction modes: every mode, atom lengths 1..6 and every
// activation length 1..8 that mode_axis_ok admits, exhaustively.  Built with ASan + UBSan by tests/test_modes_cpu.py: the pad
// and the fold run on heap rows of exactly the activation and the padded length, so an index one past either aborts the run.
//
//   * the padded positions that copy activation u (pad_src) are u + a - 1 and pad_dup(u): pad and fold are adjoint
//   * axis_images returns that same set ('valid': the shift itself); axis_whole: one image, wholly inside [0, D)
//   * printed for the Python side: `src <mode> <a> <S> : pad_src(0) ..` and `img <mode> <a> <S> <u> : q0 [q1]`
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "modes.h"

#define REQUIRE(cond)                                                                                   \
    do {                                                                                                \
        if (!(cond)) {                                                                                  \
            printf("FAILED %s:%d: %s (mode %d a %d S %d)\n", __FILE__, __LINE__, #cond, mode, a, S);    \
            return 1;                                                                                   \
        }                                                                                               \
    } while (0)

int main() {
    {
        const int a = 0, S = 0;
        for (int mode = -2; mode <= 5; ++mode) REQUIRE(mode_known(mode) == (mode >= 0 && mode <= 3));
    }
    for (int mode = TNMF_MODE_VALID; mode <= TNMF_MODE_REFLECT; ++mode)
        for (int a = 1; a <= 6; ++a)
            for (int S = 1; S <= 8; ++S) {
                if (!mode_axis_ok(mode, S, a)) continue;
                // the axis of D samples whose activations have S entries
                const int D = mode == TNMF_MODE_VALID ? S - a + 1 : (mode == TNMF_MODE_FULL ? S + a - 1 : S);
                if (D < 1) continue;
                REQUIRE(mode_shift_len(mode, D, a) == S);
                const int P = D + a - 1;   // the padded length, in every mode
                std::vector<std::set<int>> copies(S);
                if (mode != TNMF_MODE_VALID) {
                    // pad x, fold y: <pad x, y> == <x, fold y> on rows of exactly S and P entries
                    int *x = new int[S], *y = new int[P], *px = new int[P], *fy = new int[S];
                    for (int u = 0; u < S; ++u) x[u] = 3 * u + 1;
                    for (int j = 0; j < P; ++j) y[j] = 5 * j + 2;
                    printf("src %d %d %d :", mode, a, S);
                    for (int j = 0; j < P; ++j) {
                        const int u = pad_src(j, S, a, mode);
                        REQUIRE(u >= -1 && u < S);
                        px[j] = u >= 0 ? x[u] : 0;
                        if (u >= 0) copies[u].insert(j);
                        printf(" %d", u);
                    }
                    printf("\n");
                    long lhs = 0, rhs = 0;
                    for (int u = 0; u < S; ++u) {
                        const int dup = pad_dup(u, S, a, mode);
                        REQUIRE(dup >= -1 && dup < P && dup != u + a - 1);
                        fy[u] = y[u + a - 1] + (dup >= 0 ? y[dup] : 0);
                        std::set<int> want = {u + a - 1};
                        if (dup >= 0) want.insert(dup);
                        REQUIRE(copies[u] == want);
                        rhs += (long)x[u] * fy[u];
                    }
                    for (int j = 0; j < P; ++j) lhs += (long)px[j] * y[j];
                    REQUIRE(lhs == rhs);
                    delete[] x, delete[] y, delete[] px, delete[] fy;
                } else {
                    REQUIRE(P == S);
                    for (int u = 0; u < S; ++u) copies[u] = {u};
                }
                for (int u = 0; u < S; ++u) {
                    int q[2] = {-7, -7};
                    const int n = axis_images(mode, u, a, S, q);
                    REQUIRE(n == 1 || n == 2);
                    REQUIRE(std::set<int>(q, q + n) == copies[u] && (int)copies[u].size() == n);
                    printf("img %d %d %d %d :", mode, a, S, u);
                    for (int i = 0; i < n; ++i) printf(" %d", q[i]);
                    printf("\n");
                }
                for (int u = -2; u < S + 2; ++u) {
                    bool whole = u >= 0 && u < S && copies[u].size() == 1;
                    if (whole) {
                        const int o = *copies[u].begin() - (a - 1);   // where the image starts in the sample
                        whole = o >= 0 && o + a <= D;
                    }
                    REQUIRE(axis_whole(mode, u, a, S, D) == whole);
                }
            }
    printf("OK\n");
    return 0;
}

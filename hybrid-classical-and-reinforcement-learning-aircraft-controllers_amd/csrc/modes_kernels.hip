// modes_kernels.hip -- flight modes for whole fleets, gfx950: where the poles are, beside lqr_kernels.hip's gains, kf_kernels.hip's
// filters and margin_kernels.hip's margins.
//
// fdyn_flight_modes   per aircraft and per block the four eigenvalues of a (K = NULL: the open loop) or of a - b Kb (the loop
//                     fdyn_lqr_design closes), a, b cut out of fdyn_linearize's A, B exactly as lqr_design_kernel cuts them.
// fdyn_block_modes    the same report on two 4 x 4 per aircraft taken as they are: matrices composed on the device (the filter's
//                     Phi (I - L), the sampled loop Phi - Gamma Kb, the F_c of the margins).
// Both: eigenvalues in canonical order, six summary words per block (FD_MO_*), QR sweeps, status.  fp64, one lane per aircraft;
// the arithmetic is fdyn_eig.hpp's, which the host check compiles too.
//
// Registers, not scratch (as lqr_kernels.hip): a 4 x 4, the 3 x 3 a deflation leaves and eight result words, all indexed by
// compile-time constants; the two blocks go through ONE rolled loop, so the solver is inlined once, and what depends on the block
// is a scalar offset into global memory.  A block's words are stored as soon as they are known; a lane that ends with a
// non-zero status stores NaN over both blocks afterwards (same thread, same addresses, program order).  64-thread workgroups:
// 65 536 aircraft are 1024 waves.  Every store has the lane as its fast index.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "fdyn_fleet.hpp"
#include "fdyn_eig.hpp"
#include "../../include/fdyn_modes.h"

using namespace fdyn;

namespace {

constexpr int TB = 64;                   // threads per workgroup

// BLOCKS = false: m = a - b Kb from A [144][n], B [48][n], K [16][n] (K null: m = a; B is then not read).
// BLOCKS = true:  m from M [2][16][n] (passed as A).
template <bool BLOCKS>
__global__ void __launch_bounds__(TB)
modes_kernel(const double* __restrict__ A, const double* __restrict__ B, const double* __restrict__ K, int64_t n,
             double* __restrict__ eig_re /*[8][n]*/, double* __restrict__ eig_im /*[8][n]*/, double* __restrict__ summary /*[2][FD_NMO][n] or null*/,
             int32_t* __restrict__ iters /*[n] or null*/, int32_t* __restrict__ status /*[n]*/)
{
#pragma clang fp contract(off)
    const int64_t i = int64_t(blockIdx.x) * TB + threadIdx.x;
    if (i >= n) return;
    bool bad = false, failed = false;
    int it_max = 0;

#pragma unroll 1
    for (int blk = 0; blk < 2; ++blk) {
        double m[EIG_N][EIG_N];
        bool fin = true;
        if constexpr (BLOCKS) {
#pragma unroll
            for (int r = 0; r < EIG_N; ++r)
#pragma unroll
                for (int c = 0; c < EIG_N; ++c) m[r][c] = A[int64_t(blk * 16 + r * EIG_N + c) * n + i];
        } else {
            // rows of the block inside the 12 states and its two controls, as lqr_design_kernel reads them
            const int s0 = blk ? FD_X_V : FD_X_U, s1 = blk ? FD_X_P : FD_X_W, s2 = blk ? FD_X_R : FD_X_Q, s3 = blk ? FD_X_ROLL : FD_X_PITCH;
            const int c0 = blk ? FD_U_AILERON : FD_U_ELEVATOR, c1 = blk ? FD_U_RUDDER : FD_U_THROTTLE;
            const int sr[EIG_N] = { s0, s1, s2, s3 };
#pragma unroll
            for (int r = 0; r < EIG_N; ++r)
#pragma unroll
                for (int c = 0; c < EIG_N; ++c) m[r][c] = A[int64_t(sr[r] * FD_NX + sr[c]) * n + i];
            if (K) {
                double b[EIG_N][2], kb[2][EIG_N];
#pragma unroll
                for (int r = 0; r < EIG_N; ++r) {
                    b[r][0] = B[int64_t(sr[r] * FD_NU + c0) * n + i];
                    b[r][1] = B[int64_t(sr[r] * FD_NU + c1) * n + i];
                    fin = fin && ::isfinite(b[r][0]) && ::isfinite(b[r][1]);
                }
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int c = 0; c < EIG_N; ++c) {
                        kb[j][c] = K[int64_t((blk ? FD_LQK_LAT : FD_LQK_LON) + j * EIG_N + c) * n + i];
                        fin = fin && ::isfinite(kb[j][c]);
                    }
#pragma unroll
                for (int r = 0; r < EIG_N; ++r)
#pragma unroll
                    for (int c = 0; c < EIG_N; ++c) m[r][c] = m[r][c] - (b[r][0] * kb[0][c] + b[r][1] * kb[1][c]);
            }
        }
#pragma unroll
        for (int r = 0; r < EIG_N; ++r)
#pragma unroll
            for (int c = 0; c < EIG_N; ++c) {
                fin = fin && ::isfinite(m[r][c]);
                m[r][c] = m[r][c] + 0.0;                         // -0 enters as +0: K = NULL and K = 0 then agree to the bit
            }
        bad = bad || !fin;
        if (bad) continue;                                       // BAD_INPUT (either block): nothing is solved

        double re[EIG_N], im[EIG_N];
        int sweeps;
        failed = !eig4(m, re, im, sweeps) || failed;
        it_max = sweeps > it_max ? sweeps : it_max;
#pragma unroll
        for (int k = 0; k < EIG_N; ++k) {
            eig_re[int64_t(blk * EIG_N + k) * n + i] = re[k];
            eig_im[int64_t(blk * EIG_N + k) * n + i] = im[k];
        }
        if (summary) {
            double s[FD_NMO];
            mode_summary(re, im, s);
#pragma unroll
            for (int k = 0; k < FD_NMO; ++k) summary[int64_t(blk * FD_NMO + k) * n + i] = s[k];
        }
    }

    const int st = bad ? FD_MO_BAD_INPUT : (failed ? FD_MO_NOT_CONVERGED : 0);
    if (st) {
        const double nan = __builtin_nan("");
#pragma unroll
        for (int k = 0; k < 2 * EIG_N; ++k) { eig_re[int64_t(k) * n + i] = nan; eig_im[int64_t(k) * n + i] = nan; }
        if (summary) {
#pragma unroll
            for (int k = 0; k < 2 * FD_NMO; ++k) summary[int64_t(k) * n + i] = nan;
        }
    }
    if (iters) iters[i] = bad ? 0 : it_max;
    status[i] = st;
}

}  // namespace

extern "C" {

int fdyn_flight_modes(const double* A, const double* B, const double* K, int64_t n, double* eig_re, double* eig_im, double* summary,
                      int32_t* iters, int32_t* status, void* stream)
{
    if (n < 1 || n > (int64_t(1) << 31) - TB) return FDYN_ERR_BAD_SIZE;
    if (!A || (K && !B) || !eig_re || !eig_im || !status) return FDYN_ERR_NULL;
    return launch<TB>(modes_kernel<false>, n, stream, A, B, K, n, eig_re, eig_im, summary, iters, status);
}

int fdyn_block_modes(const double* M, int64_t n, double* eig_re, double* eig_im, double* summary, int32_t* iters, int32_t* status,
                     void* stream)
{
    if (n < 1 || n > (int64_t(1) << 31) - TB) return FDYN_ERR_BAD_SIZE;
    if (!M || !eig_re || !eig_im || !status) return FDYN_ERR_NULL;
    return launch<TB>(modes_kernel<true>, n, stream, M, (const double*)nullptr, (const double*)nullptr, n, eig_re, eig_im, summary, iters, status);
}

}  // extern "C"

// servo_covariance_kernels.hip -- predicted performance of the LQ servo for whole fleets, gfx950: the steady-state covariances of
// the loop that servo_margin_kernels.hip certifies and servo_modes_kernels.hip locates, beside servo_kernels.hip's gains and
// filters.
//
// fdyn_servo_covariance   per aircraft the variance of the state, the estimate, the tracking errors, the integrators, the controls
//                         and their step-to-step change under truth, measurement or estimate feedback: three Smith-doubling solves
//                         per block (5 x 5, 7 x 5 | 6 x 5, 7 x 7 | 6 x 6)
// fdyn_stein_solve        X = A X B^T + Q on one N x M per aircraft taken as it is, 1 <= N, M <= 7
// fp64, one lane per aircraft, 64-lane workgroups, both blocks through the same templated code; the arithmetic is
// fdyn_stein_n.hpp's, which the host check compiles too.
//
// Where the working set lives.  A doubling needs A^(2^k), X, one product and the increment at once, and the residual the A and Q it
// started from: at N = 7 six 49-word matrices, about 300 fp64 words per lane.  LDS laid out [word][lane] holds 128 words per lane in
// the 64 KB a workgroup may declare statically, and 320 with all 160 KB of the CU as dynamic LDS -- one wave per CU instead of one per
// SIMD, and every operand of the 343-term products read back from LDS.  Every index of the doubling is a compile-time constant, so
// the matrices are named words instead: registers, 512 per lane at one wave per SIMD (256 fp64 words), the rest in scratch, which
// the compiler fills with what is live across the loop but not read inside it (the A and Q kept for the residual).  That is the
// placement of servo_design_kernel and servo_kf_design_kernel, whose Riccati doubling has the same shape.  Every global load and
// store has the lane as its fast index.  Resources and throughput: DESIGN.md 7q.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "fdyn_fleet.hpp"
#include "fdyn_stein_n.hpp"
#include "../../include/fdyn_servo_covariance.h"

using namespace fdyn;

namespace {

constexpr int SB = 64;                   // threads per workgroup

__global__ void __launch_bounds__(SB)
servo_covariance_kernel(const double* __restrict__ K /*[26][n]*/, const double* __restrict__ F /*[120][n]*/,
                        const double* __restrict__ x0 /*[12][n]*/, double dt, const double* __restrict__ sigma /*[10] or [10][n]*/,
                        int sigma_per_lane, const double* __restrict__ w_rate /*null, [10] or [10][n]*/, int w_rate_per_lane, int feedback,
                        int64_t n, double* __restrict__ report /*[34][n]*/, double* __restrict__ cov /*[200][n] or null*/,
                        double* __restrict__ residual /*[n]*/, int32_t* __restrict__ iters /*[n] or null*/, int32_t* __restrict__ status /*[n]*/)
{
    const int64_t i = int64_t(blockIdx.x) * SB + threadIdx.x;
    if (i >= n) return;
    servo_covariance_lane(K + i, F + i, x0 + i, n, dt, sigma_per_lane ? sigma + i : sigma, sigma_per_lane ? n : int64_t(1),
                          w_rate ? (w_rate_per_lane ? w_rate + i : w_rate) : nullptr, w_rate_per_lane ? n : int64_t(1), feedback,
                          report + i, cov ? cov + i : nullptr, residual + i, iters ? iters + i : nullptr, status + i);
}

template <int N, int M>
__global__ void __launch_bounds__(SB)
stein_solve_kernel(const double* __restrict__ A /*[N * N][n]*/, const double* __restrict__ B /*[M * M][n]*/,
                   const double* __restrict__ Q /*[N * M][n]*/, int64_t n, double* __restrict__ X /*[N * M][n]*/,
                   double* __restrict__ residual /*[n] or null*/, int32_t* __restrict__ iters /*[n] or null*/, int32_t* __restrict__ status /*[n]*/)
{
    const int64_t i = int64_t(blockIdx.x) * SB + threadIdx.x;
    if (i >= n) return;
    stein_solve_lane<N, M>(A + i, B + i, Q + i, n, X + i, residual ? residual + i : nullptr, iters ? iters + i : nullptr, status + i);
}

bool bad_fleet(int64_t n) { return n < 1 || n > (int64_t(1) << 31) - SB; }

template <int N>
int stein_launch(int M, const double* A, const double* B, const double* Q, int64_t n, double* X, double* residual, int32_t* iters,
                 int32_t* status, void* stream)
{
    switch (M) {
    case 1: return launch<SB>(stein_solve_kernel<N, 1>, n, stream, A, B, Q, n, X, residual, iters, status);
    case 2: return launch<SB>(stein_solve_kernel<N, 2>, n, stream, A, B, Q, n, X, residual, iters, status);
    case 3: return launch<SB>(stein_solve_kernel<N, 3>, n, stream, A, B, Q, n, X, residual, iters, status);
    case 4: return launch<SB>(stein_solve_kernel<N, 4>, n, stream, A, B, Q, n, X, residual, iters, status);
    case 5: return launch<SB>(stein_solve_kernel<N, 5>, n, stream, A, B, Q, n, X, residual, iters, status);
    case 6: return launch<SB>(stein_solve_kernel<N, 6>, n, stream, A, B, Q, n, X, residual, iters, status);
    default: return launch<SB>(stein_solve_kernel<N, 7>, n, stream, A, B, Q, n, X, residual, iters, status);
    }
}

}  // namespace

extern "C" {

int fdyn_servo_covariance(const double* K, const double* F, const double* x0, double dt, const double* sigma, int sigma_per_lane,
                          const double* w_rate, int w_rate_per_lane, int feedback, int64_t n, double* report, double* cov,
                          double* residual, int32_t* iters, int32_t* status, void* stream)
{
    if (bad_fleet(n) || (feedback != FD_LQG_ESTIMATE && feedback != FD_LQG_MEASUREMENT && feedback != FD_LQG_TRUTH)) return FDYN_ERR_BAD_SIZE;
    if (!K || !F || !x0 || !sigma || !report || !residual || !status) return FDYN_ERR_NULL;
    if (bad_dt(dt)) return FDYN_ERR_BAD_DT;
    return launch<SB>(servo_covariance_kernel, n, stream, K, F, x0, dt, sigma, sigma_per_lane, w_rate, w_rate_per_lane, feedback, n, report,
                      cov, residual, iters, status);
}

int fdyn_stein_solve(const double* A, const double* B, const double* Q, int N, int M, int64_t n, double* X, double* residual,
                     int32_t* iters, int32_t* status, void* stream)
{
    if (bad_fleet(n) || N < FD_SCV_MIN_N || N > FD_SCV_MAX_N || M < FD_SCV_MIN_N || M > FD_SCV_MAX_N) return FDYN_ERR_BAD_SIZE;
    if (!A || !B || !Q || !X || !status) return FDYN_ERR_NULL;
    switch (N) {
    case 1: return stein_launch<1>(M, A, B, Q, n, X, residual, iters, status, stream);
    case 2: return stein_launch<2>(M, A, B, Q, n, X, residual, iters, status, stream);
    case 3: return stein_launch<3>(M, A, B, Q, n, X, residual, iters, status, stream);
    case 4: return stein_launch<4>(M, A, B, Q, n, X, residual, iters, status, stream);
    case 5: return stein_launch<5>(M, A, B, Q, n, X, residual, iters, status, stream);
    case 6: return stein_launch<6>(M, A, B, Q, n, X, residual, iters, status, stream);
    default: return stein_launch<7>(M, A, B, Q, n, X, residual, iters, status, stream);
    }
}

}  // extern "C"

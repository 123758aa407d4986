// servo_modes_kernels.hip -- flight modes of the LQ servo for whole fleets, gfx950: where the poles of the servo loop are, beside
// servo_kernels.hip's gains and filters and servo_margin_kernels.hip's margins, as modes_kernels.hip is the report beside the
// regulators'.
//
// fdyn_servo_flight_modes    per aircraft the seven longitudinal and six lateral poles of the continuous augmented closed loop
// fdyn_servo_sampled_modes   the same loops as they are flown at dt: zero-order hold, forward-Euler integrators
// fdyn_servo_filter_modes    the five + five poles of the filter's error dynamics (I - L) Phi
// fdyn_square_modes          the report on one N x N per aircraft taken as it is, 2 <= N <= 7
// All: eigenvalues in canonical order, six summary words per block (FD_MO_*), QR sweeps, status.  fp64, one lane per aircraft; the
// arithmetic is fdyn_eig_n.hpp's, which the host check compiles too.
//
// Unlike the 4 x 4 of modes_kernels.hip the QR window has a lane-varying position, and a matrix in registers indexed by run-time
// rows would become scratch.  So a lane composes its matrix and reduces it to Hessenberg form in registers (compile-time indices),
// then keeps it in LDS laid out [word][lane] for the sweeps: 64-thread workgroups, every row of the array 128 dwords, so a lane's
// bank depends on its lane number alone and lane-varying word indices stay conflict-free; a lane touches only its own column, so
// there is no barrier.  49 words x 64 lanes x 8 B = 25 088 B per workgroup; the 7 x 7 and the 6 x 6 (or the two 5 x 5) use it one
// after the other.  Every global load and store has the lane as its fast index.  Resources and throughput: DESIGN.md 7o.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "fdyn_fleet.hpp"
#include "fdyn_eig_n.hpp"
#include "../../include/fdyn_servo_modes.h"

using namespace fdyn;

namespace {

constexpr int SB = 64;                   // threads per workgroup (what keeps the LDS columns conflict-free and barrier-free)
constexpr int STORE_WORDS = EIGN_MAX * EIGN_MAX;

template <bool CONTINUOUS>
__global__ void __launch_bounds__(SB)
servo_modes_kernel(const double* __restrict__ A /*[144][n], or F [120][n]*/, const double* __restrict__ B /*[48][n] or null*/,
                   const double* __restrict__ x0 /*[12][n]*/, const double* __restrict__ K /*[26][n]*/, double dt, int64_t n,
                   double* __restrict__ eig_re /*[13][n]*/, double* __restrict__ eig_im /*[13][n]*/,
                   double* __restrict__ summary /*[2][FD_NMO][n] or null*/, int32_t* __restrict__ iters /*[n] or null*/,
                   int32_t* __restrict__ status /*[n]*/)
{
    __shared__ double s_words[STORE_WORDS * SB];
    const int64_t i = int64_t(blockIdx.x) * SB + threadIdx.x;
    if (i >= n) return;
    servo_modes_lane<CONTINUOUS, SB>(s_words + threadIdx.x, A + i, CONTINUOUS ? B + i : nullptr, x0 + i, K + i, dt, n, eig_re + i, eig_im + i,
                                     summary ? summary + i : nullptr, iters ? iters + i : nullptr, status + i);
}

__global__ void __launch_bounds__(SB)
servo_filter_modes_kernel(const double* __restrict__ F /*[120][n]*/, int64_t n, double* __restrict__ eig_re /*[10][n]*/,
                          double* __restrict__ eig_im /*[10][n]*/, double* __restrict__ summary /*[2][FD_NMO][n] or null*/,
                          int32_t* __restrict__ iters /*[n] or null*/, int32_t* __restrict__ status /*[n]*/)
{
    __shared__ double s_words[FD_SK_NB * FD_SK_NB * SB];
    const int64_t i = int64_t(blockIdx.x) * SB + threadIdx.x;
    if (i >= n) return;
    servo_filter_modes_lane<SB>(s_words + threadIdx.x, F + i, n, eig_re + i, eig_im + i, summary ? summary + i : nullptr,
                                iters ? iters + i : nullptr, status + i);
}

template <int N>
__global__ void __launch_bounds__(SB)
square_modes_kernel(const double* __restrict__ M /*[N * N][n]*/, int64_t n, double* __restrict__ eig_re /*[N][n]*/,
                    double* __restrict__ eig_im /*[N][n]*/, double* __restrict__ summary /*[FD_NMO][n] or null*/,
                    int32_t* __restrict__ iters /*[n] or null*/, int32_t* __restrict__ status /*[n]*/)
{
    __shared__ double s_words[N * N * SB];
    const int64_t i = int64_t(blockIdx.x) * SB + threadIdx.x;
    if (i >= n) return;
    square_modes_lane<N, SB>(s_words + threadIdx.x, M + i, n, eig_re + i, eig_im + i, summary ? summary + i : nullptr,
                             iters ? iters + i : nullptr, status + i);
}

bool bad_fleet(int64_t n) { return n < 1 || n > (int64_t(1) << 31) - SB; }

}  // namespace

extern "C" {

int fdyn_servo_flight_modes(const double* A, const double* B, const double* x0, const double* K, int64_t n, double* eig_re,
                            double* eig_im, double* summary, int32_t* iters, int32_t* status, void* stream)
{
    if (bad_fleet(n)) return FDYN_ERR_BAD_SIZE;
    if (!A || !B || !x0 || !K || !eig_re || !eig_im || !status) return FDYN_ERR_NULL;
    return launch<SB>(servo_modes_kernel<true>, n, stream, A, B, x0, K, 0.0, n, eig_re, eig_im, summary, iters, status);
}

int fdyn_servo_sampled_modes(const double* K, const double* F, const double* x0, double dt, int64_t n, double* eig_re,
                             double* eig_im, double* summary, int32_t* iters, int32_t* status, void* stream)
{
    if (bad_fleet(n)) return FDYN_ERR_BAD_SIZE;
    if (!K || !F || !x0 || !eig_re || !eig_im || !status) return FDYN_ERR_NULL;
    return launch<SB>(servo_modes_kernel<false>, n, stream, F, (const double*)nullptr, x0, K, dt, n, eig_re, eig_im, summary, iters, status);
}

int fdyn_servo_filter_modes(const double* F, int64_t n, double* eig_re, double* eig_im, double* summary, int32_t* iters,
                            int32_t* status, void* stream)
{
    if (bad_fleet(n)) return FDYN_ERR_BAD_SIZE;
    if (!F || !eig_re || !eig_im || !status) return FDYN_ERR_NULL;
    return launch<SB>(servo_filter_modes_kernel, n, stream, F, n, eig_re, eig_im, summary, iters, status);
}

int fdyn_square_modes(const double* M, int N, int64_t n, double* eig_re, double* eig_im, double* summary, int32_t* iters,
                      int32_t* status, void* stream)
{
    if (N < FD_SMO_MIN_N || N > FD_SMO_MAX_N || bad_fleet(n)) return FDYN_ERR_BAD_SIZE;
    if (!M || !eig_re || !eig_im || !status) return FDYN_ERR_NULL;
    switch (N) {
    case 2: return launch<SB>(square_modes_kernel<2>, n, stream, M, n, eig_re, eig_im, summary, iters, status);
    case 3: return launch<SB>(square_modes_kernel<3>, n, stream, M, n, eig_re, eig_im, summary, iters, status);
    case 4: return launch<SB>(square_modes_kernel<4>, n, stream, M, n, eig_re, eig_im, summary, iters, status);
    case 5: return launch<SB>(square_modes_kernel<5>, n, stream, M, n, eig_re, eig_im, summary, iters, status);
    case 6: return launch<SB>(square_modes_kernel<6>, n, stream, M, n, eig_re, eig_im, summary, iters, status);
    default: return launch<SB>(square_modes_kernel<7>, n, stream, M, n, eig_re, eig_im, summary, iters, status);
    }
}

}  // extern "C"

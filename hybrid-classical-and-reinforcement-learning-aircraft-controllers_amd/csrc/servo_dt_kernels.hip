// servo_dt_kernels.hip -- the sampled-data design of the LQ servo for whole fleets, gfx950 (include/fdyn_servo_dt.h).
//
// fdyn_servo_design_dt  fdyn_servo_design's cut of each aircraft's A, B and trim x0, designed for the loop as fdyn_servo_step_* flies
//                     it at dt: the five physical states of each block are discretised (fdyn_kalman_n.hpp's series, as
//                     fdyn_servo_kf_design forms Phi and Gamma), the Euler integrators are appended, and the block's DISCRETE Riccati
//                     equation is solved in fp64, one lane per aircraft, by fdyn_servo_dt.hpp on fdyn_riccati_n.hpp's doubling loop
//                     at N = 7 and N = 6: K = (R_d + B_d^T X B_d)^-1 B_d^T X A_d, certified by fdyn_servo_margin.hpp's squaring.
//
// servo_design_kernel's shape: 64-lane workgroups, the kernel runs once per design.  The doubling loop's own 7 x 7 words do not fit
// the register file and what the compiler cannot keep of them goes to scratch, as there.  The sampled model (A_d, B_d: 63 words) has
// to outlive that loop; it waits in LDS as [word][lane] columns.  A lane reads and writes its own column only: no barrier.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "fdyn_fleet.hpp"
#include "fdyn_servo_dt.hpp"
#include "../../include/fdyn_servo_dt.h"

using namespace fdyn;

namespace {

constexpr int DB = 64;                   // threads per workgroup

struct LaneColumn {                      // the words of one lane in LDS laid out [word][lane]
    double* col;
    FD_DEV double get(int k) const { return col[k * DB]; }
    FD_DEV void set(int k, double v) { col[k * DB] = v; }
};

__global__ void __launch_bounds__(DB)
servo_design_dt_kernel(const double* __restrict__ A /*[144][n]*/, const double* __restrict__ B /*[48][n]*/, const double* __restrict__ x0 /*[12][n]*/,
                       const double* __restrict__ weights /*[17] or [17][n]*/, int weights_per_lane, double dt, int64_t n,
                       double* __restrict__ K /*[26][n]*/, double* __restrict__ residual, int32_t* __restrict__ iters,
                       int32_t* __restrict__ status)
{
    __shared__ double s_words[SDW_N * DB];
    const int64_t i = int64_t(blockIdx.x) * DB + threadIdx.x;
    if (i >= n) return;
    LaneColumn col{ s_words + threadIdx.x };
    servo_dt_lane(col, A + i, B + i, x0 + i, n, weights_per_lane ? weights + i : weights, weights_per_lane ? n : int64_t(1), dt,
                  K + i, residual + i, iters + i, status + i);
}

}  // namespace

extern "C" {

int fdyn_servo_design_dt(const double* A, const double* B, const double* x0, const double* weights, int weights_per_lane,
                         double dt, int64_t n, double* K, double* residual, int32_t* iters, int32_t* status, void* stream)
{
    FD_CHECK_FLEET(n, 1, DB)
    if (!A || !B || !x0 || !weights || !K || !residual || !iters || !status) return FDYN_ERR_NULL;
    if (bad_dt(dt)) return FDYN_ERR_BAD_DT;
    return launch<DB>(servo_design_dt_kernel, n, stream, A, B, x0, weights, weights_per_lane, dt, n, K, residual, iters, status);
}

}  // extern "C"

// margin_kernels.hip -- loop margins for whole fleets, gfx950: the report beside lqr_kernels.hip's gains and kf_kernels.hip's filters.
//
// fdyn_loop_margins   per aircraft and per block the smallest singular value of the return difference I + L_i(z) at the plant
//                     input over a grid of points z = exp(j omega dt), the loop as it is flown: the continuous-time gain through
//                     a zero-order hold (Phi, Gamma of fdyn_kf_design) and, under estimate feedback, through the steady-state
//                     filter.  fp64, one lane per aircraft; the arithmetic is fdyn_margin.hpp's, which the host check compiles too.
//
// Registers, not scratch: a complex 4 x 4 elimination with two right-hand sides is 64 fp64 words on its own, and the lane's block
// matrices (Phi, Gamma, Kb, L_kf, F_c) are 64 more.  The matrices sit in LDS laid out [word][lane], 64-lane workgroups (64 x 64 x
// 8 B = 32 KB), the way lqg_step_kernel parks its filter, and are re-read at every grid point; the grid loop, the block loop and
// the two passes of the estimate loop are rolled around ONE inlined copy of the elimination.  Every lane touches only its own
// column, consecutive lanes consecutive addresses: no bank conflict, no barrier.  The grid z is the same for every lane and is
// read through scalar loads.  Every store has the lane as its fast index.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "fdyn_fleet.hpp"
#include "fdyn_margin.hpp"

using namespace fdyn;

namespace {

constexpr int MB = 64;                   // threads per workgroup (what keeps the LDS columns conflict-free and barrier-free)

struct LaneColumn {                      // the words of one lane in LDS laid out [word][lane]
    double* col;
    FD_DEV explicit LaneColumn(double* lds) : col(lds + threadIdx.x) {}
    FD_DEV double get(int k) const { return col[k * MB]; }
    FD_DEV void set(int k, double v) { col[k * MB] = v; }
};

__global__ void __launch_bounds__(MB)
loop_margins_kernel(const double* __restrict__ K /*[16][n]*/, const double* __restrict__ F /*[80][n]*/, int feedback,
                    const double* __restrict__ zre /*[n_omega]*/, const double* __restrict__ zim /*[n_omega]*/, int n_omega, int64_t n,
                    double* __restrict__ alpha_s /*[2][n]*/, int32_t* __restrict__ idx_s /*[2][n]*/, double* __restrict__ alpha_t /*[2][n]*/,
                    int32_t* __restrict__ idx_t /*[2][n]*/, double* __restrict__ curve /*[2][n_omega][n] or null*/,
                    int32_t* __restrict__ status /*[n]*/)
{
    __shared__ double s_words[MW_N * MB];
    const int64_t i = int64_t(blockIdx.x) * MB + threadIdx.x;
    if (i >= n) return;
    LaneColumn w(s_words);
    margin_lane(w, K + i, F + i, n, feedback, zre, zim, n_omega, alpha_s + i, idx_s + i, alpha_t + i, idx_t + i,
                curve ? curve + i : nullptr, status + i);
}

}  // namespace

extern "C" {

int fdyn_loop_margins(const double* K, const double* F, int feedback, const double* zre, const double* zim, int n_omega, int64_t n,
                      double* alpha_s, int32_t* idx_s, double* alpha_t, int32_t* idx_t, double* curve, int32_t* status, void* stream)
{
    if (n_omega < 1 || n_omega > MRG_MAX_OMEGA) return FDYN_ERR_BAD_SIZE;
    if (feedback != FD_LQG_ESTIMATE && feedback != FD_LQG_MEASUREMENT && feedback != FD_LQG_TRUTH) return FDYN_ERR_BAD_SIZE;
    FD_CHECK_FLEET(n, 1, MB)
    if (!K || !F || !zre || !zim || !alpha_s || !idx_s || !alpha_t || !idx_t || !status) return FDYN_ERR_NULL;
    return launch<MB>(loop_margins_kernel, n, stream, K, F, feedback, zre, zim, n_omega, n, alpha_s, idx_s, alpha_t, idx_t, curve, status);
}

}  // extern "C"

// servo_margin_kernels.hip -- loop margins of the LQ servo for whole fleets, gfx950: the report beside servo_kernels.hip's gains and
// filters, as margin_kernels.hip is the report beside the regulators'.
//
// fdyn_servo_loop_margins   per aircraft and per block the smallest singular value of the return difference I + L_i(z) at the plant
//                           input over a grid of points z = exp(j omega dt), the servo loop as it is flown: gain through a zero-order
//                           hold, integrators by forward Euler, and under estimate feedback through the steady-state filter, whose
//                           closed-loop matrix F_c(z) is complex.  fp64, one lane per aircraft; the arithmetic is
//                           fdyn_servo_margin.hpp's, which the host check compiles too.
//
// Registers, not scratch: a complex 5 x 5 elimination with two right-hand sides is about 90 fp64 words on its own, and the lane's
// real block matrices (Phi, Gamma, Kx, E, L, (I - L) Phi, (I - L) Gamma) are 115 more.  The matrices sit behind a word store and are
// re-read at every grid point; the grid loop, the block loop and the two passes of the estimate loop are rolled around ONE inlined
// copy of the elimination.  Two placements of the store were built and timed in the same run:
//   LaneRows     Phi, Gamma, L and Kx re-read from F and K through L2 (every load has the lane as its fast index, a wave reads 512
//                contiguous bytes per word), only the 45 derived words -- E, (I - L) Phi, (I - L) Gamma -- in LDS laid out
//                [word][lane]: 45 x 64 x 8 B = 23 040 B per 64-lane workgroup.  The one the entry point launches: the registers, not
//                LDS, then set the occupancy (one wave per SIMD, four workgroups per CU), and it ran the 65 536-aircraft fleet
//                1.55 (estimate) and 1.69 (truth) times faster than the other.
//   LaneColumn   all 115 words in LDS: 115 x 64 x 8 B = 58 880 B of static LDS, two workgroups per CU.  Built with
//                -DFDYN_SERVO_MARGIN_COLUMNS so that the comparison can be repeated (scripts/servo_margin_throughput.py --alt-lib).
// In both a lane touches only its own LDS column, consecutive lanes consecutive addresses: no bank conflict, no barrier.  The grid z
// is the same for every lane and is read by uniform index.  Every store has the lane as its fast index.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "fdyn_fleet.hpp"
#include "fdyn_servo_margin.hpp"
#include "../../include/fdyn_servo_margins.h"

using namespace fdyn;

namespace {

constexpr int MB = 64;                   // threads per workgroup (what keeps the LDS columns conflict-free and barrier-free)

#ifdef FDYN_SERVO_MARGIN_COLUMNS
constexpr int LDS_WORDS = SW_N;
struct LaneStore {                       // LaneColumn: the words of one lane in LDS laid out [word][lane]
    double* col;
    FD_DEV LaneStore(double* lds, const double*, const double*, int64_t) : col(lds + threadIdx.x) {}
    FD_DEV void begin_block(int) {}
    FD_DEV double get(int k) const { return col[k * MB]; }
    FD_DEV void set(int k, double v) { col[k * MB] = v; }
};
#else
constexpr int LDS_WORDS = SW_L - SW_E + SW_N - SW_A1;            // E, then (I - L) Phi and (I - L) Gamma
struct LaneStore {                       // LaneRows: what F and K hold is read from them, the derived words from LDS
    double* col;
    const double *K, *F, *kb, *phi, *gam, *l;
    int64_t n;
    int stride;
    FD_DEV LaneStore(double* lds, const double* K_, const double* F_, int64_t n_) : col(lds + threadIdx.x), K(K_), F(F_), n(n_) { begin_block(0); }
    FD_DEV void begin_block(int blk)
    {
        stride = SM_N + (blk ? 1 : 2);
        kb = K + int64_t(blk ? FD_SVK_LAT : FD_SVK_LON) * n;
        phi = F + int64_t(FD_SKF_PHI_LON + blk * (FD_SKF_PHI_LAT - FD_SKF_PHI_LON)) * n;
        gam = F + int64_t(FD_SKF_GAMMA_LON + blk * (FD_SKF_GAMMA_LAT - FD_SKF_GAMMA_LON)) * n;
        l = F + int64_t(FD_SKF_L_LON + blk * (FD_SKF_L_LAT - FD_SKF_L_LON)) * n;
    }
    FD_DEV double get(int k) const
    {
        if (k < SW_GAMMA) return phi[int64_t(k - SW_PHI) * n];
        if (k < SW_KX) return gam[int64_t(k - SW_GAMMA) * n];
        if (k < SW_E) return kb[int64_t(((k - SW_KX) / SM_N) * stride + (k - SW_KX) % SM_N) * n];
        if (k < SW_L) return col[(k - SW_E) * MB];
        if (k < SW_A1) return l[int64_t(k - SW_L) * n];
        return col[(k - SW_A1 + SW_L - SW_E) * MB];
    }
    FD_DEV void set(int k, double v)
    {
        if (k >= SW_E && k < SW_L) col[(k - SW_E) * MB] = v;
        else if (k >= SW_A1) col[(k - SW_A1 + SW_L - SW_E) * MB] = v;
    }
};
#endif

__global__ void __launch_bounds__(MB)
servo_loop_margins_kernel(const double* __restrict__ K /*[26][n]*/, const double* __restrict__ F /*[120][n]*/,
                          const double* __restrict__ x0 /*[12][n]*/, double dt, int feedback, const double* __restrict__ zre /*[n_omega]*/,
                          const double* __restrict__ zim /*[n_omega]*/, int n_omega, int64_t n, double* __restrict__ alpha_s /*[2][n]*/,
                          int32_t* __restrict__ idx_s /*[2][n]*/, double* __restrict__ alpha_t /*[2][n]*/, int32_t* __restrict__ idx_t /*[2][n]*/,
                          double* __restrict__ curve /*[2][n_omega][n] or null*/, int32_t* __restrict__ status /*[n]*/)
{
    __shared__ double s_words[LDS_WORDS * MB];
    const int64_t i = int64_t(blockIdx.x) * MB + threadIdx.x;
    if (i >= n) return;
    LaneStore w(s_words, K + i, F + i, n);
    servo_margin_lane(w, K + i, F + i, x0 + i, n, dt, feedback, zre, zim, n_omega, alpha_s + i, idx_s + i, alpha_t + i, idx_t + i,
                      curve ? curve + i : nullptr, status + i);
}

}  // namespace

extern "C" {

int fdyn_servo_loop_margins(const double* K, const double* F, const double* x0, double dt, int feedback, const double* zre,
                            const double* zim, int n_omega, int64_t n, double* alpha_s, int32_t* idx_s, double* alpha_t,
                            int32_t* idx_t, double* curve, int32_t* status, void* stream)
{
    if (n_omega < 1 || n_omega > MRG_MAX_OMEGA) return FDYN_ERR_BAD_SIZE;
    if (feedback != FD_LQG_ESTIMATE && feedback != FD_LQG_MEASUREMENT && feedback != FD_LQG_TRUTH) return FDYN_ERR_BAD_SIZE;
    if (n < 1 || n > (int64_t(1) << 31) - MB) return FDYN_ERR_BAD_SIZE;
    if (!K || !F || !x0 || !zre || !zim || !alpha_s || !idx_s || !alpha_t || !idx_t || !status) return FDYN_ERR_NULL;
    return launch<MB>(servo_loop_margins_kernel, n, stream, K, F, x0, dt, feedback, zre, zim, n_omega, n, alpha_s, idx_s, alpha_t, idx_t,
                      curve, status);
}

}  // extern "C"

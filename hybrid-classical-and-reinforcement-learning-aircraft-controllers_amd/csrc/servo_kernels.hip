// servo_kernels.hip -- LQ servo for whole fleets, gfx950: LQR with integral action on airspeed, altitude and heading, so that a
// fleet designed at a trim can be told to climb, turn and change speed (include/fdyn_servo.h).
//
// fdyn_servo_design   each aircraft's own A, B (fdyn_linearize) and trim x0 are cut into the augmented longitudinal block
//                     (u, w, q, theta, z, i_V, i_h | elevator, throttle) and the augmented lateral block (v, p, r, phi, psi, i_psi |
//                     aileron, rudder); each block's continuous Riccati equation is solved in fp64, one lane per aircraft, by
//                     fdyn_riccati_n.hpp (the 4 x 4 solver of lqr_kernels.hip at N = 7 and N = 6): K = R^-1 b^T X per block.
// fdyn_servo_step_*   n_steps x { errors against the references -> u = u0 - K d -> Controls::set (clips as set_controls does) ->
//                     integrators, frozen per block while one of its controls is clipped -> one RK4 of dt -> the references move
//                     at their own rates }, one launch, through the steppers of fdyn_core.hpp exactly as lqr_step_kernel calls them.
// fdyn_servo_mission_* the same step with the PID cascade's mission update and waypoint guidance (fdyn_guidance.hpp) in front of it:
//                     n_steps x { waypoint reached? -> heading, speed and altitude command -> the references -> the control step
//                     above }, one launch (include/fdyn_mission.h).  One body, servo_step_body, behind a compile-time switch.
//
// Design: two 7 x 7 / 6 x 6 solves in fp64 do not fit the register file; the matrices the compiler cannot keep go to scratch.  The
// kernel runs once per design, 64-lane workgroups.
// Step: the lane's law (26 gains, the trim point, references, integrators) does not fit beside the fp64 physics either: the words
// live in LDS as [word][lane] columns of 64-lane workgroups, as lqg_step_kernel keeps its filter; a lane reads and writes its
// own column only, so no barrier follows the staging one.
// fdyn_servo_step_wind_*, fdyn_servo_mission_wind_*  the same body once more, in a moving air mass (include/fdyn_wind.h): steady
//                     wind and a Gauss-Markov gust per aircraft.  Everything they add is behind the wind argument type; the still-
//                     air kernels are built with NoWind.
// fdyn_servo_kf_design, fdyn_servo_lqg_step_*  the servo on noisy sensors (include/fdyn_servo_lqg.h): a steady-state Kalman filter
//                     on the five physical states of each block (fdyn_kalman_n.hpp at N = 5), and the same body a third time with
//                     the measurement, the filter and the accounting around the law, behind the estimator argument type.  The
//                     estimate, du_prev and -- fp32 glue -- the filter's 120 words are further glue columns; with fp64 glue the
//                     filter would not fit the 64 KB a workgroup may declare and is read from the caller's rows every step.
// fdyn_servo_lqg_mission_*  the mission flown on the estimate (include/fdyn_servo_lqg_mission.h): the body a fourth time, with
//                     MISSION and an estimator both on.  The estimator runs FIRST here; a fixed-gain filter on a north / east
//                     position measurement (the two spare normals of the estimator's draw) gives the guidance its position, and the
//                     statistics stay on the true state.  Everything it adds is behind the EstimatorPos argument type.
// fdyn_servo_sched_step_*, fdyn_servo_sched_mission_*  the servo gain-scheduled over airspeed in flight
//                     (include/fdyn_servo_sched.h): the body a fifth time, behind the Schedule argument type.  The law reads its
//                     trim point and gains from LDS columns every step anyway; in front of each control step those columns are
//                     rewritten from the two nodes of the aircraft's table that bracket its airspeed (or its speed command).
//                     The table stays in global memory, [node][word][lane], so that a wave reads each word in one burst.
// fdyn_servo_sched_lqg_step_*  the scheduled servo on noisy sensors (include/fdyn_servo_sched_lqg.h): the body a sixth time, with
//                     an Estimator and a ScheduleLqg both on.  `reschedule` then interpolates the filter's 120 words as well and
//                     moves the estimate and du_prev to the new operating point; everything it adds is behind the ScheduleLqg
//                     argument type.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "fdyn_fleet.hpp"
#include "fdyn_guidance.hpp"
#include "fdyn_riccati_n.hpp"
#include "fdyn_kalman_n.hpp"
#include "fdyn_wind.hpp"
#include "philox.hpp"
#include "../../include/fdyn_servo.h"
#include "../../include/fdyn_mission.h"
#include "../../include/fdyn_wind.h"
#include "../../include/fdyn_servo_lqg.h"
#include "../../include/fdyn_servo_lqg_mission.h"
#include "../../include/fdyn_servo_sched.h"
#include "../../include/fdyn_servo_sched_lqg.h"

using namespace fdyn;

namespace {

constexpr int TB = 64;                   // design: threads per workgroup
constexpr int LB = 64;                   // step: threads per workgroup (what the LDS columns allow)
constexpr int NLON = FD_SV_NLON, NLAT = FD_SV_NLAT;

// the rows / columns of A and B a block reads: the first five states of each block
__device__ constexpr int LON_W[5] = { FD_X_U, FD_X_W, FD_X_Q, FD_X_PITCH, FD_X_D };
__device__ constexpr int LAT_W[5] = { FD_X_V, FD_X_P, FD_X_R, FD_X_ROLL, FD_X_YAW };

// the 5 x 5 part of an augmented block and its two control columns; everything else of a, b is zero.  False when a word is not finite.
template <int N>
FD_DEV bool load_block(const double* __restrict__ A, const double* __restrict__ B, int64_t n, int64_t i, const int (&sr)[5], int c0, int c1,
                       MN<N>& a, double (&b)[N][2])
{
    bool fin = true;
#pragma unroll
    for (int r = 0; r < N; ++r) {
#pragma unroll
        for (int c = 0; c < N; ++c) a.v[r][c] = 0.0;
        b[r][0] = b[r][1] = 0.0;
    }
#pragma unroll
    for (int r = 0; r < 5; ++r) {
#pragma unroll
        for (int c = 0; c < 5; ++c) { a.v[r][c] = A[int64_t(sr[r] * FD_NX + sr[c]) * n + i]; fin = fin && ::isfinite(a.v[r][c]); }
        b[r][0] = B[int64_t(sr[r] * FD_NU + c0) * n + i];
        b[r][1] = B[int64_t(sr[r] * FD_NU + c1) * n + i];
        fin = fin && ::isfinite(b[r][0]) && ::isfinite(b[r][1]);
    }
    return fin;
}

__global__ void __launch_bounds__(TB)
servo_design_kernel(const double* __restrict__ A /*[144][n]*/, const double* __restrict__ B /*[48][n]*/, const double* __restrict__ x0 /*[12][n]*/,
                    const double* __restrict__ weights /*[17] or [17][n]*/, int weights_per_lane, int64_t n,
                    double* __restrict__ K /*[26][n]*/, double* __restrict__ residual, int32_t* __restrict__ iters,
                    int32_t* __restrict__ status)
{
#pragma clang fp contract(off)
    const int64_t i = int64_t(blockIdx.x) * TB + threadIdx.x;
    if (i >= n) return;
    double w[FD_NSVW];
    bool bad = false;
#pragma unroll
    for (int k = 0; k < FD_NSVW; ++k) {
        w[k] = weights_per_lane ? weights[k * n + i] : weights[k];
        bad = bad || !(::isfinite(w[k]) && w[k] > 0.0);
    }
    const double u0 = x0[FD_X_U * n + i], w0 = x0[FD_X_W * n + i];
    const double V0 = ::sqrt(u0 * u0 + w0 * w0);
    bad = bad || !(::isfinite(u0) && ::isfinite(w0) && V0 > 0.0);

    double Kall[FD_NSVK];
#pragma unroll
    for (int k = 0; k < FD_NSVK; ++k) Kall[k] = 0.0;
    double res = 0.0;
    int it_max = 0, st = 0;

    {   // longitudinal: (u, w, q, theta, z) of A, then i_V' = (u0 du + w0 dw) / V0 and i_h' = -dz
        MN<NLON> a;
        double b[NLON][2], q[NLON], rinv[2];
        bad = !load_block<NLON>(A, B, n, i, LON_W, FD_U_ELEVATOR, FD_U_THROTTLE, a, b) || bad;
        a.v[5][0] = u0 / V0;
        a.v[5][1] = w0 / V0;
        a.v[6][4] = -1.0;
#pragma unroll
        for (int r = 0; r < NLON; ++r) q[r] = w[FD_SVW_Q_LON + r];
        rinv[0] = 1.0 / w[FD_SVW_R_LON];
        rinv[1] = 1.0 / w[FD_SVW_R_LON + 1];
        // the lateral block's words are read before anything is solved: BAD_INPUT (weights, trim, either block) solves nothing
        {
            bool fin = true;
#pragma unroll
            for (int r = 0; r < 5; ++r) {
#pragma unroll
                for (int c = 0; c < 5; ++c) fin = fin && ::isfinite(A[int64_t(LAT_W[r] * FD_NX + LAT_W[c]) * n + i]);
                fin = fin && ::isfinite(B[int64_t(LAT_W[r] * FD_NU + FD_U_AILERON) * n + i]) && ::isfinite(B[int64_t(LAT_W[r] * FD_NU + FD_U_RUDDER) * n + i]);
            }
            bad = bad || !fin;
        }
        if (!bad) {
            CareResult<NLON> r;
            care_solve<NLON>(a, b, q, rinv, r);
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int c = 0; c < NLON; ++c) Kall[FD_SVK_LON + j * NLON + c] = r.K[j][c];
            res = nan_max(res, r.residual);
            it_max = r.iters > it_max ? r.iters : it_max;
            if (r.failed || !r.converged) st |= FD_SV_NOT_CONVERGED;
            if (!r.positive || !(r.residual <= RIC_RES_MAX)) st |= FD_SV_NO_CERTIFICATE;
        }
    }
    if (!bad) {   // lateral: (v, p, r, phi, psi) of A, then i_psi' = dpsi
        MN<NLAT> a;
        double b[NLAT][2], q[NLAT], rinv[2];
        load_block<NLAT>(A, B, n, i, LAT_W, FD_U_AILERON, FD_U_RUDDER, a, b);
        a.v[5][4] = 1.0;
#pragma unroll
        for (int r = 0; r < NLAT; ++r) q[r] = w[FD_SVW_Q_LAT + r];
        rinv[0] = 1.0 / w[FD_SVW_R_LAT];
        rinv[1] = 1.0 / w[FD_SVW_R_LAT + 1];
        CareResult<NLAT> r;
        care_solve<NLAT>(a, b, q, rinv, r);
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int c = 0; c < NLAT; ++c) Kall[FD_SVK_LAT + j * NLAT + c] = r.K[j][c];
        res = nan_max(res, r.residual);
        it_max = r.iters > it_max ? r.iters : it_max;
        if (r.failed || !r.converged) st |= FD_SV_NOT_CONVERGED;
        if (!r.positive || !(r.residual <= RIC_RES_MAX)) st |= FD_SV_NO_CERTIFICATE;
    }

    if (bad) { st = FD_SV_BAD_INPUT; res = __builtin_nan(""); it_max = 0; }
#pragma unroll
    for (int k = 0; k < FD_NSVK; ++k) K[k * n + i] = st ? 0.0 : Kall[k];
    residual[i] = res;
    iters[i] = it_max;
    status[i] = st;
}

// The servo's estimator (include/fdyn_servo_lqg.h): the steady-state Kalman filter of the five physical states of each block,
// fdyn_kalman_n.hpp at N = 5 -- kf_design_kernel's design, one lane per aircraft.  Both blocks go through one rolled loop; what
// the compiler cannot keep of the 5 x 5 matrices goes to scratch, as in servo_design_kernel.
__global__ void __launch_bounds__(TB)
servo_kf_design_kernel(const double* __restrict__ A /*[144][n]*/, const double* __restrict__ B /*[48][n]*/, double dt,
                       const double* __restrict__ noise /*[20] or [20][n]*/, int noise_per_lane, int64_t n,
                       double* __restrict__ F /*[120][n]*/, double* __restrict__ residual, int32_t* __restrict__ iters,
                       int32_t* __restrict__ status)
{
#pragma clang fp contract(off)
    constexpr int NB = FD_SK_NB;
    const int64_t i = int64_t(blockIdx.x) * TB + threadIdx.x;
    if (i >= n) return;
    double nz[FD_NSKN];
    bool bad = !(dt > 1e-6) || dt > 1.0;
#pragma unroll
    for (int k = 0; k < FD_NSKN; ++k) {
        nz[k] = noise_per_lane ? noise[k * n + i] : noise[k];
        bad = bad || !(::isfinite(nz[k]) && nz[k] > 0.0);
    }
    // both blocks' words are read and tested before anything is solved: BAD_INPUT (dt, noise, either block) solves nothing
#pragma unroll 1
    for (int blk = 0; blk < 2; ++blk) {
        MN<NB> a;
        double b[NB][2];
        bad = !load_block<NB>(A, B, n, i, blk ? LAT_W : LON_W, blk ? FD_U_AILERON : FD_U_ELEVATOR, blk ? FD_U_RUDDER : FD_U_THROTTLE, a, b) || bad;
        bad = bad || !(row_norm<NB>(a) * dt <= KFN_NORM_MAX);
    }
    double res = 0.0;
    int it_max = 0, st = 0;
    if (!bad) {
#pragma unroll 1
        for (int blk = 0; blk < 2; ++blk) {
            MN<NB> a, Phi;
            double b[NB][2], Gam[NB][2], sg[NB], rate[NB];
            load_block<NB>(A, B, n, i, blk ? LAT_W : LON_W, blk ? FD_U_AILERON : FD_U_ELEVATOR, blk ? FD_U_RUDDER : FD_U_THROTTLE, a, b);
#pragma unroll
            for (int r = 0; r < NB; ++r) {
                sg[r] = blk ? nz[FD_SKN_SIGMA + NB + r] : nz[FD_SKN_SIGMA + r];
                rate[r] = blk ? nz[FD_SKN_RATE + NB + r] : nz[FD_SKN_RATE + r];
            }
            discretise<NB>(a, b, dt, Phi, Gam);
            KalmanResult<NB> r;
            kalman_solve<NB>(Phi, sg, rate, dt, r);
            res = nan_max(res, r.residual);
            it_max = r.iters > it_max ? r.iters : it_max;
            if (r.failed || !r.converged) st |= FD_KF_NOT_CONVERGED;
            if (!r.gain_ok || !r.positive || !(r.residual <= RIC_RES_MAX)) st |= FD_KF_NO_CERTIFICATE;

            double* Fphi = F + int64_t(FD_SKF_PHI_LON + blk * (FD_SKF_PHI_LAT - FD_SKF_PHI_LON)) * n + i;
            double* Fgam = F + int64_t(FD_SKF_GAMMA_LON + blk * (FD_SKF_GAMMA_LAT - FD_SKF_GAMMA_LON)) * n + i;
            double* Fl = F + int64_t(FD_SKF_L_LON + blk * (FD_SKF_L_LAT - FD_SKF_L_LON)) * n + i;
#pragma unroll
            for (int rr = 0; rr < NB; ++rr) {
#pragma unroll
                for (int c = 0; c < NB; ++c) { Fphi[int64_t(rr * NB + c) * n] = Phi.v[rr][c]; Fl[int64_t(rr * NB + c) * n] = r.L.v[rr][c]; }
                Fgam[int64_t(rr * 2) * n] = Gam[rr][0];
                Fgam[int64_t(rr * 2 + 1) * n] = Gam[rr][1];
            }
        }
    }
    if (bad) { st = FD_KF_BAD_INPUT; res = __builtin_nan(""); it_max = 0; }
    if (st) {                                                    // pass-through: Phi = I, Gamma = 0, L = I -> xhat = y
#pragma unroll
        for (int k = 0; k < FD_NSKF; ++k) {
            const bool gam = k >= FD_SKF_GAMMA_LON && k < FD_SKF_L_LON;
            const int at = (k < FD_SKF_GAMMA_LON ? k : k - FD_SKF_L_LON) % (NB * NB);
            F[int64_t(k) * n + i] = (!gam && at % (NB + 1) == 0) ? 1.0 : 0.0;
        }
    }
    residual[i] = res;
    iters[i] = it_max;
    status[i] = st;
}

// ---- the closed loop ------------------------------------------------------------------------------------------------------------
// One lane's column of [word][lane] LDS words.
template <typename W> struct Column {
    W* col;
    FD_DEV explicit Column(W* lds) : col(lds + threadIdx.x) {}
    FD_DEV W get(int k) const { return col[k * LB]; }
    FD_DEV void set(int k, W v) { col[k * LB] = v; }
};
// fp64 words: the eight regulated words of the trim (LqrLaw's order), its airspeed V0, then the references
enum { SD_X0 = 0, SD_V0 = 8, SD_REF = 9, SD_N = SD_REF + FD_NSVR };
// glue-type words: the gains, u0, the direction (u0, w0) / V0 of the trim's velocity, the integrators
enum { SG_K = 0, SG_U0 = FD_NSVK, SG_CU = SG_U0 + FD_NU, SG_CW, SG_INT, SG_N = SG_INT + FD_NSVI };

template <typename G> FD_DEV bool outside(G v, G lo, G hi) { return !(v >= lo && v <= hi); }     // true for NaN, as any_clipped

// What fdyn_servo_mission_* adds to a servo step (include/fdyn_mission.h); NoMission is the plain servo step.
struct NoMission {};
struct Mission {
    int32_t* wp_idx; const double* consts /*[FD_NC]*/; const double* wps /*[n_wp][4]*/; int n_wp;
    int32_t* reached_total; int32_t* steps_flown; double* stats /*[4][n]*/;
};

// What fdyn_*_wind_* add (include/fdyn_wind.h); NoWind is still air.
struct NoWind {};
struct AirMass { double* rows /*[FD_NSW][n]*/; uint64_t seed; const int32_t* step; const double* z /*[n_steps][3][n]*/; };
// three standard normals from one Philox block, as the rate env's gust update forms and pairs them (fp32 Box-Muller: statistical use)
FD_DEV void gust_normals(uint64_t seed, int64_t row, uint32_t step, double (&z)[3])
{
    uint32_t r[4];
    philox4(seed, uint32_t(row), uint32_t(uint64_t(row) >> 32), step, FD_PHX_SERVO_GUST, r);
    const float m0 = fast::sqrt(-2.0f * __logf(philox_u01(r[0]))), m1 = fast::sqrt(-2.0f * __logf(philox_u01(r[2])));
    float s0, c0, s1, c1;
    fast::sincos(6.283185307179586f * philox_u01(r[1]), s0, c0);
    fast::sincos(6.283185307179586f * philox_u01(r[3]), s1, c1);
    z[0] = double(m0 * c0); z[1] = double(m0 * s0); z[2] = double(m1 * c1);
}

// What fdyn_servo_lqg_step_* add (include/fdyn_servo_lqg.h); NoEstimator is the servo on the true state.
struct NoEstimator {};
struct Estimator {
    const double* F /*[120][n]*/; const double* sigma /*[10]*/; double* xhat /*[10][n]*/; double* du_prev /*[4][n]*/;
    uint64_t seed; const int32_t* step; const double* z /*[n_steps][10][n]*/; int feedback;
    double* err_est; double* err_meas; double* chatter; double* meas_out;
};
// the f64 step with the filter's 120 fp64 words in dynamic LDS (61 440 B behind the static columns) instead of read from F: the
// slower of the two placements on MI355X (one workgroup per CU instead of three), kept as fdyn_servo_lqg_step_f64_lds so that the
// comparison can be repeated (scripts/servo_lqg_throughput.py)
struct EstimatorDynLds : Estimator {};
// what fdyn_servo_lqg_mission_* add to the estimator (include/fdyn_servo_lqg_mission.h): the position filter of the guidance
struct EstimatorPos : Estimator { const double* pos /*[2]*/; double* phat /*[2][n]*/; double* err_pos /*[2][n]*/; };
// What fdyn_servo_sched_* add (include/fdyn_servo_sched.h); NoSchedule is the one design of x0, u0, K.
struct NoSchedule {};
struct Schedule { const double* table /*[n_nodes][FD_NSS][n]*/; int n_nodes; int on; double* sigma_out /*[2][n]*/; };
// what fdyn_servo_sched_lqg_step_* add to the schedule (include/fdyn_servo_sched_lqg.h): the filters' table, the origin of the z and
// psi words of the estimate, and the operating point the estimate is relative to
struct ScheduleLqg : Schedule { const double* table_f /*[n_nodes][FD_NSKF][n]*/; const double* origin /*[2][n]*/; double* state /*[2][n]*/; };
constexpr int DYN_F_BYTES = FD_NSKF * 64 * int(sizeof(double));
// the ten estimated words inside x, their angles, and where the trim's word sits among the fp64 columns (z0, psi0 behind SD_LQG)
__device__ constexpr int EST_W[FD_NSKX] = { FD_X_U, FD_X_W, FD_X_Q, FD_X_PITCH, FD_X_D, FD_X_V, FD_X_P, FD_X_R, FD_X_ROLL, FD_X_YAW };
constexpr int EST_PSI = 9;
constexpr bool est_angle(int j) { return j == 3 || j == 8 || j == EST_PSI; }
// twelve standard normals for lane i at this step: three Philox blocks, Box-Muller paired as lqg_step_kernel pairs its eight
FD_DEV void servo_lqg_normals(uint64_t seed, int64_t i, uint32_t step, float (&z)[12])
{
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        uint32_t r[4];
        philox4(seed, uint32_t(i), uint32_t(i >> 32), step, FD_PHX_SERVO_LQG + uint32_t(b), r);
        const float u0 = philox_u01(r[0]), u1 = philox_u01(r[1]);
        const float u2 = philox_u01(r[2]), u3 = philox_u01(r[3]);
        const float ra = sqrtf(-2.0f * __logf(u0)), rb = sqrtf(-2.0f * __logf(u2));
        z[4 * b + 0] = ra * __cosf(6.283185307f * u1); z[4 * b + 1] = ra * __sinf(6.283185307f * u1);
        z[4 * b + 2] = rb * __cosf(6.283185307f * u3); z[4 * b + 3] = rb * __sinf(6.283185307f * u3);
    }
}

// The servo step, and with MISSION the mission update and the waypoint guidance in front of each control step: guidance writes its
// three commands into the lane's SD_REF words, which the control step reads anyway, and the statistics into SD_STAT; of the
// mission only the waypoint index and two counters live in registers across the RK4.
// With an AirMass (WINDY) the lane's W + g, as the stepper takes it, and its g, A, B and W live in further columns: the law and the
// guidance read the air-relative velocity `air`, formed at the top of each control step and dead before the RK4.
// With an Estimator (LQG) each control step measures, filters and accounts around the law (`estimate`, `account`): the law is the one
// below, and reads the state the lane holds in `x`, into which the estimate's or the measurement's ten words are put for the
// duration of the call while the true ones wait in `keep`.
// With MISSION and an EstimatorPos (LM) the order of a control step changes: estimate, position filter, then the guidance on `xg`
// (the law's input with the filtered position), the law, `account`, and the statistics on the true state.
// With a Schedule (SCHED) x0, u0 and K are not read: `reschedule`, in front of the law, fills the columns the prologue fills
// otherwise, and two more fp64 columns hold the sigma they were built from and the table position.
template <typename S, typename T, bool MISSION, typename MA, typename WA = NoWind, typename EA = NoEstimator, typename SA = NoSchedule>
FD_DEV void servo_step_body(S* __restrict__ xs /*[12][n]*/, const double* __restrict__ x0 /*[12][n]*/, const double* __restrict__ u0 /*[4][n]*/,
                            const double* __restrict__ K /*[26][n]*/, double* __restrict__ ref /*[5][n]*/, double* __restrict__ integ /*[3][n]*/,
                            const double* __restrict__ limits /*[3]*/, const uint8_t* __restrict__ type, const double* __restrict__ params,
                            int n_types, int64_t n, S dt, int n_steps, S* __restrict__ surf_out /*[4][n]*/, int32_t* __restrict__ sat_steps,
                            double* __restrict__ err_out /*[3][n]*/, const MA& m, const WA& wa = WA{}, const EA& ea = EA{}, const SA& sa = SA{})
{
    using G = typename GlueOf<S, T>::type;
    constexpr bool FAST = sizeof(T) == 4;
    constexpr bool WINDY = !__is_same(WA, NoWind);
    constexpr bool LQG = !__is_same(EA, NoEstimator);
    constexpr bool LM = __is_same(EA, EstimatorPos);                             // the mission on the estimate
    static_assert(!LM || (MISSION && !WINDY), "the position filter belongs to the still-air mission");
    constexpr bool SCHED = !__is_same(SA, NoSchedule);
    constexpr bool SL = __is_same(SA, ScheduleLqg);                              // the schedule on the estimate: the filter scheduled too
    static_assert(!SCHED || (!WINDY && (!LQG || SL)), "the schedule is flown in still air; on noisy sensors only with a scheduled filter");
    static_assert(!SL || (LQG && !LM && !MISSION && !__is_same(EA, EstimatorDynLds)), "the scheduled filter belongs to the control step");
    constexpr int NZ = LM ? FD_NSKZ : FD_NSKX;                                   // normals per step of a replayed z
    constexpr bool F_DYN = __is_same(EA, EstimatorDynLds);                       // fp64 glue: the filter's words in dynamic LDS
    constexpr bool F_LDS = LQG && sizeof(G) == 4;                                // the filter's words in LDS (fp32 glue) or read from F
    static_assert(!F_DYN || sizeof(G) == 8, "the fp32 glue keeps the filter in its static columns");
    static_assert(__is_same(G, T), "the air-mass words are kept in the glue columns in the type the stepper takes");
    constexpr int SD_STAT = SD_N, SD_GUST = MISSION ? SD_N + FD_NMST : SD_N;      // WINDY: g [3], then A, B, then W [3]
    constexpr int SD_WIND = SD_GUST + 5, SD_LQG = WINDY ? SD_WIND + 3 : SD_GUST; // LQG: the trim's z and psi
    constexpr int SD_KEEP = SD_LQG + 2, SD_PHAT = SD_KEEP + FD_NSKX;             // and the true ten words while the law reads x_f; LM: phat [2]
    constexpr int SD_SIG = SL ? SD_PHAT : SD_LQG, SD_POS = SD_SIG + 1;           // SCHED: the sigma the law's columns hold, the position
    constexpr int SD_KN = SD_POS + 1, SD_T = SD_KN + 1;                          // SL: the lower node and t of the filter's words (t < 0: exact)
    constexpr int SD_WORDS = SL ? SD_T + 1 : (SCHED ? SD_POS + 1 : (LM ? SD_PHAT + 2 : (LQG ? SD_PHAT : SD_LQG)));
    constexpr int SG_AIR = SG_N, SG_XHAT = WINDY ? SG_N + 3 : SG_N;              // WINDY: W + g [3]; LQG: xhat [10], du_prev [4], F [120]
    constexpr int SG_DU = SG_XHAT + FD_NSKX, SG_F = SG_DU + FD_NU;
    constexpr int SG_WORDS = LQG ? (F_LDS ? SG_F + FD_NSKF : SG_F) : SG_XHAT;
    __shared__ double s_params[FD_MAX_TYPES * FD_NP_STAGED];
    __shared__ double s_d[SD_WORDS * LB];
    __shared__ G s_g[SG_WORDS * LB];
    __shared__ G s_consts[MISSION ? FD_NC_STAGED : 1];
    __shared__ G s_wps[MISSION ? FD_MAX_WAYPOINTS * FD_NWP : 1];
    stage_params<FAST>(s_params, params, n_types);
    if constexpr (MISSION) {
        stage_guidance_consts<G>(s_consts, m.consts);
        for (int k = threadIdx.x; k < m.n_wp * FD_NWP; k += blockDim.x) s_wps[k] = G(m.wps[k]);
    }
    __syncthreads();
    const int64_t i = int64_t(blockIdx.x) * LB + threadIdx.x;
    if (i >= n) return;
    Column<double> ld(s_d);
    Column<G> lg(s_g);
    int32_t idx = 0, reached = 0, flown = 0;                     // mission: the lane's waypoint, the waypoints reached and the steps flown here
    bool restart = false;
    if constexpr (MISSION) {
        idx = m.wp_idx[i];
        idx = idx < 0 ? 0 : idx;
        restart = int(m.consts[FD_C_ON_COMPLETE]) == 1;
        constexpr double START[FD_NMST] = { 0.0, 0.0, __builtin_inf(), 0.0 };
#pragma unroll
        for (int k = 0; k < FD_NMST; ++k) ld.set(SD_STAT + k, m.stats ? m.stats[int64_t(k) * n + i] : START[k]);
        if constexpr (LM) { if (idx >= m.n_wp && !restart) return; }   // complete at entry: not even a measurement
    }
    {
#pragma clang fp contract(off)
        if constexpr (SL) {                                      // the operating point the caller's xhat and du_prev are relative to
            ld.set(SD_SIG, sa.state[i]);
            ld.set(SD_POS, sa.state[n + i]);
        } else if constexpr (SCHED) {
            ld.set(SD_POS, -1.0);                                // no position is negative: the law's columns hold nothing yet
        } else {
            constexpr int W[8] = { FD_X_U, FD_X_W, FD_X_Q, FD_X_PITCH, FD_X_V, FD_X_P, FD_X_R, FD_X_ROLL };
#pragma unroll
            for (int j = 0; j < 8; ++j) ld.set(SD_X0 + j, x0[W[j] * n + i]);
            const double tu = x0[FD_X_U * n + i], tw = x0[FD_X_W * n + i];
            const double V0 = ::sqrt(tu * tu + tw * tw);
            const bool moving = V0 > 0.0;                        // false only for a lane whose design was refused (K = 0)
            ld.set(SD_V0, V0);
            lg.set(SG_CU, G(moving ? tu / V0 : 0.0));
            lg.set(SG_CW, G(moving ? tw / V0 : 0.0));
        }
#pragma unroll
        for (int k = 0; k < FD_NSVR; ++k) ld.set(SD_REF + k, ref[int64_t(k) * n + i]);
        if constexpr (!SCHED) {
#pragma unroll
            for (int k = 0; k < FD_NSVK; ++k) lg.set(SG_K + k, G(K[int64_t(k) * n + i]));
#pragma unroll
            for (int k = 0; k < FD_NU; ++k) lg.set(SG_U0 + k, G(u0[int64_t(k) * n + i]));
        }
#pragma unroll
        for (int k = 0; k < FD_NSVI; ++k) lg.set(SG_INT + k, G(integ[int64_t(k) * n + i]));
        if constexpr (WINDY) {
#pragma unroll
            for (int k = 0; k < 5; ++k) ld.set(SD_GUST + k, wa.rows[int64_t(FD_SW_GUST_N + k) * n + i]);
            // the steady wind too, so that the step loop reads nothing of the air mass from memory but z
#pragma unroll
            for (int k = 0; k < 3; ++k) ld.set(SD_WIND + k, wa.rows[int64_t(FD_SW_WIND_N + k) * n + i]);
        }
        if constexpr (LQG) {
            if constexpr (SL) {
                ld.set(SD_LQG + 0, sa.origin[i]);
                ld.set(SD_LQG + 1, sa.origin[n + i]);
            } else {
                ld.set(SD_LQG + 0, x0[FD_X_D * n + i]);
                ld.set(SD_LQG + 1, x0[FD_X_YAW * n + i]);
            }
#pragma unroll
            for (int j = 0; j < FD_NSKX; ++j) lg.set(SG_XHAT + j, G(ea.xhat[int64_t(j) * n + i]));
#pragma unroll
            for (int k = 0; k < FD_NU; ++k) lg.set(SG_DU + k, G(ea.du_prev[int64_t(k) * n + i]));
            if constexpr (LM) {
#pragma unroll
                for (int k = 0; k < 2; ++k) ld.set(SD_PHAT + k, ea.phat[int64_t(k) * n + i]);
            }
            if constexpr (F_LDS && !SL) {                        // a few words at a time, before the physics' own registers are loaded
#pragma unroll
                for (int k = 0; k < FD_NSKF; ++k) {
                    if (k % 16 == 0) asm volatile("" ::: "memory");
                    lg.set(SG_F + k, G(ea.F[int64_t(k) * n + i]));
                }
            }
            if constexpr (F_DYN) {
                extern __shared__ double s_dyn_f[];              // [120][lane]; the static columns before it end on a 16-byte boundary
#pragma unroll
                for (int k = 0; k < FD_NSKF; ++k) {
                    if (k % 16 == 0) asm volatile("" ::: "memory");
                    s_dyn_f[k * LB + threadIdx.x] = ea.F[int64_t(k) * n + i];
                }
            }
        }
    }
    S x[FD_NX];
#pragma unroll
    for (int k = 0; k < FD_NX; ++k) x[k] = xs[k * n + i];
    asm volatile("" ::: "memory");
    const double* blk = s_params + lane_type(type, i, n_types) * FD_NP_STAGED;
    Params<T> P; P.load(blk);
    Limits<S> Lm; Lm.load(blk);
    Surfaces<G> surf{ G(0), G(0), G(0), G(0) };
    G err[FD_NSVI] = { G(0), G(0), G(0) };
    int sat = 0;
    // WINDY: the air-relative body velocity of this control step and its length, in the storage type
    S air[3] = { S(0), S(0), S(0) }, Vair = S(0);
    G Vguide = G(0);                                             // |v_air| as the guidance reads it (mixed, f32: derived_fast's form)
    float nbw[3] = { 0.0f, 0.0f, 0.0f };                         // mixed, f32: -R^T (W + g)
    uint32_t step0 = 0u;
    if constexpr (WINDY) step0 = wa.step ? uint32_t(*wa.step) : 0u;
    // a. the air mass of this control step, W + g summed in fp64, into its columns
    auto set_air_mass = [&]() {
        if constexpr (WINDY) {
#pragma clang fp contract(off)
#pragma unroll
            for (int k = 0; k < 3; ++k) lg.set(SG_AIR + k, G(ld.get(SD_WIND + k) + ld.get(SD_GUST + k)));
        }
    };
    // b. v_air = v - R^T (W + g) from the given sines and cosines
    auto set_air = [&](auto sphi, auto cphi, auto sth, auto cth, auto spsi, auto cpsi) {
        if constexpr (WINDY) {
#pragma clang fp contract(off)
            using A = decltype(sphi);
            A ua, va, wv;
            if constexpr (FAST) {                                // the rotation in fp32, the difference in the storage type
                air_relative<A>(A(0), A(0), A(0), sphi, cphi, sth, cth, spsi, cpsi, lg.get(SG_AIR + 0), lg.get(SG_AIR + 1), lg.get(SG_AIR + 2), ua, va, wv);
                air[0] = x[FD_X_U] + S(ua); air[1] = x[FD_X_V] + S(va); air[2] = x[FD_X_W] + S(wv);
                nbw[0] = ua; nbw[1] = va; nbw[2] = wv;
            } else {
                air_relative<A>(x[FD_X_U], x[FD_X_V], x[FD_X_W], sphi, cphi, sth, cth, spsi, cpsi, lg.get(SG_AIR + 0), lg.get(SG_AIR + 1), lg.get(SG_AIR + 2), ua, va, wv);
                air[0] = ua; air[1] = va; air[2] = wv;
            }
            Vair = M<S>::sqrt((air[0] * air[0] + air[1] * air[1]) + air[2] * air[2]);
            if constexpr (!FAST) Vguide = G(Vair);
        }
    };
    auto air_mass = [&]() -> Wind<T> {
        if constexpr (WINDY) return Wind<T>{ lg.get(SG_AIR + 0), lg.get(SG_AIR + 1), lg.get(SG_AIR + 2) };
        else return Wind<T>{};
    };
    // f. the gust update of control step s of this launch
    auto gust = [&](int s) {
        if constexpr (WINDY) {
            double zn[3];
            if (wa.z) {
#pragma unroll
                for (int k = 0; k < 3; ++k) zn[k] = wa.z[(int64_t(s) * 3 + k) * n + i];
            } else {
                gust_normals(wa.seed, i, step0 + uint32_t(s) + 1u, zn);
            }
            const double ga = ld.get(SD_GUST + 3), gb = ld.get(SD_GUST + 4);
#pragma unroll
            for (int k = 0; k < 3; ++k) ld.set(SD_GUST + k, gust_update(ld.get(SD_GUST + k), ga, gb, zn[k]));
        }
    };

    // SCHED, steps 0a-0c (include/fdyn_servo_sched.h): the law's columns from the two nodes that bracket sigma.  Skipped when sigma
    // is bitwise the one the columns were built from (on the command: nearly every step); the columns are then what this would
    // write.  Eight words in flight at a time, and everything it computes is dead when it returns.
    // SL (include/fdyn_servo_sched_lqg.h): the filter's words are interpolated with the others -- fp32 glue: into their columns;
    // fp64 glue: the lower node and t are kept and `fword` interpolates from the table -- and the estimate and du_prev are moved to
    // the new operating point.  `entry`: the call at launch entry, which rebuilds the columns from the stored sigma (or enters the
    // table with V_c) and moves nothing.
    auto reschedule = [&](bool entry = false) {
        if constexpr (SCHED) {
#pragma clang fp contract(off)
            asm volatile("" ::: "memory");
            double sg;
            if constexpr (SL) {
                if (entry) sg = ld.get(SD_POS) >= 0.0 ? ld.get(SD_SIG) : ld.get(SD_REF + FD_SVR_SPEED);
                else if (sa.on == FD_SCHED_ON_COMMAND) sg = ld.get(SD_REF + FD_SVR_SPEED);
                else sg = double(M<S>::sqrt((x[FD_X_U] * x[FD_X_U] + x[FD_X_V] * x[FD_X_V]) + x[FD_X_W] * x[FD_X_W]));
                if (!entry && __double_as_longlong(sg) == __double_as_longlong(ld.get(SD_SIG))) return;
            } else {
                if (sa.on == FD_SCHED_ON_COMMAND) sg = ld.get(SD_REF + FD_SVR_SPEED);
                else sg = double(M<S>::sqrt((x[FD_X_U] * x[FD_X_U] + x[FD_X_V] * x[FD_X_V]) + x[FD_X_W] * x[FD_X_W]));
                if (ld.get(SD_POS) >= 0.0 && __double_as_longlong(sg) == __double_as_longlong(ld.get(SD_SIG))) return;
            }
            // the lane index and the row stride made opaque, as the estimator's: none of these addresses lives across the RK4
            int64_t il = i, nl = n;
            asm volatile("" : "+v"(il), "+s"(nl));
            const double* __restrict__ tb = sa.table + il;
            const int last = sa.n_nodes - 1;
            int k = 0;
            double t = 0.0, pos = 0.0;
            bool exact = true;                                   // a node's words as they are: below, above, NaN
            const double v0 = tb[int64_t(FD_SS_V) * nl];
            if (sg > v0) {
                const double vl = tb[int64_t(last * FD_NSS + FD_SS_V) * nl];
                if (sg >= vl) { k = last; pos = double(last); }
                else {                                           // V_0 < sigma < V_last: last >= 1, and k + 1 <= last
                    double vk = v0;
#pragma unroll 1
                    for (int j = 1; j < last; ++j) {
                        const double vj = tb[int64_t(j * FD_NSS + FD_SS_V) * nl];
                        if (vj <= sg) { k = j; vk = vj; }
                    }
                    const double vn = tb[int64_t((k + 1) * FD_NSS + FD_SS_V) * nl];
                    t = (sg - vk) / (vn - vk);
                    pos = double(k) + t;
                    exact = false;
                }
            }
            const double* __restrict__ lo = tb + int64_t(k * FD_NSS) * nl;
            const double* __restrict__ hi = exact ? lo : lo + int64_t(FD_NSS) * nl;
            auto word = [&](int r) -> double {
                const double a = lo[int64_t(r) * nl], b = hi[int64_t(r) * nl];
                return exact ? a : a + t * (b - a);
            };
            if constexpr (SL) {
                // step 4: the estimate and du_prev to the new operating point, differences and sums in fp64
                constexpr int XH[8] = { 0, 1, 2, 3, 5, 6, 7, 8 };  // (u, w, q, theta | v, p, r, phi) among the ten estimated words
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    const double was = ld.get(SD_X0 + r), now = word(FD_SS_X0 + r);
                    ld.set(SD_X0 + r, now);
                    if (!entry) {
                        G xh = G(double(lg.get(SG_XHAT + XH[r])) + (was - now));
                        if (est_angle(XH[r]) && !(xh >= G(-FD_PI) && xh < G(FD_PI))) xh = wrap_angle<G>(xh);
                        lg.set(SG_XHAT + XH[r], xh);
                    }
                }
                asm volatile("" ::: "memory");
#pragma unroll
                for (int r = 0; r < FD_NU; ++r) {
                    const G was = lg.get(SG_U0 + r), now = G(word(FD_SS_U0 + r));
                    lg.set(SG_U0 + r, now);
                    if (!entry) lg.set(SG_DU + r, G(double(lg.get(SG_DU + r)) + (double(was) - double(now))));
                }
                if constexpr (F_LDS) {
                    const double* __restrict__ flo = sa.table_f + il + int64_t(k * FD_NSKF) * nl;
                    const double* __restrict__ fhi = exact ? flo : flo + int64_t(FD_NSKF) * nl;
#pragma unroll
                    for (int r = 0; r < FD_NSKF; ++r) {
                        if (r % 8 == 0) asm volatile("" ::: "memory");
                        const double a = flo[int64_t(r) * nl], b = fhi[int64_t(r) * nl];
                        lg.set(SG_F + r, G(exact ? a : a + t * (b - a)));
                    }
                } else {
                    ld.set(SD_KN, double(k));
                    ld.set(SD_T, exact ? -1.0 : t);
                }
            } else {
#pragma unroll
                for (int r = 0; r < 8; ++r) ld.set(SD_X0 + r, word(FD_SS_X0 + r));
                asm volatile("" ::: "memory");
#pragma unroll
                for (int r = 0; r < FD_NU; ++r) lg.set(SG_U0 + r, G(word(FD_SS_U0 + r)));
            }
#pragma unroll
            for (int r = 0; r < FD_NSVK; ++r) {
                if (r % 8 == 4) asm volatile("" ::: "memory");
                lg.set(SG_K + r, G(word(FD_SS_K + r)));
            }
            const double tu = ld.get(SD_X0 + 0), tw = ld.get(SD_X0 + 1);
            const double V0 = ::sqrt(tu * tu + tw * tw);
            const bool moving = V0 > 0.0;
            ld.set(SD_V0, V0);
            lg.set(SG_CU, G(moving ? tu / V0 : 0.0));
            lg.set(SG_CW, G(moving ? tw / V0 : 0.0));
            ld.set(SD_SIG, sg);
            ld.set(SD_POS, pos);
        }
    };
    if constexpr (SL) reschedule(true);

    // one control step up to the integrators: returns the unclipped controls (Controls::set clips).  `advance` is false for the
    // controls-only call (n_steps = 0), which writes nothing.
    auto control = [&](bool advance) -> Surfaces<G> {
#pragma clang fp contract(off)
        // the law's words never change within a launch; re-read every step, or the compiler keeps them in registers across the RK4
        asm volatile("" ::: "memory");
        const double Vc = ld.get(SD_REF + FD_SVR_SPEED), hc = ld.get(SD_REF + FD_SVR_ALTITUDE), pc = ld.get(SD_REF + FD_SVR_HEADING);
        // 1. errors: differences in fp64 from the stored state, then the glue type
        S V, xu = x[FD_X_U], xv = x[FD_X_V], xw = x[FD_X_W];
        if constexpr (WINDY) { V = Vair; xu = air[0]; xv = air[1]; xw = air[2]; }
        else V = M<S>::sqrt((x[FD_X_U] * x[FD_X_U] + x[FD_X_V] * x[FD_X_V]) + x[FD_X_W] * x[FD_X_W]);
        err[FD_SVI_SPEED] = G(double(V) - Vc);
        err[FD_SVI_ALTITUDE] = G(-double(x[FD_X_D]) - hc);
        err[FD_SVI_HEADING] = wrap_angle<G>(G(double(x[FD_X_YAW]) - pc));
        G e[FD_NSVI];
#pragma unroll
        for (int k = 0; k < FD_NSVI; ++k) { const G lim = G(limits[k]); e[k] = clipv<G>(err[k], -lim, lim); }
        // 2. deviations
        const G dV = G(Vc - ld.get(SD_V0));
        G dl[NLON], da[NLAT];
        dl[0] = G(double(xu) - ld.get(SD_X0 + 0)) - dV * lg.get(SG_CU);
        dl[1] = G(double(xw) - ld.get(SD_X0 + 1)) - dV * lg.get(SG_CW);
        dl[2] = G(double(x[FD_X_Q]) - ld.get(SD_X0 + 2));
        dl[3] = wrap_angle<G>(G(double(x[FD_X_PITCH]) - ld.get(SD_X0 + 3)));
        dl[4] = -e[FD_SVI_ALTITUDE];
        dl[5] = lg.get(SG_INT + FD_SVI_SPEED);
        dl[6] = lg.get(SG_INT + FD_SVI_ALTITUDE);
        da[0] = G(double(xv) - ld.get(SD_X0 + 4));
        da[1] = G(double(x[FD_X_P]) - ld.get(SD_X0 + 5));
        da[2] = G(double(x[FD_X_R]) - ld.get(SD_X0 + 6));
        da[3] = wrap_angle<G>(G(double(x[FD_X_ROLL]) - ld.get(SD_X0 + 7)));
        da[4] = e[FD_SVI_HEADING];
        da[5] = lg.get(SG_INT + FD_SVI_HEADING);
        // 3. u = u0 - K d, each row summed left to right
        G s[4];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            G a = lg.get(SG_K + FD_SVK_LON + r * NLON) * dl[0];
#pragma unroll
            for (int c = 1; c < NLON; ++c) a = a + lg.get(SG_K + FD_SVK_LON + r * NLON + c) * dl[c];
            s[r] = a;
            G t = lg.get(SG_K + FD_SVK_LAT + r * NLAT) * da[0];
#pragma unroll
            for (int c = 1; c < NLAT; ++c) t = t + lg.get(SG_K + FD_SVK_LAT + r * NLAT + c) * da[c];
            s[2 + r] = t;
        }
        Surfaces<G> u;
        u.elevator = lg.get(SG_U0 + FD_U_ELEVATOR) - s[0]; u.throttle = lg.get(SG_U0 + FD_U_THROTTLE) - s[1];
        u.aileron = lg.get(SG_U0 + FD_U_AILERON) - s[2]; u.rudder = lg.get(SG_U0 + FD_U_RUDDER) - s[3];
        if (advance) {
            const bool lon = outside(u.elevator, G(-1), G(1)) || outside(u.throttle, G(0), G(1));
            const bool lat = outside(u.aileron, G(-1), G(1)) || outside(u.rudder, G(-1), G(1));
            sat += (lon || lat) ? 1 : 0;
            // 4. anti-windup: a block's integrators hold while one of its controls is clipped
            const G gdt = G(dt);
            if (!lon) {
                lg.set(SG_INT + FD_SVI_SPEED, dl[5] + e[FD_SVI_SPEED] * gdt);
                lg.set(SG_INT + FD_SVI_ALTITUDE, dl[6] + e[FD_SVI_ALTITUDE] * gdt);
            }
            if (!lat) lg.set(SG_INT + FD_SVI_HEADING, da[5] + e[FD_SVI_HEADING] * gdt);
        }
        return u;
    };
    // 6. the references move at their own rates, in fp64
    auto move_refs = [&]() {
#pragma clang fp contract(off)
        const double ddt = double(dt);
        ld.set(SD_REF + FD_SVR_ALTITUDE, ld.get(SD_REF + FD_SVR_ALTITUDE) + ld.get(SD_REF + FD_SVR_CLIMB_RATE) * ddt);
        ld.set(SD_REF + FD_SVR_HEADING, wrap_angle<double>(ld.get(SD_REF + FD_SVR_HEADING) + ld.get(SD_REF + FD_SVR_TURN_RATE) * ddt));
    };

    // ---- LQG (include/fdyn_servo_lqg.h): everything below is empty without an Estimator
    uint32_t lstep0 = 0u;
    // the lane index of the estimator's global addresses, made opaque anew every step: computed from `i` they are loop invariants,
    // hoisted out of the step loop into registers that live across the RK4
    int64_t il = i, nl = n;                                      // and the row stride, or every row's offset is hoisted as well
    if constexpr (LQG) lstep0 = ea.step ? uint32_t(*ea.step) : 0u;
    // the fp64 column of the trim's word j of the ten: SD_X0 holds (u, w, q, theta | v, p, r, phi), SD_LQG z and psi
    auto trim_word = [&](int j) -> double { return ld.get(j == 4 ? SD_LQG : (j == EST_PSI ? SD_LQG + 1 : (j < 4 ? SD_X0 + j : SD_X0 + j - 1))); };
    // SL, fp64 glue: the two nodes' rows of the filter at this lane and t, set at the top of `estimate` and dead when it returns
    const double* __restrict__ f_lo = nullptr;
    const double* __restrict__ f_hi = nullptr;
    double f_t = 0.0;
    bool f_exact = true;
    auto fword = [&](int k) -> G {
        if constexpr (F_LDS) return lg.get(SG_F + k);
        else if constexpr (SL) {
#pragma clang fp contract(off)
            const double a = f_lo[int64_t(k) * nl], b = f_hi[int64_t(k) * nl];
            return G(f_exact ? a : a + f_t * (b - a));
        }
        else if constexpr (F_DYN) { extern __shared__ double s_dyn_f[]; return G(s_dyn_f[k * LB + threadIdx.x]); }
        else if constexpr (LQG) return G(ea.F[int64_t(k) * nl + il]);
        else return G(0);
    };
    // the accumulators are the caller's words in global memory, added to step by step: no instantiation has 24 fp64 registers
    // to spare across the RK4
    auto add_square = [&](double* __restrict__ words, int row, double t) {
#pragma clang fp contract(off)
        if (words) words[int64_t(row) * nl + il] = words[int64_t(row) * nl + il] + t * t;
    };
    // step 5 for the five words of block b: x_f = x0 + f, in fp64 with psi wrapped, into x; the true words wait in their columns
    // (exact: the storage type widened to fp64)
    auto put = [&](int b, const G (&f)[FD_SK_NB]) {
        if constexpr (LQG) {
#pragma clang fp contract(off)
#pragma unroll
            for (int r = 0; r < FD_SK_NB; ++r) {
                const int j = FD_SK_NB * b + r;
                double xf = trim_word(j) + double(f[r]);
                if (j == EST_PSI) xf = wrap_angle<double>(xf);
                ld.set(SD_KEEP + j, double(x[EST_W[j]]));
                x[EST_W[j]] = S(xf);
            }
        }
    };
    float zpos[2] = { 0.0f, 0.0f };                              // LM: the two normals of the draw the estimator leaves over
    G xg[LM ? FD_NX : 1];                                        // LM: the state the guidance reads
    // steps 1-5 of control step s: measure, filter, account, block by block; then the law's input goes into x
    auto estimate = [&](int s) {
        if constexpr (LQG) {
#pragma clang fp contract(off)
            constexpr int NB = FD_SK_NB;
            // LM: the step loop has a divergent exit, and a scalar carried round it through these statements would need a vector
            // register at the join: start again from the arguments instead
            if constexpr (LM) { il = i; nl = n; }
            asm volatile("" : "+v"(il), "+s"(nl) :: "memory");   // the filter words are re-read every step, as the law's
            if constexpr (SL && !F_LDS) {
                const double tt = ld.get(SD_T);
                f_exact = tt < 0.0;
                f_t = f_exact ? 0.0 : tt;
                f_lo = sa.table_f + il + int64_t(int(ld.get(SD_KN)) * FD_NSKF) * nl;
                f_hi = f_exact ? f_lo : f_lo + int64_t(FD_NSKF) * nl;
            }
            float zn[12] = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };
            if (!ea.z) servo_lqg_normals(ea.seed, i, lstep0 + uint32_t(s) + 1u, zn);
            if constexpr (LM) { zpos[0] = zn[FD_NSKX]; zpos[1] = zn[FD_NSKX + 1]; }
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const int o = NB * b, phi = b ? FD_SKF_PHI_LAT : FD_SKF_PHI_LON, gam = b ? FD_SKF_GAMMA_LAT : FD_SKF_GAMMA_LON;
                const int lgn = b ? FD_SKF_L_LAT : FD_SKF_L_LON;
                G d[NB], y[NB], old[NB], pred[NB], e[NB], xh[NB];
#pragma unroll
                for (int r = 0; r < NB; ++r) {
                    const G t = G(double(x[EST_W[o + r]]) - trim_word(o + r));
                    d[r] = est_angle(o + r) ? wrap_angle<G>(t) : t;
                    const G z = ea.z ? G(ea.z[(int64_t(s) * NZ + o + r) * nl + il]) : G(zn[o + r]);
                    y[r] = d[r] + G(ea.sigma[o + r]) * z;
                    old[r] = lg.get(SG_XHAT + o + r);
                }
                const G du0 = lg.get(SG_DU + (b ? FD_U_AILERON : FD_U_ELEVATOR)), du1 = lg.get(SG_DU + (b ? FD_U_RUDDER : FD_U_THROTTLE));
#pragma unroll
                for (int r = 0; r < NB; ++r) {
                    if constexpr (!F_LDS) asm volatile("" ::: "memory");   // one row of F in flight at a time, not all 120 words
                    G p = fword(phi + NB * r) * old[0];
#pragma unroll
                    for (int c = 1; c < NB; ++c) p = p + fword(phi + NB * r + c) * old[c];
                    const G g = fword(gam + 2 * r) * du0 + fword(gam + 2 * r + 1) * du1;
                    pred[r] = p + g;
                    e[r] = y[r] - pred[r];
                }
                if (b) e[NB - 1] = wrap_angle<G>(e[NB - 1]);     // the heading innovation
#pragma unroll
                for (int r = 0; r < NB; ++r) {
                    if constexpr (!F_LDS) asm volatile("" ::: "memory");
                    G c = fword(lgn + NB * r) * e[0];
#pragma unroll
                    for (int k = 1; k < NB; ++k) c = c + fword(lgn + NB * r + k) * e[k];
                    xh[r] = pred[r] + c;
                }
                if (b) xh[NB - 1] = wrap_angle<G>(xh[NB - 1]);
#pragma unroll
                for (int r = 0; r < NB; ++r) {
                    G de = xh[r] - d[r];
                    if (o + r == EST_PSI) de = wrap_angle<G>(de);
                    add_square(ea.err_est, o + r, double(de));
                    add_square(ea.err_meas, o + r, double(y[r] - d[r]));
                    if (ea.meas_out) ea.meas_out[int64_t(o + r) * nl + il] = double(y[r]);
                    lg.set(SG_XHAT + o + r, xh[r]);
                }
                // the law's input of this block; the other block's d is still formed from the true words, which are its own
                if (ea.feedback == FD_LQG_MEASUREMENT) put(b, y);
                else if (ea.feedback == FD_LQG_ESTIMATE) put(b, xh);
            }
        }
    };
    // LM, after estimate(): steps 1 (y_p), 4 and 5 of include/fdyn_servo_lqg_mission.h on the law's input in x, then the guidance's
    // state: `seen` (what servo_mission_kernel's guidance reads) for truth, else x_f with the filtered or the measured position
    auto position = [&](int s, bool adv, const G (&seen)[FD_NX]) {
        if constexpr (LM) {
#pragma clang fp contract(off)
            const bool truth = ea.feedback == FD_LQG_TRUTH;
            double yp[2] = { ld.get(SD_PHAT + 0), ld.get(SD_PHAT + 1) };
            if (adv) {
                G sphi, cphi, sth, cth, spsi, cpsi;
                M<G>::sincos(G(x[FD_X_ROLL]), sphi, cphi);
                M<G>::sincos(G(x[FD_X_PITCH]), sth, cth);
                M<G>::sincos(G(x[FD_X_YAW]), spsi, cpsi);
                const G u = G(x[FD_X_U]), v = G(x[FD_X_V]), w = G(x[FD_X_W]);
                const G vne[2] = { (cth * cpsi) * u + ((sphi * sth) * cpsi - cphi * spsi) * v + ((cphi * sth) * cpsi + sphi * spsi) * w,
                                   (cth * spsi) * u + ((sphi * sth) * spsi + cphi * cpsi) * v + ((cphi * sth) * spsi - sphi * cpsi) * w };
                const double sp = ea.pos[FD_SPF_SIGMA], gain = ea.pos[FD_SPF_GAIN];
                const double p[2] = { double(x[FD_X_N]), double(x[FD_X_E]) };    // never replaced by the law's input: the true position
                double e2[2] = { 0.0, 0.0 };
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const double z = ea.z ? ea.z[(int64_t(s) * NZ + FD_NSKX + k) * nl + il] : double(zpos[k]);
                    yp[k] = p[k] + sp * z;
                    const double pm = ld.get(SD_PHAT + k) + double(dt) * double(vne[k]);
                    const double ph = pm + gain * (yp[k] - pm);
                    ld.set(SD_PHAT + k, ph);
                    e2[0] = e2[0] + (ph - p[k]) * (ph - p[k]);
                    e2[1] = e2[1] + (yp[k] - p[k]) * (yp[k] - p[k]);
                }
                if (ea.err_pos) {
#pragma unroll
                    for (int k = 0; k < 2; ++k) ea.err_pos[int64_t(k) * nl + il] = ea.err_pos[int64_t(k) * nl + il] + e2[k];
                }
            }
#pragma unroll
            for (int k = 0; k < FD_NX; ++k) xg[k] = truth ? seen[k] : G(x[k]);
            if (!truth) {
                const bool est = ea.feedback == FD_LQG_ESTIMATE;
                xg[FD_X_N] = G(est ? ld.get(SD_PHAT + 0) : yp[0]);
                xg[FD_X_E] = G(est ? ld.get(SD_PHAT + 1) : yp[1]);
            }
        }
    };
    // the state the guidance reads: LM's own, else the caller's
    auto seen_by_guidance = [&](const G (&own)[FD_NX]) -> const G (&)[FD_NX] { if constexpr (LM) return xg; else return own; };
    // LM, a lane found complete: the true words back into x, as account() puts them back after the law
    auto restore = [&]() {
        if constexpr (LM) {
            if (ea.feedback != FD_LQG_TRUTH) {
#pragma unroll
                for (int j = 0; j < FD_NSKX; ++j) x[EST_W[j]] = S(ld.get(SD_KEEP + j));
            }
        }
    };
    // n_steps = 0: the law's input from the stored estimate
    auto estimate_stored = [&]() {
        if constexpr (LQG) {
            if (ea.feedback != FD_LQG_TRUTH) {
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    G xh[FD_SK_NB];
#pragma unroll
                    for (int r = 0; r < FD_SK_NB; ++r) xh[r] = lg.get(SG_XHAT + FD_SK_NB * b + r);
                    put(b, xh);
                }
            }
        }
    };
    // step 6, after the law: the true words back into x, the errors of the true state, chatter and du_prev
    auto account = [&](const Surfaces<G>& u) {
        if constexpr (LQG) {
#pragma clang fp contract(off)
            if constexpr (LM) { il = i; nl = n; }
            asm volatile("" : "+v"(il), "+s"(nl));
            if (ea.feedback != FD_LQG_TRUTH) {
#pragma unroll
                for (int j = 0; j < FD_NSKX; ++j) x[EST_W[j]] = S(ld.get(SD_KEEP + j));
            }
            // the errors of the true state, the law's own step 1, on the words the RK4 is about to read.  Formed HERE, and for every
            // feedback: with this placement the f64 physics rounds as it does in servo_step_kernel and feedback = truth is that
            // kernel bit for bit; formed before the law it had nine more fused multiply-adds and was not (supposed, not proven:
            // the uncontracted products u u, v v, w w are then common to this expression and the integrator's first stage)
            const S V = M<S>::sqrt((x[FD_X_U] * x[FD_X_U] + x[FD_X_V] * x[FD_X_V]) + x[FD_X_W] * x[FD_X_W]);
            err[FD_SVI_SPEED] = G(double(V) - ld.get(SD_REF + FD_SVR_SPEED));
            err[FD_SVI_ALTITUDE] = G(-double(x[FD_X_D]) - ld.get(SD_REF + FD_SVR_ALTITUDE));
            err[FD_SVI_HEADING] = wrap_angle<G>(G(double(x[FD_X_YAW]) - ld.get(SD_REF + FD_SVR_HEADING)));
            const G c[FD_NU] = { clipv<G>(u.elevator, G(-1), G(1)), clipv<G>(u.aileron, G(-1), G(1)), clipv<G>(u.rudder, G(-1), G(1)),
                                 clipv<G>(u.throttle, G(0), G(1)) };
            static_assert(FD_U_ELEVATOR == 0 && FD_U_AILERON == 1 && FD_U_RUDDER == 2 && FD_U_THROTTLE == 3, "control order");
#pragma unroll
            for (int k = 0; k < FD_NU; ++k) {
                const G u0k = lg.get(SG_U0 + k);
                add_square(ea.chatter, k, double(c[k] - (u0k + lg.get(SG_DU + k))));
                lg.set(SG_DU + k, c[k] - u0k);
            }
        }
    };

    // mission step 4 (include/fdyn_mission.h): the running extrema, on the state `xt` with its airspeed and altitude.  LM only, for
    // the true state after the law; `guide` keeps its own copy of these lines in place, for the state it saw: calling this from
    // there compiled the six mission kernels to other listings than the parent's
    auto mission_stats = [&](const G (&xt)[FD_NX], G airspeed, G altitude) {
        if constexpr (MISSION) {
#pragma clang fp contract(off)
            const G* wp = s_wps + idx * FD_NWP;
            auto raise = [&](int k, double v) { if (v > ld.get(SD_STAT + k)) ld.set(SD_STAT + k, v); };
            raise(FD_MST_ALTITUDE_ERROR, double(M<G>::abs(altitude - wp[FD_WP_ALTITUDE])));
            raise(FD_MST_ROLL, double(M<G>::abs(xt[FD_X_ROLL])));
            if (double(airspeed) < ld.get(SD_STAT + FD_MST_MIN_AIRSPEED)) ld.set(SD_STAT + FD_MST_MIN_AIRSPEED, double(airspeed));
            if (idx >= 1) {                                      // the leg wps[idx - 1] -> wps[idx], in the horizontal plane
                const G* from = wp - FD_NWP;
                const G ln = wp[FD_WP_NORTH] - from[FD_WP_NORTH], le = wp[FD_WP_EAST] - from[FD_WP_EAST];
                const G len = M<G>::sqrt(ln * ln + le * le);
                if (len >= G(1))
                    raise(FD_MST_CROSS_TRACK, double(fdiv(M<G>::abs(ln * (xt[FD_X_E] - from[FD_WP_EAST]) - le * (xt[FD_X_N] - from[FD_WP_NORTH])), len)));
            }
        }
    };
    // mission steps 1-4 (include/fdyn_mission.h) on the glue-type state `xg`: false when the mission is complete.  With `advance`
    // false (n_steps = 0) only the commands are formed.  Everything it computes is dead when it returns.
    auto guide = [&](const G (&xg)[FD_NX], auto&& derive, bool advance) -> bool {
        if constexpr (MISSION) {
            asm volatile("" ::: "memory");                       // the constants and the waypoints are re-read every step too
            if (idx < m.n_wp && waypoint_reached<G>(s_consts, s_wps + idx * FD_NWP, xg)) { idx += 1; reached += 1; }   // mission.update
            if (idx >= m.n_wp) { if (restart) idx = 0; else return false; }                                           // COMPLETE
            const G* wp = s_wps + idx * FD_NWP;
            Derived<G> d = derive();
            if constexpr (WINDY) d.airspeed = Vguide;            // d. course, ground speed, position and altitude stay ground quantities
            const GuidanceCmd<G> c = waypoint_guidance<G>(s_consts, wp, xg, d);
            ld.set(SD_REF + FD_SVR_SPEED, double(c.speed));
            ld.set(SD_REF + FD_SVR_ALTITUDE, double(c.altitude));
            ld.set(SD_REF + FD_SVR_HEADING, double(c.heading));
            ld.set(SD_REF + FD_SVR_CLIMB_RATE, 0.0);
            ld.set(SD_REF + FD_SVR_TURN_RATE, 0.0);
            if (advance) {
                bool seen = true;                                // LM: the statistics are the TRUE state's, formed after the law
                if constexpr (LM) seen = ea.feedback == FD_LQG_TRUTH;
                if (seen) {
#pragma clang fp contract(off)
                    auto raise = [&](int k, double v) { if (v > ld.get(SD_STAT + k)) ld.set(SD_STAT + k, v); };
                    raise(FD_MST_ALTITUDE_ERROR, double(M<G>::abs(d.altitude - wp[FD_WP_ALTITUDE])));
                    raise(FD_MST_ROLL, double(M<G>::abs(xg[FD_X_ROLL])));
                    if (double(d.airspeed) < ld.get(SD_STAT + FD_MST_MIN_AIRSPEED)) ld.set(SD_STAT + FD_MST_MIN_AIRSPEED, double(d.airspeed));
                    if (idx >= 1) {                              // the leg wps[idx - 1] -> wps[idx], in the horizontal plane
                        const G* from = wp - FD_NWP;
                        const G ln = wp[FD_WP_NORTH] - from[FD_WP_NORTH], le = wp[FD_WP_EAST] - from[FD_WP_EAST];
                        const G len = M<G>::sqrt(ln * ln + le * le);
                        if (len >= G(1))
                            raise(FD_MST_CROSS_TRACK, double(fdiv(M<G>::abs(ln * (xg[FD_X_E] - from[FD_WP_EAST]) - le * (xg[FD_X_N] - from[FD_WP_NORTH])), len)));
                    }
                }
                flown += 1;
            }
        }
        return true;
    };

    // With a mission the controls-only call (n_steps = 0) is the first half of one pass through the step loop: guidance and the law have
    // ONE call site per kernel, so the controls of an agent (n_steps = 0) equal those of a fleet lane (n_steps = 1) to the bit.
    bool only = false, advance = true;
    int iters = n_steps;
    if constexpr (MISSION) { advance = n_steps > 0; iters = advance ? n_steps : 1; }
    else only = n_steps == 0;
    // WINDY, f64: the sines and cosines of the stored angles, in the state type
    auto set_air_stored = [&]() {
        if constexpr (WINDY) {
            S sphi, cphi, sth, cth, spsi, cpsi;
            M<S>::sincos(x[FD_X_ROLL], sphi, cphi);
            M<S>::sincos(x[FD_X_PITCH], sth, cth);
            M<S>::sincos(x[FD_X_YAW], spsi, cpsi);
            set_air(sphi, cphi, sth, cth, spsi, cpsi);
        }
    };
    // WINDY, mixed and f32: the integrator's carried ones, as derived_fast reads them
    auto set_air_carried = [&](FastRK& f) {
        if constexpr (WINDY) {
            f.ensure_trig();
            set_air(f.t0.phi.x, f.t0.phi.y, f.t0.th.x, f.t0.th.y, f.t0.psi.x, f.t0.psi.y);
            if constexpr (MISSION) {                             // the guidance's airspeed: derived_fast's expression on the fp32 copy
                const float u = f.x0[3] + nbw[0], v = f.x0[4] + nbw[1], w = f.x0[5] + nbw[2];
                Vguide = fast::sqrt(__builtin_fmaf(u, u, __builtin_fmaf(v, v, w * w)));
            }
        }
    };
    if (only) {
        if constexpr (WINDY) {
            set_air_mass();
            if constexpr (FAST) { FastRK f; f.init(x); set_air_carried(f); }
            else set_air_stored();
        }
        if constexpr (LQG) estimate_stored();
        reschedule();
        surf = control(false);
    } else if constexpr (FAST) {
        FastRK f;
        f.init(x);
        const float hdt = float(S(0.5) * dt), fdt = float(dt), dt6 = float(dt / S(6));
        for (int s = 0; s < iters; ++s) {
            set_air_mass();
            set_air_carried(f);
            if constexpr (LM) {
                if (advance) estimate(s); else estimate_stored();
                position(s, advance, f.x0);
            }
            if (!guide(seen_by_guidance(f.x0), [&]() {
                    if constexpr (LM) { if (ea.feedback != FD_LQG_TRUTH) return derived<G>(xg); }
                    return derived_fast(f);
                }, advance)) {
                if (!advance) return;                            // controls only: a complete lane writes nothing at all
                break;
            }
            if constexpr (LQG && !LM) estimate(s);
            reschedule();
            surf = control(advance);
            if constexpr (LM) {
                if (advance) {
                    account(surf);
                    if (ea.feedback != FD_LQG_TRUTH)             // x is the true state again, f.x0 never was anything else
                        mission_stats(f.x0, fast::sqrt(__builtin_fmaf(f.x0[3], f.x0[3], __builtin_fmaf(f.x0[4], f.x0[4], f.x0[5] * f.x0[5]))), -f.x0[2]);
                }
            } else if constexpr (LQG) account(surf);
            if constexpr (MISSION) { if (!advance) break; }
            Controls<T> C;
            C.set(P, surf.elevator, surf.aileron, surf.rudder, surf.throttle);
            if constexpr (WINDY) { rk4_fast_step<S, false, true>(P, Lm, C, x, f, hdt, fdt, dt6, air_mass()); gust(s); }
            else rk4_fast_step<S, false>(P, Lm, C, x, f, hdt, fdt, dt6);
            if constexpr (!MISSION) move_refs();
        }
    } else {
        for (int s = 0; s < iters; ++s) {
            set_air_mass();
            set_air_stored();
            if constexpr (LM) {
                if (advance) estimate(s); else estimate_stored();
                position(s, advance, x);
            }
            if (!guide(seen_by_guidance(x), [&]() { return derived<S>(seen_by_guidance(x)); }, advance)) {
                if (!advance) return;
                break;
            }
            if constexpr (LQG && !LM) estimate(s);
            reschedule();
            surf = control(advance);
            if constexpr (LM) {
                if (advance) {
                    account(surf);
                    if (ea.feedback != FD_LQG_TRUTH)
                        mission_stats(x, M<S>::sqrt(x[3] * x[3] + x[4] * x[4] + x[5] * x[5]), -x[2]);
                }
            } else if constexpr (LQG) account(surf);
            if constexpr (MISSION) { if (!advance) break; }
            Controls<T> C;
            C.set(P, surf.elevator, surf.aileron, surf.rudder, surf.throttle);
            if constexpr (WINDY) { rk4_substeps<S, T, true, true>(P, Lm, C, x, dt, 1, air_mass()); gust(s); }
            else rk4_substeps<S, T>(P, Lm, C, x, dt, 1);
            if constexpr (!MISSION) move_refs();
        }
    }
    if constexpr (LM) { if (idx >= m.n_wp) restore(); }           // left the loop complete, after the law's input went into x
    // the addresses of the stores below are recomputed from a lane index the compiler cannot equate with `i`, so that none of
    // them lives across the step loop
    int64_t ie = i;
    asm volatile("" : "+v"(ie));
    if constexpr (MISSION) {
        if (n_steps > 0) {
            m.wp_idx[ie] = idx;
            if (m.reached_total) m.reached_total[ie] += reached;
            if constexpr (LM) {                                  // the measurement and the filters of a completing step stand
#pragma unroll
                for (int j = 0; j < FD_NSKX; ++j) ea.xhat[int64_t(j) * n + ie] = double(lg.get(SG_XHAT + j));
#pragma unroll
                for (int k = 0; k < 2; ++k) ea.phat[int64_t(k) * n + ie] = ld.get(SD_PHAT + k);
            }
            if (flown == 0) return;                              // complete before its first step here: nothing else of the lane changes
            if (m.steps_flown) m.steps_flown[ie] += flown;
            ref[int64_t(FD_SVR_SPEED) * n + ie] = ld.get(SD_REF + FD_SVR_SPEED);
            ref[int64_t(FD_SVR_CLIMB_RATE) * n + ie] = 0.0;
            ref[int64_t(FD_SVR_TURN_RATE) * n + ie] = 0.0;
            if (m.stats) {
#pragma unroll
                for (int k = 0; k < FD_NMST; ++k) m.stats[int64_t(k) * n + ie] = ld.get(SD_STAT + k);
            }
        }
    }
    if (n_steps > 0) {
#pragma unroll
        for (int k = 0; k < FD_NX; ++k) xs[k * n + ie] = x[k];
        if (sat_steps) sat_steps[ie] += sat;
        ref[int64_t(FD_SVR_ALTITUDE) * n + ie] = ld.get(SD_REF + FD_SVR_ALTITUDE);
        ref[int64_t(FD_SVR_HEADING) * n + ie] = ld.get(SD_REF + FD_SVR_HEADING);
#pragma unroll
        for (int k = 0; k < FD_NSVI; ++k) integ[int64_t(k) * n + ie] = double(lg.get(SG_INT + k));
        if (err_out) {
#pragma unroll
            for (int k = 0; k < FD_NSVI; ++k) err_out[int64_t(k) * n + ie] = double(err[k]);
        }
        if constexpr (WINDY) {
#pragma unroll
            for (int k = 0; k < 3; ++k) wa.rows[int64_t(FD_SW_GUST_N + k) * n + ie] = ld.get(SD_GUST + k);
        }
        if constexpr (LQG) {
            if constexpr (!LM) {
#pragma unroll
                for (int j = 0; j < FD_NSKX; ++j) ea.xhat[int64_t(j) * n + ie] = double(lg.get(SG_XHAT + j));
            }
#pragma unroll
            for (int k = 0; k < FD_NU; ++k) ea.du_prev[int64_t(k) * n + ie] = double(lg.get(SG_DU + k));
        }
    }
    if constexpr (SL) {
        if (n_steps > 0) { sa.state[ie] = ld.get(SD_SIG); sa.state[n + ie] = ld.get(SD_POS); }
    } else if constexpr (SCHED) {
        if (sa.sigma_out) { sa.sigma_out[ie] = ld.get(SD_SIG); sa.sigma_out[n + ie] = ld.get(SD_POS); }
    }
    if (surf_out) {                                              // the controls as applied: after set_controls' clip
        surf_out[FD_U_ELEVATOR * n + ie] = S(clipv<G>(surf.elevator, G(-1), G(1)));
        surf_out[FD_U_AILERON * n + ie] = S(clipv<G>(surf.aileron, G(-1), G(1)));
        surf_out[FD_U_RUDDER * n + ie] = S(clipv<G>(surf.rudder, G(-1), G(1)));
        surf_out[FD_U_THROTTLE * n + ie] = S(clipv<G>(surf.throttle, G(0), G(1)));
    }
}

template <typename S, typename T>
__global__ void __launch_bounds__(LB, 1)
servo_step_kernel(S* __restrict__ xs, const double* __restrict__ x0, const double* __restrict__ u0, const double* __restrict__ K,
                  double* __restrict__ ref, double* __restrict__ integ, const double* __restrict__ limits, const uint8_t* __restrict__ type,
                  const double* __restrict__ params, int n_types, int64_t n, S dt, int n_steps, S* __restrict__ surf_out,
                  int32_t* __restrict__ sat_steps, double* __restrict__ err_out)
{
    servo_step_body<S, T, false>(xs, x0, u0, K, ref, integ, limits, type, params, n_types, n, dt, n_steps, surf_out, sat_steps, err_out, NoMission{});
}

template <typename S, typename T>
__global__ void __launch_bounds__(LB, 1)
servo_mission_kernel(S* __restrict__ xs, const double* __restrict__ x0, const double* __restrict__ u0, const double* __restrict__ K,
                     double* __restrict__ ref, double* __restrict__ integ, const double* __restrict__ limits, const uint8_t* __restrict__ type,
                     const double* __restrict__ params, int n_types, int64_t n, S dt, int n_steps, S* __restrict__ surf_out,
                     int32_t* __restrict__ sat_steps, double* __restrict__ err_out, Mission m)
{
    servo_step_body<S, T, true>(xs, x0, u0, K, ref, integ, limits, type, params, n_types, n, dt, n_steps, surf_out, sat_steps, err_out, m);
}

template <typename S, typename T>
__global__ void __launch_bounds__(LB, 1)
servo_step_wind_kernel(S* __restrict__ xs, const double* __restrict__ x0, const double* __restrict__ u0, const double* __restrict__ K,
                       double* __restrict__ ref, double* __restrict__ integ, const double* __restrict__ limits, const uint8_t* __restrict__ type,
                       const double* __restrict__ params, int n_types, int64_t n, S dt, int n_steps, S* __restrict__ surf_out,
                       int32_t* __restrict__ sat_steps, double* __restrict__ err_out, AirMass w)
{
    servo_step_body<S, T, false>(xs, x0, u0, K, ref, integ, limits, type, params, n_types, n, dt, n_steps, surf_out, sat_steps, err_out, NoMission{}, w);
}

template <typename S, typename T>
__global__ void __launch_bounds__(LB, 1)
servo_mission_wind_kernel(S* __restrict__ xs, const double* __restrict__ x0, const double* __restrict__ u0, const double* __restrict__ K,
                          double* __restrict__ ref, double* __restrict__ integ, const double* __restrict__ limits, const uint8_t* __restrict__ type,
                          const double* __restrict__ params, int n_types, int64_t n, S dt, int n_steps, S* __restrict__ surf_out,
                          int32_t* __restrict__ sat_steps, double* __restrict__ err_out, Mission m, AirMass w)
{
    servo_step_body<S, T, true>(xs, x0, u0, K, ref, integ, limits, type, params, n_types, n, dt, n_steps, surf_out, sat_steps, err_out, m, w);
}

template <typename S, typename T, typename EA = Estimator>
__global__ void __launch_bounds__(LB, 1)
servo_lqg_step_kernel(S* __restrict__ xs, const double* __restrict__ x0, const double* __restrict__ u0, const double* __restrict__ K,
                      double* __restrict__ ref, double* __restrict__ integ, const double* __restrict__ limits, const uint8_t* __restrict__ type,
                      const double* __restrict__ params, int n_types, int64_t n, S dt, int n_steps, S* __restrict__ surf_out,
                      int32_t* __restrict__ sat_steps, double* __restrict__ err_out, EA e)
{
    servo_step_body<S, T, false>(xs, x0, u0, K, ref, integ, limits, type, params, n_types, n, dt, n_steps, surf_out, sat_steps, err_out, NoMission{},
                                 NoWind{}, e);
}

template <typename S, typename T>
__global__ void __launch_bounds__(LB, 1)
servo_lqg_mission_kernel(S* __restrict__ xs, const double* __restrict__ x0, const double* __restrict__ u0, const double* __restrict__ K,
                         double* __restrict__ ref, double* __restrict__ integ, const double* __restrict__ limits, const uint8_t* __restrict__ type,
                         const double* __restrict__ params, int n_types, int64_t n, S dt, int n_steps, S* __restrict__ surf_out,
                         int32_t* __restrict__ sat_steps, double* __restrict__ err_out, Mission m, EstimatorPos e)
{
    servo_step_body<S, T, true>(xs, x0, u0, K, ref, integ, limits, type, params, n_types, n, dt, n_steps, surf_out, sat_steps, err_out, m, NoWind{}, e);
}

template <typename S, typename T>
__global__ void __launch_bounds__(LB, 1)
servo_sched_step_kernel(S* __restrict__ xs, double* __restrict__ ref, double* __restrict__ integ, const double* __restrict__ limits,
                        const uint8_t* __restrict__ type, const double* __restrict__ params, int n_types, int64_t n, S dt, int n_steps,
                        S* __restrict__ surf_out, int32_t* __restrict__ sat_steps, double* __restrict__ err_out, Schedule sc)
{
    servo_step_body<S, T, false>(xs, nullptr, nullptr, nullptr, ref, integ, limits, type, params, n_types, n, dt, n_steps, surf_out, sat_steps,
                                 err_out, NoMission{}, NoWind{}, NoEstimator{}, sc);
}

template <typename S, typename T>
__global__ void __launch_bounds__(LB, 1)
servo_sched_mission_kernel(S* __restrict__ xs, double* __restrict__ ref, double* __restrict__ integ, const double* __restrict__ limits,
                           const uint8_t* __restrict__ type, const double* __restrict__ params, int n_types, int64_t n, S dt, int n_steps,
                           S* __restrict__ surf_out, int32_t* __restrict__ sat_steps, double* __restrict__ err_out, Mission m, Schedule sc)
{
    servo_step_body<S, T, true>(xs, nullptr, nullptr, nullptr, ref, integ, limits, type, params, n_types, n, dt, n_steps, surf_out, sat_steps,
                                err_out, m, NoWind{}, NoEstimator{}, sc);
}

template <typename S, typename T>
__global__ void __launch_bounds__(LB, 1)
servo_sched_lqg_step_kernel(S* __restrict__ xs, double* __restrict__ ref, double* __restrict__ integ, const double* __restrict__ limits,
                            const uint8_t* __restrict__ type, const double* __restrict__ params, int n_types, int64_t n, S dt, int n_steps,
                            S* __restrict__ surf_out, int32_t* __restrict__ sat_steps, double* __restrict__ err_out, Estimator e, ScheduleLqg sc)
{
    servo_step_body<S, T, false>(xs, nullptr, nullptr, nullptr, ref, integ, limits, type, params, n_types, n, dt, n_steps, surf_out, sat_steps,
                                 err_out, NoMission{}, NoWind{}, e, sc);
}

// refusals in launch_sched's order, then launch_lqg_step's
template <typename S, typename T>
int launch_sched_lqg(S* x, const ScheduleLqg& sc, double* ref, double* integ, const double* limits, const uint8_t* type, const double* params,
                     int n_types, int64_t n, double dt, int n_steps, S* surf_out, int32_t* sat_steps, double* err_out, const Estimator& e,
                     void* stream)
{
    if (n_steps < 0) return FDYN_ERR_BAD_SIZE;
    if (sc.n_nodes < 1 || sc.n_nodes > FD_MAX_SCHED_NODES) return FDYN_ERR_BAD_SIZE;
    if (sc.on != FD_SCHED_ON_AIRSPEED && sc.on != FD_SCHED_ON_COMMAND) return FDYN_ERR_BAD_SIZE;
    FD_CHECK_FLEET(n, n_types, LB)
    if (!x || !sc.table || !sc.table_f || !sc.origin || !ref || !integ || !limits || !params) return FDYN_ERR_NULL;
    if (!e.sigma || !e.xhat || !e.du_prev || !sc.state) return FDYN_ERR_NULL;
    if (e.feedback != FD_LQG_ESTIMATE && e.feedback != FD_LQG_MEASUREMENT && e.feedback != FD_LQG_TRUTH) return FDYN_ERR_BAD_SIZE;
    if (bad_dt(dt)) return FDYN_ERR_BAD_DT;
    return launch<LB>(servo_sched_lqg_step_kernel<S, T>, n, stream, x, ref, integ, limits, type, params, n_types, n, S(dt), n_steps, surf_out,
                      sat_steps, err_out, e, sc);
}

// `m`: NULL for fdyn_servo_sched_step_*.  Refusals in launch_step's / launch_mission's order, the schedule's own with the sizes
template <typename S, typename T>
int launch_sched(S* x, const Schedule& sc, double* ref, double* integ, const double* limits, const Mission* m, const uint8_t* type,
                 const double* params, int n_types, int64_t n, double dt, int n_steps, S* surf_out, int32_t* sat_steps, double* err_out,
                 void* stream)
{
    if (n_steps < 0 || (m && (m->n_wp < 1 || m->n_wp > FD_MAX_WAYPOINTS))) return FDYN_ERR_BAD_SIZE;
    if (sc.n_nodes < 1 || sc.n_nodes > FD_MAX_SCHED_NODES) return FDYN_ERR_BAD_SIZE;
    if (sc.on != FD_SCHED_ON_AIRSPEED && sc.on != FD_SCHED_ON_COMMAND) return FDYN_ERR_BAD_SIZE;
    FD_CHECK_FLEET(n, n_types, LB)
    if (!x || !sc.table || !ref || !integ || !limits || !params) return FDYN_ERR_NULL;
    if (m && (!m->wp_idx || !m->consts || !m->wps)) return FDYN_ERR_NULL;
    if (bad_dt(dt)) return FDYN_ERR_BAD_DT;
    if (!m) return launch<LB>(servo_sched_step_kernel<S, T>, n, stream, x, ref, integ, limits, type, params, n_types, n, S(dt), n_steps,
                              surf_out, sat_steps, err_out, sc);
    return launch<LB>(servo_sched_mission_kernel<S, T>, n, stream, x, ref, integ, limits, type, params, n_types, n, S(dt), n_steps,
                      surf_out, sat_steps, err_out, *m, sc);
}

// refusals in launch_mission's order, then launch_lqg_step's; the two words of pos are the host layer's to check
template <typename S, typename T>
int launch_lqg_mission(S* x, const double* x0, const double* u0, const double* K, double* ref, double* integ, const double* limits,
                       const Mission& m, const uint8_t* type, const double* params, int n_types, int64_t n, double dt, int n_steps,
                       S* surf_out, int32_t* sat_steps, double* err_out, const EstimatorPos& e, void* stream)
{
    if (n_steps < 0 || m.n_wp < 1 || m.n_wp > FD_MAX_WAYPOINTS) return FDYN_ERR_BAD_SIZE;
    FD_CHECK_FLEET(n, n_types, LB)
    if (!x || !x0 || !u0 || !K || !ref || !integ || !limits || !params || !m.wp_idx || !m.consts || !m.wps) return FDYN_ERR_NULL;
    if (!e.F || !e.sigma || !e.xhat || !e.du_prev || !e.pos || !e.phat) return FDYN_ERR_NULL;
    if (e.feedback != FD_LQG_ESTIMATE && e.feedback != FD_LQG_MEASUREMENT && e.feedback != FD_LQG_TRUTH) return FDYN_ERR_BAD_SIZE;
    if (bad_dt(dt)) return FDYN_ERR_BAD_DT;
    return launch<LB>(servo_lqg_mission_kernel<S, T>, n, stream, x, x0, u0, K, ref, integ, limits, type, params, n_types, n, S(dt), n_steps,
                      surf_out, sat_steps, err_out, m, e);
}

// dyn_lds: the f64 step with the filter in dynamic LDS (fdyn_servo_lqg_step_f64_lds)
template <typename S, typename T, bool DYN = false>
int launch_lqg_step(S* x, const double* x0, const double* u0, const double* K, double* ref, double* integ, const double* limits,
                    const uint8_t* type, const double* params, int n_types, int64_t n, double dt, int n_steps, S* surf_out,
                    int32_t* sat_steps, double* err_out, const Estimator& e, void* stream)
{
    if (n_steps < 0) return FDYN_ERR_BAD_SIZE;
    FD_CHECK_FLEET(n, n_types, LB)
    if (!x || !x0 || !u0 || !K || !ref || !integ || !limits || !params || !e.F || !e.sigma || !e.xhat || !e.du_prev) return FDYN_ERR_NULL;
    if (e.feedback != FD_LQG_ESTIMATE && e.feedback != FD_LQG_MEASUREMENT && e.feedback != FD_LQG_TRUTH) return FDYN_ERR_BAD_SIZE;
    if (bad_dt(dt)) return FDYN_ERR_BAD_DT;
    if constexpr (DYN) {
        EstimatorDynLds ed;
        static_cast<Estimator&>(ed) = e;
        auto kernel = servo_lqg_step_kernel<S, T, EstimatorDynLds>;
        // static + dynamic LDS pass 64 KB: the kernel is told once that it may ask for them
        static const hipError_t allowed = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, DYN_F_BYTES);
        (void)allowed;
        hipLaunchKernelGGL(kernel, dim3(unsigned((n + LB - 1) / LB)), dim3(LB), DYN_F_BYTES, (hipStream_t)stream, x, x0, u0, K, ref, integ, limits,
                           type, params, n_types, n, S(dt), n_steps, surf_out, sat_steps, err_out, ed);
        return int(hipGetLastError());
    } else {
        return launch<LB>(servo_lqg_step_kernel<S, T>, n, stream, x, x0, u0, K, ref, integ, limits, type, params, n_types, n, S(dt), n_steps,
                          surf_out, sat_steps, err_out, e);
    }
}

// `w`: NULL for the still-air entries, the air mass for the _wind ones (its rows are required)
template <typename S, typename T>
int launch_mission(S* x, const double* x0, const double* u0, const double* K, double* ref, double* integ, const double* limits,
                   const Mission& m, const uint8_t* type, const double* params, int n_types, int64_t n, double dt, int n_steps,
                   S* surf_out, int32_t* sat_steps, double* err_out, void* stream, const AirMass* w = nullptr)
{
    if (n_steps < 0 || m.n_wp < 1 || m.n_wp > FD_MAX_WAYPOINTS) return FDYN_ERR_BAD_SIZE;
    FD_CHECK_FLEET(n, n_types, LB)
    if (!x || !x0 || !u0 || !K || !ref || !integ || !limits || !params || !m.wp_idx || !m.consts || !m.wps) return FDYN_ERR_NULL;
    if (w && !w->rows) return FDYN_ERR_NULL;
    if (bad_dt(dt)) return FDYN_ERR_BAD_DT;
    if (!w) return launch<LB>(servo_mission_kernel<S, T>, n, stream, x, x0, u0, K, ref, integ, limits, type, params, n_types, n, S(dt), n_steps,
                              surf_out, sat_steps, err_out, m);
    return launch<LB>(servo_mission_wind_kernel<S, T>, n, stream, x, x0, u0, K, ref, integ, limits, type, params, n_types, n, S(dt), n_steps,
                      surf_out, sat_steps, err_out, m, *w);
}

template <typename S, typename T>
int launch_step(S* x, const double* x0, const double* u0, const double* K, double* ref, double* integ, const double* limits,
                const uint8_t* type, const double* params, int n_types, int64_t n, double dt, int n_steps, S* surf_out,
                int32_t* sat_steps, double* err_out, void* stream, const AirMass* w = nullptr)
{
    static_assert(LB >= FD_MAX_TYPES * Params<double>::FD_ND_LANES, "stage_params needs that many threads");
    if (n_steps < 0) return FDYN_ERR_BAD_SIZE;
    FD_CHECK_FLEET(n, n_types, LB)
    if (!x || !x0 || !u0 || !K || !ref || !integ || !limits || !params) return FDYN_ERR_NULL;
    if (w && !w->rows) return FDYN_ERR_NULL;
    if (bad_dt(dt)) return FDYN_ERR_BAD_DT;
    if (!w) return launch<LB>(servo_step_kernel<S, T>, n, stream, x, x0, u0, K, ref, integ, limits, type, params, n_types, n, S(dt), n_steps,
                              surf_out, sat_steps, err_out);
    return launch<LB>(servo_step_wind_kernel<S, T>, n, stream, x, x0, u0, K, ref, integ, limits, type, params, n_types, n, S(dt), n_steps,
                      surf_out, sat_steps, err_out, *w);
}

}  // namespace

extern "C" {

int fdyn_servo_design(const double* A, const double* B, const double* x0, const double* weights, int weights_per_lane, int64_t n,
                      double* K, double* residual, int32_t* iters, int32_t* status, void* stream)
{
    FD_CHECK_FLEET(n, 1, TB)
    if (!A || !B || !x0 || !weights || !K || !residual || !iters || !status) return FDYN_ERR_NULL;
    return launch<TB>(servo_design_kernel, n, stream, A, B, x0, weights, weights_per_lane, n, K, residual, iters, status);
}

int fdyn_servo_step_f64(double* x, const double* x0, const double* u0, const double* K, double* ref, double* integ, const double* limits,
                        const uint8_t* type, const double* params, int n_types, int64_t n, double dt, int n_steps, double* surf_out,
                        int32_t* sat_steps, double* err_out, void* stream)
{ return launch_step<double, double>(x, x0, u0, K, ref, integ, limits, type, params, n_types, n, dt, n_steps, surf_out, sat_steps, err_out, stream); }

int fdyn_servo_step_mixed(double* x, const double* x0, const double* u0, const double* K, double* ref, double* integ, const double* limits,
                          const uint8_t* type, const double* params, int n_types, int64_t n, double dt, int n_steps, double* surf_out,
                          int32_t* sat_steps, double* err_out, void* stream)
{ return launch_step<double, float>(x, x0, u0, K, ref, integ, limits, type, params, n_types, n, dt, n_steps, surf_out, sat_steps, err_out, stream); }

int fdyn_servo_step_f32(float* x, const double* x0, const double* u0, const double* K, double* ref, double* integ, const double* limits,
                        const uint8_t* type, const double* params, int n_types, int64_t n, double dt, int n_steps, float* surf_out,
                        int32_t* sat_steps, double* err_out, void* stream)
{ return launch_step<float, float>(x, x0, u0, K, ref, integ, limits, type, params, n_types, n, dt, n_steps, surf_out, sat_steps, err_out, stream); }

#define FD_SERVO_MISSION(NAME, S, T)                                                                                                   \
    int fdyn_servo_mission_##NAME(S* x, const double* x0, const double* u0, const double* K, double* ref, double* integ,              \
                                  const double* limits, int32_t* wp_idx, const double* consts, const double* wps, int n_wp,           \
                                  const uint8_t* type, const double* params, int n_types, int64_t n, double dt, int n_steps,          \
                                  S* surf_out, int32_t* sat_steps, double* err_out, int32_t* reached_total, int32_t* steps_flown,     \
                                  double* stats, void* stream)                                                                        \
    {                                                                                                                                  \
        return launch_mission<S, T>(x, x0, u0, K, ref, integ, limits, Mission{ wp_idx, consts, wps, n_wp, reached_total, steps_flown, stats }, \
                                    type, params, n_types, n, dt, n_steps, surf_out, sat_steps, err_out, stream);                     \
    }
FD_SERVO_MISSION(f64, double, double)
FD_SERVO_MISSION(mixed, double, float)
FD_SERVO_MISSION(f32, float, float)
#undef FD_SERVO_MISSION

#define FD_SERVO_WIND(NAME, S, T)                                                                                                      \
    int fdyn_servo_step_wind_##NAME(S* x, const double* x0, const double* u0, const double* K, double* ref, double* integ,            \
                                    const double* limits, const uint8_t* type, const double* params, int n_types, int64_t n, double dt, \
                                    int n_steps, S* surf_out, int32_t* sat_steps, double* err_out, double* wind, uint64_t seed,        \
                                    const int32_t* step, const double* z, void* stream)                                                \
    {                                                                                                                                  \
        const AirMass w{ wind, seed, step, z };                                                                                        \
        return launch_step<S, T>(x, x0, u0, K, ref, integ, limits, type, params, n_types, n, dt, n_steps, surf_out, sat_steps, err_out, \
                                 stream, &w);                                                                                          \
    }                                                                                                                                  \
    int fdyn_servo_mission_wind_##NAME(S* x, const double* x0, const double* u0, const double* K, double* ref, double* integ,         \
                                       const double* limits, int32_t* wp_idx, const double* consts, const double* wps, int n_wp,      \
                                       const uint8_t* type, const double* params, int n_types, int64_t n, double dt, int n_steps,     \
                                       S* surf_out, int32_t* sat_steps, double* err_out, int32_t* reached_total, int32_t* steps_flown, \
                                       double* stats, double* wind, uint64_t seed, const int32_t* step, const double* z, void* stream) \
    {                                                                                                                                  \
        const AirMass w{ wind, seed, step, z };                                                                                        \
        return launch_mission<S, T>(x, x0, u0, K, ref, integ, limits, Mission{ wp_idx, consts, wps, n_wp, reached_total, steps_flown, stats }, \
                                    type, params, n_types, n, dt, n_steps, surf_out, sat_steps, err_out, stream, &w);                  \
    }
FD_SERVO_WIND(f64, double, double)
FD_SERVO_WIND(mixed, double, float)
FD_SERVO_WIND(f32, float, float)
#undef FD_SERVO_WIND

int fdyn_servo_kf_design(const double* A, const double* B, double dt, const double* noise, int noise_per_lane, int64_t n, double* F,
                         double* residual, int32_t* iters, int32_t* status, void* stream)
{
    FD_CHECK_FLEET(n, 1, TB)
    if (!A || !B || !noise || !F || !residual || !iters || !status) return FDYN_ERR_NULL;
    return launch<TB>(servo_kf_design_kernel, n, stream, A, B, dt, noise, noise_per_lane, n, F, residual, iters, status);
}

#define FD_SERVO_LQG(NAME, S, T, DYN)                                                                                                     \
    int fdyn_servo_lqg_step_##NAME(S* x, const double* x0, const double* u0, const double* K, double* ref, double* integ,             \
                                   const double* limits, const uint8_t* type, const double* params, int n_types, int64_t n, double dt, \
                                   int n_steps, S* surf_out, int32_t* sat_steps, double* err_out, const double* F, const double* sigma, \
                                   double* xhat, double* du_prev, uint64_t seed, const int32_t* step, const double* z, int feedback,   \
                                   double* err_est, double* err_meas, double* chatter, double* meas_out, void* stream)                 \
    {                                                                                                                                  \
        const Estimator e{ F, sigma, xhat, du_prev, seed, step, z, feedback, err_est, err_meas, chatter, meas_out };                   \
        return launch_lqg_step<S, T, DYN>(x, x0, u0, K, ref, integ, limits, type, params, n_types, n, dt, n_steps, surf_out, sat_steps,     \
                                     err_out, e, stream);                                                                              \
    }
FD_SERVO_LQG(f64, double, double, false)
FD_SERVO_LQG(mixed, double, float, false)
FD_SERVO_LQG(f32, float, float, false)
FD_SERVO_LQG(f64_lds, double, double, true)
#undef FD_SERVO_LQG

#define FD_SERVO_LQG_MISSION(NAME, S, T)                                                                                              \
    int fdyn_servo_lqg_mission_##NAME(S* x, const double* x0, const double* u0, const double* K, double* ref, double* integ,          \
                                      const double* limits, int32_t* wp_idx, const double* consts, const double* wps, int n_wp,       \
                                      const uint8_t* type, const double* params, int n_types, int64_t n, double dt, int n_steps,      \
                                      S* surf_out, int32_t* sat_steps, double* err_out, int32_t* reached_total, int32_t* steps_flown, \
                                      double* stats, const double* F, const double* sigma, double* xhat, double* du_prev,            \
                                      uint64_t seed, const int32_t* step, const double* z, int feedback, double* err_est,            \
                                      double* err_meas, double* chatter, double* meas_out, const double* pos, double* phat,          \
                                      double* err_pos, void* stream)                                                                  \
    {                                                                                                                                  \
        EstimatorPos e;                                                                                                                \
        static_cast<Estimator&>(e) = Estimator{ F, sigma, xhat, du_prev, seed, step, z, feedback, err_est, err_meas, chatter, meas_out }; \
        e.pos = pos; e.phat = phat; e.err_pos = err_pos;                                                                               \
        return launch_lqg_mission<S, T>(x, x0, u0, K, ref, integ, limits, Mission{ wp_idx, consts, wps, n_wp, reached_total, steps_flown, stats }, \
                                        type, params, n_types, n, dt, n_steps, surf_out, sat_steps, err_out, e, stream);               \
    }
FD_SERVO_LQG_MISSION(f64, double, double)
FD_SERVO_LQG_MISSION(mixed, double, float)
FD_SERVO_LQG_MISSION(f32, float, float)
#undef FD_SERVO_LQG_MISSION

#define FD_SERVO_SCHED(NAME, S, T)                                                                                                     \
    int fdyn_servo_sched_step_##NAME(S* x, const double* sched, int n_nodes, int sched_on, double* ref, double* integ,                \
                                     const double* limits, const uint8_t* type, const double* params, int n_types, int64_t n,         \
                                     double dt, int n_steps, S* surf_out, int32_t* sat_steps, double* err_out, double* sigma_out,     \
                                     void* stream)                                                                                     \
    {                                                                                                                                  \
        return launch_sched<S, T>(x, Schedule{ sched, n_nodes, sched_on, sigma_out }, ref, integ, limits, nullptr, type, params, n_types, n, \
                                  dt, n_steps, surf_out, sat_steps, err_out, stream);                                                 \
    }                                                                                                                                  \
    int fdyn_servo_sched_mission_##NAME(S* x, const double* sched, int n_nodes, int sched_on, double* ref, double* integ,             \
                                        const double* limits, int32_t* wp_idx, const double* consts, const double* wps, int n_wp,     \
                                        const uint8_t* type, const double* params, int n_types, int64_t n, double dt, int n_steps,    \
                                        S* surf_out, int32_t* sat_steps, double* err_out, int32_t* reached_total,                      \
                                        int32_t* steps_flown, double* stats, double* sigma_out, void* stream)                          \
    {                                                                                                                                  \
        const Mission m{ wp_idx, consts, wps, n_wp, reached_total, steps_flown, stats };                                               \
        return launch_sched<S, T>(x, Schedule{ sched, n_nodes, sched_on, sigma_out }, ref, integ, limits, &m, type, params, n_types, n, \
                                  dt, n_steps, surf_out, sat_steps, err_out, stream);                                                 \
    }
FD_SERVO_SCHED(f64, double, double)
FD_SERVO_SCHED(mixed, double, float)
FD_SERVO_SCHED(f32, float, float)
#undef FD_SERVO_SCHED

#define FD_SERVO_SCHED_LQG(NAME, S, T)                                                                                                 \
    int fdyn_servo_sched_lqg_step_##NAME(S* x, const double* sched, const double* sched_f, int n_nodes, int sched_on, const double* origin, \
                                         double* ref, double* integ, const double* limits, const uint8_t* type, const double* params, \
                                         int n_types, int64_t n, double dt, int n_steps, S* surf_out, int32_t* sat_steps,             \
                                         double* err_out, const double* sigma, double* xhat, double* du_prev, double* sched_state,    \
                                         uint64_t seed, const int32_t* step, const double* z, int feedback, double* err_est,          \
                                         double* err_meas, double* chatter, double* meas_out, void* stream)                           \
    {                                                                                                                                  \
        ScheduleLqg sc;                                                                                                                \
        static_cast<Schedule&>(sc) = Schedule{ sched, n_nodes, sched_on, nullptr };                                                    \
        sc.table_f = sched_f; sc.origin = origin; sc.state = sched_state;                                                              \
        const Estimator e{ nullptr, sigma, xhat, du_prev, seed, step, z, feedback, err_est, err_meas, chatter, meas_out };             \
        return launch_sched_lqg<S, T>(x, sc, ref, integ, limits, type, params, n_types, n, dt, n_steps, surf_out, sat_steps, err_out,  \
                                      e, stream);                                                                                      \
    }
FD_SERVO_SCHED_LQG(f64, double, double)
FD_SERVO_SCHED_LQG(mixed, double, float)
FD_SERVO_SCHED_LQG(f32, float, float)
#undef FD_SERVO_SCHED_LQG

}  // extern "C"

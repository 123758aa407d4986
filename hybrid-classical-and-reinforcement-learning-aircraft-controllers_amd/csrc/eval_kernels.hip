// eval_kernels.hip -- evaluation on the device (gfx950): per-episode rate-control metrics, rewards on recorded sequences and
// the streamed comparison of two fleets' trajectories (at the end of the file).
//
// Reference: learned_controllers/eval/metrics.py:95-362 (MetricsCalculator.compute_metrics and its helpers), fed by
// the recording loops of learned_controllers/eval_rate.py:70-118,170-233.  The reference walks one Python episode at a
// time; here one lane owns one episode of a recorded [T][..][N] trajectory block (word-major, so every load is a
// coalesced row read) and streams over it three times:
//   pass A  max |cmd| per axis, the steady-state command mean, RMSE / smoothness / return sums
//   pass B  settling run-length, overshoot, rise crossing, mean |error|      (need pass A's per-axis scalars)
//   pass C  mean |error| after the settling index                            (needs pass B's index)
// HBM-bound by construction: (6 S + 16 B + 1 S) per recorded step per pass; fp64 arithmetic throughout.
// Sums run sequentially (NumPy sums pairwise): means agree with the reference to ~1e-15 relative, times / flags exactly.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/fdyn.h"
#include "fdyn_core.hpp"

namespace {

using namespace fdyn;

template <typename S>
__global__ void __launch_bounds__(256)
rate_metrics_kernel(const double* __restrict__ times /*[T]*/, const S* __restrict__ rates /*[T][3][n]*/,
                    const S* __restrict__ commands /*[T][3][n]*/, const float* __restrict__ actions /*[T][n][4]*/,
                    const S* __restrict__ rewards /*[T][n]*/, const int32_t* __restrict__ lengths /*[n]*/,
                    double settling_threshold, int settle_steps, int T, int64_t n, double* __restrict__ out /*[FD_NM][n]*/)
{
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int len = lengths[i];
    len = len < 0 ? 0 : (len > T ? T : len);
    if (len == 0) {
#pragma unroll
        for (int k = 0; k < FD_NM; ++k) out[int64_t(k) * n + i] = 0.0;
        return;
    }
    const double t_end = times[len - 1];
    const int n_ss = len / 5 > 1 ? len / 5 : 1;                           // metrics.py:274

    // ---- pass A -----------------------------------------------------------------------------------------------
    double maxc0 = 0.0, maxc1 = 0.0, maxc2 = 0.0, ss0 = 0.0, ss1 = 0.0, ss2 = 0.0;
    double sum_sq = 0.0, sum_diff = 0.0, sum_rew = 0.0;
    float4 prev = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int t = 0; t < len; ++t) {
        const int64_t row = int64_t(t) * 3 * n + i;
        const double c0 = double(commands[row]), c1 = double(commands[row + n]), c2 = double(commands[row + 2 * n]);
        const double r0 = double(rates[row]), r1 = double(rates[row + n]), r2 = double(rates[row + 2 * n]);
        maxc0 = fmax(maxc0, fabs(c0)); maxc1 = fmax(maxc1, fabs(c1)); maxc2 = fmax(maxc2, fabs(c2));
        const double e0 = c0 - r0, e1 = c1 - r1, e2 = c2 - r2;
        sum_sq += e0 * e0; sum_sq += e1 * e1; sum_sq += e2 * e2;          // :356-357, row-major order
        const float4 a = reinterpret_cast<const float4*>(actions)[int64_t(t) * n + i];
        if (t > 0) {                                                      // :334-338, surfaces only
            sum_diff += fabs(double(a.x) - double(prev.x));
            sum_diff += fabs(double(a.y) - double(prev.y));
            sum_diff += fabs(double(a.z) - double(prev.z));
        }
        prev = a;
        sum_rew += double(rewards[int64_t(t) * n + i]);
        if (t >= len - n_ss) { ss0 += c0; ss1 += c1; ss2 += c2; }
    }
    const int64_t mid = int64_t(len / 2) * 3 * n + i;                     // :236
    const double cm0 = double(commands[mid]), cm1 = double(commands[mid + n]), cm2 = double(commands[mid + 2 * n]);

    // ---- per-axis scalars -----------------------------------------------------------------------------------------
    struct Axis {
        double maxc, thr, sgn, cmd_ss, rise_thr, over, sum_abs, sum_tail;
        int run, settle_idx, rise_idx;
        bool skip, rise_on;
    };
    auto axis_init = [&](double maxc, double cmid, double ss_sum) {
        Axis A;
        A.maxc = maxc;
        A.skip = maxc < 0.01;                                             // :144-145
        const double rel = settling_threshold * maxc;
        A.thr = rel > 0.05 ? rel : 0.05;                                  // :201-203
        A.sgn = cmid > 0.0 ? 1.0 : (cmid < 0.0 ? -1.0 : 0.0);
        A.cmd_ss = ss_sum / double(n_ss);
        A.rise_on = !(fabs(A.cmd_ss) < 0.01);                             // :277-278
        A.rise_thr = 0.9 * A.cmd_ss;
        A.over = -1.0; A.sum_abs = 0.0; A.sum_tail = 0.0;
        A.run = 0; A.settle_idx = (settle_steps <= 0) ? 0 : -1; A.rise_idx = -1;
        return A;
    };
    Axis A0 = axis_init(maxc0, cm0, ss0), A1 = axis_init(maxc1, cm1, ss1), A2 = axis_init(maxc2, cm2, ss2);

    // ---- pass B -----------------------------------------------------------------------------------------------
    auto axis_step = [&](Axis& A, double c, double r, int t) {
        const double e = c - r;
        const double ae = fabs(e);
        A.run = ae < A.thr ? A.run + 1 : 0;                               // :206-214: window [t-ss+1, t] all inside
        if (A.settle_idx < 0 && A.run >= settle_steps && t < len - 1) A.settle_idx = t - settle_steps + 1;
        if (A.sgn * (r - c) > 0.0) A.over = fmax(A.over, ae);             // :243-248
        if (A.rise_idx < 0 && (A.cmd_ss > 0.0 ? r >= A.rise_thr : r <= A.rise_thr)) A.rise_idx = t;   // :284-292
        A.sum_abs += ae;
    };
    for (int t = 0; t < len; ++t) {
        const int64_t row = int64_t(t) * 3 * n + i;
        axis_step(A0, double(commands[row]), double(rates[row]), t);
        axis_step(A1, double(commands[row + n]), double(rates[row + n]), t);
        axis_step(A2, double(commands[row + 2 * n]), double(rates[row + 2 * n]), t);
    }

    // ---- pass C: mean |error| from the settling index on (:296-321) ----------------------------------------------
    auto tail_from = [&](const Axis& A) { return (A.settle_idx >= 0 && A.settle_idx < len - 1) ? A.settle_idx : len; };
    const int f0 = tail_from(A0), f1 = tail_from(A1), f2 = tail_from(A2);
    int first = f0 < f1 ? f0 : f1;
    first = first < f2 ? first : f2;
    for (int t = first; t < len; ++t) {
        const int64_t row = int64_t(t) * 3 * n + i;
        if (t >= f0) A0.sum_tail += fabs(double(commands[row]) - double(rates[row]));
        if (t >= f1) A1.sum_tail += fabs(double(commands[row + n]) - double(rates[row + n]));
        if (t >= f2) A2.sum_tail += fabs(double(commands[row + 2 * n]) - double(rates[row + 2 * n]));
    }

    auto axis_store = [&](const Axis& A, int from, int ax) {
        double settle = 0.0, over = 0.0, sserr = 0.0, rise = 0.0;
        if (!A.skip) {
            settle = A.settle_idx >= 0 ? times[A.settle_idx] : t_end;
            over = (A.sgn != 0.0 && A.over >= 0.0) ? (A.over / A.maxc) * 100.0 : 0.0;
            rise = A.rise_on ? (A.rise_idx >= 0 ? times[A.rise_idx] : t_end) : 0.0;
            sserr = from < len ? A.sum_tail / double(len - from) : A.sum_abs / double(len);
        }
        out[int64_t(FD_M_SETTLE_ROLL + ax) * n + i] = settle;
        out[int64_t(FD_M_OVERSHOOT_ROLL + ax) * n + i] = over;
        out[int64_t(FD_M_SSERR_ROLL + ax) * n + i] = sserr;
        out[int64_t(FD_M_RISE_ROLL + ax) * n + i] = rise;
        return settle;
    };
    const double s0 = axis_store(A0, f0, 0), s1 = axis_store(A1, f1, 1), s2 = axis_store(A2, f2, 2);
    out[int64_t(FD_M_SMOOTHNESS) * n + i] = sum_diff / double((len - 1) * 3);         // len == 1: 0/0 = NaN, as NumPy
    out[int64_t(FD_M_RMSE) * n + i] = sqrt(sum_sq / double(len * 3));
    out[int64_t(FD_M_SUCCESS) * n + i] = (s0 < t_end && s1 < t_end && s2 < t_end) ? 1.0 : 0.0;   // :171-176
    out[int64_t(FD_M_EPISODE_LENGTH) * n + i] = t_end;
    out[int64_t(FD_M_TOTAL_REWARD) * n + i] = sum_rew;
}

template <typename S>
int launch_metrics(const double* times, const S* rates, const S* commands, const float* actions, const S* rewards,
                   const int32_t* lengths, double settling_threshold, int settle_steps, int T, int64_t n, double* out,
                   void* stream)
{
    if (T < 0 || n < 0 || settle_steps < 0) return FDYN_ERR_BAD_SIZE;
    if (n == 0) return FDYN_OK;
    if (!lengths || !out || (T > 0 && (!times || !rates || !commands || !actions || !rewards))) return FDYN_ERR_NULL;
    const unsigned blocks = unsigned((n + 255) / 256);
    hipLaunchKernelGGL(rate_metrics_kernel<S>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, times, rates, commands,
                       actions, rewards, lengths, settling_threshold, settle_steps, T, n, out);
    return int(hipGetLastError());
}

// RateTrackingReward.compute + SettlingTimeBonus.compute over recorded sequences (rewards.py:75-137,193-221): the operation
// order of env_reward (fdyn_core.hpp), with the weights as parameters and the components written out.
template <typename S>
__global__ void __launch_bounds__(256)
rate_reward_seq_kernel(const S* __restrict__ errs /*[T][3][n]*/, const S* __restrict__ actions /*[T][4][n]*/,
                       const S* __restrict__ prev0 /*[4][n]*/, const S* __restrict__ flight /*[T][FD_NRF][n]*/,
                       const S* __restrict__ cmd /*[3][n]*/, const double* __restrict__ params /*[FD_NRW]*/,
                       S* __restrict__ rstate /*[FD_NRS][n]*/, S dt, int T, int64_t n, S* __restrict__ tracking,
                       S* __restrict__ components, S* __restrict__ settle, uint8_t* __restrict__ settled)
{
#pragma clang fp contract(off)
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const S w_track = S(params[FD_RW_TRACKING]), w_smooth = S(params[FD_RW_SMOOTHNESS]), w_stab = S(params[FD_RW_STABILITY]);
    const S w_osc = S(params[FD_RW_OSCILLATION]), w_surv = S(params[FD_RW_SURVIVAL]);
    const S thr = S(params[FD_RW_SETTLE_THRESHOLD]), min_t = S(params[FD_RW_MIN_SETTLE_TIME]), mult = S(params[FD_RW_BONUS_MULTIPLIER]);
    S perr[3], sc[3], c[3], prev[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        perr[k] = rstate[int64_t(FD_RS_PERR_P + k) * n + i];
        sc[k] = rstate[int64_t(FD_RS_SIGN_P + k) * n + i];
        c[k] = cmd[int64_t(k) * n + i];
        prev[k] = prev0[int64_t(k) * n + i];
    }
    S timer = rstate[int64_t(FD_RS_SETTLE_TIMER) * n + i], is_settled = rstate[int64_t(FD_RS_IS_SETTLED) * n + i];
    for (int t = 0; t < T; ++t) {
        S err[3], a[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            err[k] = errs[(int64_t(t) * 3 + k) * n + i];
            a[k] = actions[(int64_t(t) * 4 + k) * n + i];
        }
        const S airspeed = flight[(int64_t(t) * FD_NRF + FD_RF_AIRSPEED) * n + i];
        const S altitude = flight[(int64_t(t) * FD_NRF + FD_RF_ALTITUDE) * n + i];
        const S roll = flight[(int64_t(t) * FD_NRF + FD_RF_ROLL) * n + i], pitch = flight[(int64_t(t) * FD_NRF + FD_RF_PITCH) * n + i];
        const S tracking_error = (err[0] * err[0] + err[1] * err[1] + err[2] * err[2]) / S(3);           // :76
        const S r_tracking = -w_track * tracking_error;
        const S d0 = a[0] - prev[0], d1 = a[1] - prev[1], d2 = a[2] - prev[2];
        const S r_smooth = -w_smooth * (d0 * d0 + (d1 * d1 + d2 * d2));                                  // np.sum of 3: a0 + (a1 + a2)
        const S roll_st = M<S>::exp(-M<S>::abs(roll) / deg2rad<S>(45.0));
        const S pitch_st = M<S>::exp(-M<S>::abs(pitch) / deg2rad<S>(30.0));
        const S as_st = clipv((airspeed - S(8)) / S(12), S(0), S(1));
        const S alt_st = clipv((altitude - S(10)) / S(90), S(0), S(1));
        const S r_stab = w_stab * ((roll_st + pitch_st + as_st + alt_st) / S(4));
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const bool flip = (signv(err[k]) != signv(perr[k])) && (M<S>::abs(perr[k]) > S(0.01));
            sc[k] = S(0.9) * sc[k] + (flip ? S(1) : S(0));
            perr[k] = err[k];
            prev[k] = a[k];
        }
        const S r_osc = -w_osc * (sc[0] + (sc[1] + sc[2]));
        const S total = r_tracking + r_smooth + r_stab + r_osc + w_surv;
        bool now = true;                                                                                  // :193-209
#pragma unroll
        for (int k = 0; k < 3; ++k) now = now && (M<S>::abs(err[k]) < pymax(M<S>::abs(c[k]) * thr, S(0.05)));
        S bonus = S(0);
        if (now) {
            timer += dt;
            if (timer >= min_t) { is_settled = S(1); bonus = mult * dt; }
        } else {
            timer = S(0);
            is_settled = S(0);
        }
        if (tracking) tracking[int64_t(t) * n + i] = total;
        if (components) {
            components[(int64_t(t) * FD_NRC + FD_RC_TRACKING) * n + i] = r_tracking;
            components[(int64_t(t) * FD_NRC + FD_RC_SMOOTHNESS) * n + i] = r_smooth;
            components[(int64_t(t) * FD_NRC + FD_RC_STABILITY) * n + i] = r_stab;
            components[(int64_t(t) * FD_NRC + FD_RC_OSCILLATION) * n + i] = r_osc;
            components[(int64_t(t) * FD_NRC + FD_RC_SURVIVAL) * n + i] = w_surv;
        }
        if (settle) settle[int64_t(t) * n + i] = bonus;
        if (settled) settled[int64_t(t) * n + i] = is_settled != S(0) ? 1 : 0;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        rstate[int64_t(FD_RS_PERR_P + k) * n + i] = perr[k];
        rstate[int64_t(FD_RS_SIGN_P + k) * n + i] = sc[k];
    }
    rstate[int64_t(FD_RS_SETTLE_TIMER) * n + i] = timer;
    rstate[int64_t(FD_RS_IS_SETTLED) * n + i] = is_settled;
}

template <typename S>
int launch_reward_seq(const S* errs, const S* actions, const S* prev0, const S* flight, const S* cmd, const double* params,
                      S* rstate, S dt, int T, int64_t n, S* tracking, S* components, S* settle, uint8_t* settled, void* stream)
{
    if (n < 0 || T < 0) return FDYN_ERR_BAD_SIZE;
    if (n == 0) return FDYN_OK;
    if (!params || !rstate || !cmd || !prev0 || (T > 0 && (!errs || !actions || !flight))) return FDYN_ERR_NULL;
    hipLaunchKernelGGL(rate_reward_seq_kernel<S>, dim3(unsigned((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, errs, actions,
                       prev0, flight, cmd, params, rstate, dt, T, n, tracking, components, settle, settled);
    return int(hipGetLastError());
}

// ---- trajectory comparison, streamed ----------------------------------------------------------------------------------
// Reference: validation/metrics/trajectory_metrics.py:9-174 (compute_rmse / compute_correlation / compute_max_error and
// compare_trajectories).  The reference holds both trajectories in DataFrames and reduces them with NumPy / scipy; a fleet
// cannot be recorded (65 536 aircraft x 6 000 steps x 14 channels is 44 GB), so one lane owns one PAIR of aircraft, keeps the
// FD_NTA accumulator words of acc [FD_NTA][n] in registers, consumes the launch's T steps in order and writes acc back once:
// acc traffic is 2 x FD_NTA words per launch whatever T is, every access is a coalesced row read / write along n, and
// nothing is reduced across lanes -- so feeding a trajectory in chunks of any sizes repeats the same operations in the same
// order and is bit-identical to one launch.  64-lane workgroups: the 98 carried doubles fill most of the 256 architectural
// registers of a lane, one wave per SIMD is all a 65 536-pair fleet has anyway (1024 waves on 1024 SIMDs), and small
// workgroups spread those waves over every CU.  Contraction is off so that differences and products round as NumPy's do.
constexpr int traj_corr_channel(int j)
{
    return j == 0 ? FD_TC_NORTH : j == 1 ? FD_TC_EAST : j == 2 ? FD_TC_DOWN : j == 3 ? FD_TC_ALTITUDE : j == 4 ? FD_TC_ROLL
         : j == 5 ? FD_TC_PITCH : j == 6 ? FD_TC_YAW : j == 7 ? FD_TC_P : j == 8 ? FD_TC_Q : FD_TC_R;
}
constexpr int traj_max_channel(int m)
{
    return m == 0 ? FD_TC_NORTH : m == 1 ? FD_TC_EAST : m == 2 ? FD_TC_DOWN : m == 3 ? FD_TC_ROLL : m == 4 ? FD_TC_PITCH : FD_TC_YAW;
}

// one step of one side: the 14 channels in the reference's units (np.degrees = one multiply by 180 / pi), yaw still wrapped
template <typename S>
FD_DEV void traj_channels(const S* __restrict__ x, const S* __restrict__ d, int t, int64_t n, int64_t i, double (&c)[FD_NTC])
{
#pragma clang fp contract(off)
    double xs[FD_NX];
#pragma unroll
    for (int w = 0; w < FD_NX; ++w) xs[w] = double(x[(int64_t(t) * FD_NX + w) * n + i]);
    if (d) {
        c[FD_TC_AIRSPEED] = double(d[(int64_t(t) * FD_ND + FD_D_AIRSPEED) * n + i]);
        c[FD_TC_ALTITUDE] = double(d[(int64_t(t) * FD_ND + FD_D_ALTITUDE) * n + i]);
    } else {
        const Derived<double> dv = derived<double>(xs);                   // what fdyn_derived_f64 writes
        c[FD_TC_AIRSPEED] = dv.airspeed;
        c[FD_TC_ALTITUDE] = dv.altitude;
    }
    constexpr double RAD2DEG = 180.0 / 3.141592653589793238462643383279502884;
    c[FD_TC_NORTH] = xs[FD_X_N]; c[FD_TC_EAST] = xs[FD_X_E]; c[FD_TC_DOWN] = xs[FD_X_D];
    c[FD_TC_U] = xs[FD_X_U]; c[FD_TC_V] = xs[FD_X_V]; c[FD_TC_W] = xs[FD_X_W];
    c[FD_TC_ROLL] = xs[FD_X_ROLL] * RAD2DEG; c[FD_TC_PITCH] = xs[FD_X_PITCH] * RAD2DEG; c[FD_TC_YAW] = xs[FD_X_YAW] * RAD2DEG;
    c[FD_TC_P] = xs[FD_X_P] * RAD2DEG; c[FD_TC_Q] = xs[FD_X_Q] * RAD2DEG; c[FD_TC_R] = xs[FD_X_R] * RAD2DEG;
}

// np.unwrap(., period=360), one sample: numpy/lib/function_base.py (unwrap) with discont = period / 2
FD_DEV double traj_unwrap(double cur, double& prev, double& off)
{
#pragma clang fp contract(off)
    const double dd = cur - prev;
    double m = fmod(dd + 180.0, 360.0);
    if (m < 0.0) m += 360.0;                                              // np.mod: the result takes the divisor's sign
    double ddmod = m - 180.0;
    if (ddmod == -180.0 && dd > 0.0) ddmod = 180.0;
    double corr = ddmod - dd;
    if (fabs(dd) < 180.0) corr = 0.0;
    off += corr;
    prev = cur;
    return cur + off;
}

FD_DEV double traj_correlation(const double (&A)[FD_NTA], int j, double k, unsigned varied)
{
#pragma clang fp contract(off)
    if (k < 2.0) return 0.0;                                              // trajectory_metrics.py:51-52
    if (((varied >> (2 * j)) & 3u) != 3u) return __builtin_nan("");       // scipy.stats.pearsonr on a constant input
    const double* w = &A[FD_TA_CORR + j * FD_TA_CORR_WORDS];
    const double su = w[FD_TA_SU], sv = w[FD_TA_SV];
    const double cov = w[FD_TA_SUV] - su * sv / k;
    const double vu = w[FD_TA_SUU] - su * su / k, vv = w[FD_TA_SVV] - sv * sv / k;
    const double r = cov / (sqrt(vu) * sqrt(vv));
    return r > 1.0 ? 1.0 : (r < -1.0 ? -1.0 : r);                         // scipy clamps; NaN stays NaN
}

template <typename SA, typename SB>
__global__ void __launch_bounds__(64)
traj_compare_kernel(const SA* __restrict__ xa, const SA* __restrict__ da, const SB* __restrict__ xb, const SB* __restrict__ db,
                    int T, int64_t n, double* __restrict__ acc /*[FD_NTA][n]*/, double* __restrict__ out /*[FD_NTM][n] or null*/)
{
#pragma clang fp contract(off)
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double A[FD_NTA];
#pragma unroll
    for (int r = 0; r < FD_NTA; ++r) A[r] = acc[int64_t(r) * n + i];
    unsigned varied = unsigned(A[FD_TA_VARIED]);
    for (int t = 0; t < T; ++t) {
        double a[FD_NTC], b[FD_NTC];
        traj_channels<SA>(xa, da, t, n, i, a);
        traj_channels<SB>(xb, db, t, n, i, b);
        const bool first = A[FD_TA_COUNT] == 0.0;
        if (first) {
            A[FD_TA_YAW_PREV_A] = a[FD_TC_YAW]; A[FD_TA_YAW_PREV_B] = b[FD_TC_YAW];
            A[FD_TA_YAW_OFF_A] = 0.0; A[FD_TA_YAW_OFF_B] = 0.0;
        }
        a[FD_TC_YAW] = traj_unwrap(a[FD_TC_YAW], A[FD_TA_YAW_PREV_A], A[FD_TA_YAW_OFF_A]);
        b[FD_TC_YAW] = traj_unwrap(b[FD_TC_YAW], A[FD_TA_YAW_PREV_B], A[FD_TA_YAW_OFF_B]);
        double e[FD_NTC];
#pragma unroll
        for (int c = 0; c < FD_NTC; ++c) {
            e[c] = a[c] - b[c];
            A[FD_TA_SSQ + c] += e[c] * e[c];
        }
#pragma unroll
        for (int m = 0; m < FD_TA_NMAX; ++m) A[FD_TA_MAX + m] = fmax(A[FD_TA_MAX + m], fabs(e[traj_max_channel(m)]));
        const double pos = sqrt(e[FD_TC_NORTH] * e[FD_TC_NORTH] + e[FD_TC_EAST] * e[FD_TC_EAST] + e[FD_TC_DOWN] * e[FD_TC_DOWN]);
        A[FD_TA_POS3D_SSQ] += pos * pos;                                  // :108-109: the norm, squared again
        A[FD_TA_POS3D_MAX] = fmax(A[FD_TA_POS3D_MAX], pos);
#pragma unroll
        for (int j = 0; j < FD_TA_NCORR; ++j) {
            double* w = &A[FD_TA_CORR + j * FD_TA_CORR_WORDS];
            const double ca = a[traj_corr_channel(j)], cb = b[traj_corr_channel(j)];
            if (first) { w[FD_TA_PIVOT_A] = ca; w[FD_TA_PIVOT_B] = cb; }
            const double u = ca - w[FD_TA_PIVOT_A], v = cb - w[FD_TA_PIVOT_B];
            if (u != 0.0) varied |= 1u << (2 * j);
            if (v != 0.0) varied |= 2u << (2 * j);
            w[FD_TA_SU] += u; w[FD_TA_SV] += v;
            w[FD_TA_SUU] += u * u; w[FD_TA_SVV] += v * v; w[FD_TA_SUV] += u * v;
        }
        A[FD_TA_COUNT] += 1.0;
    }
    if (T > 0) {
        A[FD_TA_VARIED] = double(varied);
#pragma unroll
        for (int r = 0; r < FD_NTA; ++r) acc[int64_t(r) * n + i] = A[r];
    }
    if (!out) return;
    const double k = A[FD_TA_COUNT];
    double M[FD_NTM];
    if (k == 0.0) {
#pragma unroll
        for (int r = 0; r < FD_NTM; ++r) M[r] = 0.0;
    } else {
        auto rmse = [&](int c) { return sqrt(A[FD_TA_SSQ + c] / k); };
        double corr[FD_TA_NCORR];
#pragma unroll
        for (int j = 0; j < FD_TA_NCORR; ++j) corr[j] = traj_correlation(A, j, k, varied);
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {                                  // north, east, down; roll, pitch, yaw; p, q, r
            M[FD_TM_POSITION_NORTH_RMSE + 3 * ax] = rmse(FD_TC_NORTH + ax);
            M[FD_TM_POSITION_NORTH_CORRELATION + 3 * ax] = corr[ax];
            M[FD_TM_POSITION_NORTH_MAX_ERROR + 3 * ax] = A[FD_TA_MAX + ax];
            M[FD_TM_ATTITUDE_ROLL_RMSE_DEG + 3 * ax] = rmse(FD_TC_ROLL + ax);
            M[FD_TM_ATTITUDE_ROLL_CORRELATION + 3 * ax] = corr[4 + ax];
            M[FD_TM_ATTITUDE_ROLL_MAX_ERROR_DEG + 3 * ax] = A[FD_TA_MAX + 3 + ax];
            M[FD_TM_RATE_P_RMSE_DPS + 2 * ax] = rmse(FD_TC_P + ax);
            M[FD_TM_RATE_P_CORRELATION + 2 * ax] = corr[7 + ax];
            M[FD_TM_VELOCITY_U_RMSE + ax] = rmse(FD_TC_U + ax);
        }
        M[FD_TM_POSITION_3D_RMSE] = sqrt(A[FD_TA_POS3D_SSQ] / k);
        M[FD_TM_POSITION_3D_MAX_ERROR] = A[FD_TA_POS3D_MAX];
        M[FD_TM_ALTITUDE_RMSE] = rmse(FD_TC_ALTITUDE);
        M[FD_TM_ALTITUDE_CORRELATION] = corr[3];
        M[FD_TM_AIRSPEED_RMSE] = rmse(FD_TC_AIRSPEED);
        M[FD_TM_MEAN_POSITION_CORRELATION] = (corr[0] + corr[1] + corr[2]) / 3.0;        // np.mean: NaN propagates
        M[FD_TM_MEAN_ATTITUDE_CORRELATION] = (corr[4] + corr[5] + corr[6]) / 3.0;
        M[FD_TM_OVERALL_CORRELATION] = (M[FD_TM_MEAN_POSITION_CORRELATION] + M[FD_TM_MEAN_ATTITUDE_CORRELATION]) / 2.0;
    }
#pragma unroll
    for (int r = 0; r < FD_NTM; ++r) out[int64_t(r) * n + i] = M[r];
}

template <typename SA, typename SB>
int launch_traj_compare(const void* xa, const void* da, const void* xb, const void* db, int T, int64_t n, double* acc,
                        double* out, void* stream)
{
    hipLaunchKernelGGL((traj_compare_kernel<SA, SB>), dim3(unsigned((n + 63) / 64)), dim3(64), 0, (hipStream_t)stream,
                       static_cast<const SA*>(xa), static_cast<const SA*>(da), static_cast<const SB*>(xb),
                       static_cast<const SB*>(db), T, n, acc, out);
    return int(hipGetLastError());
}

}  // namespace

extern "C" {

int fdyn_rate_metrics_f64(const double* times, const double* rates, const double* commands, const float* actions,
                          const double* rewards, const int32_t* lengths, double settling_threshold, int settle_steps,
                          int T, int64_t n, double* out, void* stream)
{
    return launch_metrics<double>(times, rates, commands, actions, rewards, lengths, settling_threshold, settle_steps, T, n,
                                  out, stream);
}

int fdyn_rate_metrics_f32(const double* times, const float* rates, const float* commands, const float* actions,
                          const float* rewards, const int32_t* lengths, double settling_threshold, int settle_steps,
                          int T, int64_t n, double* out, void* stream)
{
    return launch_metrics<float>(times, rates, commands, actions, rewards, lengths, settling_threshold, settle_steps, T, n,
                                 out, stream);
}

int fdyn_rate_reward_seq_f64(const double* errs, const double* actions, const double* prev0, const double* flight,
                             const double* cmd, const double* params, double* rstate, double dt, int T, int64_t n,
                             double* tracking, double* components, double* settle, uint8_t* settled, void* stream)
{
    return launch_reward_seq<double>(errs, actions, prev0, flight, cmd, params, rstate, dt, T, n, tracking, components, settle, settled, stream);
}

int fdyn_rate_reward_seq_f32(const float* errs, const float* actions, const float* prev0, const float* flight,
                             const float* cmd, const double* params, float* rstate, float dt, int T, int64_t n,
                             float* tracking, float* components, float* settle, uint8_t* settled, void* stream)
{
    return launch_reward_seq<float>(errs, actions, prev0, flight, cmd, params, rstate, dt, T, n, tracking, components, settle, settled, stream);
}

int fdyn_traj_compare(const void* xa, int a_f32, const void* da, const void* xb, int b_f32, const void* db, int T, int64_t n,
                      double* acc, double* out, void* stream)
{
    if (T < 0 || n < 0) return FDYN_ERR_BAD_SIZE;
    if (n == 0 || (T == 0 && !out)) return FDYN_OK;
    if (!acc || (T > 0 && (!xa || !xb))) return FDYN_ERR_NULL;
    if (a_f32) return b_f32 ? launch_traj_compare<float, float>(xa, da, xb, db, T, n, acc, out, stream)
                            : launch_traj_compare<float, double>(xa, da, xb, db, T, n, acc, out, stream);
    return b_f32 ? launch_traj_compare<double, float>(xa, da, xb, db, T, n, acc, out, stream)
                 : launch_traj_compare<double, double>(xa, da, xb, db, T, n, acc, out, stream);
}

}  // extern "C"

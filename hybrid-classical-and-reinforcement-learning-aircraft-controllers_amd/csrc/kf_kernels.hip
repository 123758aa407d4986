// kf_kernels.hip -- LQG for whole fleets, gfx950: the estimator beside lqr_kernels.hip's regulator.
//
// fdyn_kf_design    the steady-state discrete Kalman filter of each aircraft on its own A, B (fdyn_linearize): per block the
//                   model is discretised (a scaled Taylor series of the matrix exponential and of its integral) and the filter
//                   Riccati equation P = Phi (P - P (P + V)^-1 P) Phi^T + W is solved in fp64, one lane per aircraft, by the
//                   doubling loop fdyn_lqr_design runs (fdyn_riccati.hpp): L = P (P + V)^-1.  Every state of a block is
//                   measured, C = I.
// fdyn_lqg_step_*   n_steps x { y = delta + sigma z -> xhat = pred + L (y - pred) -> u = u0 - K xhat -> Controls::set -> one
//                   RK4 of dt }, one launch, through fdyn_lqr_law.hpp's law and the steppers of fdyn_core.hpp exactly as
//                   lqr_step_kernel calls them; the normals come from Philox in the kernel or from the caller.
//
// Registers, not scratch: the design keeps every matrix as named words of an M4 and sends its two blocks through ONE rolled
// loop, whose block-dependent part is a scalar offset into global memory.  The step kernel has no room for the estimator
// beside the physics (lqr_step_kernel<double, double> fills the register file; 80 filter words, 20 accumulators and the
// estimate on top spill), so nothing of the control step lives in a register across the RK4: the filter, xhat, du_prev and
// the law's own K, u0, x0 sit in LDS laid out [word][lane], 64-lane workgroups (fp64 glue: 120 x 8 B per lane = 60 KB, under
// the 64 KB a workgroup may declare; fp32 glue: 32 KB).  The accumulators are registers in the fp32 instantiations, which
// have them; the f64 instantiation adds to the caller's words in global memory step by step.
// Every lane touches only its own column, consecutive lanes consecutive addresses: no bank conflict, no barrier.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "fdyn_fleet.hpp"
#include "fdyn_riccati.hpp"
#include "fdyn_lqr_law.hpp"
#include "philox.hpp"

using namespace fdyn;

namespace {

constexpr int TB = 64;                   // design: threads per workgroup
constexpr int NB = RIC_N;                // states per block
constexpr int KF_SERIES_TERMS = 17;
constexpr double KF_NORM_MAX = 1.5;      // |a|_inf dt above which the first dropped series term exceeds 1e-14
constexpr int LB = 64;                   // LQG step: threads per workgroup (what the LDS columns allow)

__global__ void __launch_bounds__(TB)
kf_design_kernel(const double* __restrict__ A /*[144][n]*/, const double* __restrict__ B /*[48][n]*/, double dt,
                 const double* __restrict__ noise /*[16] or [16][n]*/, int noise_per_lane, int64_t n,
                 double* __restrict__ F /*[80][n]*/, double* __restrict__ residual, int32_t* __restrict__ iters,
                 int32_t* __restrict__ status)
{
#pragma clang fp contract(off)
    const int64_t i = int64_t(blockIdx.x) * TB + threadIdx.x;
    if (i >= n) return;
    double nz[FD_NKFN];
    bool bad = !(dt > 1e-6) || dt > 1.0;
#pragma unroll
    for (int k = 0; k < FD_NKFN; ++k) {
        nz[k] = noise_per_lane ? noise[k * n + i] : noise[k];
        bad = bad || !(::isfinite(nz[k]) && nz[k] > 0.0);
    }
    double res = 0.0;
    int it_max = 0, st = 0;

#pragma unroll 1
    for (int blk = 0; blk < 2; ++blk) {
        const int s0 = blk ? FD_X_V : FD_X_U, s1 = blk ? FD_X_P : FD_X_W, s2 = blk ? FD_X_R : FD_X_Q, s3 = blk ? FD_X_ROLL : FD_X_PITCH;
        const int c0 = blk ? FD_U_AILERON : FD_U_ELEVATOR, c1 = blk ? FD_U_RUDDER : FD_U_THROTTLE;
        const int sr[NB] = { s0, s1, s2, s3 };
        M4 a;
        double b[NB][2], v[NB], w[NB];
        bool fin = true;
#pragma unroll
        for (int r = 0; r < NB; ++r) {
#pragma unroll
            for (int c = 0; c < NB; ++c) { a.v[r][c] = A[int64_t(sr[r] * FD_NX + sr[c]) * n + i]; fin = fin && ::isfinite(a.v[r][c]); }
            b[r][0] = B[int64_t(sr[r] * FD_NU + c0) * n + i];
            b[r][1] = B[int64_t(sr[r] * FD_NU + c1) * n + i];
            fin = fin && ::isfinite(b[r][0]) && ::isfinite(b[r][1]);
            const double sg = blk ? nz[FD_KFN_SIGMA + NB + r] : nz[FD_KFN_SIGMA + r], rate = blk ? nz[FD_KFN_RATE + NB + r] : nz[FD_KFN_RATE + r];
            v[r] = sg * sg;
            w[r] = (rate * rate) * dt;
        }
        double norm = 0.0;
#pragma unroll
        for (int r = 0; r < NB; ++r) {
            double rs = ::fabs(a.v[r][0]);
#pragma unroll
            for (int c = 1; c < NB; ++c) rs = rs + ::fabs(a.v[r][c]);
            norm = rs > norm ? rs : norm;
        }
        bad = bad || !fin || !(norm * dt <= KF_NORM_MAX);
        if (bad) continue;                                       // BAD_INPUT (dt, noise, or either block): nothing is solved

        // discretise: S = sum_k (a dt)^k / (k + 1)!, Phi = I + a dt S = exp(a dt), Gamma = dt S b = int_0^dt exp(a t) dt b
        M4 ad, T, S;
#pragma unroll
        for (int r = 0; r < NB; ++r)
#pragma unroll
            for (int c = 0; c < NB; ++c) { ad.v[r][c] = a.v[r][c] * dt; T.v[r][c] = S.v[r][c] = r == c ? 1.0 : 0.0; }
#pragma unroll 1
        for (int k = 1; k <= KF_SERIES_TERMS; ++k) {
            const M4 Ta = mul<false, false>(T, ad);
            const double div = double(k + 1);
#pragma unroll
            for (int r = 0; r < NB; ++r)
#pragma unroll
                for (int c = 0; c < NB; ++c) { T.v[r][c] = Ta.v[r][c] / div; S.v[r][c] = S.v[r][c] + T.v[r][c]; }
        }
        M4 Phi = mul<false, false>(ad, S);
#pragma unroll
        for (int r = 0; r < NB; ++r) Phi.v[r][r] = 1.0 + Phi.v[r][r];
        double Gam[NB][2];
#pragma unroll
        for (int r = 0; r < NB; ++r)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                double s = S.v[r][0] * b[0][j];
#pragma unroll
                for (int k = 1; k < NB; ++k) s = s + S.v[r][k] * b[k][j];
                Gam[r][j] = dt * s;
            }

        // solve: the dual of the regulator's problem, A_0 = Phi^T, G_0 = V^-1, H_0 = W
        M4 Ak, Gk, Hk;
#pragma unroll
        for (int r = 0; r < NB; ++r)
#pragma unroll
            for (int c = 0; c < NB; ++c) {
                Ak.v[r][c] = Phi.v[c][r];
                Gk.v[r][c] = r == c ? 1.0 / v[r] : 0.0;
                Hk.v[r][c] = r == c ? w[r] : 0.0;
            }
        int it;
        bool failed = false, converged;
        riccati_doubling(Ak, Gk, Hk, it, failed, converged);

        M4 P, PV, PVi;
#pragma unroll
        for (int r = 0; r < NB; ++r)
#pragma unroll
            for (int c = 0; c < NB; ++c) {
                P.v[r][c] = 0.5 * (Hk.v[r][c] + Hk.v[c][r]);
                PV.v[r][c] = r == c ? P.v[r][c] + v[r] : P.v[r][c];
            }
        const bool gain_ok = inverse(PV, PVi);
        const M4 Lg = mul<false, false>(P, PVi);
        // residual of the filter equation at P
        const M4 LP = mul<false, false>(Lg, P);
        M4 D;
#pragma unroll
        for (int r = 0; r < NB; ++r)
#pragma unroll
            for (int c = 0; c < NB; ++c) D.v[r][c] = P.v[r][c] - LP.v[r][c];
        const M4 PDP = mul<false, true>(mul<false, false>(Phi, D), Phi);
        M4 R;
#pragma unroll
        for (int r = 0; r < NB; ++r)
#pragma unroll
            for (int c = 0; c < NB; ++c) R.v[r][c] = (r == c ? PDP.v[r][c] + w[r] : PDP.v[r][c]) - P.v[r][c];
        const double bres = max_abs(R.v) / max_abs(P.v);
        res = nan_max(res, bres);
        it_max = it > it_max ? it : it_max;
        if (failed || !converged) st |= FD_KF_NOT_CONVERGED;
        if (!gain_ok || !positive_definite(P) || !(bres <= RIC_RES_MAX)) st |= FD_KF_NO_CERTIFICATE;

        double* Fphi = F + int64_t(FD_KF_PHI_LON + blk * (FD_KF_PHI_LAT - FD_KF_PHI_LON)) * n + i;
        double* Fgam = F + int64_t(FD_KF_GAMMA_LON + blk * (FD_KF_GAMMA_LAT - FD_KF_GAMMA_LON)) * n + i;
        double* Fl = F + int64_t(FD_KF_L_LON + blk * (FD_KF_L_LAT - FD_KF_L_LON)) * n + i;
#pragma unroll
        for (int r = 0; r < NB; ++r) {
#pragma unroll
            for (int c = 0; c < NB; ++c) { Fphi[int64_t(r * NB + c) * n] = Phi.v[r][c]; Fl[int64_t(r * NB + c) * n] = Lg.v[r][c]; }
            Fgam[int64_t(r * 2) * n] = Gam[r][0];
            Fgam[int64_t(r * 2 + 1) * n] = Gam[r][1];
        }
    }

    if (bad) { st = FD_KF_BAD_INPUT; res = __builtin_nan(""); it_max = 0; }
    if (st) {                                                    // pass-through: Phi = I, Gamma = 0, L = I -> xhat = y
#pragma unroll
        for (int k = 0; k < FD_NKF; ++k) {
            const bool gam = k >= FD_KF_GAMMA_LON && k < FD_KF_L_LON;
            F[int64_t(k) * n + i] = (!gam && (k & 15) % 5 == 0) ? 1.0 : 0.0;
        }
    }
    residual[i] = res;
    iters[i] = it_max;
    status[i] = st;
}

// ---- the output-feedback loop ---------------------------------------------------------------------------------------------------
// the words of one lane in LDS laid out [word][lane]; every index is a compile-time constant once unrolled
template <typename W, int BLK> struct LaneWords {
    W* col;
    FD_DEV explicit LaneWords(W* lds) : col(lds + threadIdx.x) {}
    FD_DEV W get(int k) const { return col[k * BLK]; }
    FD_DEV void set(int k, W v) { col[k * BLK] = v; }
};
// the glue-type words behind the filter's FD_NKF: the estimate, the last applied control offset, the law's gains and u0
enum { LW_XHAT = FD_NKF, LW_DU = LW_XHAT + 8, LW_K = LW_DU + FD_NU, LW_U0 = LW_K + FD_NLQK, LW_N = LW_U0 + FD_NU };

// eight standard normals for lane i at this step: two Philox blocks, Box-Muller paired as sensor_kernels.hip pairs it
template <typename G>
FD_DEV void lqg_normals(uint64_t seed, int64_t i, uint32_t step, G (&z)[8])
{
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        uint32_t r[4];
        philox4(seed, uint32_t(i), uint32_t(i >> 32), step, FD_PHX_LQG + uint32_t(b), r);
        const float u0 = philox_u01(r[0]), u1 = philox_u01(r[1]);
        const float u2 = philox_u01(r[2]), u3 = philox_u01(r[3]);
        const float ra = sqrtf(-2.0f * __logf(u0)), rb = sqrtf(-2.0f * __logf(u2));
        z[4 * b + 0] = G(ra * __cosf(6.283185307f * u1)); z[4 * b + 1] = G(ra * __sinf(6.283185307f * u1));
        z[4 * b + 2] = G(rb * __cosf(6.283185307f * u3)); z[4 * b + 3] = G(rb * __sinf(6.283185307f * u3));
    }
}

// pred = Phi xhat + Gamma du_prev, xhat = pred + L (y - pred) per block, every sum left to right, no contraction
template <typename G, typename FW>
FD_DEV void kalman_update(const FW& f, const G (&y)[8], const G (&du)[FD_NU], G (&xh)[8])
{
#pragma clang fp contract(off)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const int o = NB * b, phi = b ? FD_KF_PHI_LAT : FD_KF_PHI_LON, gam = b ? FD_KF_GAMMA_LAT : FD_KF_GAMMA_LON, lg = b ? FD_KF_L_LAT : FD_KF_L_LON;
        const G du0 = b ? du[FD_U_AILERON] : du[FD_U_ELEVATOR], du1 = b ? du[FD_U_RUDDER] : du[FD_U_THROTTLE];
        G pred[NB], e[NB];
#pragma unroll
        for (int r = 0; r < NB; ++r) {
            G p = f.get(phi + NB * r) * xh[o];
#pragma unroll
            for (int c = 1; c < NB; ++c) p = p + f.get(phi + NB * r + c) * xh[o + c];
            const G g = f.get(gam + 2 * r) * du0 + f.get(gam + 2 * r + 1) * du1;
            pred[r] = p + g;
            e[r] = y[o + r] - pred[r];
        }
#pragma unroll
        for (int r = 0; r < NB; ++r) {
            G c = f.get(lg + NB * r) * e[0];
#pragma unroll
            for (int k = 1; k < NB; ++k) c = c + f.get(lg + NB * r + k) * e[k];
            xh[o + r] = pred[r] + c;
        }
    }
}

template <typename G, typename S>
FD_DEV void store_controls(S* __restrict__ surf_out, int64_t n, int64_t at, const Surfaces<G>& surf)
{                                                                // the controls as applied: after set_controls' clip
    surf_out[FD_U_ELEVATOR * n + at] = S(clipv<G>(surf.elevator, G(-1), G(1)));
    surf_out[FD_U_AILERON * n + at] = S(clipv<G>(surf.aileron, G(-1), G(1)));
    surf_out[FD_U_RUDDER * n + at] = S(clipv<G>(surf.rudder, G(-1), G(1)));
    surf_out[FD_U_THROTTLE * n + at] = S(clipv<G>(surf.throttle, G(0), G(1)));
}

// n_steps = 0: the controls from the stored estimate (from the true state for FD_LQG_TRUTH), nothing else is written
template <typename S, typename T>
__global__ void __launch_bounds__(256)
lqg_controls_kernel(const S* __restrict__ xs, const double* __restrict__ x0, const double* __restrict__ u0, const double* __restrict__ K,
                    int64_t n, const double* __restrict__ xhat, int feedback, S* __restrict__ surf_out)
{
    using G = typename GlueOf<S, T>::type;
    const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    constexpr int W[8] = { FD_X_U, FD_X_W, FD_X_Q, FD_X_PITCH, FD_X_V, FD_X_P, FD_X_R, FD_X_ROLL };
    LqrLaw<G> law;
#pragma unroll
    for (int k = 0; k < FD_NLQK; ++k) law.k[k] = G(K[k * n + i]);
#pragma unroll
    for (int k = 0; k < FD_NU; ++k) law.u0[k] = G(u0[k * n + i]);
#pragma unroll
    for (int j = 0; j < 8; ++j) law.x0[j] = x0[W[j] * n + i];
    G f[8];
    if (feedback == FD_LQG_TRUTH) {
        S x[FD_NX];
#pragma unroll
        for (int k = 0; k < FD_NX; ++k) x[k] = xs[k * n + i];
        law.delta(x, f);
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) f[j] = G(xhat[int64_t(j) * n + i]);
    }
    store_controls<G>(surf_out, n, i, law.feedback(f));
}

template <typename S, typename T>
__global__ void __launch_bounds__(LB, 1)
lqg_step_kernel(S* __restrict__ xs /*[12][n]*/, const double* __restrict__ x0 /*[12][n]*/, const double* __restrict__ u0 /*[4][n]*/,
                const double* __restrict__ K /*[16][n]*/, const uint8_t* __restrict__ type, const double* __restrict__ params,
                int n_types, int64_t n, S dt, int n_steps, S* __restrict__ surf_out /*[4][n]*/, int32_t* __restrict__ sat_steps,
                const double* __restrict__ F /*[80][n]*/, const double* __restrict__ sigma /*[8]*/, double* __restrict__ xhat /*[8][n]*/,
                double* __restrict__ du_prev /*[4][n]*/, uint64_t seed, const int32_t* __restrict__ step,
                const double* __restrict__ zin /*[n_steps][8][n] or null*/, int feedback, double* __restrict__ err_est /*[8][n]*/,
                double* __restrict__ err_meas /*[8][n]*/, double* __restrict__ chatter /*[4][n]*/, double* __restrict__ meas_out /*[8][n]*/)
{
    using G = typename GlueOf<S, T>::type;
    constexpr bool FAST = sizeof(T) == 4;
    __shared__ double s_params[FD_MAX_TYPES * FD_NP_STAGED];
    __shared__ G s_words[LW_N * LB];
    __shared__ double s_x0[8 * LB];
    stage_params<FAST>(s_params, params, n_types);
    __syncthreads();
    const int64_t i = int64_t(blockIdx.x) * LB + threadIdx.x;
    if (i >= n) return;
    // the lane's columns are filled first, a few words at a time, before the physics' own registers are loaded
    LaneWords<G, LB> lw(s_words);
    LaneWords<double, LB> lx0(s_x0);
#pragma unroll
    for (int k = 0; k < FD_NKF; ++k) {
        if (k % 16 == 0) asm volatile("" ::: "memory");
        lw.set(k, G(F[int64_t(k) * n + i]));
    }
#pragma unroll
    for (int k = 0; k < FD_NLQK; ++k) lw.set(LW_K + k, G(K[k * n + i]));
#pragma unroll
    for (int k = 0; k < FD_NU; ++k) { lw.set(LW_U0 + k, G(u0[k * n + i])); lw.set(LW_DU + k, G(du_prev[int64_t(k) * n + i])); }
    {
        constexpr int W[8] = { FD_X_U, FD_X_W, FD_X_Q, FD_X_PITCH, FD_X_V, FD_X_P, FD_X_R, FD_X_ROLL };
#pragma unroll
        for (int j = 0; j < 8; ++j) { lx0.set(j, x0[W[j] * n + i]); lw.set(LW_XHAT + j, G(xhat[int64_t(j) * n + i])); }
    }
    // the law of lqr_step_kernel, rebuilt from LDS where it is needed
    auto the_law = [&]() -> LqrLaw<G> {
        LqrLaw<G> law;
#pragma unroll
        for (int k = 0; k < FD_NLQK; ++k) law.k[k] = lw.get(LW_K + k);
#pragma unroll
        for (int k = 0; k < FD_NU; ++k) law.u0[k] = lw.get(LW_U0 + k);
#pragma unroll
        for (int j = 0; j < 8; ++j) law.x0[j] = lx0.get(j);
        return law;
    };
    S x[FD_NX];
#pragma unroll
    for (int k = 0; k < FD_NX; ++k) x[k] = xs[k * n + i];
    asm volatile("" ::: "memory");
    const double* blk = s_params + lane_type(type, i, n_types) * FD_NP_STAGED;
    Params<T> P; P.load(blk);
    Limits<S> Lm; Lm.load(blk);
    const uint32_t step0 = step ? uint32_t(*step) : 0u;
    Surfaces<G> surf{ G(0), G(0), G(0), G(0) };
    int sat = 0;
    // the accumulators (err_est 8, err_meas 8, chatter 4) continue from what the caller holds.  The fp32 instantiations have
    // the registers for them; the f64 instantiation has none, and adds to the caller's words in global memory step by step.
    constexpr bool ACC_REGS = FAST;
    double acc[ACC_REGS ? 16 + FD_NU : 1];
    if constexpr (ACC_REGS) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            acc[k] = err_est ? err_est[int64_t(k) * n + i] : 0.0;
            acc[8 + k] = err_meas ? err_meas[int64_t(k) * n + i] : 0.0;
        }
#pragma unroll
        for (int k = 0; k < FD_NU; ++k) acc[16 + k] = chatter ? chatter[int64_t(k) * n + i] : 0.0;
    }
    auto add_square = [&](int k, double* __restrict__ words, int row, double t) {
#pragma clang fp contract(off)
        if constexpr (ACC_REGS) acc[k] = acc[k] + t * t;
        else if (words) words[int64_t(row) * n + i] = words[int64_t(row) * n + i] + t * t;
    };

    // one control step: measure, estimate, feed back, account.  Returns the unclipped controls (Controls::set clips).
    auto control = [&](int s) -> Surfaces<G> {
#pragma clang fp contract(off)
        // the filter words never change, and a compiler that sees it hoists their LDS loads out of the step loop into
        // registers that then live across the RK4 (396 spilled words in the f64 instantiation): they are re-read every step
        asm volatile("" ::: "memory");
        const LqrLaw<G> law = the_law();
        G d[8], z[8], y[8], xh[8], du[FD_NU];
        law.delta(x, d);
#pragma unroll
        for (int j = 0; j < 8; ++j) xh[j] = lw.get(LW_XHAT + j);
#pragma unroll
        for (int k = 0; k < FD_NU; ++k) du[k] = lw.get(LW_DU + k);
        if (zin) {
#pragma unroll
            for (int j = 0; j < 8; ++j) z[j] = G(zin[(int64_t(s) * 8 + j) * n + i]);
        } else {
            lqg_normals<G>(seed, i, step0 + uint32_t(s) + 1u, z);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) y[j] = d[j] + G(sigma[j]) * z[j];
        kalman_update<G>(lw, y, du, xh);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const double ee = double(xh[j] - d[j]), em = double(y[j] - d[j]);
            add_square(j, err_est, j, ee);
            add_square(8 + j, err_meas, j, em);
            if (meas_out) meas_out[int64_t(j) * n + i] = double(y[j]);
            lw.set(LW_XHAT + j, xh[j]);
        }
        const Surfaces<G> u = feedback == FD_LQG_TRUTH ? law.feedback(d) : (feedback == FD_LQG_MEASUREMENT ? law.feedback(y) : law.feedback(xh));
        sat += any_clipped(u) ? 1 : 0;
        const G c[FD_NU] = { clipv<G>(u.elevator, G(-1), G(1)), clipv<G>(u.aileron, G(-1), G(1)), clipv<G>(u.rudder, G(-1), G(1)),
                             clipv<G>(u.throttle, G(0), G(1)) };
        static_assert(FD_U_ELEVATOR == 0 && FD_U_AILERON == 1 && FD_U_RUDDER == 2 && FD_U_THROTTLE == 3, "control order");
#pragma unroll
        for (int k = 0; k < FD_NU; ++k) {
            const double t = double(c[k] - (law.u0[k] + du[k]));
            add_square(16 + k, chatter, k, t);
            lw.set(LW_DU + k, c[k] - law.u0[k]);
        }
        return u;
    };

    if constexpr (FAST) {
        FastRK f;
        f.init(x);
        const float hdt = float(S(0.5) * dt), fdt = float(dt), dt6 = float(dt / S(6));
        for (int s = 0; s < n_steps; ++s) {
            surf = control(s);
            Controls<T> C;
            C.set(P, surf.elevator, surf.aileron, surf.rudder, surf.throttle);
            rk4_fast_step<S, false>(P, Lm, C, x, f, hdt, fdt, dt6);
        }
    } else {
        for (int s = 0; s < n_steps; ++s) {
            surf = control(s);
            Controls<T> C;
            C.set(P, surf.elevator, surf.aileron, surf.rudder, surf.throttle);
            rk4_substeps<S, T>(P, Lm, C, x, dt, 1);
        }
    }
    // the addresses of the stores below are recomputed from a lane index the compiler cannot equate with `i`: kept from the
    // loads at the top they would live across the step loop, where the f64 instantiation has no register left for them
    int64_t ie = i;
    asm volatile("" : "+v"(ie));
#pragma unroll
    for (int k = 0; k < FD_NX; ++k) xs[k * n + ie] = x[k];
    if (sat_steps) sat_steps[ie] += sat;
    if constexpr (ACC_REGS) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (err_est) err_est[int64_t(k) * n + ie] = acc[k];
            if (err_meas) err_meas[int64_t(k) * n + ie] = acc[8 + k];
        }
#pragma unroll
        for (int k = 0; k < FD_NU; ++k)
            if (chatter) chatter[int64_t(k) * n + ie] = acc[16 + k];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) xhat[int64_t(j) * n + ie] = double(lw.get(LW_XHAT + j));
#pragma unroll
    for (int k = 0; k < FD_NU; ++k) du_prev[int64_t(k) * n + ie] = double(lw.get(LW_DU + k));
    if (surf_out) store_controls<G>(surf_out, n, ie, surf);
}

template <typename S, typename T>
int launch_step(S* x, const double* x0, const double* u0, const double* K, const uint8_t* type, const double* params, int n_types,
                int64_t n, double dt, int n_steps, S* surf_out, int32_t* sat_steps, const double* F, const double* sigma, double* xhat,
                double* du_prev, uint64_t seed, const int32_t* step, const double* z, int feedback, double* err_est, double* err_meas,
                double* chatter, double* meas_out, void* stream)
{
    static_assert(LB >= FD_MAX_TYPES * Params<double>::FD_ND_LANES, "stage_params needs that many threads");
    if (n_steps < 0) return FDYN_ERR_BAD_SIZE;
    FD_CHECK_FLEET(n, n_types, LB)
    if (!x || !x0 || !u0 || !K || !params || !F || !sigma || !xhat || !du_prev) return FDYN_ERR_NULL;
    if (feedback != FD_LQG_ESTIMATE && feedback != FD_LQG_MEASUREMENT && feedback != FD_LQG_TRUTH) return FDYN_ERR_BAD_SIZE;
    if (bad_dt(dt)) return FDYN_ERR_BAD_DT;
    if (n_steps == 0) {
        if (!surf_out) return FDYN_OK;
        return launch<256>(lqg_controls_kernel<S, T>, n, stream, (const S*)x, x0, u0, K, n, (const double*)xhat, feedback, surf_out);
    }
    return launch<LB>(lqg_step_kernel<S, T>, n, stream, x, x0, u0, K, type, params, n_types, n, S(dt), n_steps, surf_out,
                       sat_steps, F, sigma, xhat, du_prev, seed, step, z, feedback, err_est, err_meas, chatter, meas_out);
}

}  // namespace

extern "C" {

int fdyn_kf_design(const double* A, const double* B, double dt, const double* noise, int noise_per_lane, int64_t n, double* F,
                   double* residual, int32_t* iters, int32_t* status, void* stream)
{
    FD_CHECK_FLEET(n, 1, TB)
    if (!A || !B || !noise || !F || !residual || !iters || !status) return FDYN_ERR_NULL;
    return launch<TB>(kf_design_kernel, n, stream, A, B, dt, noise, noise_per_lane, n, F, residual, iters, status);
}

#define FD_LQG_STEP(NAME, S, T)                                                                                                    \
    int NAME(S* x, const double* x0, const double* u0, const double* K, const uint8_t* type, const double* params, int n_types,   \
             int64_t n, double dt, int n_steps, S* surf_out, int32_t* sat_steps, const double* F, const double* sigma,            \
             double* xhat, double* du_prev, uint64_t seed, const int32_t* step, const double* z, int feedback, double* err_est,   \
             double* err_meas, double* chatter, double* meas_out, void* stream)                                                    \
    {                                                                                                                              \
        return launch_step<S, T>(x, x0, u0, K, type, params, n_types, n, dt, n_steps, surf_out, sat_steps, F, sigma, xhat,       \
                                 du_prev, seed, step, z, feedback, err_est, err_meas, chatter, meas_out, stream);                  \
    }
FD_LQG_STEP(fdyn_lqg_step_f64, double, double)
FD_LQG_STEP(fdyn_lqg_step_mixed, double, float)
FD_LQG_STEP(fdyn_lqg_step_f32, float, float)
#undef FD_LQG_STEP

}  // extern "C"

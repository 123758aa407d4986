// lqr_kernels.hip -- gain-scheduled LQR for whole fleets, gfx950: the design step between fdyn_linearize and flight.
//
// fdyn_lqr_design   docs/control_hierarchy_design.tex:282 derives the PID structure from "linearised rate dynamics near trim" and
//                   stops there.  Here each aircraft's own A, B (fdyn_linearize) are cut into the longitudinal and the lateral
//                   4-state / 2-control block and each block's continuous Riccati equation is solved in fp64, one lane per
//                   aircraft, by the structure-preserving doubling algorithm: K = R^-1 b^T X per block.
// fdyn_lqr_step_*   n_steps x { u = u0 - K (x - x0) -> Controls::set (clips as set_controls does) -> one RK4 of dt }, one launch,
//                   through the steppers of fdyn_core.hpp exactly as agent_step_kernel calls them.
//
// Registers, not scratch (as trim_kernels.hip): every matrix is a 4 x 4 of named words indexed by compile-time constants; the
// two blocks go through ONE rolled loop, so the solver is inlined once, and what depends on the block -- which rows of A and B,
// which weights, which half of K -- is a scalar offset into global memory or a select.  64-thread workgroups: 65 536 aircraft
// are 1024 waves, one per SIMD, each with the whole register file.
// Shared with the other fleet files: the 4 x 4 matrix type, its products, inverse and L D L^T test are fdyn_riccati.hpp's
// (kf_kernels.hip solves the filter equation with them), on fdyn_dense.hpp's elimination (the one trim_kernels.hip solves its
// Newton step with); parameter staging, lane type, glue type, entry checks and launch are fdyn_fleet.hpp's.  The doubling loop
// below is also fdyn_riccati.hpp's riccati_doubling, word for word: called from there this kernel compiled to 44 more
// instructions and its time left the spread of three runs of the listing below (+1 %), so it keeps the loop in line and
// the file compiles to the ISA it had before the headers existed.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "fdyn_fleet.hpp"
#include "fdyn_riccati.hpp"
#include "fdyn_lqr_law.hpp"

using namespace fdyn;

namespace {

constexpr int TB = 64;                   // design: threads per workgroup
constexpr int SB = 256;                  // step: threads per workgroup, as every fleet kernel of fdyn_kernels.hip
constexpr int NB = RIC_N;                // states per block
constexpr double LQR_RES_MAX = RIC_RES_MAX;

__global__ void __launch_bounds__(TB)
lqr_design_kernel(const double* __restrict__ A /*[144][n]*/, const double* __restrict__ B /*[48][n]*/,
                  const double* __restrict__ weights /*[12] or [12][n]*/, int weights_per_lane, int64_t n,
                  double* __restrict__ K /*[16][n]*/, double* __restrict__ residual, int32_t* __restrict__ iters,
                  int32_t* __restrict__ status)
{
#pragma clang fp contract(off)
    const int64_t i = int64_t(blockIdx.x) * TB + threadIdx.x;
    if (i >= n) return;
    double w[FD_NLQW];
    bool bad = false;
#pragma unroll
    for (int k = 0; k < FD_NLQW; ++k) {
        w[k] = weights_per_lane ? weights[k * n + i] : weights[k];
        bad = bad || !(::isfinite(w[k]) && w[k] > 0.0);
    }
    double Kall[FD_NLQK];
#pragma unroll
    for (int k = 0; k < FD_NLQK; ++k) Kall[k] = 0.0;
    double res = 0.0;
    int it_max = 0, st = 0;

#pragma unroll 1
    for (int blk = 0; blk < 2; ++blk) {
        // rows of the block inside the 12 states and its two controls: scalars, the loads below take them as offsets
        const int s0 = blk ? FD_X_V : FD_X_U, s1 = blk ? FD_X_P : FD_X_W, s2 = blk ? FD_X_R : FD_X_Q, s3 = blk ? FD_X_ROLL : FD_X_PITCH;
        const int c0 = blk ? FD_U_AILERON : FD_U_ELEVATOR, c1 = blk ? FD_U_RUDDER : FD_U_THROTTLE;
        const int sr[NB] = { s0, s1, s2, s3 };
        M4 a;
        double b[NB][2], q[NB], rinv[2];
        bool fin = true;
#pragma unroll
        for (int r = 0; r < NB; ++r) {
#pragma unroll
            for (int c = 0; c < NB; ++c) { a.v[r][c] = A[int64_t(sr[r] * FD_NX + sr[c]) * n + i]; fin = fin && ::isfinite(a.v[r][c]); }
            b[r][0] = B[int64_t(sr[r] * FD_NU + c0) * n + i];
            b[r][1] = B[int64_t(sr[r] * FD_NU + c1) * n + i];
            fin = fin && ::isfinite(b[r][0]) && ::isfinite(b[r][1]);
            q[r] = blk ? w[NB + r] : w[r];
        }
        rinv[0] = 1.0 / (blk ? w[10] : w[8]);
        rinv[1] = 1.0 / (blk ? w[11] : w[9]);
        bad = bad || !fin;
        if (bad) continue;                                       // BAD_INPUT (weights, or either block): nothing is solved

        double bs[NB][2];
        M4 G;
#pragma unroll
        for (int r = 0; r < NB; ++r) { bs[r][0] = b[r][0] * rinv[0]; bs[r][1] = b[r][1] * rinv[1]; }
#pragma unroll
        for (int r = 0; r < NB; ++r)
#pragma unroll
            for (int c = 0; c < NB; ++c) G.v[r][c] = bs[r][0] * b[c][0] + bs[r][1] * b[c][1];
        double gamma = 1.0;
#pragma unroll
        for (int r = 0; r < NB; ++r) {
            double rs = ::fabs(a.v[r][0]);
#pragma unroll
            for (int c = 1; c < NB; ++c) rs = rs + ::fabs(a.v[r][c]);
            gamma = rs > gamma ? rs : gamma;
        }
        const double g2 = 2.0 * gamma;
        M4 ag = a, agi, S1, W, Wi, Ak, Gk, Hk, T0;
#pragma unroll
        for (int r = 0; r < NB; ++r) ag.v[r][r] = a.v[r][r] - gamma;
        bool failed = !inverse(ag, agi);
        S1 = mul<false, false>(agi, G);
#pragma unroll
        for (int r = 0; r < NB; ++r)
#pragma unroll
            for (int c = 0; c < NB; ++c) W.v[r][c] = ag.v[c][r] + q[r] * S1.v[r][c];
        failed = !inverse(W, Wi) || failed;
#pragma unroll
        for (int r = 0; r < NB; ++r)
#pragma unroll
            for (int c = 0; c < NB; ++c) { Ak.v[r][c] = (r == c ? 1.0 : 0.0) + g2 * Wi.v[c][r]; T0.v[r][c] = q[r] * agi.v[r][c]; }
        Gk = mul<false, false>(S1, Wi);
        Hk = mul<false, false>(Wi, T0);
#pragma unroll
        for (int r = 0; r < NB; ++r)
#pragma unroll
            for (int c = 0; c < NB; ++c) { Gk.v[r][c] = g2 * Gk.v[r][c]; Hk.v[r][c] = g2 * Hk.v[r][c]; }

        int it = 0;
        bool converged = false;
#pragma unroll 1
        while (!failed && !converged && it < RIC_MAX_ITERS) {
            M4 Mi, IGH = mul<false, false>(Gk, Hk);
#pragma unroll
            for (int r = 0; r < NB; ++r) IGH.v[r][r] = 1.0 + IGH.v[r][r];
            if (!inverse(IGH, Mi)) { failed = true; break; }
            const M4 AM = mul<false, false>(Ak, Mi), MA = mul<false, false>(Mi, Ak);
            const M4 A1 = mul<false, false>(AM, Ak);
            const M4 dG = mul<false, true>(mul<false, false>(AM, Gk), Ak);
            const M4 dH = mul<true, false>(Ak, mul<false, false>(Hk, MA));
            M4 dif;
#pragma unroll
            for (int r = 0; r < NB; ++r)
#pragma unroll
                for (int c = 0; c < NB; ++c) {
                    const double h1 = Hk.v[r][c] + dH.v[r][c];
                    dif.v[r][c] = h1 - Hk.v[r][c];
                    Hk.v[r][c] = h1;
                    Gk.v[r][c] = Gk.v[r][c] + dG.v[r][c];
                }
            Ak = A1;
            ++it;
            const double hmax = max_abs(Hk.v), diff = max_abs(dif.v);
            if (!(::isfinite(hmax) && ::isfinite(diff))) { failed = true; break; }
            converged = diff <= RIC_TOL * (hmax > 1.0 ? hmax : 1.0);
        }

        M4 X;
#pragma unroll
        for (int r = 0; r < NB; ++r)
#pragma unroll
            for (int c = 0; c < NB; ++c) X.v[r][c] = 0.5 * (Hk.v[r][c] + Hk.v[c][r]);
        // K = R^-1 b^T X
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int c = 0; c < NB; ++c) {
                double s = bs[0][j] * X.v[0][c];
#pragma unroll
                for (int r = 1; r < NB; ++r) s = s + bs[r][j] * X.v[r][c];
                Kall[j * NB + c] = blk ? Kall[j * NB + c] : s;
                Kall[2 * NB + j * NB + c] = blk ? s : Kall[2 * NB + j * NB + c];
            }
        // residual of the Riccati equation at X
        const M4 AtX = mul<true, false>(a, X), Xa = mul<false, false>(X, a), XGX = mul<false, false>(mul<false, false>(X, G), X);
        M4 R;
#pragma unroll
        for (int r = 0; r < NB; ++r)
#pragma unroll
            for (int c = 0; c < NB; ++c) {
                const double t = (AtX.v[r][c] + Xa.v[r][c]) - XGX.v[r][c];
                R.v[r][c] = r == c ? t + q[r] : t;
            }
        const double xmax = max_abs(X.v);
        const double bres = max_abs(R.v) / (xmax > 1.0 ? xmax : (xmax == xmax ? 1.0 : xmax));
        res = nan_max(res, bres);
        it_max = it > it_max ? it : it_max;
        if (failed || !converged) st |= FD_LQR_NOT_CONVERGED;
        if (!positive_definite(X) || !(bres <= LQR_RES_MAX)) st |= FD_LQR_NO_CERTIFICATE;
    }

    if (bad) { st = FD_LQR_BAD_INPUT; res = __builtin_nan(""); it_max = 0; }
#pragma unroll
    for (int k = 0; k < FD_NLQK; ++k) K[k * n + i] = st ? 0.0 : Kall[k];
    residual[i] = res;
    iters[i] = it_max;
    status[i] = st;
}

// ---- the closed loop (the law u = u0 - K delta is fdyn_lqr_law.hpp's: kf_kernels.hip feeds it an estimate) ---------------------------
template <typename S, typename T>
__global__ void __launch_bounds__(SB, 1)
lqr_step_kernel(S* __restrict__ xs /*[12][n]*/, const double* __restrict__ x0 /*[12][n]*/, const double* __restrict__ u0 /*[4][n]*/,
                const double* __restrict__ K /*[16][n]*/, const uint8_t* __restrict__ type, const double* __restrict__ params,
                int n_types, int64_t n, S dt, int n_steps, S* __restrict__ surf_out /*[4][n]*/, int32_t* __restrict__ sat_steps)
{
    using G = typename GlueOf<S, T>::type;
    constexpr bool FAST = sizeof(T) == 4;
    __shared__ double s_params[FD_MAX_TYPES * FD_NP_STAGED];
    stage_params<FAST>(s_params, params, n_types);
    __syncthreads();
    const int64_t i = int64_t(blockIdx.x) * SB + threadIdx.x;
    if (i >= n) return;
    const double* blk = s_params + lane_type(type, i, n_types) * FD_NP_STAGED;
    Params<T> P; P.load(blk);
    Limits<S> Lm; Lm.load(blk);
    LqrLaw<G> law;
#pragma unroll
    for (int k = 0; k < FD_NLQK; ++k) law.k[k] = G(K[k * n + i]);
#pragma unroll
    for (int k = 0; k < FD_NU; ++k) law.u0[k] = G(u0[k * n + i]);
    {
        constexpr int W[8] = { FD_X_U, FD_X_W, FD_X_Q, FD_X_PITCH, FD_X_V, FD_X_P, FD_X_R, FD_X_ROLL };
#pragma unroll
        for (int j = 0; j < 8; ++j) law.x0[j] = x0[W[j] * n + i];
    }
    S x[FD_NX];
#pragma unroll
    for (int k = 0; k < FD_NX; ++k) x[k] = xs[k * n + i];
    Surfaces<G> surf{ G(0), G(0), G(0), G(0) };
    const int iters = n_steps > 0 ? n_steps : 1;
    int sat = 0;
    if constexpr (FAST) {
        FastRK f;
        f.init(x);
        const float hdt = float(S(0.5) * dt), fdt = float(dt), dt6 = float(dt / S(6));
        for (int s = 0; s < iters; ++s) {
            surf = law(x);
            if (n_steps > 0) {
                sat += any_clipped(surf) ? 1 : 0;
                Controls<T> C;
                C.set(P, surf.elevator, surf.aileron, surf.rudder, surf.throttle);
                rk4_fast_step<S, false>(P, Lm, C, x, f, hdt, fdt, dt6);
            }
        }
    } else {
        for (int s = 0; s < iters; ++s) {
            surf = law(x);
            if (n_steps > 0) {
                sat += any_clipped(surf) ? 1 : 0;
                Controls<T> C;
                C.set(P, surf.elevator, surf.aileron, surf.rudder, surf.throttle);
                rk4_substeps<S, T>(P, Lm, C, x, dt, 1);
            }
        }
    }
    if (n_steps > 0) {
#pragma unroll
        for (int k = 0; k < FD_NX; ++k) xs[k * n + i] = x[k];
        if (sat_steps) sat_steps[i] += sat;
    }
    if (surf_out) {                                              // the controls as applied: after set_controls' clip
        surf_out[FD_U_ELEVATOR * n + i] = S(clipv<G>(surf.elevator, G(-1), G(1)));
        surf_out[FD_U_AILERON * n + i] = S(clipv<G>(surf.aileron, G(-1), G(1)));
        surf_out[FD_U_RUDDER * n + i] = S(clipv<G>(surf.rudder, G(-1), G(1)));
        surf_out[FD_U_THROTTLE * n + i] = S(clipv<G>(surf.throttle, G(0), G(1)));
    }
}

template <typename S, typename T>
int launch_step(S* x, const double* x0, const double* u0, const double* K, const uint8_t* type, const double* params, int n_types,
                int64_t n, double dt, int n_steps, S* surf_out, int32_t* sat_steps, void* stream)
{
    if (n_steps < 0) return FDYN_ERR_BAD_SIZE;
    FD_CHECK_FLEET(n, n_types, SB)
    if (!x || !x0 || !u0 || !K || !params) return FDYN_ERR_NULL;
    if (bad_dt(dt)) return FDYN_ERR_BAD_DT;
    return launch<SB>(lqr_step_kernel<S, T>, n, stream, x, x0, u0, K, type, params, n_types, n, S(dt), n_steps, surf_out, sat_steps);
}

}  // namespace

extern "C" {

int fdyn_lqr_design(const double* A, const double* B, const double* weights, int weights_per_lane, int64_t n, double* K,
                    double* residual, int32_t* iters, int32_t* status, void* stream)
{
    FD_CHECK_FLEET(n, 1, TB)
    if (!A || !B || !weights || !K || !residual || !iters || !status) return FDYN_ERR_NULL;
    return launch<TB>(lqr_design_kernel, n, stream, A, B, weights, weights_per_lane, n, K, residual, iters, status);
}

int fdyn_lqr_step_f64(double* x, const double* x0, const double* u0, const double* K, const uint8_t* type, const double* params,
                      int n_types, int64_t n, double dt, int n_steps, double* surf_out, int32_t* sat_steps, void* stream)
{ return launch_step<double, double>(x, x0, u0, K, type, params, n_types, n, dt, n_steps, surf_out, sat_steps, stream); }

int fdyn_lqr_step_mixed(double* x, const double* x0, const double* u0, const double* K, const uint8_t* type, const double* params,
                        int n_types, int64_t n, double dt, int n_steps, double* surf_out, int32_t* sat_steps, void* stream)
{ return launch_step<double, float>(x, x0, u0, K, type, params, n_types, n, dt, n_steps, surf_out, sat_steps, stream); }

int fdyn_lqr_step_f32(float* x, const double* x0, const double* u0, const double* K, const uint8_t* type, const double* params,
                      int n_types, int64_t n, double dt, int n_steps, float* surf_out, int32_t* sat_steps, void* stream)
{ return launch_step<float, float>(x, x0, u0, K, type, params, n_types, n, dt, n_steps, surf_out, sat_steps, stream); }

}  // extern "C"

// trim_kernels.hip -- steady-flight solver and linearisation for whole fleets, gfx950, fp64, one lane per aircraft.
//
// fdyn_trim       docs/6dof_mathematical_formulation.tex:1380-1410 ("trimmed flight": x_dot = 0, "set controls to estimated
//                 trim values") -- the reference states the condition and codes no solver.  Here: Newton on seven unknowns
//                 z = (alpha, theta, phi, de, da, dr, dt) against seven residuals of fdyn::dynamics<double>, per aircraft.
// fdyn_linearize  docs/control_hierarchy_design.tex:282 ("linearised rate dynamics near trim") -- A = d xdot / d x and
//                 B = d xdot / d u by central differences of the same function, at any state.
//
// Both kernels evaluate the equations of motion through fdyn::dynamics<double> unchanged, with the controls NOT clipped
// (Controls<double> filled directly): a clipped control has a zero column in the Jacobian at its bound.  Feasibility is
// reported afterwards (FD_TRIM_*).
//
// Registers, not scratch: the 7 x 7 system, the 12-word states and the perturbed copies are only ever indexed by compile-time
// constants (fully unrolled loops); the loops that stay rolled -- Newton iterations, Jacobian columns, the +- sides of a
// difference -- select their element with compare-and-select chains (the Jacobian's columns wait in per-lane LDS slots).  The rolled column loop also keeps ONE inlined copy of
// the dynamics per use instead of fifteen (each is a few thousand instructions with the fp64 ocml sincos / atan2 / asin).
// 64-thread workgroups: 65 536 aircraft are 1024 waves, one per SIMD of the chip, each with the whole register file.
// Shared with the other fleet files: the Newton step is fdyn_dense.hpp's elimination (gauss_solve<7, 1>; lqr_kernels.hip inverts
// with the same one); parameter staging, lane type and launch are fdyn_fleet.hpp's.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "fdyn_fleet.hpp"
#include "fdyn_dense.hpp"

using namespace fdyn;

namespace {

constexpr int TB = 64;                   // threads per workgroup
constexpr int NZ = 7;                    // unknowns of the trim problem
constexpr int TRIM_MAX_ITERS = 20;
constexpr double TRIM_FD_STEP = 1e-6, TRIM_TOL = 1e-12, TRIM_PIVOT_REL = 1e-14;
constexpr double LIN_STEP = 1e-5;

static_assert(FD_MAX_TYPES * Params<double>::FD_ND_LANES <= TB, "stage_params: one derive lane per word and type");

FD_DEV void lane_params(Params<double>& P, const double* s_params, const uint8_t* __restrict__ type,
                        const double* __restrict__ scales, int n_types, int64_t n, int64_t i)
{
    P.load(s_params + lane_type(type, i, n_types) * FD_NP_STAGED);
    if (scales) scale_params<double>(P, scales[0 * n + i], scales[1 * n + i], scales[2 * n + i], scales[3 * n + i], scales[4 * n + i]);
}

// normalised controls (elevator, aileron, rudder, throttle) -> Controls<double>, no clip
FD_DEV Controls<double> raw_controls(const Params<double>& P, double de, double da, double dr, double dt)
{
    Controls<double> C{};
    C.de_rad = de * P.max_de; C.da_rad = da * P.max_da; C.dr_rad = dr * P.max_dr; C.throttle = dt;
    return C;
}

struct TrimSpec { double V, gamma, psi_dot, h, psi0; };

// the state a set of unknowns stands for
FD_DEV void trim_state(const TrimSpec& s, const double (&z)[NZ], double (&x)[FD_NX])
{
#pragma clang fp contract(off)
    double sa, ca, st, ct, sp, cp;
    ::sincos(z[0], &sa, &ca);
    ::sincos(z[1], &st, &ct);
    ::sincos(z[2], &sp, &cp);
    x[FD_X_N] = 0.0; x[FD_X_E] = 0.0; x[FD_X_D] = -s.h;
    x[FD_X_U] = s.V * ca; x[FD_X_V] = 0.0; x[FD_X_W] = s.V * sa;
    x[FD_X_ROLL] = z[2]; x[FD_X_PITCH] = z[1]; x[FD_X_YAW] = s.psi0;
    x[FD_X_P] = -s.psi_dot * st; x[FD_X_Q] = s.psi_dot * sp * ct; x[FD_X_R] = s.psi_dot * cp * ct;
}

// F(z) = (u_dot, v_dot, w_dot, p_dot, q_dot, r_dot, D_dot + V sin gamma)
FD_DEV void trim_residual(const Params<double>& P, const TrimSpec& s, double v_sin_gamma, const double (&z)[NZ], double (&F)[NZ])
{
#pragma clang fp contract(off)
    double x[FD_NX], xd[FD_NX];
    trim_state(s, z, x);
    const Controls<double> C = raw_controls(P, z[3], z[4], z[5], z[6]);
    dynamics<double>(P, C, x, xd);
    F[0] = xd[FD_X_U]; F[1] = xd[FD_X_V]; F[2] = xd[FD_X_W];
    F[3] = xd[FD_X_P]; F[4] = xd[FD_X_Q]; F[5] = xd[FD_X_R];
    F[6] = xd[FD_X_D] + v_sin_gamma;
}

__global__ void __launch_bounds__(TB)
trim_kernel(const double* __restrict__ spec /*[5][n]*/, const uint8_t* __restrict__ type, const double* __restrict__ scales /*[5][n]*/,
            const double* __restrict__ params, int n_types, int64_t n, double* __restrict__ x0 /*[12][n]*/,
            double* __restrict__ u0 /*[4][n]*/, double* __restrict__ residual, int32_t* __restrict__ iters,
            int32_t* __restrict__ status)
{
#pragma clang fp contract(off)
    __shared__ double s_params[FD_MAX_TYPES * FD_NP_STAGED];
    // the Jacobian is built one column per pass of a rolled loop: each lane parks its columns in its own LDS slots (the column
    // index is a run-time value there, where it costs nothing) and pulls the finished matrix into registers for the elimination,
    // so the 98 registers of J are not live across the fourteen evaluations that fill it.  No other lane reads these words.
    __shared__ double s_J[NZ * NZ * TB];
    const int64_t i = int64_t(blockIdx.x) * TB + threadIdx.x;
    const bool on = i < n;
    TrimSpec s{ 1.0, 0.0, 0.0, 0.0, 0.0 };
    if (on) { s.V = spec[0 * n + i]; s.gamma = spec[1 * n + i]; s.psi_dot = spec[2 * n + i]; s.h = spec[3 * n + i]; s.psi0 = spec[4 * n + i]; }
    stage_params<false>(s_params, params, n_types);
    __syncthreads();
    if (!on) return;
    Params<double> P;
    lane_params(P, s_params, type, scales, n_types, n, i);

    const bool bad_spec = !(::isfinite(s.V) && ::isfinite(s.gamma) && ::isfinite(s.psi_dot) && ::isfinite(s.h) && ::isfinite(s.psi0)
                            && s.V > 0.0);
    const double v_sin_gamma = s.V * ::sin(s.gamma);
    double z[NZ] = { 0.05, 0.05 + s.gamma, ::atan(s.V * s.psi_dot / P.g), 0.0, 0.0, 0.0, 0.5 };
    double F[NZ], res = __builtin_nan("");
    int it = 0;
    bool failed = false, converged = false;
    if (!bad_spec) {
#pragma unroll 1
        for (;;) {
            trim_residual(P, s, v_sin_gamma, z, F);
            res = max_abs(F);
            if (converged || it == TRIM_MAX_ITERS) break;
            if (!::isfinite(res)) { failed = true; break; }
#pragma unroll 1
            for (int j = 0; j < NZ; ++j) {
                double zp[NZ], zm[NZ], Fp[NZ] = {}, Fm[NZ] = {};
#pragma unroll
                for (int k = 0; k < NZ; ++k) { zp[k] = k == j ? z[k] + TRIM_FD_STEP : z[k]; zm[k] = k == j ? z[k] - TRIM_FD_STEP : z[k]; }
                double step = 0.0;
#pragma unroll
                for (int k = 0; k < NZ; ++k) step = k == j ? zp[k] - zm[k] : step;
#pragma unroll 1
                for (int side = 0; side < 2; ++side) {
                    double zs[NZ], Fs[NZ];
#pragma unroll
                    for (int k = 0; k < NZ; ++k) zs[k] = side ? zm[k] : zp[k];
                    trim_residual(P, s, v_sin_gamma, zs, Fs);
#pragma unroll
                    for (int k = 0; k < NZ; ++k) { Fp[k] = side ? Fp[k] : Fs[k]; Fm[k] = Fs[k]; }
                }
#pragma unroll
                for (int r = 0; r < NZ; ++r) s_J[((r * NZ + j) * TB) + threadIdx.x] = (Fp[r] - Fm[r]) / step;
            }
            double J[NZ][NZ], rhs[NZ][1], dz[NZ][1];
#pragma unroll
            for (int r = 0; r < NZ; ++r)
#pragma unroll
                for (int c = 0; c < NZ; ++c) J[r][c] = s_J[((r * NZ + c) * TB) + threadIdx.x];
#pragma unroll
            for (int k = 0; k < NZ; ++k) rhs[k][0] = -F[k];
            if (!gauss_solve<NZ, 1>(J, rhs, dz, TRIM_PIVOT_REL)) { failed = true; break; }
#pragma unroll
            for (int k = 0; k < NZ; ++k) z[k] = z[k] + dz[k][0];
            ++it;
            const double step_norm = max_abs(dz);
            if (!::isfinite(step_norm)) { failed = true; break; }
            converged = step_norm < TRIM_TOL;
        }
    }

    int st = 0;
    if (bad_spec) st = FD_TRIM_BAD_SPEC;
    else {
        if (failed || !converged || !::isfinite(res)) st |= FD_TRIM_NOT_CONVERGED;
        if (::fabs(z[3]) > 1.0 || ::fabs(z[4]) > 1.0 || ::fabs(z[5]) > 1.0 || z[6] < 0.0 || z[6] > 1.0) st |= FD_TRIM_CONTROL_RANGE;
        if (::fabs(z[0]) >= P.max_alpha) st |= FD_TRIM_ALPHA_LIMIT;
        if (::fabs(z[1]) >= P.max_pitch) st |= FD_TRIM_PITCH_LIMIT;
    }
    double x[FD_NX];
    trim_state(s, z, x);
#pragma unroll
    for (int k = 0; k < FD_NX; ++k) x0[k * n + i] = x[k];
    u0[FD_U_ELEVATOR * n + i] = z[3]; u0[FD_U_AILERON * n + i] = z[4]; u0[FD_U_RUDDER * n + i] = z[5]; u0[FD_U_THROTTLE * n + i] = z[6];
    residual[i] = res;
    iters[i] = it;
    status[i] = st;
}

// A[12 i + j][n] = d xdot_i / d x_j, B[4 i + k][n] = d xdot_i / d u_k: 16 columns x 2 sides = 32 evaluations
template <typename S>
__global__ void __launch_bounds__(TB)
linearize_kernel(const S* __restrict__ xs /*[12][n]*/, const S* __restrict__ us /*[4][n]*/, const uint8_t* __restrict__ type,
                 const double* __restrict__ scales, const double* __restrict__ params, int n_types, int64_t n,
                 double* __restrict__ A /*[144][n]*/, double* __restrict__ B /*[48][n]*/)
{
#pragma clang fp contract(off)
    __shared__ double s_params[FD_MAX_TYPES * FD_NP_STAGED];
    const int64_t i = int64_t(blockIdx.x) * TB + threadIdx.x;
    const bool on = i < n;
    constexpr int NV = FD_NX + FD_NU;
    double v[NV];                                             // the 12 state words, then the 4 normalised controls
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = 0.0;
    if (on) {
#pragma unroll
        for (int k = 0; k < FD_NX; ++k) v[k] = double(xs[k * n + i]);
#pragma unroll
        for (int k = 0; k < FD_NU; ++k) v[FD_NX + k] = double(us[k * n + i]);
    }
    stage_params<false>(s_params, params, n_types);
    __syncthreads();
    if (!on) return;
    Params<double> P;
    lane_params(P, s_params, type, scales, n_types, n, i);

#pragma unroll 1
    for (int j = 0; j < NV; ++j) {
        double vj = 0.0;
#pragma unroll
        for (int k = 0; k < NV; ++k) vj = k == j ? v[k] : vj;
        const double a = ::fabs(vj);
        const double h = j < FD_NX ? LIN_STEP * (a > 1.0 ? a : 1.0) : LIN_STEP;
        const double hi = vj + h, lo = vj - h;
        const double step = hi - lo;
        double dp[FD_NX] = {}, dm[FD_NX] = {};
#pragma unroll 1
        for (int side = 0; side < 2; ++side) {
            double x[FD_NX], xd[FD_NX], u[FD_NU];
            const double put = side ? lo : hi;
#pragma unroll
            for (int k = 0; k < FD_NX; ++k) x[k] = k == j ? put : v[k];
#pragma unroll
            for (int k = 0; k < FD_NU; ++k) u[k] = FD_NX + k == j ? put : v[FD_NX + k];
            const Controls<double> C = raw_controls(P, u[FD_U_ELEVATOR], u[FD_U_AILERON], u[FD_U_RUDDER], u[FD_U_THROTTLE]);
            dynamics<double>(P, C, x, xd);
#pragma unroll
            for (int k = 0; k < FD_NX; ++k) { dp[k] = side ? dp[k] : xd[k]; dm[k] = xd[k]; }
        }
        // column j of A (stride 12) or column j - 12 of B (stride 4): the row offset is a run-time scalar, the lane the fast index
        double* __restrict__ dst = j < FD_NX ? A + int64_t(j) * n + i : B + int64_t(j - FD_NX) * n + i;
        const int64_t row_stride = (j < FD_NX ? FD_NX : FD_NU) * n;
#pragma unroll
        for (int k = 0; k < FD_NX; ++k) dst[k * row_stride] = (dp[k] - dm[k]) / step;
    }
}

template <typename S>
int launch_linearize(const void* x, const void* u, const uint8_t* type, const double* scales, const double* params, int n_types,
                     int64_t n, double* A, double* B, void* stream)
{
    return launch<TB>(linearize_kernel<S>, n, stream, static_cast<const S*>(x), static_cast<const S*>(u), type, scales, params, n_types,
                      n, A, B);
}

}  // namespace

extern "C" {

int fdyn_trim(const double* spec, const uint8_t* type, const double* scales, const double* params, int n_types, int64_t n,
              double* x0, double* u0, double* residual, int32_t* iters, int32_t* status, void* stream)
{
    if (n < 0) return FDYN_ERR_BAD_SIZE;
    if (n_types < 1 || n_types > FD_MAX_TYPES) return FDYN_ERR_BAD_TYPES;
    if (n == 0) return FDYN_OK;
    if (!spec || !params || !x0 || !u0 || !residual || !iters || !status) return FDYN_ERR_NULL;
    return launch<TB>(trim_kernel, n, stream, spec, type, scales, params, n_types, n, x0, u0, residual, iters, status);
}

int fdyn_linearize(const void* x, const void* u, int xu_f32, const uint8_t* type, const double* scales, const double* params,
                   int n_types, int64_t n, double* A, double* B, void* stream)
{
    if (n < 0) return FDYN_ERR_BAD_SIZE;
    if (n_types < 1 || n_types > FD_MAX_TYPES) return FDYN_ERR_BAD_TYPES;
    if (n == 0) return FDYN_OK;
    if (!x || !u || !params || !A || !B) return FDYN_ERR_NULL;
    return xu_f32 ? launch_linearize<float>(x, u, type, scales, params, n_types, n, A, B, stream)
                  : launch_linearize<double>(x, u, type, scales, params, n_types, n, A, B, stream);
}

}  // extern "C"

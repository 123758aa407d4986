// fdyn_kalman_n.hpp -- the steady-state Kalman design of kf_design_kernel (kf_kernels.hip) for a block of any size N, every state
// measured (C = I): the scaled Taylor series of the matrix exponential and of its integral, then the filter Riccati equation
// P = Phi (P - P (P + V)^-1 P) Phi^T + W through fdyn_riccati_n.hpp's doubling loop, inverse and L D L^T test.  servo_kernels.hip
// compiles it at N = 5: the five physical states of each augmented block of the LQ servo (include/fdyn_servo_lqg.h).
//
// Plain C++ templates, __host__ __device__ under hipcc, so the host check (tests/host/servo_lqg_check.cpp) runs the very code the
// kernel compiles.  kf_design_kernel's arithmetic word for word at block size N: no contraction, one rounding per operation,
// products summed k = 0..N-1 in that order, the same series length, norm cap, stopping rule and 30-step cap -- the order the
// NumPy restatement of the tests (tests/servo_lqg_numpy.py) follows.
#pragma once
#include "fdyn_riccati_n.hpp"

namespace fdyn {

constexpr int KFN_SERIES_TERMS = 17;
constexpr double KFN_NORM_MAX = 1.5;     // |a|_inf dt above which the first dropped series term exceeds 1e-14

// |a|_inf: the largest row sum of |a_rc|, each row summed left to right.  A NaN row sum never becomes the maximum: the caller tests
// the words themselves.
template <int N>
FD_HD double row_norm(const MN<N>& a)
{
#pragma clang fp contract(off)
    double norm = 0.0;
#pragma unroll
    for (int r = 0; r < N; ++r) {
        double rs = ::fabs(a.v[r][0]);
#pragma unroll
        for (int c = 1; c < N; ++c) rs = rs + ::fabs(a.v[r][c]);
        norm = rs > norm ? rs : norm;
    }
    return norm;
}

// S = sum_k (a dt)^k / (k + 1)!, Phi = I + a dt S = exp(a dt), Gamma = dt S b = int_0^dt exp(a t) dt b
template <int N>
FD_HD void discretise(const MN<N>& a, const double (&b)[N][2], double dt, MN<N>& Phi, double (&Gam)[N][2])
{
#pragma clang fp contract(off)
    MN<N> ad, T, S;
#pragma unroll
    for (int r = 0; r < N; ++r)
#pragma unroll
        for (int c = 0; c < N; ++c) { ad.v[r][c] = a.v[r][c] * dt; T.v[r][c] = S.v[r][c] = r == c ? 1.0 : 0.0; }
#pragma unroll 1
    for (int k = 1; k <= KFN_SERIES_TERMS; ++k) {
        const MN<N> Ta = mul<false, false>(T, ad);
        const double div = double(k + 1);
#pragma unroll
        for (int r = 0; r < N; ++r)
#pragma unroll
            for (int c = 0; c < N; ++c) { T.v[r][c] = Ta.v[r][c] / div; S.v[r][c] = S.v[r][c] + T.v[r][c]; }
    }
    Phi = mul<false, false>(ad, S);
#pragma unroll
    for (int r = 0; r < N; ++r) Phi.v[r][r] = 1.0 + Phi.v[r][r];
#pragma unroll
    for (int r = 0; r < N; ++r)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            double s = S.v[r][0] * b[0][j];
#pragma unroll
            for (int k = 1; k < N; ++k) s = s + S.v[r][k] * b[k][j];
            Gam[r][j] = dt * s;
        }
}

// What one block's filter design returns.  NOT_CONVERGED = failed || !converged; NO_CERTIFICATE = !gain_ok || !positive ||
// !(residual <= RIC_RES_MAX).
template <int N> struct KalmanResult {
    MN<N> L, P;
    double residual;
    int iters;
    bool failed, converged, gain_ok, positive;
};

// V = diag sigma^2, W = diag s^2 dt; the dual of the regulator's problem from A_0 = Phi^T, G_0 = V^-1, H_0 = W; P = (H + H^T) / 2,
// L = P (P + V)^-1; residual max|Phi (P - L P) Phi^T + W - P| / max|P|.
template <int N>
FD_HD void kalman_solve(const MN<N>& Phi, const double (&sigma)[N], const double (&s)[N], double dt, KalmanResult<N>& out)
{
#pragma clang fp contract(off)
    double v[N], w[N];
#pragma unroll
    for (int r = 0; r < N; ++r) { v[r] = sigma[r] * sigma[r]; w[r] = (s[r] * s[r]) * dt; }
    MN<N> Ak, Gk, Hk;
#pragma unroll
    for (int r = 0; r < N; ++r)
#pragma unroll
        for (int c = 0; c < N; ++c) {
            Ak.v[r][c] = Phi.v[c][r];
            Gk.v[r][c] = r == c ? 1.0 / v[r] : 0.0;
            Hk.v[r][c] = r == c ? w[r] : 0.0;
        }
    out.failed = false;
    riccati_doubling(Ak, Gk, Hk, out.iters, out.failed, out.converged);

    MN<N>& P = out.P;
    MN<N> PV, PVi;
#pragma unroll
    for (int r = 0; r < N; ++r)
#pragma unroll
        for (int c = 0; c < N; ++c) {
            P.v[r][c] = 0.5 * (Hk.v[r][c] + Hk.v[c][r]);
            PV.v[r][c] = r == c ? P.v[r][c] + v[r] : P.v[r][c];
        }
    out.gain_ok = inverse(PV, PVi);
    out.L = mul<false, false>(P, PVi);
    // residual of the filter equation at P
    const MN<N> LP = mul<false, false>(out.L, P);
    MN<N> D;
#pragma unroll
    for (int r = 0; r < N; ++r)
#pragma unroll
        for (int c = 0; c < N; ++c) D.v[r][c] = P.v[r][c] - LP.v[r][c];
    const MN<N> PDP = mul<false, true>(mul<false, false>(Phi, D), Phi);
    MN<N> R;
#pragma unroll
    for (int r = 0; r < N; ++r)
#pragma unroll
        for (int c = 0; c < N; ++c) R.v[r][c] = (r == c ? PDP.v[r][c] + w[r] : PDP.v[r][c]) - P.v[r][c];
    out.residual = max_abs(R.v) / max_abs(P.v);
    out.positive = positive_definite(P);
}

}  // namespace fdyn

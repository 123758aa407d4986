// fdyn_riccati_n.hpp -- the Riccati solver of fdyn_riccati.hpp / lqr_design_kernel for a block of any size N (servo_kernels.hip:
// the 7-state longitudinal and the 6-state lateral block of the LQ servo): the matrix type, its products, the inverse, the
// L D L^T test, the Cayley start and the structure-preserving doubling loop, on top of fdyn_dense.hpp's elimination.
//
// Plain C++ templates, __host__ __device__ under hipcc, so the host check (tests/host/servo_check.cpp) runs the very code the
// kernel compiles.  The same arithmetic as the 4 x 4 solver in the same order: no contraction, one rounding per operation,
// products summed k = 0..N-1 in that order, the same constants and the same failure flags -- the order the NumPy restatement of
// the tests (tests/servo_numpy.py) follows.  fdyn_riccati.hpp is included for the constants alone; its 4 x 4 functions take M4 and
// are not used here.
#pragma once
#include "fdyn_dense.hpp"
#include "fdyn_riccati.hpp"

namespace fdyn {

template <int N> struct MN { double v[N][N]; };

// a b, a^T b, a b^T: every element summed k = 0..N-1 in that order, no contraction
template <bool TA, bool TBB, int N>
FD_HD MN<N> mul(const MN<N>& a, const MN<N>& b)
{
#pragma clang fp contract(off)
    MN<N> c;
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = 0; j < N; ++j) {
            double s = (TA ? a.v[0][i] : a.v[i][0]) * (TBB ? b.v[j][0] : b.v[0][j]);
#pragma unroll
            for (int k = 1; k < N; ++k) s = s + (TA ? a.v[k][i] : a.v[i][k]) * (TBB ? b.v[j][k] : b.v[k][j]);
            c.v[i][j] = s;
        }
    return c;
}

// a^-1: fdyn_dense.hpp's elimination on [a | I].  False (singular) when a pivot is below RIC_PIVOT_REL * max|a| or not a number.
template <int N>
FD_HD bool inverse(MN<N> a, MN<N>& x)
{
    MN<N> b;
#pragma unroll
    for (int r = 0; r < N; ++r)
#pragma unroll
        for (int c = 0; c < N; ++c) b.v[r][c] = r == c ? 1.0 : 0.0;
    return gauss_solve<N, N>(a.v, b.v, x.v, RIC_PIVOT_REL);
}

// x = L D L^T with every d > 0 <=> x is positive definite (a Cholesky factorisation without the square roots)
template <int N>
FD_HD bool positive_definite(const MN<N>& x)
{
#pragma clang fp contract(off)
    double L[N][N], d[N];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        double s = x.v[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) s = s - L[j][k] * L[j][k] * d[k];
        d[j] = s;
        ok = ok && (s > 0.0);                                    // false for NaN
#pragma unroll
        for (int i = j + 1; i < N; ++i) {
            double t = x.v[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) t = t - L[i][k] * L[j][k] * d[k];
            L[i][j] = t / s;
        }
    }
    return ok;
}

// The doubling loop of fdyn_riccati.hpp's riccati_doubling on N x N words: M = (I + G_k H_k)^-1, A_{k+1} = A_k M A_k,
// G_{k+1} = G_k + A_k M G_k A_k^T, H_{k+1} = H_k + A_k^T H_k M A_k, until max|H_{k+1} - H_k| <= RIC_TOL max(1, max|H_{k+1}|) or
// RIC_MAX_ITERS steps.  `failed` comes in as the caller's own start failure and goes out true as well when an inverse is
// singular or a word stops being finite.
template <int N>
FD_HD void riccati_doubling(MN<N>& Ak, MN<N>& Gk, MN<N>& Hk, int& it, bool& failed, bool& converged)
{
#pragma clang fp contract(off)
    it = 0;
    converged = false;
#pragma unroll 1
    while (!failed && !converged && it < RIC_MAX_ITERS) {
        MN<N> Mi, IGH = mul<false, false>(Gk, Hk);
#pragma unroll
        for (int r = 0; r < N; ++r) IGH.v[r][r] = 1.0 + IGH.v[r][r];
        if (!inverse(IGH, Mi)) { failed = true; break; }
        const MN<N> AM = mul<false, false>(Ak, Mi), MA = mul<false, false>(Mi, Ak);
        const MN<N> A1 = mul<false, false>(AM, Ak);
        const MN<N> dG = mul<false, true>(mul<false, false>(AM, Gk), Ak);
        const MN<N> dH = mul<true, false>(Ak, mul<false, false>(Hk, MA));
        MN<N> dif;
#pragma unroll
        for (int r = 0; r < N; ++r)
#pragma unroll
            for (int c = 0; c < N; ++c) {
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
}

// What one block's design returns: X, K = R^-1 b^T X, the relative residual of the Riccati equation at X and the flags.
template <int N> struct CareResult {
    MN<N> X;
    double K[2][N];
    double residual;
    int iters;
    bool failed, converged, positive;      // NOT_CONVERGED = failed || !converged; NO_CERTIFICATE = !positive || !(residual <= RIC_RES_MAX)
};

// a^T X + X a - X b R^-1 b^T X + diag(q) = 0 for one block with two controls, as lqr_design_kernel solves its 4 x 4: the Cayley
// transform with gamma = max(1, |a|_inf) gives the start triple, the doubling loop its stabilising solution.  rinv = 1 / r.
template <int N>
FD_HD void care_solve(const MN<N>& a, const double (&b)[N][2], const double (&q)[N], const double (&rinv)[2], CareResult<N>& out)
{
#pragma clang fp contract(off)
    double bs[N][2];
    MN<N> G;
#pragma unroll
    for (int r = 0; r < N; ++r) { bs[r][0] = b[r][0] * rinv[0]; bs[r][1] = b[r][1] * rinv[1]; }
#pragma unroll
    for (int r = 0; r < N; ++r)
#pragma unroll
        for (int c = 0; c < N; ++c) G.v[r][c] = bs[r][0] * b[c][0] + bs[r][1] * b[c][1];
    double gamma = 1.0;
#pragma unroll
    for (int r = 0; r < N; ++r) {
        double rs = ::fabs(a.v[r][0]);
#pragma unroll
        for (int c = 1; c < N; ++c) rs = rs + ::fabs(a.v[r][c]);
        gamma = rs > gamma ? rs : gamma;
    }
    const double g2 = 2.0 * gamma;
    MN<N> ag = a, agi, S1, W, Wi, Ak, Gk, Hk, T0;
#pragma unroll
    for (int r = 0; r < N; ++r) ag.v[r][r] = a.v[r][r] - gamma;
    bool failed = !inverse(ag, agi);
    S1 = mul<false, false>(agi, G);
#pragma unroll
    for (int r = 0; r < N; ++r)
#pragma unroll
        for (int c = 0; c < N; ++c) W.v[r][c] = ag.v[c][r] + q[r] * S1.v[r][c];
    failed = !inverse(W, Wi) || failed;
#pragma unroll
    for (int r = 0; r < N; ++r)
#pragma unroll
        for (int c = 0; c < N; ++c) { Ak.v[r][c] = (r == c ? 1.0 : 0.0) + g2 * Wi.v[c][r]; T0.v[r][c] = q[r] * agi.v[r][c]; }
    Gk = mul<false, false>(S1, Wi);
    Hk = mul<false, false>(Wi, T0);
#pragma unroll
    for (int r = 0; r < N; ++r)
#pragma unroll
        for (int c = 0; c < N; ++c) { Gk.v[r][c] = g2 * Gk.v[r][c]; Hk.v[r][c] = g2 * Hk.v[r][c]; }

    riccati_doubling(Ak, Gk, Hk, out.iters, failed, out.converged);
    out.failed = failed;

    MN<N>& X = out.X;
#pragma unroll
    for (int r = 0; r < N; ++r)
#pragma unroll
        for (int c = 0; c < N; ++c) X.v[r][c] = 0.5 * (Hk.v[r][c] + Hk.v[c][r]);
    // K = R^-1 b^T X
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int c = 0; c < N; ++c) {
            double s = bs[0][j] * X.v[0][c];
#pragma unroll
            for (int r = 1; r < N; ++r) s = s + bs[r][j] * X.v[r][c];
            out.K[j][c] = s;
        }
    // residual of the Riccati equation at X
    const MN<N> AtX = mul<true, false>(a, X), Xa = mul<false, false>(X, a), XGX = mul<false, false>(mul<false, false>(X, G), X);
    MN<N> R;
#pragma unroll
    for (int r = 0; r < N; ++r)
#pragma unroll
        for (int c = 0; c < N; ++c) {
            const double t = (AtX.v[r][c] + Xa.v[r][c]) - XGX.v[r][c];
            R.v[r][c] = r == c ? t + q[r] : t;
        }
    const double xmax = max_abs(X.v);
    out.residual = max_abs(R.v) / (xmax > 1.0 ? xmax : (xmax == xmax ? 1.0 : xmax));
    out.positive = positive_definite(X);
}

}  // namespace fdyn

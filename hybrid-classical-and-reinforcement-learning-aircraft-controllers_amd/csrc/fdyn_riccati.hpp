// fdyn_riccati.hpp -- the 4 x 4 Riccati solver of the design kernels (lqr_kernels.hip: the continuous equation after its Cayley
// transform; kf_kernels.hip: the discrete filter equation as it stands): the matrix type, its products, the inverse, the
// L D L^T test and the structure-preserving doubling loop, on top of fdyn_dense.hpp's elimination.
//
// Plain C++ templates, __host__ __device__ under hipcc, so the host check (tests/host/riccati_check.cpp) runs the very code the
// kernels compile.  Every matrix is a 4 x 4 of named words indexed by compile-time constants: registers on the device, never
// scratch.  No contraction: one rounding per operation, products summed k = 0..3 in that order, which is the order the NumPy
// restatements of the tests follow.
#pragma once
#include "fdyn_dense.hpp"

namespace fdyn {

constexpr int RIC_N = 4;                 // states per block
constexpr int RIC_MAX_ITERS = 30;
constexpr double RIC_TOL = 1e-13, RIC_PIVOT_REL = 1e-14, RIC_RES_MAX = 1e-8;

struct M4 { double v[RIC_N][RIC_N]; };

// a b, a^T b, a b^T: every element summed k = 0..3 in that order, no contraction
template <bool TA, bool TBB>
FD_HD M4 mul(const M4& a, const M4& b)
{
#pragma clang fp contract(off)
    M4 c;
#pragma unroll
    for (int i = 0; i < RIC_N; ++i)
#pragma unroll
        for (int j = 0; j < RIC_N; ++j) {
            double s = (TA ? a.v[0][i] : a.v[i][0]) * (TBB ? b.v[j][0] : b.v[0][j]);
#pragma unroll
            for (int k = 1; k < RIC_N; ++k) s = s + (TA ? a.v[k][i] : a.v[i][k]) * (TBB ? b.v[j][k] : b.v[k][j]);
            c.v[i][j] = s;
        }
    return c;
}

// a^-1: fdyn_dense.hpp's elimination on [a | I].  False (singular) when a pivot is below RIC_PIVOT_REL * max|a| or not a number.
FD_HD bool inverse(M4 a, M4& x)
{
    M4 b;
#pragma unroll
    for (int r = 0; r < RIC_N; ++r)
#pragma unroll
        for (int c = 0; c < RIC_N; ++c) b.v[r][c] = r == c ? 1.0 : 0.0;
    return gauss_solve<RIC_N, RIC_N>(a.v, b.v, x.v, RIC_PIVOT_REL);
}

// x = L D L^T with every d > 0 <=> x is positive definite (a Cholesky factorisation without the square roots)
FD_HD bool positive_definite(const M4& x)
{
#pragma clang fp contract(off)
    double L[RIC_N][RIC_N], d[RIC_N];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < RIC_N; ++j) {
        double s = x.v[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) s = s - L[j][k] * L[j][k] * d[k];
        d[j] = s;
        ok = ok && (s > 0.0);                                    // false for NaN
#pragma unroll
        for (int i = j + 1; i < RIC_N; ++i) {
            double t = x.v[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) t = t - L[i][k] * L[j][k] * d[k];
            L[i][j] = t / s;
        }
    }
    return ok;
}

// The doubling loop on (A_k, G_k, H_k): M = (I + G_k H_k)^-1, A_{k+1} = A_k M A_k, G_{k+1} = G_k + A_k M G_k A_k^T,
// H_{k+1} = H_k + A_k^T H_k M A_k, until max|H_{k+1} - H_k| <= RIC_TOL max(1, max|H_{k+1}|) or RIC_MAX_ITERS steps.  H_k converges
// to the stabilising solution of the equation the caller's start values encode.  `failed` comes in as the caller's own start
// failure and goes out true as well when an inverse is singular or a word stops being finite.
// lqr_design_kernel keeps a copy of this loop in line (its listing is then the one it had before this header existed); a change
// here belongs there too, and tests/test_gpu_lqr.py and tests/test_gpu_lqg.py hold both to the same NumPy loop bit for bit.
FD_HD void riccati_doubling(M4& Ak, M4& Gk, M4& Hk, int& it, bool& failed, bool& converged)
{
#pragma clang fp contract(off)
    it = 0;
    converged = false;
#pragma unroll 1
    while (!failed && !converged && it < RIC_MAX_ITERS) {
        M4 Mi, IGH = mul<false, false>(Gk, Hk);
#pragma unroll
        for (int r = 0; r < RIC_N; ++r) IGH.v[r][r] = 1.0 + IGH.v[r][r];
        if (!inverse(IGH, Mi)) { failed = true; break; }
        const M4 AM = mul<false, false>(Ak, Mi), MA = mul<false, false>(Mi, Ak);
        const M4 A1 = mul<false, false>(AM, Ak);
        const M4 dG = mul<false, true>(mul<false, false>(AM, Gk), Ak);
        const M4 dH = mul<true, false>(Ak, mul<false, false>(Hk, MA));
        M4 dif;
#pragma unroll
        for (int r = 0; r < RIC_N; ++r)
#pragma unroll
            for (int c = 0; c < RIC_N; ++c) {
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

}  // namespace fdyn

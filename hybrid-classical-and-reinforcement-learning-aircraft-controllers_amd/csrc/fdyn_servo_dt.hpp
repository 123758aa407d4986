// fdyn_servo_dt.hpp -- the sampled-data design of the LQ servo (servo_dt_kernels.hip, include/fdyn_servo_dt.h): the gain of one
// augmented block designed for the loop as fdyn_servo_step_* flies it -- the plant behind a zero-order hold at dt, the integrators
// advanced by forward Euler -- by the DISCRETE Riccati equation X = A_d^T X A_d - A_d^T X B_d (R_d + B_d^T X B_d)^-1 B_d^T X A_d + H_0.
// fdyn_riccati_n.hpp's doubling loop is that equation's own iteration (X = A^T X (I + G X)^-1 A + H, G = B_d R_d^-1 B_d^T), so it is
// called directly from (A_d, G_0, H_0): no Cayley start.  fdyn_kalman_n.hpp's discretise<5> gives Phi and Gamma,
// fdyn_servo_margin.hpp's schur_by_squaring_n certifies A_d - B_d K: the matrix fdyn_servo_loop_margins certifies for this K at this dt.
//
// Plain C++ templates, __host__ __device__ under hipcc, so the host check (tests/host/servo_dt_check.cpp) runs the very code the
// kernel compiles.  No contraction, one rounding per operation, every sum k = 0..N-1 in that order (the zero rows of B_d and the
// zero and unit words of A_d are multiplied and added like any other word) -- the order the NumPy restatement of the tests
// (tests/servo_dt_numpy.py) follows.
//
// Operation order, fixed, for a block of N = 5 + n_i words (n_i = 2 longitudinal | 1 lateral integrators, rows ci of C_i):
//   A_d = [[Phi, 0], [dt ci, I]],  B_d = [[Gamma], [0]],  h_r = q_r dt,  rd_j = r_j dt,  rdi_j = 1 / rd_j
//   bs_rj = B_d[r][j] rdi_j,  G_0[r][c] = bs_r0 B_d[c][0] + bs_r1 B_d[c][1],  H_0 = diag(h)
//   riccati_doubling(A_d, G_0, H_0) -> H;  X = (H + H^T) / 2
//   XB = X B_d,  S = B_d^T XB with rd_j added to its diagonal (rd_j + sum),  det = S00 S11 - S01 S10,
//   gain_ok = S00 > 0 and det > 0,  S^-1 = [[S11 / det, -S01 / det], [-S10 / det, S00 / det]]
//   XA = X A_d,  BXA = B_d^T XA,  K[j][c] = Si[j][0] BXA[0][c] + Si[j][1] BXA[1][c]
//   T = A_d^T XA,  AXB = A_d^T XB,  E[r][c] = T[r][c] - (AXB[r][0] K[0][c] + AXB[r][1] K[1][c]), h_r added on the diagonal (E + h_r),
//   residual = max|X - E| / max(1, max|X|)  (NaN stays NaN),  positive = L D L^T test of X
//   A_cl[r][c] = A_d[r][c] - (B_d[r][0] K[0][c] + B_d[r][1] K[1][c]),  stable = schur_by_squaring_n(A_cl)
#pragma once
#include "fdyn_kalman_n.hpp"
#include "fdyn_servo_margin.hpp"

namespace fdyn {

constexpr int SDT_NB = 5;                // physical states of a block: what discretise sees
// a lane's words in the store: A_d [N][N] row-major, then B_d [N][2], at the offsets of the larger block
enum { SDW_AD = 0, SDW_BD = FD_SV_NLON * FD_SV_NLON, SDW_N = SDW_BD + 2 * FD_SV_NLON };

// What one block's sampled design returns.  NOT_CONVERGED = failed || !converged; NO_CERTIFICATE = !positive ||
// !(residual <= RIC_RES_MAX) || !gain_ok || !stable.
template <int N> struct DareResult {
    MN<N> X;
    double K[2][N];
    double residual;
    int iters;
    bool failed, converged, positive, gain_ok, stable;
};

// A_d and B_d of one block from Phi, Gamma and the integrator rows ci [N - 5][5] of the continuous augmented model, written to the
// store: the sampled model has to outlive the doubling loop, whose own N x N words already exceed the register file at N = 7, so it
// waits behind get(k) / set(k, v) -- LDS columns on the device, an array on the host -- as fdyn_servo_margin.hpp keeps its words.
template <int N, typename W>
FD_HD void sampled_model(const MN<SDT_NB>& Phi, const double (&Gam)[SDT_NB][2], const double (&ci)[N - SDT_NB][SDT_NB], double dt, W& w)
{
#pragma clang fp contract(off)
    MN<N> Ad;
    double Bd[N][2];
#pragma unroll
    for (int r = 0; r < N; ++r) {
#pragma unroll
        for (int c = 0; c < N; ++c) Ad.v[r][c] = (r == c && r >= SDT_NB) ? 1.0 : 0.0;
        Bd[r][0] = Bd[r][1] = 0.0;
    }
#pragma unroll
    for (int r = 0; r < SDT_NB; ++r) {
#pragma unroll
        for (int c = 0; c < SDT_NB; ++c) Ad.v[r][c] = Phi.v[r][c];
        Bd[r][0] = Gam[r][0];
        Bd[r][1] = Gam[r][1];
    }
#pragma unroll
    for (int j = 0; j < N - SDT_NB; ++j)
#pragma unroll
        for (int c = 0; c < SDT_NB; ++c) Ad.v[SDT_NB + j][c] = dt * ci[j][c];
#pragma unroll
    for (int r = 0; r < N; ++r) {
#pragma unroll
        for (int c = 0; c < N; ++c) w.set(SDW_AD + N * r + c, Ad.v[r][c]);
        w.set(SDW_BD + 2 * r, Bd[r][0]);
        w.set(SDW_BD + 2 * r + 1, Bd[r][1]);
    }
}

// A_d and B_d back out of the store; reread_words keeps the compiler from carrying them in registers from the last read instead
template <int N, typename W>
FD_HD void read_model(const W& w, MN<N>& Ad, double (&Bd)[N][2])
{
    reread_words();
#pragma unroll
    for (int r = 0; r < N; ++r) {
#pragma unroll
        for (int c = 0; c < N; ++c) Ad.v[r][c] = w.get(SDW_AD + N * r + c);
        Bd[r][0] = w.get(SDW_BD + 2 * r);
        Bd[r][1] = w.get(SDW_BD + 2 * r + 1);
    }
}

// The discrete Riccati equation of one sampled block with two controls, its model in the store: q [N], r [2] the CONTINUOUS weights
// (scaled by dt here).  The model is read twice: for the start triple, and again after the doubling loop.
template <int N, typename W>
FD_HD void dare_solve(const W& w, const double (&q)[N], const double (&r)[2], double dt, DareResult<N>& out)
{
#pragma clang fp contract(off)
    double h[N], rd[2], rdi[2], bs[N][2];
    MN<N> Ad;
    double Bd[N][2];
    read_model<N>(w, Ad, Bd);
#pragma unroll
    for (int k = 0; k < N; ++k) h[k] = q[k] * dt;
#pragma unroll
    for (int j = 0; j < 2; ++j) { rd[j] = r[j] * dt; rdi[j] = 1.0 / rd[j]; }
    MN<N> Ak = Ad, Gk, Hk;
#pragma unroll
    for (int k = 0; k < N; ++k) { bs[k][0] = Bd[k][0] * rdi[0]; bs[k][1] = Bd[k][1] * rdi[1]; }
#pragma unroll
    for (int a = 0; a < N; ++a)
#pragma unroll
        for (int c = 0; c < N; ++c) {
            Gk.v[a][c] = bs[a][0] * Bd[c][0] + bs[a][1] * Bd[c][1];
            Hk.v[a][c] = a == c ? h[a] : 0.0;
        }
    out.failed = false;
    riccati_doubling(Ak, Gk, Hk, out.iters, out.failed, out.converged);
    read_model<N>(w, Ad, Bd);

    MN<N>& X = out.X;
#pragma unroll
    for (int a = 0; a < N; ++a)
#pragma unroll
        for (int c = 0; c < N; ++c) X.v[a][c] = 0.5 * (Hk.v[a][c] + Hk.v[c][a]);
    // S = R_d + B_d^T X B_d and its closed-form inverse
    double XB[N][2], S[2][2], Si[2][2];
#pragma unroll
    for (int a = 0; a < N; ++a)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            double s = X.v[a][0] * Bd[0][j];
#pragma unroll
            for (int k = 1; k < N; ++k) s = s + X.v[a][k] * Bd[k][j];
            XB[a][j] = s;
        }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            double s = Bd[0][i] * XB[0][j];
#pragma unroll
            for (int k = 1; k < N; ++k) s = s + Bd[k][i] * XB[k][j];
            S[i][j] = i == j ? rd[i] + s : s;
        }
    const double det = S[0][0] * S[1][1] - S[0][1] * S[1][0];
    out.gain_ok = S[0][0] > 0.0 && det > 0.0;                    // false for NaN
    Si[0][0] = S[1][1] / det;
    Si[0][1] = -S[0][1] / det;
    Si[1][0] = -S[1][0] / det;
    Si[1][1] = S[0][0] / det;
    // K = S^-1 B_d^T X A_d
    const MN<N> XA = mul<false, false>(X, Ad);
    double BXA[2][N];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int c = 0; c < N; ++c) {
            double s = Bd[0][j] * XA.v[0][c];
#pragma unroll
            for (int k = 1; k < N; ++k) s = s + Bd[k][j] * XA.v[k][c];
            BXA[j][c] = s;
        }
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int c = 0; c < N; ++c) out.K[j][c] = Si[j][0] * BXA[0][c] + Si[j][1] * BXA[1][c];
    // residual of the discrete Riccati equation at X
    const MN<N> T = mul<true, false>(Ad, XA);
    MN<N> R;
#pragma unroll
    for (int a = 0; a < N; ++a) {
        double axb[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            double s = Ad.v[0][a] * XB[0][j];
#pragma unroll
            for (int k = 1; k < N; ++k) s = s + Ad.v[k][a] * XB[k][j];
            axb[j] = s;
        }
#pragma unroll
        for (int c = 0; c < N; ++c) {
            const double e = T.v[a][c] - (axb[0] * out.K[0][c] + axb[1] * out.K[1][c]);
            R.v[a][c] = X.v[a][c] - (a == c ? e + h[a] : e);
        }
    }
    const double xmax = max_abs(X.v);
    out.residual = max_abs(R.v) / (xmax > 1.0 ? xmax : (xmax == xmax ? 1.0 : xmax));
    out.positive = positive_definite(X);
    // the loop as it is flown: A_d - B_d K, certified by squaring
    MN<N> Acl;
#pragma unroll
    for (int a = 0; a < N; ++a)
#pragma unroll
        for (int c = 0; c < N; ++c) Acl.v[a][c] = Ad.v[a][c] - (Bd[a][0] * out.K[0][c] + Bd[a][1] * out.K[1][c]);
    out.stable = schur_by_squaring_n(Acl);
}

// the 5 x 5 part of a block and its two control columns out of the lane's A, B (words `n` apart).  False when a word is not finite.
FD_HD bool sampled_load_block(const double* __restrict__ A, const double* __restrict__ B, int64_t n, const int (&sr)[SDT_NB], int c0, int c1,
                      MN<SDT_NB>& a, double (&b)[SDT_NB][2])
{
    bool fin = true;
#pragma unroll
    for (int r = 0; r < SDT_NB; ++r) {
#pragma unroll
        for (int c = 0; c < SDT_NB; ++c) { a.v[r][c] = A[int64_t(sr[r] * FD_NX + sr[c]) * n]; fin = fin && ::isfinite(a.v[r][c]); }
        b[r][0] = B[int64_t(sr[r] * FD_NU + c0) * n];
        b[r][1] = B[int64_t(sr[r] * FD_NU + c1) * n];
        fin = fin && ::isfinite(b[r][0]) && ::isfinite(b[r][1]);
    }
    return fin;
}

// one block of one lane: discretise, the sampled model into the store, the discrete Riccati equation, the gain into Kall at KAT
template <int N, int QAT, int RAT, int KAT, typename W>
FD_HD void sampled_design_block(W& w, const MN<SDT_NB>& a, const double (&b)[SDT_NB][2], const double (&ci)[N - SDT_NB][SDT_NB],
                        const double (&wt)[FD_NSVW], double dt, double (&Kall)[FD_NSVK], double& res, int& it_max, int& st)
{
#pragma clang fp contract(off)
    {
        MN<SDT_NB> Phi;
        double Gam[SDT_NB][2];
        discretise<SDT_NB>(a, b, dt, Phi, Gam);
        sampled_model<N>(Phi, Gam, ci, dt, w);
    }
    double q[N], r[2];
#pragma unroll
    for (int k = 0; k < N; ++k) q[k] = wt[QAT + k];
    r[0] = wt[RAT];
    r[1] = wt[RAT + 1];
    DareResult<N> d;
    dare_solve<N>(w, q, r, dt, d);
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int c = 0; c < N; ++c) Kall[KAT + j * N + c] = d.K[j][c];
    res = nan_max(res, d.residual);
    it_max = d.iters > it_max ? d.iters : it_max;
    if (d.failed || !d.converged) st |= FD_SV_NOT_CONVERGED;
    if (!d.positive || !(d.residual <= RIC_RES_MAX) || !d.gain_ok || !d.stable) st |= FD_SV_NO_CERTIFICATE;
}

// One lane, both blocks.  A, B, x0, K, residual, iters and status point at the lane's own column, `n` the distance between consecutive
// words of it (1 on the host); weights at the lane's first weight, its words `wn` apart.  See include/fdyn_servo_dt.h for what is
// written.
template <typename W>
FD_HD void servo_dt_lane(W& w, const double* __restrict__ A, const double* __restrict__ B, const double* __restrict__ x0, int64_t n,
                         const double* __restrict__ weights, int64_t wn, double dt, double* __restrict__ K, double* __restrict__ residual,
                         int32_t* __restrict__ iters, int32_t* __restrict__ status)
{
#pragma clang fp contract(off)
    // the rows / columns of A and B a block reads: the five physical states of each block
    const int LON_W[SDT_NB] = { FD_X_U, FD_X_W, FD_X_Q, FD_X_PITCH, FD_X_D };
    const int LAT_W[SDT_NB] = { FD_X_V, FD_X_P, FD_X_R, FD_X_ROLL, FD_X_YAW };
    double wt[FD_NSVW];
    bool bad = !(dt > 1e-6) || dt > 1.0;
#pragma unroll
    for (int k = 0; k < FD_NSVW; ++k) {
        wt[k] = weights[int64_t(k) * wn];
        bad = bad || !(::isfinite(wt[k]) && wt[k] > 0.0);
    }
    const double u0 = x0[int64_t(FD_X_U) * n], w0 = x0[int64_t(FD_X_W) * n];
    const double V0 = ::sqrt(u0 * u0 + w0 * w0);
    bad = bad || !(::isfinite(u0) && ::isfinite(w0) && V0 > 0.0);
    // both blocks' words are read and tested before anything is solved: BAD_INPUT (weights, trim, dt, either block) solves nothing
    MN<SDT_NB> a;
    double b[SDT_NB][2];
    bad = !sampled_load_block(A, B, n, LAT_W, FD_U_AILERON, FD_U_RUDDER, a, b) || bad;
    bad = bad || !(row_norm<SDT_NB>(a) * dt <= KFN_NORM_MAX);
    bad = !sampled_load_block(A, B, n, LON_W, FD_U_ELEVATOR, FD_U_THROTTLE, a, b) || bad;
    bad = bad || !(row_norm<SDT_NB>(a) * dt <= KFN_NORM_MAX);

    double Kall[FD_NSVK];
#pragma unroll
    for (int k = 0; k < FD_NSVK; ++k) Kall[k] = 0.0;
    double res = 0.0;
    int it_max = 0, st = 0;
    if (!bad) {
        {   // longitudinal: (u, w, q, theta, z), then i_V += dt (u0 du + w0 dw) / V0 and i_h += dt (-dz)
            const double ci[FD_SV_NLON - SDT_NB][SDT_NB] = { { u0 / V0, w0 / V0, 0.0, 0.0, 0.0 }, { 0.0, 0.0, 0.0, 0.0, -1.0 } };
            sampled_design_block<FD_SV_NLON, FD_SVW_Q_LON, FD_SVW_R_LON, FD_SVK_LON>(w, a, b, ci, wt, dt, Kall, res, it_max, st);
        }
        {   // lateral: (v, p, r, phi, psi), then i_psi += dt dpsi
            sampled_load_block(A, B, n, LAT_W, FD_U_AILERON, FD_U_RUDDER, a, b);
            const double ci[FD_SV_NLAT - SDT_NB][SDT_NB] = { { 0.0, 0.0, 0.0, 0.0, 1.0 } };
            sampled_design_block<FD_SV_NLAT, FD_SVW_Q_LAT, FD_SVW_R_LAT, FD_SVK_LAT>(w, a, b, ci, wt, dt, Kall, res, it_max, st);
        }
    }
    if (bad) { st = FD_SV_BAD_INPUT; res = __builtin_nan(""); it_max = 0; }
#pragma unroll
    for (int k = 0; k < FD_NSVK; ++k) K[int64_t(k) * n] = st ? 0.0 : Kall[k];
    *residual = res;
    *iters = it_max;
    *status = st;
}

}  // namespace fdyn

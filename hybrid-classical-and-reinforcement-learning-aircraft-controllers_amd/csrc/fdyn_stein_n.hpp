// fdyn_stein_n.hpp -- the discrete Stein equation X = A X B^T + Q for A N x N, B M x M, 1 <= N, M <= 7, by Smith doubling, and on
// top of it the predicted steady-state covariances of the LQ servo loop (servo_covariance_kernels.hip): what the loop that
// fdyn_servo_loop_margins certifies and fdyn_servo_sampled_modes / fdyn_servo_filter_modes locate will hold on its sensors -- the
// variance of the state, of the estimate, of the three tracking errors, of the integrators, of the controls and of their step to
// step change.  The loop matrices are fdyn_eig_n.hpp's servo_sampled_block and servo_filter_block, the stability test is
// fdyn_servo_margin.hpp's schur_by_squaring_n: the four reports speak of the same numbers.
//
// Solver.  X_0 = Q, then D = (A_k X_k) B_k^T, X_{k+1} = X_k + D, A_{k+1} = A_k A_k, B_{k+1} = B_k B_k: after k doublings X_k holds
// 2^k terms of sum_j A^j Q B^Tj.  It stops when max|D| <= STEIN_TOL max|X_{k+1}| (below one rounding of the largest word: the sum has
// stopped moving) or after STEIN_MAX_DOUBLINGS doublings, and fails when max|X| or max|D| is not finite.  A spectral radius of
// 0.9972, the largest of the fixture set's loops, takes 14 doublings.  The symmetric case (B = A, Q symmetric) squares A once and
// returns (X + X^T) / 2, as kalman_solve does.  The residual max|(A X) B^T + Q - X| / max|X| is taken with the A, B, Q given and the
// X returned; 0 when X is exactly 0, NaN when the loop failed.
//
// Model (per block, n_b = 5 physical states, n_i = 2 | 1 integrators, xi = (d, i), e = d - xhat after the update, n = f - d what
// the law is fed beside the truth):
//   Acl = [[Phi - Gamma Kx, -Gamma Ki], [dt C_i, I]]    Bf = [-Gamma Kx ; dt C_i]    Ae = (I - L) Phi    V = diag sigma^2
//   W = diag(s^2 dt)    xi+ = Acl xi + Bf n + (w, 0)    e+ = Ae e + (I - L) w - L v+    u = -Kb xi - Kx n
//   Se  = Ae Se Ae^T + (I - L) W (I - L)^T + L V L^T                                          every feedback: the estimator always runs
//   truth        n = 0:   Nn = 0,  Sxe = 0
//   measurement  n = v:   Nn = V,  Sxe = 0
//   estimate     n = -e:  Nn = Se, Sxe = E[xi e^T] = Acl Sxe Ae^T - Bf Se Ae^T + (W (I - L)^T ; 0)
//   Sx  = Acl Sx Acl^T + (Bf Nn Bf^T - G - G^T) + diag(W, 0),  G = Acl Sxe Bf^T
//   var u_a  = (kb Sx kb - 2 kb Sxe kx) + kx Nn kx,  kb, kx row a of Kb, Kx
//   var du_a = mx Sx mx + ...,  mx = -kb (Acl - I):
//       truth        + kx W kx
//       measurement  + (kx - kb Bf) V (kx - kb Bf) + kx V kx + kx W kx
//       estimate     + 2 mx Sxe me + me Se me + (kx L)(V + W)(kx L),  me = kb Bf + kx (Ae - I)
//
// Operation order, fixed: a product is summed k = 0, 1, ... left to right (mulr); a^T S b is t_i = sum_j S_ij b_j, then
// sum_i a_i t_i (quad); sum_k (a_k d_k) a_k (dquad); a^T (M - I) is sum_r a_r (M_rc - [r = c]) (vecmat).  No contraction: one
// rounding per operation, the order tests/servo_cov_numpy.py follows.  The only operations are + - * /.
//
// Plain C++ templates, __host__ __device__ under hipcc, so the host check (tests/host/stein_check.cpp) runs the very code the
// kernel compiles.  Everything is named words indexed by compile-time constants: registers on the device, as far as they reach
// (DESIGN.md 7q has the code-object metadata).
#pragma once
#include <stdint.h>
#include "fdyn_eig_n.hpp"
#include "fdyn_servo_margin.hpp"
#include "../../include/fdyn_servo_covariance.h"

namespace fdyn {

constexpr int STEIN_MAX_DOUBLINGS = 40;
constexpr double STEIN_TOL = 1e-17;
constexpr double STEIN_RES_MAX = 1e-9;

// c = a b (TB: a b^T), a R x K, b K x C (TB: C x K): every element summed k = 0 .. K-1 in that order
template <bool TB, int R, int K, int C>
FD_HD void mulr(const double (&a)[R][K], const double (&b)[TB ? C : K][TB ? K : C], double (&c)[R][C])
{
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
        for (int j = 0; j < C; ++j) {
            double s = a[i][0] * (TB ? b[j][0] : b[0][j]);
#pragma unroll
            for (int k = 1; k < K; ++k) s = s + a[i][k] * (TB ? b[j][k] : b[k][j]);
            c[i][j] = s;
        }
}

struct SteinResult {
    double residual;
    int iters;
    bool converged, failed;
    FD_HD bool ok() const { return !failed && converged && residual <= STEIN_RES_MAX; }
};

// X = A X B^T + Q.  SYM: B is not read (B = A) and X is symmetrised.
template <bool SYM, int N, int M>
FD_HD SteinResult stein_iterate(const double (&A)[N][N], const double (&B)[M][M], const double (&Q)[N][M], double (&X)[N][M])
{
#pragma clang fp contract(off)
    static_assert(!SYM || N == M, "the symmetric case is square");
    double Ak[N][N], Bk[SYM ? 1 : M][SYM ? 1 : M];
#pragma unroll
    for (int r = 0; r < N; ++r)
#pragma unroll
        for (int c = 0; c < N; ++c) Ak[r][c] = A[r][c];
    if (!SYM) {
#pragma unroll
        for (int r = 0; r < M; ++r)
#pragma unroll
            for (int c = 0; c < M; ++c) Bk[SYM ? 0 : r][SYM ? 0 : c] = B[r][c];
    }
#pragma unroll
    for (int r = 0; r < N; ++r)
#pragma unroll
        for (int c = 0; c < M; ++c) X[r][c] = Q[r][c];
    SteinResult out;
    out.iters = 0;
    out.converged = false;
    out.failed = false;
#pragma unroll 1
    while (!out.failed && !out.converged && out.iters < STEIN_MAX_DOUBLINGS) {
        double T[N][M], D[N][M];
        mulr<false>(Ak, X, T);
        if constexpr (SYM) mulr<true>(T, Ak, D); else mulr<true>(T, Bk, D);
#pragma unroll
        for (int r = 0; r < N; ++r)
#pragma unroll
            for (int c = 0; c < M; ++c) X[r][c] = X[r][c] + D[r][c];
        {
            double A2[N][N];
            mulr<false>(Ak, Ak, A2);
#pragma unroll
            for (int r = 0; r < N; ++r)
#pragma unroll
                for (int c = 0; c < N; ++c) Ak[r][c] = A2[r][c];
        }
        if constexpr (!SYM) {
            double B2[M][M];
            mulr<false>(Bk, Bk, B2);
#pragma unroll
            for (int r = 0; r < M; ++r)
#pragma unroll
                for (int c = 0; c < M; ++c) Bk[r][c] = B2[r][c];
        }
        ++out.iters;
        const double xmax = max_abs(X), dmax = max_abs(D);
        if (!(::isfinite(xmax) && ::isfinite(dmax))) { out.failed = true; break; }
        out.converged = dmax <= STEIN_TOL * xmax;
    }
    if constexpr (SYM) {
#pragma unroll
        for (int r = 0; r < N; ++r)
#pragma unroll
            for (int c = r + 1; c < N; ++c) {
                const double s = 0.5 * (X[r][c] + X[c][r]);
                X[r][c] = s;
                X[c][r] = s;
            }
#pragma unroll
        for (int r = 0; r < N; ++r) X[r][r] = 0.5 * (X[r][r] + X[r][r]);
    }
    double T[N][M], D[N][M];
    mulr<false>(A, X, T);
    if constexpr (SYM) mulr<true>(T, A, D); else mulr<true>(T, B, D);
#pragma unroll
    for (int r = 0; r < N; ++r)
#pragma unroll
        for (int c = 0; c < M; ++c) D[r][c] = (D[r][c] + Q[r][c]) - X[r][c];
    const double xmax = max_abs(X);
    out.residual = out.failed ? __builtin_nan("") : (xmax == 0.0 ? 0.0 : max_abs(D) / xmax);
    return out;
}

// X = A X B^T + Q, the general case
template <int N, int M>
FD_HD SteinResult stein_doubling(const double (&A)[N][N], const double (&B)[M][M], const double (&Q)[N][M], double (&X)[N][M], int& iters)
{
    const SteinResult r = stein_iterate<false>(A, B, Q, X);
    iters = r.iters;
    return r;
}

// X = A X A^T + Q with Q symmetric: (X + X^T) / 2 of the same loop, A squared once per doubling
template <int N>
FD_HD SteinResult lyapunov_doubling(const double (&A)[N][N], const double (&Q)[N][N], double (&X)[N][N], int& iters)
{
    const SteinResult r = stein_iterate<true>(A, A, Q, X);
    iters = r.iters;
    return r;
}

// fdyn_stein_solve: one lane.  Every pointer is at the lane's own column, `n` is the distance between consecutive words of it.
template <int N, int M>
FD_HD void stein_solve_lane(const double* __restrict__ A, const double* __restrict__ B, const double* __restrict__ Q, int64_t n,
                            double* __restrict__ X, double* __restrict__ residual, int32_t* __restrict__ iters, int32_t* __restrict__ status)
{
    double a[N][N], b[M][M], q[N][M], x[N][M];
    bool fin = true;
#pragma unroll
    for (int r = 0; r < N; ++r)
#pragma unroll
        for (int c = 0; c < N; ++c) { a[r][c] = A[int64_t(r * N + c) * n]; fin = fin && ::isfinite(a[r][c]); }
#pragma unroll
    for (int r = 0; r < M; ++r)
#pragma unroll
        for (int c = 0; c < M; ++c) { b[r][c] = B[int64_t(r * M + c) * n]; fin = fin && ::isfinite(b[r][c]); }
#pragma unroll
    for (int r = 0; r < N; ++r)
#pragma unroll
        for (int c = 0; c < M; ++c) { q[r][c] = Q[int64_t(r * M + c) * n]; fin = fin && ::isfinite(q[r][c]); }
    const double nan = __builtin_nan("");
    int st = FD_SCV_BAD_INPUT, it = 0;
    double res = nan;
    if (fin) {
        const SteinResult r = stein_doubling(a, b, q, x, it);
        res = r.residual;
        st = r.ok() ? 0 : FD_SCV_NOT_CONVERGED;
    }
#pragma unroll
    for (int r = 0; r < N; ++r)
#pragma unroll
        for (int c = 0; c < M; ++c) X[int64_t(r * M + c) * n] = st ? nan : x[r][c];
    if (residual) *residual = res;
    if (iters) *iters = it;
    *status = st;
}

// a^T S b: t_i = sum_j S_ij b_j, then sum_i a_i t_i
template <int R, int C>
FD_HD double quad(const double (&a)[R], const double (&S)[R][C], const double (&b)[C])
{
#pragma clang fp contract(off)
    double out = 0.0;
#pragma unroll
    for (int i = 0; i < R; ++i) {
        double t = S[i][0] * b[0];
#pragma unroll
        for (int j = 1; j < C; ++j) t = t + S[i][j] * b[j];
        out = i ? out + a[i] * t : a[i] * t;
    }
    return out;
}

// a^T S b over the leading R x R of a larger S
template <int R, int NS>
FD_HD double quad_lead(const double (&a)[R], const double (&S)[NS][NS], const double (&b)[R])
{
#pragma clang fp contract(off)
    double out = 0.0;
#pragma unroll
    for (int i = 0; i < R; ++i) {
        double t = S[i][0] * b[0];
#pragma unroll
        for (int j = 1; j < R; ++j) t = t + S[i][j] * b[j];
        out = i ? out + a[i] * t : a[i] * t;
    }
    return out;
}

// sum_k (a_k d_k) a_k
template <int R>
FD_HD double dquad(const double (&a)[R], const double (&d)[R])
{
#pragma clang fp contract(off)
    double out = (a[0] * d[0]) * a[0];
#pragma unroll
    for (int k = 1; k < R; ++k) out = out + (a[k] * d[k]) * a[k];
    return out;
}

// out_c = sum_r a_r (M_rc - [MINUS_I and r = c])
template <bool MINUS_I, int R, int C>
FD_HD void vecmat(const double (&a)[R], const double (&m)[R][C], double (&out)[C])
{
#pragma clang fp contract(off)
#pragma unroll
    for (int c = 0; c < C; ++c) {
        double s = 0.0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const double e = (MINUS_I && r == c) ? m[r][c] - 1.0 : (MINUS_I ? m[r][c] - 0.0 : m[r][c]);
            s = r ? s + a[r] * e : a[r] * e;
        }
        out[c] = s;
    }
}

// Both loop matrices of block BLK and their Schur test: false in `fin` for a word read that is not finite
template <int BLK>
FD_HD bool servo_covariance_stable(const double* __restrict__ K, const double* __restrict__ F, int64_t n, double dt, double cu, double cw, bool& fin)
{
    constexpr int NA = BLK ? FD_SV_NLAT : FD_SV_NLON, NB = FD_SK_NB;
    bool stable = true;
    {
        MN<NA> m;
        fin = servo_sampled_block<BLK>(K, F, n, dt, cu, cw, m.v) && fin;
        stable = schur_by_squaring_n(m) && stable;
    }
    {
        MN<NB> m;
        fin = servo_filter_block(F, BLK, n, m.v) && fin;
        stable = schur_by_squaring_n(m) && stable;
    }
    return stable;
}

// One block of fdyn_servo_covariance for a lane whose inputs are finite and whose loops are Schur.  sig and rate point at the
// block's five words (strides sn, wn); rate may be null.  Writes the block's report and cov words; returns whether every solve
// converged, and folds the residuals and the doublings into res and it.  Acl and Ae are composed again here (a few dozen operations)
// and not handed over from servo_covariance_stable: held across the Schur tests of both blocks they would be 49 + 25 and 36 + 25 more live words.
template <int BLK>
FD_HD bool servo_covariance_block(const double* __restrict__ K, const double* __restrict__ F, int64_t n, double dt, double cu, double cw,
                                  const double* __restrict__ sig, int64_t sn, const double* __restrict__ rate, int64_t wn, int feedback,
                                  double* __restrict__ report, double* __restrict__ cov, double& res, int& it)
{
#pragma clang fp contract(off)
    constexpr int NA = BLK ? FD_SV_NLAT : FD_SV_NLON, NB = FD_SK_NB, NI = NA - NB;
    const double* Kb = K + int64_t(BLK ? FD_SVK_LAT : FD_SVK_LON) * n;
    const double* Fgam = F + int64_t(BLK ? FD_SKF_GAMMA_LAT : FD_SKF_GAMMA_LON) * n;
    const double* Fl = F + int64_t(BLK ? FD_SKF_L_LAT : FD_SKF_L_LON) * n;
    const bool estimate = feedback == FD_LQG_ESTIMATE, measurement = feedback == FD_LQG_MEASUREMENT;
    double v[NB], w[NB], vw[NB];
#pragma unroll
    for (int k = 0; k < NB; ++k) {
        const double s = sig[int64_t(k) * sn], r = rate ? rate[int64_t(k) * wn] : 0.0;
        v[k] = s * s;
        w[k] = (r * r) * dt;
        vw[k] = v[k] + w[k];
    }
    double Acl[NA][NA], Ae[NB][NB], kb[2][NA], L[NB][NB], ImL[NB][NB], Bf[NA][NB];
    servo_sampled_block<BLK>(K, F, n, dt, cu, cw, Acl);
    servo_filter_block(F, BLK, n, Ae);
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < NA; ++c) kb[a][c] = Kb[int64_t(a * NA + c) * n];
#pragma unroll
    for (int r = 0; r < NB; ++r) {
        const double g0 = Fgam[int64_t(2 * r) * n], g1 = Fgam[int64_t(2 * r + 1) * n];
#pragma unroll
        for (int c = 0; c < NB; ++c) {
            L[r][c] = Fl[int64_t(r * NB + c) * n];
            ImL[r][c] = (r == c ? 1.0 : 0.0) - L[r][c];
            Bf[r][c] = -(g0 * kb[0][c] + g1 * kb[1][c]);
        }
    }
#pragma unroll
    for (int j = 0; j < NI; ++j)
#pragma unroll
        for (int c = 0; c < NB; ++c) Bf[NB + j][c] = Acl[NB + j][c];

    bool ok = true;
    int its = 0;
    // the estimation error
    double Se[NB][NB];
    {
        double Qe[NB][NB], Mw[NB][NB], Lv[NB][NB], T1[NB][NB], T2[NB][NB];
#pragma unroll
        for (int r = 0; r < NB; ++r)
#pragma unroll
            for (int c = 0; c < NB; ++c) { Mw[r][c] = ImL[r][c] * w[c]; Lv[r][c] = L[r][c] * v[c]; }
        mulr<true>(Mw, ImL, T1);
        mulr<true>(Lv, L, T2);
#pragma unroll
        for (int r = 0; r < NB; ++r)
#pragma unroll
            for (int c = 0; c < NB; ++c) Qe[r][c] = T1[r][c] + T2[r][c];
        const SteinResult s = lyapunov_doubling(Ae, Qe, Se, its);
        ok = s.ok() && ok;
        res = nan_max(res, s.residual);
        it = its > it ? its : it;
    }
    // what the law is fed beside the truth, and its covariance with the loop state
    double Sxe[NA][NB], Nn[NB][NB];
#pragma unroll
    for (int r = 0; r < NB; ++r)
#pragma unroll
        for (int c = 0; c < NB; ++c) Nn[r][c] = estimate ? Se[r][c] : ((measurement && r == c) ? v[r] : 0.0);
    if (estimate) {
        double T[NA][NB], Qxe[NA][NB];
        mulr<false>(Bf, Se, T);
        mulr<true>(T, Ae, Qxe);
#pragma unroll
        for (int r = 0; r < NA; ++r)
#pragma unroll
            for (int c = 0; c < NB; ++c) Qxe[r][c] = r < NB ? w[r < NB ? r : 0] * ImL[c][r < NB ? r : 0] + -Qxe[r][c] : -Qxe[r][c];
        const SteinResult s = stein_doubling(Acl, Ae, Qxe, Sxe, its);
        ok = s.ok() && ok;
        res = nan_max(res, s.residual);
        it = its > it ? its : it;
    } else {
#pragma unroll
        for (int r = 0; r < NA; ++r)
#pragma unroll
            for (int c = 0; c < NB; ++c) Sxe[r][c] = 0.0;
    }
    // the loop state
    double Sx[NA][NA];
    {
        double T[NA][NB], G[NA][NA], H[NA][NA], Qx[NA][NA];
        mulr<false>(Acl, Sxe, T);
        mulr<true>(T, Bf, G);
        mulr<false>(Bf, Nn, T);
        mulr<true>(T, Bf, H);
#pragma unroll
        for (int r = 0; r < NA; ++r)
#pragma unroll
            for (int c = 0; c < NA; ++c) {
                const double q = (H[r][c] - G[r][c]) - G[c][r];
                Qx[r][c] = (r == c && r < NB) ? q + w[r < NB ? r : 0] : q;
            }
        const SteinResult s = lyapunov_doubling(Acl, Qx, Sx, its);
        ok = s.ok() && ok;
        res = nan_max(res, s.residual);
        it = its > it ? its : it;
    }

    // the report words of the block
#pragma unroll
    for (int r = 0; r < NB; ++r) {
        report[int64_t(FD_SCV_VAR_X + NB * BLK + r) * n] = Sx[r][r];
        report[int64_t(FD_SCV_VAR_EST + NB * BLK + r) * n] = Se[r][r];
    }
#pragma unroll
    for (int j = 0; j < NI; ++j) {
        double ci[NB];
#pragma unroll
        for (int c = 0; c < NB; ++c) ci[c] = servo_integrator_row(BLK, j, c, cu, cw);
        report[int64_t(FD_SCV_VAR_ERR + (BLK ? 2 : 0) + j) * n] = quad_lead(ci, Sx, ci);
        report[int64_t(FD_SCV_VAR_INTEG + (BLK ? 2 : 0) + j) * n] = Sx[NB + j][NB + j];
    }
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const int word = BLK ? (a ? FD_U_RUDDER : FD_U_AILERON) : (a ? FD_U_THROTTLE : FD_U_ELEVATOR);
        double kx[NB], mx[NA], kbf[NB];
#pragma unroll
        for (int c = 0; c < NB; ++c) kx[c] = kb[a][c];
        report[int64_t(FD_SCV_VAR_U + word) * n] = (quad(kb[a], Sx, kb[a]) - 2.0 * quad(kb[a], Sxe, kx)) + quad(kx, Nn, kx);
        vecmat<true>(kb[a], Acl, mx);
#pragma unroll
        for (int c = 0; c < NA; ++c) mx[c] = -mx[c];
        vecmat<false>(kb[a], Bf, kbf);
        const double q = quad(mx, Sx, mx);
        double du;
        if (estimate) {
            double me[NB], kl[NB];
            vecmat<true>(kx, Ae, me);
#pragma unroll
            for (int c = 0; c < NB; ++c) me[c] = kbf[c] + me[c];
            vecmat<false>(kx, L, kl);
            du = ((q + 2.0 * quad(mx, Sxe, me)) + quad(me, Se, me)) + dquad(kl, vw);
        } else if (measurement) {
            double mn[NB];
#pragma unroll
            for (int c = 0; c < NB; ++c) mn[c] = kx[c] - kbf[c];
            du = ((q + dquad(mn, v)) + dquad(kx, v)) + dquad(kx, w);
        } else {
            du = q + dquad(kx, w);
        }
        report[int64_t(FD_SCV_VAR_DU + word) * n] = du;
    }
    if (cov) {
        double* ce = cov + int64_t(BLK ? FD_SCC_E_LAT : FD_SCC_E_LON) * n;
        double* cxe = cov + int64_t(BLK ? FD_SCC_XE_LAT : FD_SCC_XE_LON) * n;
        double* cx = cov + int64_t(BLK ? FD_SCC_X_LAT : FD_SCC_X_LON) * n;
#pragma unroll
        for (int r = 0; r < NB; ++r)
#pragma unroll
            for (int c = 0; c < NB; ++c) ce[int64_t(r * NB + c) * n] = Se[r][c];
#pragma unroll
        for (int r = 0; r < NA; ++r)
#pragma unroll
            for (int c = 0; c < NB; ++c) cxe[int64_t(r * NB + c) * n] = Sxe[r][c];
#pragma unroll
        for (int r = 0; r < NA; ++r)
#pragma unroll
            for (int c = 0; c < NA; ++c) cx[int64_t(r * NA + c) * n] = Sx[r][c];
    }
    return ok;
}

// fdyn_servo_covariance: one lane, both blocks.  K, F, x0 and the outputs point at the lane's own column, `n` is the distance
// between consecutive words of it (1 on the host); sigma and w_rate (or null) at the lane's first word, strides sn and wn (1 for a
// shared array).  See include/fdyn_servo_covariance.h for what is written.
FD_HD void servo_covariance_lane(const double* __restrict__ K, const double* __restrict__ F, const double* __restrict__ x0, int64_t n,
                                 double dt, const double* __restrict__ sigma, int64_t sn, const double* __restrict__ w_rate, int64_t wn,
                                 int feedback, double* __restrict__ report, double* __restrict__ cov, double* __restrict__ residual,
                                 int32_t* __restrict__ iters, int32_t* __restrict__ status)
{
#pragma clang fp contract(off)
    const double u0 = x0[int64_t(FD_X_U) * n], w0 = x0[int64_t(FD_X_W) * n];       // of x0 only these two words are read
    const double V0 = ::sqrt(u0 * u0 + w0 * w0);
    bool fin = ::isfinite(u0) && ::isfinite(w0) && V0 > 0.0 && dt > 1e-6 && !(dt > 1.0);
#pragma unroll 1
    for (int k = 0; k < FD_NSVK; ++k) fin = fin && ::isfinite(K[int64_t(k) * n]);
#pragma unroll 1
    for (int k = 0; k < FD_NSKF; ++k) fin = fin && ::isfinite(F[int64_t(k) * n]);
#pragma unroll 1
    for (int k = 0; k < FD_NSKX; ++k) {
        const double s = sigma[int64_t(k) * sn], r = w_rate ? w_rate[int64_t(k) * wn] : 0.0;
        fin = fin && ::isfinite(s) && s >= 0.0 && ::isfinite(r) && r >= 0.0;
    }
    const double cu = u0 / V0, cw = w0 / V0;
    int st = 0, it = 0;
    double res = __builtin_nan("");
    if (fin) {
        bool stable = servo_covariance_stable<0>(K, F, n, dt, cu, cw, fin);
        stable = servo_covariance_stable<1>(K, F, n, dt, cu, cw, fin) && stable;
        if (!fin) st = FD_SCV_BAD_INPUT;
        else if (!stable) st = FD_SCV_UNSTABLE;
        else {
            res = 0.0;
            bool ok = servo_covariance_block<0>(K, F, n, dt, cu, cw, sigma, sn, w_rate, wn, feedback, report, cov, res, it);
            ok = servo_covariance_block<1>(K, F, n, dt, cu, cw, sigma + int64_t(FD_SK_NB) * sn, sn,
                                           w_rate ? w_rate + int64_t(FD_SK_NB) * wn : nullptr, wn, feedback, report, cov, res, it) && ok;
            if (!ok) st = FD_SCV_NOT_CONVERGED;
        }
    } else {
        st = FD_SCV_BAD_INPUT;
    }
    if (st) {
        const double nan = __builtin_nan("");
#pragma unroll 1
        for (int k = 0; k < FD_NSCV; ++k) report[int64_t(k) * n] = nan;
        if (cov) {
#pragma unroll 1
            for (int k = 0; k < FD_NSCC; ++k) cov[int64_t(k) * n] = nan;
        }
    }
    *residual = res;
    if (iters) *iters = it;
    *status = st;
}

}  // namespace fdyn

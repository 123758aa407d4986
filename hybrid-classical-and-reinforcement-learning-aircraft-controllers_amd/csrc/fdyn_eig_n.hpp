// fdyn_eig_n.hpp -- the eigenvalues of a real N x N, 2 <= N <= 7, and on top of them the flight modes of the LQ servo
// (servo_modes_kernels.hip): the poles of the 7 x 7 longitudinal and 6 x 6 lateral augmented loops, continuous and as flown, and of
// the 5 x 5 error dynamics of the servo's filter.  fdyn_eig.hpp's 4 x 4 solver stays as it is; what it shares is used from it
// (eig2, EIG_EPS, EIG_MAX_SWEEPS).
//
// Algorithm.  Householder reduction to Hessenberg form (N - 2 reflectors; a column that is already zero below its subdiagonal is
// left alone), then EISPACK hqr's Francis double-shift QR on an active window [l, en] that shrinks from the bottom: en starts at
// N - 1; l is the largest row in 1 .. en whose subdiagonal is negligible, |h[k][k-1]| <= EIG_EPS (|h[k-1][k-1]| + |h[k][k]|) with
// the matrix norm in the place of a zero sum, or 0.  l = en deflates a 1 x 1, l = en - 1 a 2 x 2 (solved by eig2), anything else is
// swept once over [l, en].  LAPACK's exceptional shifts at sweeps 10 and 20 of a deflation, at most EIG_MAX_SWEEPS sweeps per
// deflation.  No balancing: every step is an orthogonal similarity, backward stable in |m|.
//
// The search for two small consecutive subdiagonals (hqr's second inner loop, which starts a sweep below l) is LEFT OUT, as in the
// 4 x 4.  It saves work on large matrices by starting the bulge lower; at N <= 7 a sweep over the whole window costs little more,
// and the search would add a second lane-varying start row with products that can underflow on the 1e-100 cases.  What decides it:
// on the 288 x 10 servo matrices of the fixture set (continuous, sampled and filter loops at dt 0.01 and 0.02) every deflation
// converges and the slowest takes 15 sweeps, half the cap (tests/test_eig_n_host.py); the only matrices that reach the cap are the
// weighted cyclic ones built for that (tests/servo_modes_numpy.py), which answer FD_MO_NOT_CONVERGED with or without the search.
// On a fleet of 65 536 spread flight conditions about one loop in 7000 does end at the cap: a window of two complex
// pairs under a trailing 2 x 2 with real eigenvalues, on which the standard shift wanders (an explicit double-shift QR step does the
// same) and in which no two consecutive subdiagonals are small, so the search would not have started those sweeps lower either.
//
// Storage.  Unlike the 4 x 4 the window position varies per lane, so the sweeps index the matrix by run-time rows and columns.  The
// reduction runs on named words with compile-time indices (registers on the device); the Hessenberg matrix is then written to a
// word store -- WordMat<N, STRIDE>: word r N + c at col[(r N + c) STRIDE] -- which on the device is the lane's column of an LDS
// array laid out [word][lane] (STRIDE = 64: a lane's bank depends on its lane number alone, whatever word it reads) and on the
// host a plain array (STRIDE = 1).  Deflated eigenvalues are written back into the store: the real part of eigenvalue k stays at
// (k, k), its imaginary part goes to (k, k - 1) -- the subdiagonal that was just found negligible or the one inside the 2 x 2 -- and
// for k = 0 to (0, N - 1); rows and columns above en are never touched again by a sweep.  They are read back with compile-time
// indices, sorted by a branch-free odd-even transposition network into fdyn_modes.h's canonical order (real part descending, ties
// by |Im| descending, within a pair the positive imaginary part first; any correct sort of that total order gives the same words)
// and summarised with mode_summary's formulas over N eigenvalues.
//
// Plain C++ templates, __host__ __device__ under hipcc, so the host check (tests/host/eig_n_check.cpp) runs the very code the
// kernel compiles.  No contraction: one rounding per operation, every sum left to right, in the order written, which is the order
// tests/servo_modes_numpy.py follows.  The only operations are + - * / and sqrt.
#pragma once
#include <stdint.h>
#include "fdyn_eig.hpp"
#include "fdyn_riccati_n.hpp"
#include "../../include/fdyn_servo_lqg.h"
#include "../../include/fdyn_servo_modes.h"

namespace fdyn {

constexpr int EIGN_MAX = 7;

template <int N, int STRIDE>
struct WordMat {
    double* col;
    FD_HD double get(int r, int c) const { return col[(r * N + c) * STRIDE]; }
    FD_HD void set(int r, int c, double v) { col[(r * N + c) * STRIDE] = v; }
};

// a -> Q^T a Q upper Hessenberg: hessenberg4 at size N
template <int N>
FD_HD void hessenberg_n(double (&a)[N][N])
{
#pragma clang fp contract(off)
#pragma unroll
    for (int k = 0; k < N - 2; ++k) {
        const int m = k + 1;
        double below = ::fabs(a[m + 1][k]);
#pragma unroll
        for (int i = m + 2; i < N; ++i) below = below + ::fabs(a[i][k]);
        if (below != 0.0) {
            const double scale = ::fabs(a[m][k]) + below;
            double o[N];
#pragma unroll
            for (int i = m; i < N; ++i) o[i] = a[i][k] / scale;
            double h = o[m] * o[m];
#pragma unroll
            for (int i = m + 1; i < N; ++i) h = h + o[i] * o[i];
            const double rt = ::sqrt(h);
            const double g = o[m] >= 0.0 ? -rt : rt;
            h = h - o[m] * g;
            o[m] = o[m] - g;
#pragma unroll
            for (int j = m; j < N; ++j) {                        // (I - o o^T / h) a
                double f = o[m] * a[m][j];
#pragma unroll
                for (int i = m + 1; i < N; ++i) f = f + o[i] * a[i][j];
                f = f / h;
#pragma unroll
                for (int i = m; i < N; ++i) a[i][j] = a[i][j] - f * o[i];
            }
#pragma unroll
            for (int i = 0; i < N; ++i) {                        // a (I - o o^T / h)
                double f = o[m] * a[i][m];
#pragma unroll
                for (int j = m + 1; j < N; ++j) f = f + o[j] * a[i][j];
                f = f / h;
#pragma unroll
                for (int j = m; j < N; ++j) a[i][j] = a[i][j] - f * o[j];
            }
            a[m][k] = scale * g;
#pragma unroll
            for (int i = m + 1; i < N; ++i) a[i][k] = 0.0;
        }
    }
}

// One Francis double-shift sweep over the window [l, en] of the Hessenberg matrix in the store, en - l >= 2; `its` = sweeps done
// since the last deflation, which picks the exceptional shifts.  Only the window's own rows and columns are touched (eigenvalues
// only: nothing outside it is needed again).  francis_step of fdyn_eig.hpp with 0 -> l and N - 1 -> en.
template <int N, typename H>
FD_HD void francis_window(H& h, int l, int en, int its)
{
#pragma clang fp contract(off)
    double x = h.get(en, en), y = h.get(en - 1, en - 1), w = h.get(en, en - 1) * h.get(en - 1, en);
    if (its == 10) {
        const double s = ::fabs(h.get(l + 1, l)) + ::fabs(h.get(l + 2, l + 1));
        x = 0.75 * s + h.get(l, l); y = x; w = -0.4375 * s * s;
    } else if (its == 20) {
        const double s = ::fabs(h.get(en, en - 1)) + ::fabs(h.get(en - 1, en - 2));
        x = 0.75 * s + h.get(en, en); y = x; w = -0.4375 * s * s;
    }
    // first column of (h - s1)(h - s2), s1 + s2 = x + y, s1 s2 = x y - w, scaled
    double z = h.get(l, l);
    double r = x - z, s = y - z;
    double p = (r * s - w) / h.get(l + 1, l) + h.get(l, l + 1);
    double q = ((h.get(l + 1, l + 1) - z) - r) - s;
    r = h.get(l + 2, l + 1);
    s = (::fabs(p) + ::fabs(q)) + ::fabs(r);
    p = p / s; q = q / s; r = r / s;
#pragma unroll 1
    for (int k = l; k < en; ++k) {
        const bool last = k == en - 1;                           // the reflector has two rows, not three
        double sc = 0.0;
        if (k != l) {
            p = h.get(k, k - 1); q = h.get(k + 1, k - 1);
            sc = ::fabs(p) + ::fabs(q);
            if (!last) { r = h.get(k + 2, k - 1); sc = sc + ::fabs(r); }
            if (sc != 0.0) { p = p / sc; q = q / sc; if (!last) r = r / sc; }
        }
        double nn = p * p + q * q;
        if (!last) nn = nn + r * r;
        const double rt = ::sqrt(nn);
        s = p >= 0.0 ? rt : -rt;
        if (s != 0.0) {
            if (k != l) h.set(k, k - 1, -s * sc);
            p = p + s; x = p / s; y = q / s; q = q / p;
            if (!last) { z = r / s; r = r / p; }
#pragma unroll 1
            for (int j = k; j <= en; ++j) {
                double t = h.get(k, j) + q * h.get(k + 1, j);
                if (!last) { t = t + r * h.get(k + 2, j); h.set(k + 2, j, h.get(k + 2, j) - t * z); }
                h.set(k + 1, j, h.get(k + 1, j) - t * y);
                h.set(k, j, h.get(k, j) - t * x);
            }
            const int bottom = k + 3 < en ? k + 3 : en;
#pragma unroll 1
            for (int i = l; i <= bottom; ++i) {
                double t = x * h.get(i, k) + y * h.get(i, k + 1);
                if (!last) { t = t + z * h.get(i, k + 2); h.set(i, k + 2, h.get(i, k + 2) - t * r); }
                h.set(i, k + 1, h.get(i, k + 1) - t * q);
                h.set(i, k, h.get(i, k) - t);
            }
        }
        if (k != l) {
            h.set(k + 1, k - 1, 0.0);
            if (!last) h.set(k + 2, k - 1, 0.0);
        }
    }
}

// The eigenvalues of m (overwritten by its Hessenberg form) in canonical order; h is the word store the sweeps run in.  False
// when a deflation hit the sweep cap, a word stopped being finite or an eigenvalue is not finite: re and im are then all NaN.
template <int N, typename H>
FD_HD bool eig_n(double (&m)[N][N], H& h, double (&re)[N], double (&im)[N], int& sweeps)
{
#pragma clang fp contract(off)
    static_assert(N >= 2 && N <= EIGN_MAX, "2 <= N <= 7");
    hessenberg_n<N>(m);
    double norm = 0.0;
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = (i > 0 ? i - 1 : 0); j < N; ++j) norm = norm + ::fabs(m[i][j]);
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = 0; j < N; ++j) h.set(i, j, m[i][j]);
    bool failed = !::isfinite(norm);
    sweeps = 0;
    int en = N - 1, its = 0;
#pragma unroll 1
    while (!failed && en >= 0) {
        // the largest k in 1 .. en whose subdiagonal is negligible, 0 when the window reaches the top; the sum of the subdiagonals
        int l = 0;
        double t = 0.0;
#pragma unroll
        for (int k = 1; k < N; ++k) {
            if (k <= en) {
                const double sub = ::fabs(h.get(k, k - 1));
                double s = ::fabs(h.get(k - 1, k - 1)) + ::fabs(h.get(k, k));
                s = s == 0.0 ? norm : s;
                l = sub <= EIG_EPS * s ? k : l;
                t = t + sub;
            }
        }
        if (l == en) {                                           // a real eigenvalue: its real part is in place
            h.set(en, en != 0 ? en - 1 : N - 1, 0.0);
            en -= 1; its = 0;
        } else if (l == en - 1) {                                // a 2 x 2 block
            double re0, im0, re1, im1;
            eig2(h.get(l, l), h.get(l, en), h.get(en, l), h.get(en, en), re0, im0, re1, im1);
            h.set(l, l, re0); h.set(en, en, re1);
            h.set(en, l, im1);
            h.set(l, l != 0 ? l - 1 : N - 1, im0);
            en -= 2; its = 0;
        } else if (its == EIG_MAX_SWEEPS || !::isfinite(t)) {
            failed = true;
        } else {
            francis_window<N>(h, l, en, its);
            ++its; ++sweeps;
        }
    }
#pragma unroll
    for (int k = 0; k < N; ++k) {
        re[k] = h.get(k, k);
        im[k] = h.get(k, k != 0 ? k - 1 : N - 1);
    }
    // odd-even transposition network on (re, |im|, im) descending.  One flag from the six comparisons with & and |, never && and ||:
    // see the note in eig4
#pragma unroll
    for (int round = 0; round < N; ++round)
#pragma unroll
        for (int i = round % 2; i + 1 < N; i += 2) {
            const int j = i + 1;
            const double ri = re[i], rj = re[j], ii = im[i], ij = im[j];
            const double mi = ::fabs(ii), mj = ::fabs(ij);
            const bool sw = (rj > ri) | ((rj == ri) & ((mj > mi) | ((mj == mi) & (ij > ii))));
            re[i] = sw ? rj : ri; im[i] = sw ? ij : ii;
            re[j] = sw ? ri : rj; im[j] = sw ? ii : ij;
        }
    bool fin = true;
#pragma unroll
    for (int k = 0; k < N; ++k) fin = fin && ::isfinite(re[k]) && ::isfinite(im[k]);
    const bool ok = !failed && fin;
    const double nan = __builtin_nan("");
#pragma unroll
    for (int k = 0; k < N; ++k) { re[k] = ok ? re[k] : nan; im[k] = ok ? im[k] : nan; }
    return ok;
}

// the FD_MO_* words of N eigenvalues: mode_summary at size N
template <int N>
FD_HD void mode_summary_n(const double (&re)[N], const double (&im)[N], double (&s)[FD_NMO])
{
#pragma clang fp contract(off)
    double absc = re[0], rad = 0.0, mn = 0.0, zeta = 0.0, nu = 0.0, nc = 0.0;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const double m = ::sqrt(re[k] * re[k] + im[k] * im[k]);
        const double z = m == 0.0 ? 0.0 : -re[k] / m;
        absc = re[k] > absc ? re[k] : absc;
        rad = (k == 0 || m > rad) ? m : rad;
        mn = (k == 0 || m < mn) ? m : mn;
        zeta = (k == 0 || z < zeta) ? z : zeta;
        nu = re[k] > 0.0 ? nu + 1.0 : nu;
        nc = im[k] != 0.0 ? nc + 1.0 : nc;
    }
    s[FD_MO_ABSCISSA] = absc; s[FD_MO_RADIUS] = rad; s[FD_MO_MIN_ABS] = mn; s[FD_MO_MIN_ZETA] = zeta;
    s[FD_MO_N_UNSTABLE] = nu; s[FD_MO_N_COMPLEX] = nc;
}

// ---- one block of one lane ---------------------------------------------------------------------------------------------------------
// m (every word finite) -> its N eigenvalues and summary words stored at eig_re / eig_im [k n] and summary [k n] (or NULL); -0
// enters as +0.  Returns eig_n's flag; the block's sweeps are folded into it_max.
template <int N, int STRIDE>
FD_HD bool modes_block(double (&m)[N][N], double* store, int64_t n, double* __restrict__ eig_re, double* __restrict__ eig_im,
                       double* __restrict__ summary, int& it_max)
{
#pragma clang fp contract(off)
#pragma unroll
    for (int r = 0; r < N; ++r)
#pragma unroll
        for (int c = 0; c < N; ++c) m[r][c] = m[r][c] + 0.0;
    WordMat<N, STRIDE> h{ store };
    double re[N], im[N];
    int sweeps;
    const bool ok = eig_n<N>(m, h, re, im, sweeps);
    it_max = sweeps > it_max ? sweeps : it_max;
#pragma unroll
    for (int k = 0; k < N; ++k) { eig_re[int64_t(k) * n] = re[k]; eig_im[int64_t(k) * n] = im[k]; }
    if (summary) {
        double s[FD_NMO];
        mode_summary_n<N>(re, im, s);
#pragma unroll
        for (int k = 0; k < FD_NMO; ++k) summary[int64_t(k) * n] = ok ? s[k] : __builtin_nan("");
    }
    return ok;
}

template <int N>
FD_HD bool all_finite(const double (&m)[N][N])
{
    bool fin = true;
#pragma unroll
    for (int r = 0; r < N; ++r)
#pragma unroll
        for (int c = 0; c < N; ++c) fin = fin && ::isfinite(m[r][c]);
    return fin;
}

// the end of every lane: status, iterations, and NaN over every eigenvalue and summary word of a lane that has no report
FD_HD void modes_finish(bool bad, bool failed, int it_max, int n_eig, int n_sum, int64_t n, double* __restrict__ eig_re,
                        double* __restrict__ eig_im, double* __restrict__ summary, int32_t* __restrict__ iters, int32_t* __restrict__ status)
{
    const int st = bad ? FD_MO_BAD_INPUT : (failed ? FD_MO_NOT_CONVERGED : 0);
    if (st) {
        const double nan = __builtin_nan("");
#pragma unroll 1
        for (int k = 0; k < n_eig; ++k) { eig_re[int64_t(k) * n] = nan; eig_im[int64_t(k) * n] = nan; }
        if (summary) {
#pragma unroll 1
            for (int k = 0; k < n_sum; ++k) summary[int64_t(k) * n] = nan;
        }
    }
    if (iters) *iters = bad ? 0 : it_max;
    *status = st;
}

// rows and columns of the two blocks inside the 12 states, as servo_design_kernel reads them
FD_HD int servo_state_word(int blk, int r)
{
    return blk ? (r == 0 ? FD_X_V : r == 1 ? FD_X_P : r == 2 ? FD_X_R : r == 3 ? FD_X_ROLL : FD_X_YAW)
               : (r == 0 ? FD_X_U : r == 1 ? FD_X_W : r == 2 ? FD_X_Q : r == 3 ? FD_X_PITCH : FD_X_D);
}

// element (j, c) of the integrator rows C_i of block blk: longitudinal (cu, cw, 0, 0, 0) and (0, 0, 0, 0, -1), lateral (0, 0, 0, 0, 1)
FD_HD double servo_integrator_row(int blk, int j, int c, double cu, double cw)
{
    if (blk) return c == FD_SK_NB - 1 ? 1.0 : 0.0;
    if (j == 0) return c == 0 ? cu : (c == 1 ? cw : 0.0);
    return c == FD_SK_NB - 1 ? -1.0 : 0.0;
}

// The continuous augmented closed loop of block BLK, NA = 7 | 6: rows 0-4 a - (b_0 k_0 + b_1 k_1) with a = 0.0 in the integrator
// columns, rows 5.. the integrator rows of the model (b is zero there).  False when a word read or an element is not finite.
template <int BLK>
FD_HD bool servo_continuous_block(const double* __restrict__ A, const double* __restrict__ B, const double* __restrict__ K, int64_t n,
                                  double cu, double cw, double (&m)[BLK ? FD_SV_NLAT : FD_SV_NLON][BLK ? FD_SV_NLAT : FD_SV_NLON])
{
#pragma clang fp contract(off)
    constexpr int NA = BLK ? FD_SV_NLAT : FD_SV_NLON, NB = FD_SK_NB;
    const int c0 = BLK ? FD_U_AILERON : FD_U_ELEVATOR, c1 = BLK ? FD_U_RUDDER : FD_U_THROTTLE;
    const double* Kb = K + int64_t(BLK ? FD_SVK_LAT : FD_SVK_LON) * n;
    double k[2][NA];
    bool fin = true;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int c = 0; c < NA; ++c) { k[j][c] = Kb[int64_t(j * NA + c) * n]; fin = fin && ::isfinite(k[j][c]); }
#pragma unroll
    for (int r = 0; r < NB; ++r) {
        const int sr = servo_state_word(BLK, r);
        const double b0 = B[int64_t(sr * FD_NU + c0) * n], b1 = B[int64_t(sr * FD_NU + c1) * n];
        fin = fin && ::isfinite(b0) && ::isfinite(b1);
#pragma unroll
        for (int c = 0; c < NA; ++c) {
            const double a = c < NB ? A[int64_t(sr * FD_NX + servo_state_word(BLK, c < NB ? c : 0)) * n] : 0.0;
            m[r][c] = a - (b0 * k[0][c] + b1 * k[1][c]);
        }
    }
#pragma unroll
    for (int j = 0; j < NA - NB; ++j)
#pragma unroll
        for (int c = 0; c < NA; ++c) m[NB + j][c] = c < NB ? servo_integrator_row(BLK, j, c < NB ? c : 0, cu, cw) : 0.0;
    return fin && all_finite(m);
}

// The loop of block BLK as fdyn_servo_step_* flies it in its linear region, [[Phi - Gamma Kx, -Gamma Ki], [dt C_i, I]], every element
// formed as fdyn_servo_margin.hpp forms it for its certificate (the lateral block without that header's zero integrator).
template <int BLK>
FD_HD bool servo_sampled_block(const double* __restrict__ K, const double* __restrict__ F, int64_t n, double dt, double cu, double cw,
                               double (&m)[BLK ? FD_SV_NLAT : FD_SV_NLON][BLK ? FD_SV_NLAT : FD_SV_NLON])
{
#pragma clang fp contract(off)
    constexpr int NA = BLK ? FD_SV_NLAT : FD_SV_NLON, NB = FD_SK_NB, NI = NA - NB;
    const double* Kb = K + int64_t(BLK ? FD_SVK_LAT : FD_SVK_LON) * n;
    const double* Fphi = F + int64_t(BLK ? FD_SKF_PHI_LAT : FD_SKF_PHI_LON) * n;
    const double* Fgam = F + int64_t(BLK ? FD_SKF_GAMMA_LAT : FD_SKF_GAMMA_LON) * n;
    double k[2][NA];
    bool fin = true;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int c = 0; c < NA; ++c) { k[j][c] = Kb[int64_t(j * NA + c) * n]; fin = fin && ::isfinite(k[j][c]); }
#pragma unroll
    for (int r = 0; r < NB; ++r) {
        const double g0 = Fgam[int64_t(2 * r) * n], g1 = Fgam[int64_t(2 * r + 1) * n];
        fin = fin && ::isfinite(g0) && ::isfinite(g1);
#pragma unroll
        for (int q = 0; q < NB; ++q) {
            const double phi = Fphi[int64_t(r * NB + q) * n];
            fin = fin && ::isfinite(phi);
            m[r][q] = phi - (g0 * k[0][q] + g1 * k[1][q]);
        }
#pragma unroll
        for (int j = 0; j < NI; ++j) m[r][NB + j] = -(g0 * k[0][NB + j] + g1 * k[1][NB + j]);
    }
#pragma unroll
    for (int j = 0; j < NI; ++j) {
#pragma unroll
        for (int q = 0; q < NB; ++q) m[NB + j][q] = dt * servo_integrator_row(BLK, j, q, cu, cw);
#pragma unroll
        for (int q = 0; q < NI; ++q) m[NB + j][NB + q] = j == q ? 1.0 : 0.0;
    }
    return fin && all_finite(m);
}

// ---- one lane of each entry point: see include/fdyn_servo_modes.h for what is read and written ---------------------------------------
// Every pointer is at the lane's own column, `n` is the distance between consecutive words of it (1 on the host); `store` holds
// 49 words at stride STRIDE.

// CONTINUOUS: fdyn_servo_flight_modes (A, B, x0, K); otherwise fdyn_servo_sampled_modes (K, F, x0, dt), A = F and B unused
template <bool CONTINUOUS, int STRIDE>
FD_HD void servo_modes_lane(double* store, const double* __restrict__ A, const double* __restrict__ B, const double* __restrict__ x0,
                            const double* __restrict__ K, double dt, int64_t n, double* __restrict__ eig_re, double* __restrict__ eig_im,
                            double* __restrict__ summary, int32_t* __restrict__ iters, int32_t* __restrict__ status)
{
#pragma clang fp contract(off)
    const double u0 = x0[int64_t(FD_X_U) * n], w0 = x0[int64_t(FD_X_W) * n];       // of x0 only these two words are read
    const double V0 = ::sqrt(u0 * u0 + w0 * w0);
    bool bad = !(::isfinite(u0) && ::isfinite(w0) && V0 > 0.0);
    if (!CONTINUOUS) bad = bad || !(dt > 1e-6) || dt > 1.0;
    const double cu = u0 / V0, cw = w0 / V0;
    bool failed = false;
    int it_max = 0;
    {
        double m[FD_SV_NLON][FD_SV_NLON];
        const bool fin = CONTINUOUS ? servo_continuous_block<0>(A, B, K, n, cu, cw, m) : servo_sampled_block<0>(K, A, n, dt, cu, cw, m);
        bad = bad || !fin;
        if (!bad) failed = !modes_block<FD_SV_NLON, STRIDE>(m, store, n, eig_re, eig_im, summary, it_max);
    }
    {
        double m[FD_SV_NLAT][FD_SV_NLAT];
        const bool fin = CONTINUOUS ? servo_continuous_block<1>(A, B, K, n, cu, cw, m) : servo_sampled_block<1>(K, A, n, dt, cu, cw, m);
        bad = bad || !fin;
        if (!bad)
            failed = !modes_block<FD_SV_NLAT, STRIDE>(m, store, n, eig_re + int64_t(FD_SV_NLON) * n, eig_im + int64_t(FD_SV_NLON) * n,
                                                      summary ? summary + int64_t(FD_NMO) * n : nullptr, it_max) || failed;
    }
    modes_finish(bad, failed, it_max, FD_NSMO_EIG, 2 * FD_NMO, n, eig_re, eig_im, summary, iters, status);
}

// (I - L) Phi of block blk of F, the product as fdyn_servo_margin.hpp forms its A1.  False when a word read or an element is not finite.
FD_HD bool servo_filter_block(const double* __restrict__ F, int blk, int64_t n, double (&m)[FD_SK_NB][FD_SK_NB])
{
#pragma clang fp contract(off)
    constexpr int NB = FD_SK_NB;
    const double* Fphi = F + int64_t(blk ? FD_SKF_PHI_LAT : FD_SKF_PHI_LON) * n;
    const double* Fl = F + int64_t(blk ? FD_SKF_L_LAT : FD_SKF_L_LON) * n;
    MN<NB> Phi, ImL;
    bool fin = true;
#pragma unroll
    for (int r = 0; r < NB; ++r)
#pragma unroll
        for (int c = 0; c < NB; ++c) {
            Phi.v[r][c] = Fphi[int64_t(r * NB + c) * n];
            const double l = Fl[int64_t(r * NB + c) * n];
            ImL.v[r][c] = (r == c ? 1.0 : 0.0) - l;
            fin = fin && ::isfinite(Phi.v[r][c]) && ::isfinite(l);
        }
    const MN<NB> A1 = mul<false, false>(ImL, Phi);
#pragma unroll
    for (int r = 0; r < NB; ++r)
#pragma unroll
        for (int c = 0; c < NB; ++c) m[r][c] = A1.v[r][c];
    return fin && all_finite(m);
}

// fdyn_servo_filter_modes: both 5 x 5 blocks, one after the other as the servo's two loops above
template <int STRIDE>
FD_HD void servo_filter_modes_lane(double* store, const double* __restrict__ F, int64_t n, double* __restrict__ eig_re,
                                   double* __restrict__ eig_im, double* __restrict__ summary, int32_t* __restrict__ iters,
                                   int32_t* __restrict__ status)
{
    constexpr int NB = FD_SK_NB;
    bool bad = false, failed = false;
    int it_max = 0;
    {
        double m[NB][NB];
        bad = !servo_filter_block(F, 0, n, m);
        if (!bad) failed = !modes_block<NB, STRIDE>(m, store, n, eig_re, eig_im, summary, it_max);
    }
    {
        double m[NB][NB];
        bad = !servo_filter_block(F, 1, n, m) || bad;
        if (!bad)
            failed = !modes_block<NB, STRIDE>(m, store, n, eig_re + int64_t(NB) * n, eig_im + int64_t(NB) * n,
                                              summary ? summary + int64_t(FD_NMO) * n : nullptr, it_max) || failed;
    }
    modes_finish(bad, failed, it_max, FD_NSMO_FILTER_EIG, 2 * FD_NMO, n, eig_re, eig_im, summary, iters, status);
}

// fdyn_square_modes: one row-major N x N taken as it is
template <int N, int STRIDE>
FD_HD void square_modes_lane(double* store, const double* __restrict__ M, int64_t n, double* __restrict__ eig_re,
                             double* __restrict__ eig_im, double* __restrict__ summary, int32_t* __restrict__ iters,
                             int32_t* __restrict__ status)
{
    double m[N][N];
#pragma unroll
    for (int r = 0; r < N; ++r)
#pragma unroll
        for (int c = 0; c < N; ++c) m[r][c] = M[int64_t(r * N + c) * n];
    const bool bad = !all_finite(m);
    bool failed = false;
    int it_max = 0;
    if (!bad) failed = !modes_block<N, STRIDE>(m, store, n, eig_re, eig_im, summary, it_max);
    modes_finish(bad, failed, it_max, N, FD_NMO, n, eig_re, eig_im, summary, iters, status);
}

}  // namespace fdyn

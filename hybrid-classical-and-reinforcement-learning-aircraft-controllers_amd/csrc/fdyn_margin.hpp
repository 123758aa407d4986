// fdyn_margin.hpp -- the loop margins of one aircraft as it is flown (margin_kernels.hip): sampled at dt, through the estimator.
// Per 4-state block the return difference I + L_i(z) at the plant input is evaluated on a grid of points z = exp(j omega dt) of
// the unit circle, and its smallest singular value is minimised over the grid; the nominal loop is certified stable by squaring.
//
// Plain C++ templates, __host__ __device__ under hipcc, so the host check (tests/host/margin_check.cpp) runs the very code the
// kernel compiles.  The block matrices of a lane (Phi, Gamma, Kb, L_kf, F_c: 64 words) live behind a word store W with
// get(k) / set(k, v) -- LDS columns on the device, an array on the host -- and are re-read at every grid point; everything else
// is named words indexed by compile-time constants: registers on the device, never scratch.  No contraction: one rounding per
// operation, in the order written, which is the order tests/margin_numpy.py follows.  The only operations are + - * / and sqrt.
#pragma once
#include <stdint.h>
#include "fdyn_riccati.hpp"
#include "../../include/fdyn_layout.h"

namespace fdyn {

enum { MW_PHI = 0, MW_GAMMA = 16, MW_K = 24, MW_L = 32, MW_FC = 48, MW_N = 64 };      // a lane's words in the store
constexpr int MRG_MAX_SQUARINGS = 30;
constexpr int MRG_MAX_OMEGA = 256;

// The block matrices never change inside the grid loop, and a compiler that sees it hoists their loads out of the loop into
// registers that then live across the elimination: this makes it read them again.
FD_HD void reread_words() { asm volatile("" ::: "memory"); }

// a x = b over the complex numbers, M right-hand sides: fdyn_dense.hpp's elimination with the pivot size |re| + |im| (no square
// root), row swaps as selects, every multiplier a product with the pivot's reciprocal conj(p) / |p|^2.  a and b are overwritten.
// Returns false (singular) when a pivot is below pivot_rel * max(|re| + |im|) of a, is zero or is not a number.
template <int N, int M>
FD_HD bool cgauss_solve(double (&ar)[N][N], double (&ai)[N][N], double (&br)[N][M], double (&bi)[N][M], double (&xr)[N][M],
                        double (&xi)[N][M], double pivot_rel)
{
#pragma clang fp contract(off)
    double mx = 0.0;
#pragma unroll
    for (int r = 0; r < N; ++r)
#pragma unroll
        for (int c = 0; c < N; ++c) mx = nan_max(mx, ::fabs(ar[r][c]) + ::fabs(ai[r][c]));
    const double floor_ = pivot_rel * mx;
    double ivr[N], ivi[N];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        int p = k;
        double best = ::fabs(ar[k][k]) + ::fabs(ai[k][k]);
#pragma unroll
        for (int r = k + 1; r < N; ++r) {
            const double v = ::fabs(ar[r][k]) + ::fabs(ai[r][k]);
            const bool t = v > best;
            best = t ? v : best;
            p = t ? r : p;
        }
#pragma unroll
        for (int r = k + 1; r < N; ++r) {
            const bool sw = p == r;
#pragma unroll
            for (int c = k; c < N; ++c) {
                const double t = ar[k][c]; ar[k][c] = sw ? ar[r][c] : t; ar[r][c] = sw ? t : ar[r][c];
                const double u = ai[k][c]; ai[k][c] = sw ? ai[r][c] : u; ai[r][c] = sw ? u : ai[r][c];
            }
#pragma unroll
            for (int c = 0; c < M; ++c) {
                const double t = br[k][c]; br[k][c] = sw ? br[r][c] : t; br[r][c] = sw ? t : br[r][c];
                const double u = bi[k][c]; bi[k][c] = sw ? bi[r][c] : u; bi[r][c] = sw ? u : bi[r][c];
            }
        }
        ok = ok && (best >= floor_) && (best > 0.0);             // false for NaN
        const double pr = ar[k][k], pi = ai[k][k];
        const double den = pr * pr + pi * pi;
        ivr[k] = pr / den;
        ivi[k] = -pi / den;
#pragma unroll
        for (int r = k + 1; r < N; ++r) {
            const double mr = ar[r][k] * ivr[k] - ai[r][k] * ivi[k];
            const double mi = ar[r][k] * ivi[k] + ai[r][k] * ivr[k];
#pragma unroll
            for (int c = k + 1; c < N; ++c) {
                const double tr = mr * ar[k][c] - mi * ai[k][c], ti = mr * ai[k][c] + mi * ar[k][c];
                ar[r][c] = ar[r][c] - tr;
                ai[r][c] = ai[r][c] - ti;
            }
#pragma unroll
            for (int c = 0; c < M; ++c) {
                const double tr = mr * br[k][c] - mi * bi[k][c], ti = mr * bi[k][c] + mi * br[k][c];
                br[r][c] = br[r][c] - tr;
                bi[r][c] = bi[r][c] - ti;
            }
        }
    }
#pragma unroll
    for (int k = N - 1; k >= 0; --k)
#pragma unroll
        for (int j = 0; j < M; ++j) {
            double sr = br[k][j], si = bi[k][j];
#pragma unroll
            for (int c = k + 1; c < N; ++c) {
                const double tr = ar[k][c] * xr[c][j] - ai[k][c] * xi[c][j], ti = ar[k][c] * xi[c][j] + ai[k][c] * xr[c][j];
                sr = sr - tr;
                si = si - ti;
            }
            xr[k][j] = sr * ivr[k] - si * ivi[k];
            xi[k][j] = sr * ivi[k] + si * ivr[k];
        }
    return ok;
}

// |m|_inf: the largest row sum of magnitudes, each row summed left to right; NaN in any element -> NaN
FD_HD double row_norm(const M4& m)
{
#pragma clang fp contract(off)
    double nrm = 0.0;
#pragma unroll
    for (int r = 0; r < RIC_N; ++r) {
        double rs = ::fabs(m.v[r][0]);
#pragma unroll
        for (int c = 1; c < RIC_N; ++c) rs = rs + ::fabs(m.v[r][c]);
        nrm = nan_max(nrm, rs);
    }
    return nrm;
}

// The stability certificate: m <- m m until |m|_inf < 1, at most MRG_MAX_SQUARINGS times.  |m^(2^k)|_inf < 1 proves
// rho(m)^(2^k) = rho(m^(2^k)) < 1.  A non-finite word (an unstable m overflows) or the cap: not certified.
FD_HD bool schur_by_squaring(M4 m)
{
#pragma unroll 1
    for (int squarings = 0;; ++squarings) {
        const double nrm = row_norm(m);
        if (!::isfinite(nrm)) return false;
        if (nrm < 1.0) return true;
        if (squarings == MRG_MAX_SQUARINGS) return false;
        m = mul<false, false>(m, m);
    }
}

// the larger singular value of a complex 2 x 2 and |det|, in closed form: F = |m|_F^2, D2 = |det m|^2,
// s_max^2 = (F + sqrt(max(F^2 - 4 D2, 0))) / 2; the smaller singular value is then sqrt(D2) / s_max
FD_HD void sigma_2x2(const double (&mr)[2][2], const double (&mi)[2][2], double& smax, double& absdet)
{
#pragma clang fp contract(off)
    double F = mr[0][0] * mr[0][0] + mi[0][0] * mi[0][0];
    F = F + mr[0][1] * mr[0][1]; F = F + mi[0][1] * mi[0][1];
    F = F + mr[1][0] * mr[1][0]; F = F + mi[1][0] * mi[1][0];
    F = F + mr[1][1] * mr[1][1]; F = F + mi[1][1] * mi[1][1];
    const double dr = (mr[0][0] * mr[1][1] - mi[0][0] * mi[1][1]) - (mr[0][1] * mr[1][0] - mi[0][1] * mi[1][0]);
    const double di = (mr[0][0] * mi[1][1] + mi[0][0] * mr[1][1]) - (mr[0][1] * mi[1][0] + mi[0][1] * mr[1][0]);
    const double D2 = dr * dr + di * di;
    double disc = F * F - 4.0 * D2;
    disc = disc > 0.0 ? disc : 0.0;
    smax = ::sqrt(0.5 * (F + ::sqrt(disc)));
    absdet = ::sqrt(D2);
}

// One grid point z = (zr, zi) of one block: sig_s = sigma_min(I + L_i(z)), inv_sig_t = 1 / sigma_max(T(z)), T = L_i (I + L_i)^-1.
//   G = (z I - Phi)^-1 Gamma;   L_i = Kb G   (measurement or truth feedback)
//   L_i = z Kb (z I - F_c)^-1 L_kf G   (estimate feedback): two passes through ONE rolled copy of the elimination
// False when a solve met a singular pivot.
template <typename W>
FD_HD bool margin_point(const W& w, bool estimate, double zr, double zi, double& sig_s, double& inv_sig_t)
{
#pragma clang fp contract(off)
    double xr[RIC_N][2], xi[RIC_N][2];
    bool ok = true;
    const int passes = estimate ? 2 : 1;
#pragma unroll 1
    for (int pass = 0; pass < passes; ++pass) {
        reread_words();
        const int mat = pass ? MW_FC : MW_PHI;
        double ar[RIC_N][RIC_N], ai[RIC_N][RIC_N], br[RIC_N][2], bi[RIC_N][2];
#pragma unroll
        for (int r = 0; r < RIC_N; ++r)
#pragma unroll
            for (int c = 0; c < RIC_N; ++c) {
                ar[r][c] = (r == c ? zr : 0.0) - w.get(mat + RIC_N * r + c);
                ai[r][c] = r == c ? zi : 0.0;
            }
        if (pass) {                                              // L_kf x, each element summed k = 0..3 in that order
#pragma unroll
            for (int r = 0; r < RIC_N; ++r)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    double sr = w.get(MW_L + RIC_N * r) * xr[0][j], si = w.get(MW_L + RIC_N * r) * xi[0][j];
#pragma unroll
                    for (int k = 1; k < RIC_N; ++k) {
                        sr = sr + w.get(MW_L + RIC_N * r + k) * xr[k][j];
                        si = si + w.get(MW_L + RIC_N * r + k) * xi[k][j];
                    }
                    br[r][j] = sr;
                    bi[r][j] = si;
                }
        } else {
#pragma unroll
            for (int r = 0; r < RIC_N; ++r)
#pragma unroll
                for (int j = 0; j < 2; ++j) { br[r][j] = w.get(MW_GAMMA + 2 * r + j); bi[r][j] = 0.0; }
        }
        ok = cgauss_solve<RIC_N, 2>(ar, ai, br, bi, xr, xi, RIC_PIVOT_REL) && ok;
    }
    double lr[2][2], li[2][2], mr[2][2], mi[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            double sr = w.get(MW_K + RIC_N * a) * xr[0][j], si = w.get(MW_K + RIC_N * a) * xi[0][j];
#pragma unroll
            for (int k = 1; k < RIC_N; ++k) {
                sr = sr + w.get(MW_K + RIC_N * a + k) * xr[k][j];
                si = si + w.get(MW_K + RIC_N * a + k) * xi[k][j];
            }
            const double er = sr * zr - si * zi, ei = sr * zi + si * zr;      // the estimator's one-step lead
            lr[a][j] = estimate ? er : sr;
            li[a][j] = estimate ? ei : si;
            mr[a][j] = a == j ? 1.0 + lr[a][j] : lr[a][j];
            mi[a][j] = li[a][j];
        }
    double smax, absdet;
    sigma_2x2(mr, mi, smax, absdet);
    sig_s = absdet / smax;
    // T = L_i adj(M) / det M: sigma_max(T) = sigma_max(L_i adj(M)) / |det M|
    double nr[2][2], ni[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        nr[a][0] = (lr[a][0] * mr[1][1] - li[a][0] * mi[1][1]) - (lr[a][1] * mr[1][0] - li[a][1] * mi[1][0]);
        ni[a][0] = (lr[a][0] * mi[1][1] + li[a][0] * mr[1][1]) - (lr[a][1] * mi[1][0] + li[a][1] * mr[1][0]);
        nr[a][1] = (lr[a][1] * mr[0][0] - li[a][1] * mi[0][0]) - (lr[a][0] * mr[0][1] - li[a][0] * mi[0][1]);
        ni[a][1] = (lr[a][1] * mi[0][0] + li[a][1] * mr[0][0]) - (lr[a][0] * mi[0][1] + li[a][0] * mr[0][1]);
    }
    double nmax, ndet;
    sigma_2x2(nr, ni, nmax, ndet);
    inv_sig_t = absdet / nmax;
    return ok;
}

// One lane, both blocks.  K, F, the alpha / idx words, curve and status point at the lane's own column; `n` is the distance
// between consecutive words of it (1 on the host).  See include/fdyn.h (fdyn_loop_margins) for what is written.
template <typename W>
FD_HD void margin_lane(W& w, const double* __restrict__ K, const double* __restrict__ F, int64_t n, int feedback,
                       const double* __restrict__ zre, const double* __restrict__ zim, int n_omega, double* __restrict__ alpha_s,
                       int32_t* __restrict__ idx_s, double* __restrict__ alpha_t, int32_t* __restrict__ idx_t,
                       double* __restrict__ curve, int32_t* __restrict__ status)
{
#pragma clang fp contract(off)
    const bool estimate = feedback == FD_LQG_ESTIMATE;
    const int f_words = estimate ? FD_NKF : FD_KF_L_LON;         // L_kf is read under estimate feedback only
    bool fin = true;
#pragma unroll 1
    for (int k = 0; k < FD_NLQK; ++k) fin = fin && ::isfinite(K[int64_t(k) * n]);
#pragma unroll 1
    for (int k = 0; k < f_words; ++k) fin = fin && ::isfinite(F[int64_t(k) * n]);
    int st = fin ? 0 : FD_MRG_BAD_INPUT;

    if (fin) {
#pragma unroll 1
        for (int blk = 0; blk < 2; ++blk) {
            const double* Kb = K + int64_t(FD_LQK_LON + blk * (FD_LQK_LAT - FD_LQK_LON)) * n;
            const double* Fphi = F + int64_t(FD_KF_PHI_LON + blk * (FD_KF_PHI_LAT - FD_KF_PHI_LON)) * n;
            const double* Fgam = F + int64_t(FD_KF_GAMMA_LON + blk * (FD_KF_GAMMA_LAT - FD_KF_GAMMA_LON)) * n;
            const double* Fl = F + int64_t(FD_KF_L_LON + blk * (FD_KF_L_LAT - FD_KF_L_LON)) * n;
            M4 Phi, ImL, Acl;
            double Gam[RIC_N][2], Kg[2][RIC_N];
#pragma unroll
            for (int r = 0; r < RIC_N; ++r) {
#pragma unroll
                for (int c = 0; c < RIC_N; ++c) {
                    Phi.v[r][c] = Fphi[int64_t(r * RIC_N + c) * n];
                    const double l = estimate ? Fl[int64_t(r * RIC_N + c) * n] : (r == c ? 1.0 : 0.0);
                    ImL.v[r][c] = (r == c ? 1.0 : 0.0) - l;
                    w.set(MW_PHI + RIC_N * r + c, Phi.v[r][c]);
                    w.set(MW_L + RIC_N * r + c, l);
                }
                Gam[r][0] = Fgam[int64_t(2 * r) * n];
                Gam[r][1] = Fgam[int64_t(2 * r + 1) * n];
                w.set(MW_GAMMA + 2 * r, Gam[r][0]);
                w.set(MW_GAMMA + 2 * r + 1, Gam[r][1]);
            }
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int c = 0; c < RIC_N; ++c) { Kg[a][c] = Kb[int64_t(a * RIC_N + c) * n]; w.set(MW_K + RIC_N * a + c, Kg[a][c]); }
#pragma unroll
            for (int r = 0; r < RIC_N; ++r)
#pragma unroll
                for (int c = 0; c < RIC_N; ++c) Acl.v[r][c] = Phi.v[r][c] - (Gam[r][0] * Kg[0][c] + Gam[r][1] * Kg[1][c]);
            const M4 Fc = mul<false, false>(ImL, Acl), Fe = mul<false, false>(ImL, Phi);
#pragma unroll
            for (int r = 0; r < RIC_N; ++r)
#pragma unroll
                for (int c = 0; c < RIC_N; ++c) w.set(MW_FC + RIC_N * r + c, Fc.v[r][c]);

            // nominal stability: Phi - Gamma Kb, and under estimate feedback (I - L_kf) Phi as well (separation)
            bool stable = true;
            const int certs = estimate ? 2 : 1;
#pragma unroll 1
            for (int c = 0; c < certs; ++c) {
                M4 m;
#pragma unroll
                for (int r = 0; r < RIC_N; ++r)
#pragma unroll
                    for (int q = 0; q < RIC_N; ++q) m.v[r][q] = c ? Fe.v[r][q] : Acl.v[r][q];
                stable = schur_by_squaring(m) && stable;
            }
            if (!stable) st |= FD_MRG_NOT_STABLE;

            double best_s = HUGE_VAL, best_t = HUGE_VAL;
            int at_s = 0, at_t = 0;
            bool ok = true;
#pragma unroll 1
            for (int k = 0; k < n_omega; ++k) {
                double s, t;
                const bool solved = margin_point(w, estimate, zre[k], zim[k], s, t);
                ok = ok && solved && ::isfinite(s) && t == t;     // 1 / sigma_max(T) is +inf where L_i = 0
                if (s < best_s) { best_s = s; at_s = k; }
                if (t < best_t) { best_t = t; at_t = k; }
                if (curve) curve[(int64_t(blk) * n_omega + k) * n] = s;
            }
            if (!ok) st |= FD_MRG_SINGULAR;
            alpha_s[int64_t(blk) * n] = best_s;
            alpha_t[int64_t(blk) * n] = best_t;
            idx_s[int64_t(blk) * n] = at_s;
            idx_t[int64_t(blk) * n] = at_t;
        }
    }
    if (st & (FD_MRG_SINGULAR | FD_MRG_BAD_INPUT)) {             // no margin to report: every word of the lane is NaN, index -1
        const double nan = __builtin_nan("");
#pragma unroll 1
        for (int blk = 0; blk < 2; ++blk) {
            alpha_s[int64_t(blk) * n] = nan;
            alpha_t[int64_t(blk) * n] = nan;
            idx_s[int64_t(blk) * n] = -1;
            idx_t[int64_t(blk) * n] = -1;
        }
        if (curve) {
#pragma unroll 1
            for (int k = 0; k < 2 * n_omega; ++k) curve[int64_t(k) * n] = nan;
        }
    }
    *status = st;
}

}  // namespace fdyn

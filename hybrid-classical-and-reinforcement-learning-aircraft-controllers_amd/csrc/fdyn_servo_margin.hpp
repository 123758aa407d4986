// fdyn_servo_margin.hpp -- the loop margins of the LQ servo of one aircraft as it is flown (servo_margin_kernels.hip): the gain of
// fdyn_servo_design through a zero-order hold at dt, its integrators advanced by forward Euler, and under estimate feedback through
// the filter of fdyn_servo_kf_design.  Per block (five physical states, n_i = 2 longitudinal | 1 lateral integrators) the return
// difference I + L_i(z) at the plant input is evaluated on a grid of points z of the unit circle and its smallest singular value is
// minimised over the grid; the nominal loop is certified stable by squaring.  fdyn_margin.hpp's complex elimination and closed-form
// singular values are used as they stand; what is added is the certificate at the augmented size, Kc(z) and the complex F_c(z).
//
// The integrators are scalar accumulators (i_{k+1} = i_k + dt C_i x_k, u_k formed from x_k and i_k), so they enter as a factor:
//   Kc(z) = Kx + E / (z - 1),  E = Ki (dt C_i)  (2 x 5, real);     G(z) = (z I - Phi)^-1 Gamma
//   truth or measurement feedback:  L_i = Kc(z) G(z)
//   estimate feedback:              L_i = z Kc(z) (z I - F_c(z))^-1 L G(z),  F_c(z) = (I - L) Phi - (I - L) Gamma Kc(z)
// and only 5 x 5 complex solves are needed.
//
// Plain C++ templates, __host__ __device__ under hipcc, so the host check (tests/host/servo_margin_check.cpp) runs the very code
// the kernel compiles.  A lane's real block matrices (SW_*: 115 words) live behind a word store W with get(k) / set(k, v) /
// begin_block(blk) and are re-read at every grid point; everything else is named words indexed by compile-time constants.  No
// contraction: one rounding per operation in the order written, which tests/servo_margin_numpy.py follows.  The only operations are
// + - * / and sqrt.
//
// Operation order, fixed:  every sum runs left to right over k = 0, 1, ...;  1 / (z - 1) = conj(z - 1) / |z - 1|^2 formed as
// (wr / den, -wi / den), den = wr wr + wi wi;  a complex product (a + jb)(c + jd) is (ac - bd, ad + bc);  the lateral block carries
// a second, all-zero integrator (its Ki column and C_i row are 0.0), so that both blocks run the same instructions: the zero terms
// are added where the longitudinal block adds its second integrator.  Pivot rule and reciprocal form are cgauss_solve's.
#pragma once
#include <stdint.h>
#include "fdyn_margin.hpp"
#include "fdyn_riccati_n.hpp"
#include "../../include/fdyn_servo_lqg.h"

namespace fdyn {

constexpr int SM_N = FD_SK_NB;           // physical states per block
constexpr int SM_NI = 2;                 // integrators carried per block (the lateral block's second one is zero)
constexpr int SM_NA = SM_N + SM_NI;      // the augmented matrix the certificate squares
// a lane's words in the store: Phi, Gamma, Kx, E = Ki dt C_i, L, (I - L) Phi, (I - L) Gamma
enum { SW_PHI = 0, SW_GAMMA = 25, SW_KX = 35, SW_E = 45, SW_L = 55, SW_A1 = 80, SW_B1 = 105, SW_N = 115 };

// |m|_inf of an N x N matrix: fdyn_margin.hpp's row_norm at size N
template <int N>
FD_HD double row_norm_n(const MN<N>& m)
{
#pragma clang fp contract(off)
    double nrm = 0.0;
#pragma unroll
    for (int r = 0; r < N; ++r) {
        double rs = ::fabs(m.v[r][0]);
#pragma unroll
        for (int c = 1; c < N; ++c) rs = rs + ::fabs(m.v[r][c]);
        nrm = nan_max(nrm, rs);
    }
    return nrm;
}

// fdyn_margin.hpp's stability certificate at size N: m <- m m until |m|_inf < 1, at most MRG_MAX_SQUARINGS times
template <int N>
FD_HD bool schur_by_squaring_n(MN<N> m)
{
#pragma unroll 1
    for (int squarings = 0;; ++squarings) {
        const double nrm = row_norm_n(m);
        if (!::isfinite(nrm)) return false;
        if (nrm < 1.0) return true;
        if (squarings == MRG_MAX_SQUARINGS) return false;
        m = mul<false, false>(m, m);
    }
}

// sigma_min(I + L_i) and 1 / sigma_max(L_i (I + L_i)^-1) of a complex 2 x 2 loop gain, as fdyn_margin.hpp's margin_point ends
FD_HD void return_difference_2x2(const double (&lr)[2][2], const double (&li)[2][2], double& sig_s, double& inv_sig_t)
{
#pragma clang fp contract(off)
    double mr[2][2], mi[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
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
}

// Kc(z) = Kx + E q, q = 1 / (z - 1) = (qr, qi): read from the store
template <typename W>
FD_HD void servo_kc(const W& w, double qr, double qi, double (&kr)[2][SM_N], double (&ki)[2][SM_N])
{
#pragma clang fp contract(off)
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < SM_N; ++c) {
            const double e = w.get(SW_E + SM_N * a + c);
            kr[a][c] = w.get(SW_KX + SM_N * a + c) + e * qr;
            ki[a][c] = e * qi;
        }
}

// One grid point z = (zr, zi) of one block: sig_s = sigma_min(I + L_i(z)), inv_sig_t = 1 / sigma_max(T(z)).  Under estimate feedback
// two passes through ONE rolled copy of the elimination: G = (z I - Phi)^-1 Gamma, then (z I - F_c(z))^-1 L G.  False when a solve
// met a singular pivot (z = 1 makes q, and with it every pivot of the second pass or L_i itself, not a number).
template <typename W>
FD_HD bool servo_margin_point(const W& w, bool estimate, double zr, double zi, double& sig_s, double& inv_sig_t)
{
#pragma clang fp contract(off)
    const double wr = zr - 1.0, wi = zi;
    const double den = wr * wr + wi * wi;
    const double qr = wr / den, qi = -wi / den;
    double xr[SM_N][2], xi[SM_N][2];
    bool ok = true;
    const int passes = estimate ? 2 : 1;
#pragma unroll 1
    for (int pass = 0; pass < passes; ++pass) {
        reread_words();
        double ar[SM_N][SM_N], ai[SM_N][SM_N], br[SM_N][2], bi[SM_N][2];
        if (pass) {
            double kr[2][SM_N], ki[2][SM_N];
            servo_kc(w, qr, qi, kr, ki);
#pragma unroll
            for (int r = 0; r < SM_N; ++r) {
                const double b0 = w.get(SW_B1 + 2 * r), b1 = w.get(SW_B1 + 2 * r + 1);
#pragma unroll
                for (int c = 0; c < SM_N; ++c) {
                    const double gr = b0 * kr[0][c] + b1 * kr[1][c], gi = b0 * ki[0][c] + b1 * ki[1][c];
                    const double fr = w.get(SW_A1 + SM_N * r + c) - gr;          // F_c = (fr, -gi)
                    ar[r][c] = (r == c ? zr : 0.0) - fr;
                    ai[r][c] = (r == c ? zi : 0.0) + gi;
                }
            }
#pragma unroll
            for (int r = 0; r < SM_N; ++r)                      // L x, each element summed k = 0..4 in that order
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    double sr = w.get(SW_L + SM_N * r) * xr[0][j], si = w.get(SW_L + SM_N * r) * xi[0][j];
#pragma unroll
                    for (int k = 1; k < SM_N; ++k) {
                        sr = sr + w.get(SW_L + SM_N * r + k) * xr[k][j];
                        si = si + w.get(SW_L + SM_N * r + k) * xi[k][j];
                    }
                    br[r][j] = sr;
                    bi[r][j] = si;
                }
        } else {
#pragma unroll
            for (int r = 0; r < SM_N; ++r) {
#pragma unroll
                for (int c = 0; c < SM_N; ++c) {
                    ar[r][c] = (r == c ? zr : 0.0) - w.get(SW_PHI + SM_N * r + c);
                    ai[r][c] = r == c ? zi : 0.0;
                }
#pragma unroll
                for (int j = 0; j < 2; ++j) { br[r][j] = w.get(SW_GAMMA + 2 * r + j); bi[r][j] = 0.0; }
            }
        }
        ok = cgauss_solve<SM_N, 2>(ar, ai, br, bi, xr, xi, RIC_PIVOT_REL) && ok;
    }
    reread_words();
    double kr[2][SM_N], ki[2][SM_N], lr[2][2], li[2][2];
    servo_kc(w, qr, qi, kr, ki);
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            double sr = kr[a][0] * xr[0][j] - ki[a][0] * xi[0][j], si = kr[a][0] * xi[0][j] + ki[a][0] * xr[0][j];
#pragma unroll
            for (int k = 1; k < SM_N; ++k) {
                sr = sr + (kr[a][k] * xr[k][j] - ki[a][k] * xi[k][j]);
                si = si + (kr[a][k] * xi[k][j] + ki[a][k] * xr[k][j]);
            }
            const double er = sr * zr - si * zi, ei = sr * zi + si * zr;      // the estimator's one-step lead
            lr[a][j] = estimate ? er : sr;
            li[a][j] = estimate ? ei : si;
        }
    return_difference_2x2(lr, li, sig_s, inv_sig_t);
    return ok;
}

// One lane, both blocks.  K, F, x0, the alpha / idx words, curve and status point at the lane's own column; `n` is the distance
// between consecutive words of it (1 on the host).  See include/fdyn_servo_margins.h for what is written.
template <typename W>
FD_HD void servo_margin_lane(W& w, const double* __restrict__ K, const double* __restrict__ F, const double* __restrict__ x0, int64_t n,
                             double dt, int feedback, const double* __restrict__ zre, const double* __restrict__ zim, int n_omega,
                             double* __restrict__ alpha_s, int32_t* __restrict__ idx_s, double* __restrict__ alpha_t,
                             int32_t* __restrict__ idx_t, double* __restrict__ curve, int32_t* __restrict__ status)
{
#pragma clang fp contract(off)
    const bool estimate = feedback == FD_LQG_ESTIMATE;
    const int f_words = estimate ? FD_NSKF : FD_SKF_L_LON;       // L is read under estimate feedback only
    const double u0 = x0[int64_t(FD_X_U) * n], w0 = x0[int64_t(FD_X_W) * n];     // of x0 only these two words are read
    bool fin = ::isfinite(u0) && ::isfinite(w0);
#pragma unroll 1
    for (int k = 0; k < FD_NSVK; ++k) fin = fin && ::isfinite(K[int64_t(k) * n]);
#pragma unroll 1
    for (int k = 0; k < f_words; ++k) fin = fin && ::isfinite(F[int64_t(k) * n]);
    const double V0 = ::sqrt(u0 * u0 + w0 * w0);
    const bool good = fin && V0 > 0.0 && dt > 1e-6 && !(dt > 1.0);
    int st = good ? 0 : FD_MRG_BAD_INPUT;

    if (good) {
        const double cu = u0 / V0, cw = w0 / V0;
#pragma unroll 1
        for (int blk = 0; blk < 2; ++blk) {
            const int n_i = blk ? 1 : 2, stride = SM_N + n_i;
            w.begin_block(blk);                                 // a store that reads the block's own words from K and F moves on
            const double* Kb = K + int64_t(blk ? FD_SVK_LAT : FD_SVK_LON) * n;
            const double* Fphi = F + int64_t(FD_SKF_PHI_LON + blk * (FD_SKF_PHI_LAT - FD_SKF_PHI_LON)) * n;
            const double* Fgam = F + int64_t(FD_SKF_GAMMA_LON + blk * (FD_SKF_GAMMA_LAT - FD_SKF_GAMMA_LON)) * n;
            const double* Fl = F + int64_t(FD_SKF_L_LON + blk * (FD_SKF_L_LAT - FD_SKF_L_LON)) * n;
            double Gk[SM_N][SM_NI], dC[SM_NI][SM_N];            // Gamma Ki and dt C_i: what the certificate needs beside the store
            {
                MN<SM_N> Phi, ImL;
                double Gam[SM_N][2], Kx[2][SM_N], Ki[2][SM_NI];
#pragma unroll
                for (int r = 0; r < SM_N; ++r) {
#pragma unroll
                    for (int c = 0; c < SM_N; ++c) {
                        Phi.v[r][c] = Fphi[int64_t(r * SM_N + c) * n];
                        const double l = estimate ? Fl[int64_t(r * SM_N + c) * n] : (r == c ? 1.0 : 0.0);
                        ImL.v[r][c] = (r == c ? 1.0 : 0.0) - l;
                        w.set(SW_PHI + SM_N * r + c, Phi.v[r][c]);
                        w.set(SW_L + SM_N * r + c, l);
                    }
                    Gam[r][0] = Fgam[int64_t(2 * r) * n];
                    Gam[r][1] = Fgam[int64_t(2 * r + 1) * n];
                    w.set(SW_GAMMA + 2 * r, Gam[r][0]);
                    w.set(SW_GAMMA + 2 * r + 1, Gam[r][1]);
                }
#pragma unroll
                for (int a = 0; a < 2; ++a) {
#pragma unroll
                    for (int c = 0; c < SM_N; ++c) { Kx[a][c] = Kb[int64_t(a * stride + c) * n]; w.set(SW_KX + SM_N * a + c, Kx[a][c]); }
#pragma unroll
                    for (int j = 0; j < SM_NI; ++j) Ki[a][j] = j < n_i ? Kb[int64_t(a * stride + SM_N + (j < n_i ? j : 0)) * n] : 0.0;
                }
                // C_i: longitudinal (cu, cw, 0, 0, 0) and (0, 0, 0, 0, -1); lateral (0, 0, 0, 0, 1) and a zero row
#pragma unroll
                for (int c = 0; c < SM_N; ++c) {
                    const double c0 = blk ? (c == SM_N - 1 ? 1.0 : 0.0) : (c == 0 ? cu : c == 1 ? cw : 0.0);
                    const double c1 = blk ? 0.0 : (c == SM_N - 1 ? -1.0 : 0.0);
                    dC[0][c] = dt * c0;
                    dC[1][c] = dt * c1;
                }
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int c = 0; c < SM_N; ++c) w.set(SW_E + SM_N * a + c, Ki[a][0] * dC[0][c] + Ki[a][1] * dC[1][c]);
#pragma unroll
                for (int r = 0; r < SM_N; ++r)
#pragma unroll
                    for (int j = 0; j < SM_NI; ++j) Gk[r][j] = Gam[r][0] * Ki[0][j] + Gam[r][1] * Ki[1][j];
                const MN<SM_N> A1 = mul<false, false>(ImL, Phi);
#pragma unroll
                for (int r = 0; r < SM_N; ++r) {
#pragma unroll
                    for (int c = 0; c < SM_N; ++c) w.set(SW_A1 + SM_N * r + c, A1.v[r][c]);
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        double s = ImL.v[r][0] * Gam[0][j];
#pragma unroll
                        for (int k = 1; k < SM_N; ++k) s = s + ImL.v[r][k] * Gam[k][j];
                        w.set(SW_B1 + 2 * r + j, s);
                    }
                }
            }

            // nominal stability: [[Phi - Gamma Kx, -Gamma Ki], [dt C_i, I]], and under estimate feedback (I - L) Phi as well
            // (separation: the integrators are exactly known controller states, the estimation error obeys (I - L) Phi alone);
            // the second is squared inside the same 7 x 7 words, zero outside its 5 x 5
            bool stable = true;
            const int certs = estimate ? 2 : 1;
#pragma unroll 1
            for (int c = 0; c < certs; ++c) {
                reread_words();
                MN<SM_NA> m;
                if (c) {
#pragma unroll
                    for (int r = 0; r < SM_NA; ++r)
#pragma unroll
                        for (int q = 0; q < SM_NA; ++q)
                            m.v[r][q] = (r < SM_N && q < SM_N) ? w.get(SW_A1 + SM_N * (r < SM_N ? r : 0) + (q < SM_N ? q : 0)) : 0.0;
                } else {
#pragma unroll
                    for (int r = 0; r < SM_N; ++r) {
                        const double g0 = w.get(SW_GAMMA + 2 * r), g1 = w.get(SW_GAMMA + 2 * r + 1);
#pragma unroll
                        for (int q = 0; q < SM_N; ++q)
                            m.v[r][q] = w.get(SW_PHI + SM_N * r + q) - (g0 * w.get(SW_KX + q) + g1 * w.get(SW_KX + SM_N + q));
#pragma unroll
                        for (int j = 0; j < SM_NI; ++j) m.v[r][SM_N + j] = -Gk[r][j];
                    }
#pragma unroll
                    for (int j = 0; j < SM_NI; ++j) {
#pragma unroll
                        for (int q = 0; q < SM_N; ++q) m.v[SM_N + j][q] = dC[j][q];
#pragma unroll
                        for (int q = 0; q < SM_NI; ++q) m.v[SM_N + j][SM_N + q] = (j == q && j < n_i) ? 1.0 : 0.0;
                    }
                }
                stable = schur_by_squaring_n(m) && stable;
            }
            if (!stable) st |= FD_MRG_NOT_STABLE;

            double best_s = HUGE_VAL, best_t = HUGE_VAL;
            int at_s = 0, at_t = 0;
            bool ok = true;
#pragma unroll 1
            for (int k = 0; k < n_omega; ++k) {
                double s, t;
                const bool solved = servo_margin_point(w, estimate, zre[k], zim[k], s, t);
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

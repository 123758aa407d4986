// fdyn_eig.hpp -- the eigenvalues of a real 4 x 4 and the summary words of a block's modes (modes_kernels.hip): where the poles
// of one aircraft's longitudinal or lateral block are, open or closed loop, continuous or sampled.
//
// Householder reduction to Hessenberg form (two reflectors), then the Francis double-shift QR step of EISPACK's hqr without
// its search for two small consecutive subdiagonals, with LAPACK's exceptional shifts at sweeps 10 and 20 and a cap of 30 sweeps
// per deflation.  The window never has a lane-varying position: the 4 x 4 is swept whole until a subdiagonal is negligible; a
// split in the middle leaves two 2 x 2 blocks, a split at either end leaves a 3 x 3 that is copied (selects) into a matrix of its
// own and swept whole until it splits into a 1 x 1 and a 2 x 2.  2 x 2 blocks are solved in closed form.  No balancing: the
// reduction and the sweeps are orthogonal similarities, backward stable in |m|, which is what the tests' gate is stated in
// (DESIGN.md 7i).
//
// Plain C++ templates, __host__ __device__ under hipcc, so the host check (tests/host/eig_check.cpp) runs the very code the
// kernel compiles.  Every matrix is named words indexed by compile-time constants: registers on the device, never scratch.  No
// contraction: one rounding per operation, every sum left to right, in the order written, which is the order tests/modes_numpy.py
// follows.  The only operations are + - * / and sqrt.
#pragma once
#include "fdyn_dense.hpp"
#include "../../include/fdyn_layout.h"

namespace fdyn {

constexpr int EIG_N = 4;
constexpr int EIG_MAX_SWEEPS = 30;                       // per deflation
constexpr double EIG_EPS = 2.220446049250313e-16;        // 2^-52: a subdiagonal below EIG_EPS (|h_kk| + |h_k+1,k+1|) is zero

// a -> Q^T a Q upper Hessenberg.  A column that is already zero below its subdiagonal is left alone (no reflector of norm 0, and
// the zero matrix, a diagonal, a triangular or a Hessenberg matrix pass through untouched).
FD_HD void hessenberg4(double (&a)[EIG_N][EIG_N])
{
#pragma clang fp contract(off)
#pragma unroll
    for (int k = 0; k < EIG_N - 2; ++k) {
        const int m = k + 1;
        double below = ::fabs(a[m + 1][k]);
#pragma unroll
        for (int i = m + 2; i < EIG_N; ++i) below = below + ::fabs(a[i][k]);
        if (below != 0.0) {
            const double scale = ::fabs(a[m][k]) + below;
            double o[EIG_N];
#pragma unroll
            for (int i = m; i < EIG_N; ++i) o[i] = a[i][k] / scale;
            double h = o[m] * o[m];
#pragma unroll
            for (int i = m + 1; i < EIG_N; ++i) h = h + o[i] * o[i];
            const double rt = ::sqrt(h);
            const double g = o[m] >= 0.0 ? -rt : rt;
            h = h - o[m] * g;
            o[m] = o[m] - g;
#pragma unroll
            for (int j = m; j < EIG_N; ++j) {                    // (I - o o^T / h) a
                double f = o[m] * a[m][j];
#pragma unroll
                for (int i = m + 1; i < EIG_N; ++i) f = f + o[i] * a[i][j];
                f = f / h;
#pragma unroll
                for (int i = m; i < EIG_N; ++i) a[i][j] = a[i][j] - f * o[i];
            }
#pragma unroll
            for (int i = 0; i < EIG_N; ++i) {                    // a (I - o o^T / h)
                double f = o[m] * a[i][m];
#pragma unroll
                for (int j = m + 1; j < EIG_N; ++j) f = f + o[j] * a[i][j];
                f = f / h;
#pragma unroll
                for (int j = m; j < EIG_N; ++j) a[i][j] = a[i][j] - f * o[j];
            }
            a[m][k] = scale * g;
#pragma unroll
            for (int i = m + 1; i < EIG_N; ++i) a[i][k] = 0.0;
        }
    }
}

// the largest k in 1 .. N-1 whose subdiagonal h[k][k-1] is negligible, 0 when the matrix is unreduced
template <int N>
FD_HD int find_split(const double (&h)[N][N], double norm)
{
#pragma clang fp contract(off)
    int l = 0;
#pragma unroll
    for (int k = 1; k < N; ++k) {
        double s = ::fabs(h[k - 1][k - 1]) + ::fabs(h[k][k]);
        s = s == 0.0 ? norm : s;
        l = ::fabs(h[k][k - 1]) <= EIG_EPS * s ? k : l;
    }
    return l;
}

template <int N>
FD_HD double subdiagonal_sum(const double (&h)[N][N])
{
#pragma clang fp contract(off)
    double t = ::fabs(h[1][0]);
#pragma unroll
    for (int k = 2; k < N; ++k) t = t + ::fabs(h[k][k - 1]);
    return t;
}

// One Francis double-shift sweep over the whole unreduced N x N Hessenberg h (N = 3 or 4); `its` = sweeps done since the last
// deflation, which picks the exceptional shifts.
template <int N>
FD_HD void francis_step(double (&h)[N][N], int its)
{
#pragma clang fp contract(off)
    constexpr int E = N - 1;
    double x = h[E][E], y = h[E - 1][E - 1], w = h[E][E - 1] * h[E - 1][E];
    if (its == 10) {
        const double s = ::fabs(h[1][0]) + ::fabs(h[2][1]);
        x = 0.75 * s + h[0][0]; y = x; w = -0.4375 * s * s;
    } else if (its == 20) {
        const double s = ::fabs(h[E][E - 1]) + ::fabs(h[E - 1][E - 2]);
        x = 0.75 * s + h[E][E]; y = x; w = -0.4375 * s * s;
    }
    // first column of (h - s1)(h - s2), s1 + s2 = x + y, s1 s2 = x y - w, scaled
    double z = h[0][0];
    double r = x - z, s = y - z;
    double p = (r * s - w) / h[1][0] + h[0][1];
    double q = ((h[1][1] - z) - r) - s;
    r = h[2][1];
    s = (::fabs(p) + ::fabs(q)) + ::fabs(r);
    p = p / s; q = q / s; r = r / s;
#pragma unroll
    for (int k = 0; k < E; ++k) {
        const bool last = k == E - 1;                            // the reflector has two rows, not three
        double sc = 0.0;
        if (k != 0) {
            p = h[k][k - 1]; q = h[k + 1][k - 1];
            sc = ::fabs(p) + ::fabs(q);
            if (!last) { r = h[k + 2][k - 1]; sc = sc + ::fabs(r); }
            if (sc != 0.0) { p = p / sc; q = q / sc; if (!last) r = r / sc; }
        }
        double nn = p * p + q * q;
        if (!last) nn = nn + r * r;
        const double rt = ::sqrt(nn);
        s = p >= 0.0 ? rt : -rt;
        if (s != 0.0) {
            if (k != 0) h[k][k - 1] = -s * sc;
            p = p + s; x = p / s; y = q / s; q = q / p;
            if (!last) { z = r / s; r = r / p; }
#pragma unroll
            for (int j = k; j < N; ++j) {
                double t = h[k][j] + q * h[k + 1][j];
                if (!last) { t = t + r * h[k + 2][j]; h[k + 2][j] = h[k + 2][j] - t * z; }
                h[k + 1][j] = h[k + 1][j] - t * y;
                h[k][j] = h[k][j] - t * x;
            }
#pragma unroll
            for (int i = 0; i <= (k + 3 < E ? k + 3 : E); ++i) {
                double t = x * h[i][k] + y * h[i][k + 1];
                if (!last) { t = t + z * h[i][k + 2]; h[i][k + 2] = h[i][k + 2] - t * r; }
                h[i][k + 1] = h[i][k + 1] - t * q;
                h[i][k] = h[i][k] - t;
            }
        }
        if (k != 0) {
            h[k + 1][k - 1] = 0.0;
            if (!last) h[k + 2][k - 1] = 0.0;
        }
    }
}

// Sweep until a subdiagonal is negligible: the split row (1 .. N-1), sweeps added to `its`; `failed` when the cap is reached or
// a word stops being finite.
template <int N>
FD_HD int deflate(double (&h)[N][N], double norm, int& its, bool& failed)
{
    int l = 0, k = 0;
#pragma unroll 1
    while (true) {
        l = find_split<N>(h, norm);
        if (l != 0) break;
        if (k == EIG_MAX_SWEEPS || !::isfinite(subdiagonal_sum<N>(h))) { failed = true; break; }
        francis_step<N>(h, k);
        ++k;
    }
    its += k;
    return l;
}

// eigenvalues of [[a, b], [c, d]]: a triangular block gives its diagonal as it stands; a complex pair has re = (a + d) / 2 in
// both members, the one with the positive imaginary part first
FD_HD void eig2(double a, double b, double c, double d, double& re0, double& im0, double& re1, double& im1)
{
#pragma clang fp contract(off)
    const double p = 0.5 * (a - d), bc = b * c;
    const double disc = p * p + bc;
    if (b == 0.0 || c == 0.0) {
        re0 = a; re1 = d; im0 = 0.0; im1 = 0.0;
    } else if (disc >= 0.0) {
        const double z = ::sqrt(disc);
        const double zz = p + (p >= 0.0 ? z : -z);
        re0 = d + zz;
        re1 = zz != 0.0 ? d - bc / zz : re0;
        im0 = 0.0; im1 = 0.0;
    } else {
        re0 = 0.5 * (a + d); re1 = re0;
        im0 = ::sqrt(-disc); im1 = -im0;
    }
}

// the eigenvalues of m (overwritten) in canonical order: real part descending, then |im| descending, within a pair the positive
// imaginary part first.
// False when a deflation hit the sweep cap or a word stopped being finite: re and im are then whatever the arithmetic gave.
FD_HD bool eig4(double (&h)[EIG_N][EIG_N], double (&re)[EIG_N], double (&im)[EIG_N], int& sweeps)
{
#pragma clang fp contract(off)
    hessenberg4(h);
    double norm = 0.0;
#pragma unroll
    for (int i = 0; i < EIG_N; ++i)
#pragma unroll
        for (int j = (i > 0 ? i - 1 : 0); j < EIG_N; ++j) norm = norm + ::fabs(h[i][j]);
    bool failed = !::isfinite(norm);
    sweeps = 0;
    const int l = failed ? 2 : deflate<4>(h, norm, sweeps, failed);
    // a split at either end: the 3 x 3 that is left, and the 1 x 1 that is out
    const bool top = l == 3;
    double t[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) t[r][c] = top ? h[r][c] : h[r + 1][c + 1];
    const double r1 = top ? h[3][3] : h[0][0];
    const bool two = l == 2;                                     // a split in the middle: two 2 x 2 blocks, nothing to sweep
    const int l3 = (two || failed) ? 2 : deflate<3>(t, norm, sweeps, failed);
    const bool top3 = l3 == 2;
    const double r2 = top3 ? t[2][2] : t[0][0];
    eig2(two ? h[0][0] : (top3 ? t[0][0] : t[1][1]), two ? h[0][1] : (top3 ? t[0][1] : t[1][2]),
         two ? h[1][0] : (top3 ? t[1][0] : t[2][1]), two ? h[1][1] : (top3 ? t[1][1] : t[2][2]), re[0], im[0], re[1], im[1]);
    eig2(two ? h[2][2] : r2, two ? h[2][3] : 0.0, two ? h[3][2] : 0.0, two ? h[3][3] : r1, re[2], im[2], re[3], im[3]);
    // sorting network on (re, |im|, im) descending: poles that share a real part are ordered by |im|, so the two members of a pair
    // stay next to each other (two pairs, or a pair and a real pole, on one vertical line)
    constexpr int NET[5][2] = { { 0, 1 }, { 2, 3 }, { 0, 2 }, { 1, 3 }, { 1, 2 } };
    bool fin = true;
#pragma unroll
    for (int s = 0; s < 5; ++s) {
        const int i = NET[s][0], j = NET[s][1];
        const double ri = re[i], rj = re[j], ii = im[i], ij = im[j];
        const double mi = ::fabs(ii), mj = ::fabs(ij);
        // one flag from the six comparisons with & and |, not && and ||: the swap then compiles to eight v_cndmask on one mask.  The
        // short-circuit form became divergent branches on the device, and poles that tie on the real part came out with only one
        // half of a swap applied (tests/test_gpu_modes.py holds the tie and cyclic matrices to the restatement bit for bit)
        const bool sw = (rj > ri) | ((rj == ri) & ((mj > mi) | ((mj == mi) & (ij > ii))));
        re[i] = sw ? rj : ri; im[i] = sw ? ij : ii;
        re[j] = sw ? ri : rj; im[j] = sw ? ii : ij;
    }
#pragma unroll
    for (int k = 0; k < EIG_N; ++k) fin = fin && ::isfinite(re[k]) && ::isfinite(im[k]);
    return !failed && fin;
}

// the FD_MO_* words of four eigenvalues
FD_HD void mode_summary(const double (&re)[EIG_N], const double (&im)[EIG_N], double (&s)[FD_NMO])
{
#pragma clang fp contract(off)
    double absc = re[0], rad = 0.0, mn = 0.0, zeta = 0.0, nu = 0.0, nc = 0.0;
#pragma unroll
    for (int k = 0; k < EIG_N; ++k) {
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

}  // namespace fdyn

// fdyn_dense.hpp -- the small dense fp64 linear algebra of the design kernels (trim_kernels.hip: the 7 x 7 Newton step;
// lqr_kernels.hip: the 4 x 4 inverses of the doubling algorithm): one elimination, one NaN-aware maximum.
//
// Plain C++ templates, __host__ __device__ under hipcc, so the host check (tests/host/dense_check.cpp) runs the very code the
// kernels compile.  Every loop has compile-time bounds and every index is a constant once unrolled: on the device the arrays
// live in registers, never in scratch.  No contraction: one rounding per operation, in the order written, which is the order
// the fp64 host models of the tests follow.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define FD_HD __host__ __device__ __forceinline__
#else
#define FD_HD inline
#endif

namespace fdyn {

FD_HD double nan_max(double m, double v) { return (v > m || v != v) ? v : m; }     // max, NaN wins and stays

template <int N>
FD_HD double max_abs(const double (&a)[N])                   // max |a|, NaN in any element -> NaN
{
    double m = 0.0;
#pragma unroll
    for (int k = 0; k < N; ++k) m = nan_max(m, ::fabs(a[k]));
    return m;
}

template <int N, int M>
FD_HD double max_abs(const double (&a)[N][M])
{
    double m = 0.0;
#pragma unroll
    for (int r = 0; r < N; ++r) m = nan_max(m, max_abs(a[r]));
    return m;
}

// a x = b for M right-hand sides by elimination with partial pivoting on [a | b] and back substitution; row swaps as selects.
// a and b are overwritten.  Returns false (singular) when a pivot is below pivot_rel * max|a|, is zero or is not a number;
// x is then whatever the arithmetic gave.
template <int N, int M>
FD_HD bool gauss_solve(double (&a)[N][N], double (&b)[N][M], double (&x)[N][M], double pivot_rel)
{
#pragma clang fp contract(off)
    const double floor_ = pivot_rel * max_abs(a);
    bool ok = true;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        int p = k;
        double best = ::fabs(a[k][k]);
#pragma unroll
        for (int r = k + 1; r < N; ++r) { const double v = ::fabs(a[r][k]); const bool t = v > best; best = t ? v : best; p = t ? r : p; }
#pragma unroll
        for (int r = k + 1; r < N; ++r) {
            const bool sw = p == r;
#pragma unroll
            for (int c = k; c < N; ++c) { const double t = a[k][c]; a[k][c] = sw ? a[r][c] : t; a[r][c] = sw ? t : a[r][c]; }
#pragma unroll
            for (int c = 0; c < M; ++c) { const double t = b[k][c]; b[k][c] = sw ? b[r][c] : t; b[r][c] = sw ? t : b[r][c]; }
        }
        ok = ok && (best >= floor_) && (best > 0.0);             // false for NaN
        const double piv = a[k][k];
#pragma unroll
        for (int r = k + 1; r < N; ++r) {
            const double m = a[r][k] / piv;
#pragma unroll
            for (int c = k + 1; c < N; ++c) a[r][c] = a[r][c] - m * a[k][c];
#pragma unroll
            for (int c = 0; c < M; ++c) b[r][c] = b[r][c] - m * b[k][c];
        }
    }
#pragma unroll
    for (int k = N - 1; k >= 0; --k)
#pragma unroll
        for (int j = 0; j < M; ++j) {
            double s = b[k][j];
#pragma unroll
            for (int c = k + 1; c < N; ++c) s = s - a[k][c] * x[c][j];
            x[k][j] = s / a[k][k];
        }
    return ok;
}

}  // namespace fdyn

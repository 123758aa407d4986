// fdyn_wind.hpp -- the two pieces of arithmetic the servo's wind entries (include/fdyn_wind.h) add to the servo step: the
// air-relative body velocity and the gust update.  Host and device, no other header of the library behind it, so that
// tests/host/wind_check.cpp runs the same code on the CPU under the sanitizers and compares it with the NumPy restatement bit for
// bit.  Contraction is off in both: one rounding per operation, in the order written.
#pragma once

#if defined(__HIPCC__)
#define FD_WIND_HD __host__ __device__ __forceinline__
#else
#define FD_WIND_HD inline
#endif

namespace fdyn {

// v_air = v - R^T Wa for the Euler angles given by (sin, cos) pairs and the air-mass velocity Wa (NED): yaw, then pitch, then roll
// as three plane rotations -- body_wind's operations in body_wind's order (fdyn_core.hpp, which is device code), so that the law
// sees the velocity the integrator's aerodynamics see.  With Wa = 0 every product is +-0 and v comes back bit for bit.
template <typename T>
FD_WIND_HD void air_relative(T u, T v, T w, T sphi, T cphi, T sth, T cth, T spsi, T cpsi, T wn, T we, T wd, T& ua, T& va, T& wa)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const T a = cpsi * wn + spsi * we, b = cpsi * we - spsi * wn;
    const T bu = cth * a - sth * wd;
    const T c = sth * a + cth * wd;
    const T bv = cphi * b + sphi * c;
    const T bw = cphi * c - sphi * b;
    ua = u - bu; va = v - bv; wa = w - bw;
}

// first-order Gauss-Markov gust over one control step: g <- (A g) + (B n), two products and one sum
FD_WIND_HD double gust_update(double g, double A, double B, double n)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double ag = A * g, bn = B * n;
    return ag + bn;
}

}  // namespace fdyn

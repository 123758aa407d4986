// fdyn_lqr_law.hpp -- the state-feedback law of the LQR fleets, u = u0 - K delta, for one lane: lqr_kernels.hip feeds it the true
// state, kf_kernels.hip the truth, a noisy measurement or the Kalman filter's estimate.  One copy, so that the output-feedback
// loop fed the truth IS the state-feedback loop, bit for bit.
#pragma once
#include "fdyn_core.hpp"

namespace fdyn {

// u = u0 - K delta for one lane.  The eight differences x - x0 are formed in fp64 from the stored state (exact to the
// state's own rounding, whatever the variant), then everything runs in the glue type.
template <typename G> struct LqrLaw {
    G k[FD_NLQK], u0[FD_NU];
    double x0[8];                                               // u, w, q, theta | v, p, r, phi of the trim
    // the eight regulated words of x - x0, the two angle differences wrapped
    template <typename S>
    FD_DEV void delta(const S (&x)[FD_NX], G (&d)[8]) const
    {
#pragma clang fp contract(off)
        constexpr int W[8] = { FD_X_U, FD_X_W, FD_X_Q, FD_X_PITCH, FD_X_V, FD_X_P, FD_X_R, FD_X_ROLL };
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            d[j] = G(double(x[W[j]]) - x0[j]);
            if (j == 3 || j == 7) d[j] = wrap_angle<G>(d[j]);
        }
    }
    // u0 - K f for any eight words f in delta's order: the truth, a measurement or an estimate
    FD_DEV Surfaces<G> feedback(const G (&d)[8]) const
    {
#pragma clang fp contract(off)
        G s[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int o = (r >> 1) * 4;                          // rows 0, 1: longitudinal words; rows 2, 3: lateral
            G a = k[r * 4] * d[o];
#pragma unroll
            for (int c = 1; c < 4; ++c) a = a + k[r * 4 + c] * d[o + c];
            s[r] = a;
        }
        Surfaces<G> u;
        u.elevator = u0[FD_U_ELEVATOR] - s[0]; u.throttle = u0[FD_U_THROTTLE] - s[1];
        u.aileron = u0[FD_U_AILERON] - s[2]; u.rudder = u0[FD_U_RUDDER] - s[3];
        return u;
    }
    // feedback(delta(x)), written out: only from this form does lqr_step_kernel<double, double> compile to the listing it had
    // before the law was split (the same instructions in another order otherwise); tests/test_gpu_lqg.py holds the two equal
    template <typename S>
    FD_DEV Surfaces<G> operator()(const S (&x)[FD_NX]) const
    {
#pragma clang fp contract(off)
        constexpr int W[8] = { FD_X_U, FD_X_W, FD_X_Q, FD_X_PITCH, FD_X_V, FD_X_P, FD_X_R, FD_X_ROLL };
        G d[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            d[j] = G(double(x[W[j]]) - x0[j]);
            if (j == 3 || j == 7) d[j] = wrap_angle<G>(d[j]);
        }
        G s[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int o = (r >> 1) * 4;                          // rows 0, 1: longitudinal words; rows 2, 3: lateral
            G a = k[r * 4] * d[o];
#pragma unroll
            for (int c = 1; c < 4; ++c) a = a + k[r * 4 + c] * d[o + c];
            s[r] = a;
        }
        Surfaces<G> u;
        u.elevator = u0[FD_U_ELEVATOR] - s[0]; u.throttle = u0[FD_U_THROTTLE] - s[1];
        u.aileron = u0[FD_U_AILERON] - s[2]; u.rudder = u0[FD_U_RUDDER] - s[3];
        return u;
    }
};

template <typename G> FD_DEV bool any_clipped(const Surfaces<G>& u)
{
    return !(u.elevator >= G(-1) && u.elevator <= G(1) && u.aileron >= G(-1) && u.aileron <= G(1)
             && u.rudder >= G(-1) && u.rudder <= G(1) && u.throttle >= G(0) && u.throttle <= G(1));
}

}  // namespace fdyn

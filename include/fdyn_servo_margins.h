/* fdyn_servo_margins.h -- C-ABI of the LQ servo's loop margins (csrc/servo_margin_kernels.hip): how much robustness the servo loop
 * has AS IT IS FLOWN -- the gain of fdyn_servo_design through a zero-order hold at dt, its integrators advanced by forward Euler,
 * and under estimate feedback through the filter of fdyn_servo_kf_design.  A header of its own beside fdyn_servo.h and
 * fdyn_servo_lqg.h, whose conventions hold: every array is a DEVICE pointer, SoA [word][n] row-major fp64 unless marked, `stream` is
 * a hipStream_t passed as void*, the return codes are fdyn.h's, and the entry point neither synchronises nor allocates, so it can be
 * captured into a hipGraph.
 *
 * The loop is the linear region of fdyn_servo_step_* / fdyn_servo_lqg_step_* (no error clip, no saturation, no wrap).  Per block:
 * five physical states (u, w, q, theta, z | v, p, r, phi, psi) and n_i integrators (2 longitudinal, 1 lateral); Kb = [Kx (2 x 5) |
 * Ki (2 x n_i)] from K; Phi, Gamma, L from F; C_i the integrator rows of the augmented model: longitudinal (u0 / V0, w0 / V0, 0, 0, 0)
 * and (0, 0, 0, 0, -1) with V0 = sqrt(u0^2 + w0^2) from the trim x0, lateral (0, 0, 0, 0, 1).  The law forms u_k from x_k and i_k,
 * then i_{k+1} = i_k + dt C_i x_k (xhat_k in the place of x_k under estimate feedback), then the plant steps:
 *   Kc(z) = Kx + Ki (dt C_i) / (z - 1),   G(z) = (z I - Phi)^-1 Gamma
 *   FD_LQG_TRUTH, FD_LQG_MEASUREMENT:  L_i = Kc(z) G(z)
 *   FD_LQG_ESTIMATE:                   L_i = z Kc(z) (z I - F_c(z))^-1 L G(z),   F_c(z) = (I - L) Phi - (I - L) Gamma Kc(z)
 * and per grid point z the 2 x 2 return difference M = I + L_i at the plant input gives sigma_min(M) and 1 / sigma_max(L_i M^-1) in
 * closed form, exactly as fdyn_loop_margins (fdyn.h) forms them.                                                                  */
#ifndef FDYN_SERVO_MARGINS_H
#define FDYN_SERVO_MARGINS_H

#include <stdint.h>
#include "fdyn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* fdyn_servo_loop_margins: K [FD_NSVK][n] as fdyn_servo_design writes it, F [FD_NSKF][n] as fdyn_servo_kf_design writes it at this
 * dt, x0 [FD_NX][n] the trim (only its u and w words are read); feedback FD_LQG_ESTIMATE, FD_LQG_MEASUREMENT or FD_LQG_TRUTH (the
 * last two are the same loop; L is read under FD_LQG_ESTIMATE only); zre, zim [n_omega] the grid points z on the unit circle,
 * 1 <= n_omega <= 256, the same for every aircraft.  One lane per aircraft, fp64.  Written, block 0 longitudinal, block 1 lateral:
 *   alpha_s [2][n]            min over the grid of sigma_min(I + L_i)
 *   idx_s [2][n] int32        the first grid index attaining it
 *   alpha_t [2][n]            min over the grid of 1 / sigma_max(L_i (I + L_i)^-1) (+inf where L_i = 0 on the whole grid)
 *   idx_t [2][n] int32
 *   curve [2][n_omega][n]     or NULL; sigma_min(I + L_i) at every grid point
 *   status [n] int32          FD_MRG_* bits (fdyn_layout.h) with fdyn_loop_margins' meanings, 0 = the disk guarantee holds:
 *     FD_MRG_NOT_STABLE   no certificate by squaring (at most 30 squarings, |.|_inf < 1) for the augmented (5 + n_i)-square matrix
 *                         [[Phi - Gamma Kx, -Gamma Ki], [dt C_i, I]] or, under FD_LQG_ESTIMATE, for (I - L) Phi; alpha is still written
 *     FD_MRG_SINGULAR     a singular pivot or a non-finite sigma_min on the grid; a grid point at z = 1 gives it by construction
 *     FD_MRG_BAD_INPUT    a word read is not finite, V0 is not > 0, or dt is outside (1e-6, 1]
 *   With FD_MRG_SINGULAR or FD_MRG_BAD_INPUT every alpha and curve word of the lane is NaN and every index -1.
 * Refused before any launch: FDYN_ERR_BAD_SIZE for n_omega outside 1..256, an unknown feedback or n < 1; FDYN_ERR_NULL for a missing
 * pointer other than curve.                                                                                                        */
int fdyn_servo_loop_margins(const double* K, const double* F, const double* x0, double dt, int feedback, const double* zre,
                            const double* zim, int n_omega, int64_t n, double* alpha_s, int32_t* idx_s, double* alpha_t,
                            int32_t* idx_t, double* curve, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FDYN_SERVO_MARGINS_H */

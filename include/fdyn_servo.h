/* fdyn_servo.h -- C-ABI of the LQ servo of libfdyn_hip.so (csrc/servo_kernels.hip): LQR with integral action on airspeed, altitude
 * and heading, designed per aircraft and flown in one launch.  A header of its own beside fdyn.h, whose conventions hold: every
 * array is a DEVICE pointer, SoA [word][n] row-major fp64 unless marked, `stream` is a hipStream_t passed as void*, the return
 * codes are fdyn.h's, and no entry point synchronises or allocates, so all can be captured into a hipGraph.  Layout constants
 * (FD_SV*, FD_NSV*): fdyn_layout.h.
 *
 * The model.  Per aircraft two augmented blocks are cut out of A, B as fdyn_linearize writes them, at the trim x0:
 *   longitudinal  (u, w, q, theta, z, i_V, i_h | elevator, throttle): the rows and columns of A at those five state words (z the
 *                 down-position word), then i_V' = (u0 du + w0 dw) / V0 with V0 = sqrt(u0^2 + w0^2) of the trim, and i_h' = -dz
 *   lateral       (v, p, r, phi, psi, i_psi | aileron, rudder): the five state words, then i_psi' = dpsi
 * The integrator rows of b are zero; the coupling between the blocks is dropped, as fdyn_lqr_design drops it.
 *
 * The law, one control step of fdyn_servo_step_* (differences from x0 and from the references are formed in fp64 from the stored
 * state, then everything runs in the variant's glue type):
 *   1. V = sqrt(u^2 + v^2 + w^2); e_V = clip(V - V_c, +-limits[0]); e_h = clip((-z) - h_c, +-limits[1]);
 *      e_psi = clip(wrap(psi - psi_c), +-limits[2])
 *   2. with dV = V_c - V0:  d_lon = (du - dV u0 / V0, dw - dV w0 / V0, dq, wrap(dtheta), -e_h, i_V, i_h)
 *                           d_lat = (dv, dp, dr, wrap(dphi), e_psi, i_psi)
 *   3. u = u0 - K d, each row summed left to right, clipped as set_controls clips; a step with a clipped control counts in sat_steps
 *   4. if neither longitudinal control was clipped: i_V += e_V dt, i_h += e_h dt; if neither lateral one was: i_psi += e_psi dt
 *   5. one RK4 step of dt
 *   6. h_c += hdot_c dt, psi_c = wrap(psi_c + psidot_c dt), in fp64                                                           */
#ifndef FDYN_SERVO_H
#define FDYN_SERVO_H

#include <stdint.h>
#include "fdyn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* fdyn_servo_design: A [FD_NX * FD_NX][n], B [FD_NX * FD_NU][n], x0 [FD_NX][n] (only u0 and w0 are read); weights [FD_NSVW] or, with
 * weights_per_lane != 0, [FD_NSVW][n] (FD_SVW_*).  Both blocks' continuous Riccati equations are solved in fp64, one lane per
 * aircraft, by the doubling algorithm of fdyn_lqr_design at N = 7 and N = 6: K = R^-1 b^T X.
 *   K [FD_NSVK][n]     K_lon 2 x 7 row-major, then K_lat 2 x 6 (FD_SVK_*); zero for a lane with a non-zero status
 *   residual [n]       relative Riccati residual of the worse block (NaN: invalid input)
 *   iters [n] int32    doubling steps of the slower block
 *   status [n] int32   FD_SV_* bits, 0 = a certified stabilising gain                                                          */
int fdyn_servo_design(const double* A, const double* B, const double* x0, const double* weights, int weights_per_lane, int64_t n,
                      double* K, double* residual, int32_t* iters, int32_t* status, void* stream);

/* fdyn_servo_step_*: n_steps control steps (above) in one launch.  x [FD_NX][n] in the variant's storage type, advanced in place;
 * x0 [FD_NX][n], u0 [FD_NU][n] the trim; K as fdyn_servo_design writes it; ref [FD_NSVR][n] (FD_SVR_*: its altitude and heading
 * rows are advanced), integ [FD_NSVI][n] (advanced), limits [FD_NSVI] the error clips; type [n] uint8 or NULL, params
 * [n_types][FD_NP] as every fleet entry point takes them.
 *   surf_out [FD_NU][n]   or NULL; the last controls as applied (after the clip), storage type
 *   sat_steps [n] int32   or NULL; += the steps in which a control was clipped
 *   err_out [FD_NSVI][n]  or NULL; the errors of the last control step before their clip
 * n_steps = 0 computes the controls from the current state into surf_out and writes nothing else.
 * FDYN_ERR_BAD_SIZE for n < 0 or n_steps < 0, FDYN_ERR_BAD_TYPES, FDYN_ERR_NULL for a missing required pointer, FDYN_ERR_BAD_DT,
 * each with no launch.                                                                                                        */
int fdyn_servo_step_f64(double* x, const double* x0, const double* u0, const double* K, double* ref, double* integ, const double* limits,
                        const uint8_t* type, const double* params, int n_types, int64_t n, double dt, int n_steps, double* surf_out,
                        int32_t* sat_steps, double* err_out, void* stream);
int fdyn_servo_step_mixed(double* x, const double* x0, const double* u0, const double* K, double* ref, double* integ, const double* limits,
                          const uint8_t* type, const double* params, int n_types, int64_t n, double dt, int n_steps, double* surf_out,
                          int32_t* sat_steps, double* err_out, void* stream);
int fdyn_servo_step_f32(float* x, const double* x0, const double* u0, const double* K, double* ref, double* integ, const double* limits,
                        const uint8_t* type, const double* params, int n_types, int64_t n, double dt, int n_steps, float* surf_out,
                        int32_t* sat_steps, double* err_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FDYN_SERVO_H */

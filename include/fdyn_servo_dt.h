/* fdyn_servo_dt.h -- C-ABI of the sampled-data design of the LQ servo of libfdyn_hip.so (csrc/servo_dt_kernels.hip): the gain of
 * include/fdyn_servo.h designed for the loop as fdyn_servo_step_* flies it at one step dt -- the plant behind a zero-order hold, the
 * integrators advanced by forward Euler -- by the discrete Riccati equation.  A header of its own beside fdyn_servo.h, whose
 * conventions hold: every array is a DEVICE pointer, SoA [word][n] row-major fp64 unless marked, `stream` is a hipStream_t passed as
 * void*, the return codes are fdyn.h's, and the entry point neither synchronises nor allocates, so it can be captured into a
 * hipGraph.  Layout constants (FD_SV*, FD_NSV*): fdyn_layout.h.
 *
 * Per aircraft and block (N = 7 longitudinal, N = 6 lateral; the cut of A, B and x0 is fdyn_servo_design's):
 *   (Phi, Gamma) = exp of the five physical states over dt and its integral times b (the series of fdyn_servo_kf_design)
 *   A_d = [[Phi, 0], [dt C_i, I]],  B_d = [[Gamma], [0]]        C_i: the integrator rows of the continuous augmented model
 *   H_0 = diag(q) dt,  R_d = diag(r) dt                          the weights of fdyn_servo_design (FD_SVW_*)
 *   X = A_d^T X A_d - A_d^T X B_d (R_d + B_d^T X B_d)^-1 B_d^T X A_d + H_0     by the doubling iteration, started at (A_d, B_d R_d^-1 B_d^T, H_0)
 *   K = (R_d + B_d^T X B_d)^-1 B_d^T X A_d
 * K has the layout of fdyn_servo_design's and is flown, and analysed, by every entry point that takes that one -- at THIS dt.     */
#ifndef FDYN_SERVO_DT_H
#define FDYN_SERVO_DT_H

#include <stdint.h>
#include "fdyn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* fdyn_servo_design_dt: A [FD_NX * FD_NX][n], B [FD_NX * FD_NU][n], x0 [FD_NX][n] (only u0 and w0 are read); weights [FD_NSVW] or,
 * with weights_per_lane != 0, [FD_NSVW][n]; dt the control step the gain will be flown at.  fp64, one lane per aircraft.
 *   K [FD_NSVK][n]     K_lon 2 x 7 row-major, then K_lat 2 x 6 (FD_SVK_*); zero for a lane with a non-zero status
 *   residual [n]       relative residual of the discrete Riccati equation of the worse block (NaN: invalid input)
 *   iters [n] int32    doubling steps of the slower block
 *   status [n] int32   FD_SV_* bits, 0 = a certified stabilising gain:
 *                      FD_SV_NOT_CONVERGED   the doubling loop failed or did not converge within its cap
 *                      FD_SV_NO_CERTIFICATE  X not positive definite, the residual above its bound, R_d + B_d^T X B_d not positive, or
 *                                            A_d - B_d K not certified stable by squaring (the certificate of fdyn_servo_loop_margins)
 *                      FD_SV_BAD_INPUT       what fdyn_servo_design refuses, or |a|_inf dt of a block above the series cap (1.5), as
 *                                            fdyn_servo_kf_design refuses it; nothing is solved
 * FDYN_ERR_BAD_SIZE for n < 0, FDYN_ERR_NULL for a missing pointer, FDYN_ERR_BAD_DT for dt outside (1e-6, 1], each with no launch;
 * n = 0 does nothing.                                                                                                           */
int fdyn_servo_design_dt(const double* A, const double* B, const double* x0, const double* weights, int weights_per_lane,
                         double dt, int64_t n, double* K, double* residual, int32_t* iters, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FDYN_SERVO_DT_H */

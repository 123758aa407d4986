/* fdyn_servo_lqg.h -- C-ABI of the LQ servo on noisy sensors (csrc/servo_kernels.hip): a steady-state Kalman filter on the five
 * physical states of each augmented block of the servo, designed per aircraft, and the servo's control step flown on its estimate.
 * A header of its own beside fdyn_servo.h, whose conventions hold: every array is a DEVICE pointer, SoA [word][n] row-major fp64
 * unless marked, `stream` is a hipStream_t passed as void*, the return codes are fdyn.h's, and no entry point synchronises or
 * allocates, so all can be captured into a hipGraph.
 *
 * The ten estimated words, in this order everywhere below: (u, w, q, theta, z | v, p, r, phi, psi), z the down-position word; the
 * rows and columns of A at those words and the columns (elevator, throttle | aileron, rudder) of B, as fdyn_linearize writes them.
 * Every word is measured (C = I).  The servo's integrators are states of the controller and are not estimated.
 *
 * One control step of fdyn_servo_lqg_step_*:
 *   1. d = the ten words of x - x0, differences formed in fp64 from the stored state, then the glue type; the theta, phi and psi
 *      differences wrapped
 *   2. y = d + sigma z.  With z given, z = z[s][k][i]; otherwise twelve normals from three Philox blocks, counter (row low, row
 *      high, *step + s + 1, FD_PHX_SERVO_LQG + b), b = 0..2, Box-Muller paired as fdyn_lqg_step_* pairs them: (r0, r1) -> cos, sin;
 *      (r2, r3) -> cos, sin.  Words 0..9 go in d's order, the last two are unused.
 *   3. per block, in the glue type, every sum left to right: pred = Phi xhat + Gamma du_prev; e = y - pred with the psi word of e
 *      wrapped; xhat = pred + L e; the psi word of xhat wrapped.  (psi's column of A is zero, so Phi's is the unit vector and a
 *      2 pi shift of xhat_psi commutes with the prediction: the wrap is exact for the model.)
 *   4. err_est += (xhat - d)^2 with the psi difference wrapped, err_meas += (y - d)^2, in fp64
 *   5. f = xhat (FD_LQG_ESTIMATE), y (FD_LQG_MEASUREMENT) or d (FD_LQG_TRUTH).  For the first two the law's input is x_f = x0 + f
 *      on the ten words, summed in fp64 with the psi word wrapped, and the stored state elsewhere; steps 1 to 4 of fdyn_servo.h
 *      run on x_f.  For FD_LQG_TRUTH the law reads the stored state itself, as fdyn_servo_step_* does; the estimator still runs.
 *   6. chatter += (clip(u) - (u0 + du_prev))^2, then du_prev = clip(u) - u0.  sat_steps and the anti-windup are the servo's;
 *      err_out holds the last errors of the TRUE state before their clip.
 *   7. one RK4 step of dt, then the reference motion of fdyn_servo.h step 6                                                    */
#ifndef FDYN_SERVO_LQG_H
#define FDYN_SERVO_LQG_H

#include <stdint.h>
#include "fdyn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* noise [FD_NSKN]: sigma of the ten words, then the process-noise rates s (state units per sqrt(s)) */
enum { FD_SKN_SIGMA = 0, FD_SKN_RATE = 10, FD_NSKN = 20 };
/* filter F [FD_NSKF][n], every matrix row-major: Phi 5 x 5, Gamma 5 x 2, L 5 x 5 of the longitudinal and the lateral block */
enum { FD_SKF_PHI_LON = 0, FD_SKF_PHI_LAT = 25, FD_SKF_GAMMA_LON = 50, FD_SKF_GAMMA_LAT = 60, FD_SKF_L_LON = 70, FD_SKF_L_LAT = 95, FD_NSKF = 120 };
/* states per block, estimated words */
enum { FD_SK_NB = 5, FD_NSKX = 10 };
/* fourth Philox counter word of the measurement noise: three blocks, FD_PHX_SERVO_LQG .. + 2 (fdyn_layout.h lists the others) */
enum { FD_PHX_SERVO_LQG = 0x7A };

/* fdyn_servo_kf_design: A [FD_NX * FD_NX][n], B [FD_NX * FD_NU][n]; noise [FD_NSKN] or, with noise_per_lane != 0, [FD_NSKN][n].
 * Per block the model is discretised at dt (fdyn_kf_design's series) and the filter Riccati equation is solved in fp64, one lane
 * per aircraft, by fdyn_kf_design's doubling loop at N = 5: L = P (P + V)^-1, V = diag sigma^2, W = diag s^2 dt.
 *   F [FD_NSKF][n]     the filter (FD_SKF_*); Phi = I, Gamma = 0, L = I (xhat = y) for a lane with a non-zero status
 *   residual [n]       relative residual of the filter equation, worse block (NaN: invalid input)
 *   iters [n] int32    doubling steps of the slower block
 *   status [n] int32   FD_KF_* bits with fdyn_kf_design's meanings, 0 = a certified stable filter.  FD_KF_BAD_INPUT: a word read is
 *                      not finite, a sigma or a rate is not finite and > 0, dt outside (1e-6, 1], |a|_inf dt > 1.5 for a block  */
int fdyn_servo_kf_design(const double* A, const double* B, double dt, const double* noise, int noise_per_lane, int64_t n, double* F,
                         double* residual, int32_t* iters, int32_t* status, void* stream);

/* fdyn_servo_lqg_step_*: n_steps control steps (above) in one launch.  The argument list of fdyn_servo_step_*, then before `stream`:
 *   F [FD_NSKF][n]            as fdyn_servo_kf_design writes it, designed at this dt
 *   sigma [FD_NSKX]           the measurement noise the loop applies
 *   xhat [FD_NSKX][n]         the estimate of d (advanced)
 *   du_prev [FD_NU][n]        the last applied control minus u0 (advanced)
 *   seed                      Philox key of the in-kernel draws
 *   step [1] int32            or NULL (= 0); the number of control steps drawn before this launch.  The caller advances it.
 *   z [n_steps][FD_NSKX][n]   or NULL; the normals to use instead of the in-kernel draws
 *   feedback                  FD_LQG_ESTIMATE, FD_LQG_MEASUREMENT or FD_LQG_TRUTH
 *   err_est, err_meas [FD_NSKX][n], chatter [FD_NU][n]   or NULL; the sums of steps 4 and 6 are added to them
 *   meas_out [FD_NSKX][n]     or NULL; the last measurement y
 * n_steps = 0 computes the controls from the stored xhat (from the stored state for FD_LQG_TRUTH) into surf_out and writes nothing
 * else.  Refusals as fdyn_servo_step_*, in its order: FDYN_ERR_BAD_SIZE for n < 0 or n_steps < 0, FDYN_ERR_BAD_TYPES, FDYN_ERR_NULL
 * for a missing required pointer (F, sigma, xhat and du_prev are required), FDYN_ERR_BAD_SIZE for an unknown feedback,
 * FDYN_ERR_BAD_DT, each with no launch.                                                                                        */
int fdyn_servo_lqg_step_f64(double* x, const double* x0, const double* u0, const double* K, double* ref, double* integ,
                            const double* limits, const uint8_t* type, const double* params, int n_types, int64_t n, double dt,
                            int n_steps, double* surf_out, int32_t* sat_steps, double* err_out, const double* F, const double* sigma,
                            double* xhat, double* du_prev, uint64_t seed, const int32_t* step, const double* z, int feedback,
                            double* err_est, double* err_meas, double* chatter, double* meas_out, void* stream);
int fdyn_servo_lqg_step_mixed(double* x, const double* x0, const double* u0, const double* K, double* ref, double* integ,
                              const double* limits, const uint8_t* type, const double* params, int n_types, int64_t n, double dt,
                              int n_steps, double* surf_out, int32_t* sat_steps, double* err_out, const double* F, const double* sigma,
                              double* xhat, double* du_prev, uint64_t seed, const int32_t* step, const double* z, int feedback,
                              double* err_est, double* err_meas, double* chatter, double* meas_out, void* stream);
int fdyn_servo_lqg_step_f32(float* x, const double* x0, const double* u0, const double* K, double* ref, double* integ,
                            const double* limits, const uint8_t* type, const double* params, int n_types, int64_t n, double dt,
                            int n_steps, float* surf_out, int32_t* sat_steps, double* err_out, const double* F, const double* sigma,
                            double* xhat, double* du_prev, uint64_t seed, const int32_t* step, const double* z, int feedback,
                            double* err_est, double* err_meas, double* chatter, double* meas_out, void* stream);

/* fdyn_servo_lqg_step_f64_lds: fdyn_servo_lqg_step_f64 word for word, with the filter's 120 fp64 words staged once into dynamic LDS
 * (61 440 B behind the static columns: one workgroup per CU) instead of read from F every step.  Same results to the bit.  The
 * other placement of the two that were timed; kept so that the comparison can be repeated (scripts/servo_lqg_throughput.py).  */
int fdyn_servo_lqg_step_f64_lds(double* x, const double* x0, const double* u0, const double* K, double* ref, double* integ,
                                const double* limits, const uint8_t* type, const double* params, int n_types, int64_t n, double dt,
                                int n_steps, double* surf_out, int32_t* sat_steps, double* err_out, const double* F,
                                const double* sigma, double* xhat, double* du_prev, uint64_t seed, const int32_t* step,
                                const double* z, int feedback, double* err_est, double* err_meas, double* chatter, double* meas_out,
                                void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FDYN_SERVO_LQG_H */

/* fdyn_servo_sched_lqg.h -- C-ABI of the LQ servo gain-scheduled over airspeed ON NOISY SENSORS (csrc/servo_kernels.hip): the
 * control step of fdyn_servo_lqg.h with the trim point, the gains AND the filter read from per-aircraft tables over airspeed, as
 * fdyn_servo_sched.h reads the first two, and with the estimate carried from one operating point to the next without a jump.  A
 * header of its own beside fdyn.h, whose conventions hold: every array is a DEVICE pointer, SoA [word][n] row-major fp64 unless
 * marked, `stream` is a hipStream_t passed as void*, the return codes are fdyn.h's, and no entry point synchronises or allocates,
 * so all can be captured into a hipGraph.  Layout constants: fdyn_layout.h (FD_SS_*, FD_NSS, FD_MAX_SCHED_NODES, FD_SCHED_ON_*)
 * and fdyn_servo_lqg.h (FD_SKF_*, FD_NSKF, FD_NSKX).
 *
 * The arrays.
 *   sched [n_nodes][FD_NSS][n]     exactly fdyn_servo_sched.h's table
 *   sched_f [n_nodes][FD_NSKF][n]  node k's filter, as fdyn_servo_kf_design writes it at this dt from the model at node k's trim
 *   origin [2][n]                  z0 and psi0: the fixed origin of the z and psi words of the estimate, the role x0[FD_X_D] and
 *                                  x0[FD_X_YAW] play for fdyn_servo_lqg_step_*
 *   sched_state [2][n]             required, advanced: sigma and the table position of the operating point that xhat and du_prev
 *                                  are relative to.  A position < 0 means "none yet".
 *
 * The law, in fp64 with contraction off wherever the two parents run so.  The operating point is the word list (x0, u0, K, F): the
 * eight scheduled words of the trim (u, w, q, theta, v, p, r, phi), the trim controls, the gains, the filter.
 *
 * At launch entry:
 *   - with position >= 0 the operating point's words (x0, u0, K, F) are rebuilt from the stored sigma by fdyn_servo_sched.h's
 *     step 0b (and 0c).  The lookup is a pure function of sigma and the tables, so a split launch sees the same bits.
 *   - with position < 0 the table is entered with V_c; xhat and du_prev are taken as relative to that point.
 *
 * Per control step:
 *   1. steps 1-5 of fdyn_servo_lqg.h run with the CURRENT operating point's x0 and F, and z0, psi0 from `origin`.  This gives the
 *      law's input x_f.
 *   2. sigma is the airspeed of the law's input exactly as the law's step 1 forms it -- the estimate's, the measurement's or the
 *      truth's airspeed, by `feedback` -- widened from the storage type (FD_SCHED_ON_AIRSPEED).  For FD_SCHED_ON_COMMAND it is V_c.
 *   3. fdyn_servo_sched.h's 0b and 0c give the new words x0', u0', K' and F'.  Its rule applies to F as to every other word:
 *      w_k + t (w_{k+1} - w_k), with exact nodes outside the table and for NaN.
 *   4. re-reference, only when sigma is not bitwise the stored one (fdyn_servo_sched.h's skip rule; steps 3 and 4 are skipped
 *      together):
 *        - for the eight scheduled words: xhat_j <- xhat_j + (x0_j - x0'_j); the difference and the sum are formed in fp64, then
 *          converted to the glue type; the theta and phi words are wrapped (in the glue type, after the conversion, and only
 *          where the word has left [-pi, pi): a word inside keeps its bits, which the fp64 wrap would not leave it)
 *        - for the controls: du_prev_k <- du_prev_k + (u0_k - u0'_k), u0 and u0' as the glue type holds them, the difference and
 *          the sum in fp64, then converted
 *        - x_f is NOT re-formed: it is absolute, and the re-reference leaves x0 + xhat where it was, up to rounding
 *      then sigma and the position are stored.
 *   5. the servo law's steps 1-4 (fdyn_servo.h) run on x_f with x0', u0', K'
 *   6. chatter and du_prev are formed as in fdyn_servo_lqg.h step 6, with u0'
 *   7. one RK4 step of dt and the reference motion follow
 * The next step's estimator uses x0' and F'.
 *
 * With n_nodes = 1, and with tables of equal nodes, every result equals that of fdyn_servo_lqg_step_* at that node, with
 * x0[FD_X_D] = z0 and x0[FD_X_YAW] = psi0, bit for bit (a -0.0 may come back as +0.0).  With FD_LQG_TRUTH the state, references,
 * integrators and controls equal those of fdyn_servo_sched_step_* bit for bit.  Still air only.                                */
#ifndef FDYN_SERVO_SCHED_LQG_H
#define FDYN_SERVO_SCHED_LQG_H

#include <stdint.h>
#include "fdyn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* fdyn_servo_sched_lqg_step_*: the arguments of fdyn_servo_lqg_step_* with x0, u0, K replaced by sched, sched_f, n_nodes, sched_on,
 * origin; F dropped; sched_state added behind du_prev.  n_steps = 0 computes the controls from the stored xhat (from the stored state
 * for FD_LQG_TRUTH) at the operating point of launch entry, moved to the sigma of that input by steps 2 and 3, into surf_out and
 * writes nothing else: sched_state, xhat and du_prev stay.
 * Refusals are those of both parents, in their order: FDYN_ERR_BAD_SIZE for n_steps < 0, n_nodes outside 1..FD_MAX_SCHED_NODES, an
 * unknown sched_on or n < 0, FDYN_ERR_BAD_TYPES, FDYN_ERR_NULL for a missing required pointer (x, sched, sched_f, origin, ref, integ,
 * limits, params, sigma, xhat, du_prev, sched_state), FDYN_ERR_BAD_SIZE for an unknown feedback, FDYN_ERR_BAD_DT, each with no
 * launch.                                                                                                                      */
int fdyn_servo_sched_lqg_step_f64(double* x, const double* sched, const double* sched_f, int n_nodes, int sched_on, const double* origin,
                                  double* ref, double* integ, const double* limits, const uint8_t* type, const double* params,
                                  int n_types, int64_t n, double dt, int n_steps, double* surf_out, int32_t* sat_steps, double* err_out,
                                  const double* sigma, double* xhat, double* du_prev, double* sched_state, uint64_t seed,
                                  const int32_t* step, const double* z, int feedback, double* err_est, double* err_meas,
                                  double* chatter, double* meas_out, void* stream);
int fdyn_servo_sched_lqg_step_mixed(double* x, const double* sched, const double* sched_f, int n_nodes, int sched_on, const double* origin,
                                    double* ref, double* integ, const double* limits, const uint8_t* type, const double* params,
                                    int n_types, int64_t n, double dt, int n_steps, double* surf_out, int32_t* sat_steps, double* err_out,
                                    const double* sigma, double* xhat, double* du_prev, double* sched_state, uint64_t seed,
                                    const int32_t* step, const double* z, int feedback, double* err_est, double* err_meas,
                                    double* chatter, double* meas_out, void* stream);
int fdyn_servo_sched_lqg_step_f32(float* x, const double* sched, const double* sched_f, int n_nodes, int sched_on, const double* origin,
                                  double* ref, double* integ, const double* limits, const uint8_t* type, const double* params,
                                  int n_types, int64_t n, double dt, int n_steps, float* surf_out, int32_t* sat_steps, double* err_out,
                                  const double* sigma, double* xhat, double* du_prev, double* sched_state, uint64_t seed,
                                  const int32_t* step, const double* z, int feedback, double* err_est, double* err_meas,
                                  double* chatter, double* meas_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FDYN_SERVO_SCHED_LQG_H */

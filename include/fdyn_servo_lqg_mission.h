/* fdyn_servo_lqg_mission.h -- C-ABI of the waypoint missions flown by the LQ servo ON NOISY SENSORS (csrc/servo_kernels.hip): the
 * mission update and the waypoint guidance of fdyn_mission.h fed by the estimator of fdyn_servo_lqg.h and by a filtered position
 * measurement, n control steps in one launch.  A header of its own beside those two, whose conventions hold: every array is a
 * DEVICE pointer, SoA [word][n] row-major fp64 unless marked, `stream` is a hipStream_t passed as void*, the return codes are
 * fdyn.h's, and no entry point synchronises or allocates, so all can be captured into a hipGraph.
 *
 * One control step of a lane whose mission is not complete:
 *   1. measure: d and y of the ten words exactly as steps 1-2 of fdyn_servo_lqg.h.  y_p = (N, E) of the stored state widened to
 *      fp64 + sigma_p (z10, z11), in fp64.  With z given, z = z[s][k][i], k = 0..11; otherwise the twelve normals of the three
 *      Philox blocks of fdyn_servo_lqg.h step 2 as drawn, counter (row low, row high, *step + s + 1, FD_PHX_SERVO_LQG + b): words
 *      0..9 in d's order, words 10 and 11 (the cos and sin of block 2's second pair) the north and east position normals.
 *   2. filter: step 3 of fdyn_servo_lqg.h, unchanged.
 *   3. law input: x_f as step 5 there; f = xhat, y or d according to `feedback` (for FD_LQG_TRUTH x_f is the stored state).
 *   4. position filter, for every feedback.  v_NE = the north and east components of R(phi, theta, psi) (u, v, w) on x_f's words,
 *      in the glue type, each sum left to right and no product fused:
 *        v_N = (cth cpsi) u + ((sphi sth) cpsi - cphi spsi) v + ((cphi sth) cpsi + sphi spsi) w
 *        v_E = (cth spsi) u + ((sphi sth) spsi + cphi cpsi) v + ((cphi sth) spsi - sphi cpsi) w
 *      then widened to fp64, and in fp64 per axis: pm = phat + dt v; phat = pm + g (y_p - pm).
 *   5. account: err_est, err_meas as step 4 of fdyn_servo_lqg.h; err_pos[0] += (phat_N - N)^2 + (phat_E - E)^2 (summed in that
 *      order, then added), err_pos[1] += (y_pN - N)^2 + (y_pE - E)^2, N and E the stored state widened to fp64.
 *   6. mission update, guidance, references: steps 1-3 of fdyn_mission.h on a glue-type state xg.  FD_LQG_ESTIMATE: xg = x_f with its
 *      north and east words replaced by phat; FD_LQG_MEASUREMENT: by y_p; in both the derived scalars (airspeed, altitude, ground
 *      speed, course) come from xg's own words and its own sines and cosines in all three precisions, never from the integrator's
 *      carried ones, which belong to the true state.  FD_LQG_TRUTH: the guidance reads what fdyn_servo_mission_* reads (the fp32
 *      state copy and the carried sines and cosines in mixed and f32).  A lane found COMPLETE here leaves the loop (below).
 *   7. statistics (FD_MST_*): on the TRUE state, with the expressions fdyn_servo_mission_* uses; the leg and the altitude are the
 *      active waypoint's.  A sweep is ranked by what the aircraft did, not by what it believed.
 *   8. servo law: steps 1-4 of fdyn_servo.h on x_f against the new references; then step 6 of fdyn_servo_lqg.h (the true words back,
 *      err_out of the TRUE state, chatter, du_prev; sat_steps and the anti-windup are the servo's).
 *   9. one RK4 step of dt.
 *
 * Completion.  A lane whose index is >= n_wp at entry (and consts[FD_C_ON_COMPLETE] is not restart) does nothing at all.  A lane
 * found complete at step 6 leaves the loop: the measurement, the filters and the accounting of that step stand (xhat, phat, err_est,
 * err_meas, err_pos and meas_out are written; du_prev and chatter are not touched by that step); if it flew no step in this launch
 * its x, ref, integ, du_prev, stats, sat_steps, err_out, surf_out and steps_flown words stay as they were, otherwise they hold what
 * its last flown step left.  wp_idx and reached_total are written as fdyn_servo_mission_* writes them.
 * n_steps = 0 measures nothing: the mission update runs on a local copy of the index, guidance and controls are formed from the
 * stored xhat and phat (y_p = phat for FD_LQG_MEASUREMENT; from the stored state for FD_LQG_TRUTH) and go into surf_out alone.  A
 * complete lane writes nothing.                                                                                                */
#ifndef FDYN_SERVO_LQG_MISSION_H
#define FDYN_SERVO_LQG_MISSION_H

#include <stdint.h>
#include "fdyn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* normals per control step: the ten of fdyn_servo_lqg.h, then north and east */
enum { FD_NSKZ = 12 };
/* pos [FD_NSPF]: the standard deviation of the north / east position measurement (m), the position filter's gain g in (0, 1] */
enum { FD_SPF_SIGMA = 0, FD_SPF_GAIN = 1, FD_NSPF = 2 };

/* fdyn_servo_lqg_mission_*: the arguments of fdyn_servo_mission_* up to and including `stats`, then the estimator group of
 * fdyn_servo_lqg_step_* (F .. meas_out, with z [n_steps][FD_NSKZ][n] or NULL), then before `stream`:
 *   pos [FD_NSPF]             shared by the fleet (FD_SPF_*).  A DEVICE array like every other, and the entry reads nothing from
 *                             the device: its two words are NOT checked here.  They must be host-checked values -- a sigma that
 *                             is finite and >= 0, a gain that is finite and in (0, 1] -- and the host layer
 *                             (hcrl_amd.servo_lqg_mission.ServoPositionFilter) refuses anything else before it uploads them.
 *   phat [2][n]               the estimate of (north, east) (advanced; required)
 *   err_pos [2][n]            or NULL; row 0 += |phat - p|^2, row 1 += |y_p - p|^2, both axes, step by step
 * Refusals, each with no launch, in this order: fdyn_servo_mission_*'s (FDYN_ERR_BAD_SIZE for n < 0, n_steps < 0 or n_wp outside
 * 1..FD_MAX_WAYPOINTS, FDYN_ERR_BAD_TYPES, FDYN_ERR_NULL for a missing required pointer of its list), then fdyn_servo_lqg_step_*'s
 * (FDYN_ERR_NULL for F, sigma, xhat, du_prev, and here pos and phat; FDYN_ERR_BAD_SIZE for an unknown feedback), then
 * FDYN_ERR_BAD_DT.  The words of pos are the host layer's to refuse (above).                                                    */
int fdyn_servo_lqg_mission_f64(double* x, const double* x0, const double* u0, const double* K, double* ref, double* integ,
                               const double* limits, int32_t* wp_idx, const double* consts, const double* wps, int n_wp,
                               const uint8_t* type, const double* params, int n_types, int64_t n, double dt, int n_steps,
                               double* surf_out, int32_t* sat_steps, double* err_out, int32_t* reached_total, int32_t* steps_flown,
                               double* stats, const double* F, const double* sigma, double* xhat, double* du_prev, uint64_t seed,
                               const int32_t* step, const double* z, int feedback, double* err_est, double* err_meas,
                               double* chatter, double* meas_out, const double* pos, double* phat,
                               double* err_pos, void* stream);
int fdyn_servo_lqg_mission_mixed(double* x, const double* x0, const double* u0, const double* K, double* ref, double* integ,
                                 const double* limits, int32_t* wp_idx, const double* consts, const double* wps, int n_wp,
                                 const uint8_t* type, const double* params, int n_types, int64_t n, double dt, int n_steps,
                                 double* surf_out, int32_t* sat_steps, double* err_out, int32_t* reached_total, int32_t* steps_flown,
                                 double* stats, const double* F, const double* sigma, double* xhat, double* du_prev, uint64_t seed,
                                 const int32_t* step, const double* z, int feedback, double* err_est, double* err_meas,
                                 double* chatter, double* meas_out, const double* pos, double* phat,
                                 double* err_pos, void* stream);
int fdyn_servo_lqg_mission_f32(float* x, const double* x0, const double* u0, const double* K, double* ref, double* integ,
                               const double* limits, int32_t* wp_idx, const double* consts, const double* wps, int n_wp,
                               const uint8_t* type, const double* params, int n_types, int64_t n, double dt, int n_steps,
                               float* surf_out, int32_t* sat_steps, double* err_out, int32_t* reached_total, int32_t* steps_flown,
                               double* stats, const double* F, const double* sigma, double* xhat, double* du_prev, uint64_t seed,
                               const int32_t* step, const double* z, int feedback, double* err_est, double* err_meas,
                               double* chatter, double* meas_out, const double* pos, double* phat,
                               double* err_pos, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FDYN_SERVO_LQG_MISSION_H */

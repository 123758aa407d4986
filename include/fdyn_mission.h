/* fdyn_mission.h -- C-ABI of the waypoint missions flown by the LQ servo of libfdyn_hip.so (csrc/servo_kernels.hip): the mission
 * update and the waypoint guidance of the PID cascade (fdyn_cascade_step_*) in front of the servo law (fdyn_servo_step_*), n control
 * steps in one launch.  A header of its own beside fdyn.h, whose conventions hold: every array is a DEVICE pointer, SoA [word][n]
 * row-major fp64 unless marked, `stream` is a hipStream_t passed as void*, the return codes are fdyn.h's, and no entry point
 * synchronises or allocates, so all can be captured into a hipGraph.  Layout constants (FD_C_*, FD_WP_*, FD_SV*, FD_MST_*):
 * fdyn_layout.h.
 *
 * One control step of a lane whose mission is not complete:
 *   1. mission update, as fdyn_cascade_step_* does it: if idx < n_wp and the 3-D distance to wps[idx] is below
 *      consts[FD_C_ACCEPTANCE_RADIUS], idx += 1 and reached += 1.  If idx >= n_wp: with consts[FD_C_ON_COMPLETE] = 1 (restart)
 *      idx = 0; otherwise the mission is COMPLETE: the lane leaves the loop, its state stops advancing and nothing more of it
 *      changes, in this launch and in every later one.
 *   2. guidance: the heading, speed and altitude command the cascade's waypoint agent hands to its HSA agent (line of sight with
 *      turn anticipation, pure pursuit, or the plain line of sight; the final wrap; NaN speed = the current airspeed; the speed
 *      reduction near a turn), in the variant's glue type on the inputs the cascade's guidance reads in that variant: the fp64
 *      state in f64; in mixed and f32 the integrator's fp32 state copy and its carried sines and cosines, and pure pursuit
 *      without its second atan2.
 *   3. references, in fp64: V_c = the speed command, h_c = the waypoint's altitude, psi_c = the heading command,
 *      hdot_c = psidot_c = 0.  All FD_NSVR rows of ref are written: after the launch ref holds the last commands, and a
 *      following fdyn_servo_step_* holds them.
 *   4. statistics (FD_MST_*), on the state the guidance saw, formed in the glue type and compared in fp64: |altitude - wps[idx]'s
 *      altitude|, |roll|, airspeed, and with idx >= 1 and a leg wps[idx - 1] -> wps[idx] of at least 1 m in the horizontal plane
 *      the distance from that leg's line.
 *   5. steps 1-5 of the servo law of fdyn_servo.h, unchanged: error clips, deviations, u = u0 - K d, anti-windup per block, one
 *      RK4 step of dt.  (Its step 6 has nothing to move: the rates are zero.)
 *
 * Of consts [FD_NC] these words are read: FD_C_GUIDANCE_TYPE, FD_C_WP_MAX_BANK_RAD, FD_C_LOS_MAX_BANK_RAD,
 * FD_C_LOS_LEAD_ANGLE_RAD, FD_C_LOOKAHEAD_TIME, FD_C_LOOKAHEAD_MIN, FD_C_LOOKAHEAD_MAX, FD_C_PROXIMITY_SCALE,
 * FD_C_TURN_THRESHOLD_DIST, FD_C_TURN_THRESHOLD_ANGLE_RAD, FD_C_MAX_SPEED_REDUCTION, FD_C_MIN_SPEED, FD_C_ACCEPTANCE_RADIUS,
 * FD_C_ON_COMPLETE.  The PID cascade's limits and the env words are staged with them and ignored.                            */
#ifndef FDYN_MISSION_H
#define FDYN_MISSION_H

#include <stdint.h>
#include "fdyn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* fdyn_servo_mission_*: n_steps control steps (above) in one launch.  x, x0, u0, K, ref, integ, limits, type, params, n_types,
 * surf_out, sat_steps and err_out exactly as fdyn_servo_step_* takes them; wp_idx [n] int32 (advanced; a negative index counts
 * as 0), consts [FD_NC], wps [n_wp][FD_NWP] (north, east, altitude, speed; NaN speed = keep the current airspeed) with
 * 1 <= n_wp <= FD_MAX_WAYPOINTS, and reached_total exactly as fdyn_cascade_step_* takes them.
 *   reached_total [n] int32   or NULL; += the waypoints reached in this launch
 *   steps_flown [n] int32     or NULL; += the control steps the lane flew in this launch
 *   stats [FD_NMST][n]        or NULL; running extrema carried across launches, started by the host at 0, 0, +inf, 0
 * A lane that flew no step in a launch (its mission was complete, or became so at the launch's first mission update) keeps its
 * x, ref, integ, stats, surf_out, sat_steps, err_out and steps_flown words as they were.
 * n_steps = 0, for a lane whose mission is not complete: the mission update runs on a local copy of the index, then guidance and
 * controls, into surf_out; nothing else is written.  A complete lane writes nothing at all.
 * FDYN_ERR_BAD_SIZE for n < 0, n_steps < 0 or n_wp outside 1..FD_MAX_WAYPOINTS, FDYN_ERR_BAD_TYPES, FDYN_ERR_NULL for a missing
 * required pointer (wp_idx, consts and wps included), FDYN_ERR_BAD_DT, each with no launch.                                  */
int fdyn_servo_mission_f64(double* x, const double* x0, const double* u0, const double* K, double* ref, double* integ,
                           const double* limits, int32_t* wp_idx, const double* consts, const double* wps, int n_wp,
                           const uint8_t* type, const double* params, int n_types, int64_t n, double dt, int n_steps,
                           double* surf_out, int32_t* sat_steps, double* err_out, int32_t* reached_total, int32_t* steps_flown,
                           double* stats, void* stream);
int fdyn_servo_mission_mixed(double* x, const double* x0, const double* u0, const double* K, double* ref, double* integ,
                             const double* limits, int32_t* wp_idx, const double* consts, const double* wps, int n_wp,
                             const uint8_t* type, const double* params, int n_types, int64_t n, double dt, int n_steps,
                             double* surf_out, int32_t* sat_steps, double* err_out, int32_t* reached_total, int32_t* steps_flown,
                             double* stats, void* stream);
int fdyn_servo_mission_f32(float* x, const double* x0, const double* u0, const double* K, double* ref, double* integ,
                           const double* limits, int32_t* wp_idx, const double* consts, const double* wps, int n_wp,
                           const uint8_t* type, const double* params, int n_types, int64_t n, double dt, int n_steps,
                           float* surf_out, int32_t* sat_steps, double* err_out, int32_t* reached_total, int32_t* steps_flown,
                           double* stats, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FDYN_MISSION_H */

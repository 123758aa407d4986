/* fdyn_servo_sched.h -- C-ABI of the LQ servo gain-scheduled over airspeed in flight (csrc/servo_kernels.hip): the control step of
 * fdyn_servo.h and the mission step of fdyn_mission.h with the trim point and the gains read from a per-aircraft table of designs
 * instead of from one design.  A header of its own beside fdyn.h, whose conventions hold: every array is a DEVICE pointer, SoA
 * [word][n] row-major fp64 unless marked, `stream` is a hipStream_t passed as void*, the return codes are fdyn.h's, and no entry
 * point synchronises or allocates, so all can be captured into a hipGraph.  Layout constants (FD_SS_*, FD_NSS, FD_MAX_SCHED_NODES,
 * FD_SCHED_ON_*): fdyn_layout.h.
 *
 * The table.  sched [n_nodes][FD_NSS][n]: node k of aircraft i is the FD_NSS words sched[(k * FD_NSS + row) * n + i]: the node's
 * airspeed V_k (FD_SS_V), the eight regulated words of its trim in the order u, w, q, theta, v, p, r, phi (FD_SS_X0), its trim
 * controls in FD_U_* order (FD_SS_U0) and its FD_NSVK gains as fdyn_servo_design writes them (FD_SS_K).  The node airspeeds of an
 * aircraft are strictly increasing (the host layer's to check) and may differ between aircraft.  Equal node airspeeds are
 * tolerated: the comparisons of 0b then never reach a division.
 *
 * The law.  In front of step 1 of each control step of fdyn_servo.h, in fp64 with contraction off:
 *   0a. sigma = V as step 1 forms it, widened from the storage type (FD_SCHED_ON_AIRSPEED), or V_c (FD_SCHED_ON_COMMAND; in a
 *       mission the V_c the guidance has just written)
 *   0b. if !(sigma > V_0): node 0's words exactly (this is also where a NaN goes), position 0; else if sigma >= V_{M-1}: the last
 *       node's words exactly, position M - 1; else k = the largest index with V_k <= sigma, t = (sigma - V_k) / (V_{k+1} - V_k),
 *       every word is w_k + t (w_{k+1} - w_k), position k + t
 *   0c. from the interpolated words what the prologue of fdyn_servo_step_* derives from x0, u0 and K, in the same way:
 *       V0 = sqrt(u0^2 + w0^2), the direction (u0, w0) / V0, and K and u0 converted to the glue type
 * Steps 1-6 are unchanged.  Outside the table the dV shift of step 2 extrapolates from the end node, as it does from the one
 * design of fdyn_servo_step_*.  With n_nodes = 1, and with a table of equal nodes, every result equals that of fdyn_servo_step_* /
 * fdyn_servo_mission_* at that node bit for bit.  Still air only.                                                               */
#ifndef FDYN_SERVO_SCHED_H
#define FDYN_SERVO_SCHED_H

#include <stdint.h>
#include "fdyn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* fdyn_servo_sched_step_*: the arguments of fdyn_servo_step_* with x0, u0, K replaced by sched, n_nodes, sched_on, and
 *   sigma_out [2][n]   or NULL; sigma and the table position of the last control step
 * n_steps = 0 computes the controls from the current state into surf_out, and sigma_out, and writes nothing else.
 * FDYN_ERR_BAD_SIZE for n < 0, n_steps < 0, n_nodes outside 1..FD_MAX_SCHED_NODES or an unknown sched_on, FDYN_ERR_BAD_TYPES,
 * FDYN_ERR_NULL for a missing required pointer (sched included), FDYN_ERR_BAD_DT, each with no launch.                           */
int fdyn_servo_sched_step_f64(double* x, const double* sched, int n_nodes, int sched_on, double* ref, double* integ, const double* limits,
                              const uint8_t* type, const double* params, int n_types, int64_t n, double dt, int n_steps,
                              double* surf_out, int32_t* sat_steps, double* err_out, double* sigma_out, void* stream);
int fdyn_servo_sched_step_mixed(double* x, const double* sched, int n_nodes, int sched_on, double* ref, double* integ, const double* limits,
                                const uint8_t* type, const double* params, int n_types, int64_t n, double dt, int n_steps,
                                double* surf_out, int32_t* sat_steps, double* err_out, double* sigma_out, void* stream);
int fdyn_servo_sched_step_f32(float* x, const double* sched, int n_nodes, int sched_on, double* ref, double* integ, const double* limits,
                              const uint8_t* type, const double* params, int n_types, int64_t n, double dt, int n_steps,
                              float* surf_out, int32_t* sat_steps, double* err_out, double* sigma_out, void* stream);

/* fdyn_servo_sched_mission_*: the same replacement on fdyn_servo_mission_*: per control step the mission update and the guidance,
 * which writes V_c, then 0a-0c, then the law.  sigma_out is written where surf_out is: a lane that flew no step keeps it.
 * The refusals of fdyn_servo_mission_* and those above.                                                                       */
int fdyn_servo_sched_mission_f64(double* x, const double* sched, int n_nodes, int sched_on, double* ref, double* integ,
                                 const double* limits, int32_t* wp_idx, const double* consts, const double* wps, int n_wp,
                                 const uint8_t* type, const double* params, int n_types, int64_t n, double dt, int n_steps,
                                 double* surf_out, int32_t* sat_steps, double* err_out, int32_t* reached_total, int32_t* steps_flown,
                                 double* stats, double* sigma_out, void* stream);
int fdyn_servo_sched_mission_mixed(double* x, const double* sched, int n_nodes, int sched_on, double* ref, double* integ,
                                   const double* limits, int32_t* wp_idx, const double* consts, const double* wps, int n_wp,
                                   const uint8_t* type, const double* params, int n_types, int64_t n, double dt, int n_steps,
                                   double* surf_out, int32_t* sat_steps, double* err_out, int32_t* reached_total, int32_t* steps_flown,
                                   double* stats, double* sigma_out, void* stream);
int fdyn_servo_sched_mission_f32(float* x, const double* sched, int n_nodes, int sched_on, double* ref, double* integ,
                                 const double* limits, int32_t* wp_idx, const double* consts, const double* wps, int n_wp,
                                 const uint8_t* type, const double* params, int n_types, int64_t n, double dt, int n_steps,
                                 float* surf_out, int32_t* sat_steps, double* err_out, int32_t* reached_total, int32_t* steps_flown,
                                 double* stats, double* sigma_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FDYN_SERVO_SCHED_H */

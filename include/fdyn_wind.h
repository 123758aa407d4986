/* fdyn_wind.h -- C-ABI of the LQ servo and its waypoint missions in a moving air mass (csrc/servo_kernels.hip): steady wind and
 * first-order Gauss-Markov gusts, per aircraft.  A header of its own beside fdyn_servo.h and fdyn_mission.h, whose conventions
 * hold: every array is a DEVICE pointer, SoA [word][n] row-major fp64 unless marked, `stream` is a hipStream_t passed as void*,
 * the return codes are fdyn.h's, and no entry point synchronises or allocates, so all can be captured into a hipGraph.
 *
 * The six entries take the argument lists of fdyn_servo_step_* and fdyn_servo_mission_* and add one group before `stream`:
 *   wind [FD_NSW][n]          the lane's air mass, NED, moving TOWARD +north / +east / +down: FD_SW_WIND_* the steady wind,
 *                             FD_SW_GUST_* the gust (advanced), FD_SW_GUST_A, FD_SW_GUST_B the gust's step coefficients.  The
 *                             order of FD_DR_WIND_N .. FD_DR_GUST_B.  Only the three gust rows are written.
 *   seed                      Philox key of the in-kernel draws
 *   step [1] int32            or NULL (= 0); the number of control steps drawn before this launch.  The caller advances it.
 *   z [n_steps][3][n]         or NULL; the normals to use instead of the in-kernel draws
 *
 * One control step is that of fdyn_servo.h / fdyn_mission.h with these changes and no others:
 *   a. at the top of the step the air-mass velocity W + g is summed in fp64 from the lane's rows; it is constant over the step
 *   b. the aircraft feels v_air = v - R^T (W + g): in f64 formed in fp64 from the stored state; in mixed and f32 the rotation runs
 *      in fp32 on the integrator's carried sines and cosines and is subtracted from the stored velocity in the storage type
 *      (the law) and from the integrator's fp32 copy (the guidance), the two forms the still-air entries read the velocity in
 *   c. e_V uses |v_air|, and du, dw, dv of d_lon / d_lat use v_air's components.  Rates, angles, e_h, e_psi, the clips, the
 *      anti-windup, the saturation count and the reference motion are untouched.
 *   d. the mission's guidance reads the derived scalars with the airspeed replaced by |v_air| (the NaN-speed rule, the
 *      max(V, 10) terms, the minimum-airspeed statistic); course, ground speed, position and altitude stay ground quantities
 *   e. the RK4 step is the integrator's wind form: aerodynamics on v_air, kinematics on the ground velocity
 *   f. after the physics g <- (A g) + (B n) per axis in fp64, two products and one sum.  With z given, n = z[s][k][i];
 *      otherwise three normals from one Philox block, counter (row low, row high, *step + s + 1, FD_PHX_SERVO_GUST), paired as
 *      the rate env pairs its gust normals: (r0, r1) -> cos, sin; (r2, r3) -> cos, fp32 Box-Muller widened to fp64
 *   g. a mission lane that is complete draws nothing and writes no gust row; n_steps = 0 writes no gust row
 * With A = exp(-dt V0 / L) and B = sigma sqrt(1 - A^2) the gust is stationary with standard deviation sigma and length L.      */
#ifndef FDYN_WIND_H
#define FDYN_WIND_H

#include <stdint.h>
#include "fdyn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rows of wind [FD_NSW][n] */
enum {
    FD_SW_WIND_N = 0, FD_SW_WIND_E, FD_SW_WIND_D,
    FD_SW_GUST_N, FD_SW_GUST_E, FD_SW_GUST_D,
    FD_SW_GUST_A, FD_SW_GUST_B,
    FD_NSW = 8
};
/* fourth Philox counter word of the gust update (fdyn_layout.h lists the others: FD_PHX_*) */
enum { FD_PHX_SERVO_GUST = 0x78 };

/* fdyn_servo_step_wind_*: fdyn_servo_step_* in the lane's air mass.  Refusals as fdyn_servo_step_*, and FDYN_ERR_NULL for
 * wind == NULL, each with no launch.                                                                                        */
int fdyn_servo_step_wind_f64(double* x, const double* x0, const double* u0, const double* K, double* ref, double* integ,
                             const double* limits, const uint8_t* type, const double* params, int n_types, int64_t n, double dt,
                             int n_steps, double* surf_out, int32_t* sat_steps, double* err_out, double* wind, uint64_t seed,
                             const int32_t* step, const double* z, void* stream);
int fdyn_servo_step_wind_mixed(double* x, const double* x0, const double* u0, const double* K, double* ref, double* integ,
                               const double* limits, const uint8_t* type, const double* params, int n_types, int64_t n, double dt,
                               int n_steps, double* surf_out, int32_t* sat_steps, double* err_out, double* wind, uint64_t seed,
                               const int32_t* step, const double* z, void* stream);
int fdyn_servo_step_wind_f32(float* x, const double* x0, const double* u0, const double* K, double* ref, double* integ,
                             const double* limits, const uint8_t* type, const double* params, int n_types, int64_t n, double dt,
                             int n_steps, float* surf_out, int32_t* sat_steps, double* err_out, double* wind, uint64_t seed,
                             const int32_t* step, const double* z, void* stream);

/* fdyn_servo_mission_wind_*: fdyn_servo_mission_* in the lane's air mass.  Refusals as fdyn_servo_mission_*, and FDYN_ERR_NULL
 * for wind == NULL, each with no launch.                                                                                    */
int fdyn_servo_mission_wind_f64(double* x, const double* x0, const double* u0, const double* K, double* ref, double* integ,
                                const double* limits, int32_t* wp_idx, const double* consts, const double* wps, int n_wp,
                                const uint8_t* type, const double* params, int n_types, int64_t n, double dt, int n_steps,
                                double* surf_out, int32_t* sat_steps, double* err_out, int32_t* reached_total, int32_t* steps_flown,
                                double* stats, double* wind, uint64_t seed, const int32_t* step, const double* z, void* stream);
int fdyn_servo_mission_wind_mixed(double* x, const double* x0, const double* u0, const double* K, double* ref, double* integ,
                                  const double* limits, int32_t* wp_idx, const double* consts, const double* wps, int n_wp,
                                  const uint8_t* type, const double* params, int n_types, int64_t n, double dt, int n_steps,
                                  double* surf_out, int32_t* sat_steps, double* err_out, int32_t* reached_total, int32_t* steps_flown,
                                  double* stats, double* wind, uint64_t seed, const int32_t* step, const double* z, void* stream);
int fdyn_servo_mission_wind_f32(float* x, const double* x0, const double* u0, const double* K, double* ref, double* integ,
                                const double* limits, int32_t* wp_idx, const double* consts, const double* wps, int n_wp,
                                const uint8_t* type, const double* params, int n_types, int64_t n, double dt, int n_steps,
                                float* surf_out, int32_t* sat_steps, double* err_out, int32_t* reached_total, int32_t* steps_flown,
                                double* stats, double* wind, uint64_t seed, const int32_t* step, const double* z, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FDYN_WIND_H */

/* fdyn.h -- C-ABI of libfdyn_hip.so: the MI355X (gfx950) batched flight-dynamics hot path.
 *
 * This is the drop-in boundary beneath the reference's Python interfaces.  Plain pointers and sizes only:
 * every array argument is a DEVICE pointer (hipMalloc'd / a torch tensor's data_ptr()) unless marked "host";
 * `stream` is a hipStream_t passed as void* (NULL = default stream).  Calls are asynchronous on that stream.
 * No call allocates, frees or synchronises, so every entry point can be captured into a hipGraph.
 *
 * Array layouts ("SoA" = [word][N] row-major) and all slot enums: fdyn_layout.h.
 * Precision suffixes:   _f64   state fp64, dynamics fp64  (parity variant; the reference state is float64,
 *                               simulation/simplified_6dof.py:173)
 *                       _mixed state fp64, dynamics evaluated in fp32, RK4 accumulate in fp64
 *                       _f32   state fp32, dynamics fp32   (throughput variant)
 * The PID arithmetic is fp32 in every variant, bit-faithful to cpp/src/pid_controller.cpp:24-60.
 *
 * What each entry point replaces in the reference (paths relative to its root):
 *   fdyn_sixdof_step_*     Simplified6DOF.step               simulation/simplified_6dof.py:228-293 (+ _dynamics :333-503)
 *                          looped n_sub times as             simulation/simulation_backend.py:82-101 does
 *   fdyn_num_substeps      max(1, int(dt/dt_physics))        simulation/simulation_backend.py:95
 *   fdyn_derived_*         Simplified6DOF.get_state          simulation/simplified_6dof.py:295-331,505-530
 *   fdyn_pid_compute_batch PIDController::compute            cpp/src/pid_controller.cpp:24-60 (pybind: cpp/bindings/bindings.cpp:50-62)
 *   fdyn_cascade_step_*    MissionPlanner.update + WaypointAgent/HSAAgent/AttitudeAgent/RateAgent.compute_action
 *                          + set_controls + step             examples/03_waypoint_square_demo.py:148-209,
 *                          controllers/{mission_planner.py:128-184, waypoint_agent.py:81-242, hsa_agent.py:119-231,
 *                          attitude_agent.py:86-154, rate_agent.py:65-124}
 *   fdyn_agent_step_*      {Rate,Attitude,HSA,Waypoint}Agent.compute_action (+ set_controls + step): one level commanded directly
 *   fdyn_hybrid_step_*     AttitudeAgent / HSAAgent / WaypointAgent with `rate_agent` = LearnedRateAgent or the PID RateAgent,
 *                          chosen per aircraft and switched live   controllers/attitude_agent.py:67,152,
 *                          controllers/learned_rate_agent.py:128-198, gui/simulation_worker_learned.py:51-118
 *   fdyn_rate_env_reset_*  RateControlEnv.reset              learned_controllers/envs/rate_env.py:151-210
 *   fdyn_rate_env_step_*   RateControlEnv.step (+ the vec-env's auto-reset, + optionally the PID demonstrator of
 *                          learned_controllers/utils/pid_demonstrations.py:47-77)
 *                                                            learned_controllers/envs/rate_env.py:212-300,342-460,
 *                                                            learned_controllers/envs/rewards.py:48-137,168-221
 *   fdyn_rate_metrics_*    MetricsCalculator.compute_metrics learned_controllers/eval/metrics.py:95-362 (fed by eval_rate.py:70-233)
 *   fdyn_rate_reward_seq_* RateTrackingReward.compute / SettlingTimeBonus.compute on recorded sequences (weights as parameters,
 *                          components out)                     learned_controllers/envs/rewards.py:48-137,168-221
 *   fdyn_traj_compare      compare_trajectories, streamed    validation/metrics/trajectory_metrics.py:9-174
 *   fdyn_sensor_update_*   NoisySensorInterface.update       interfaces/sensor.py:199-243
 *   fdyn_sensor_observe    the same noise model on RateControlEnv observations (rate_env.py:374-408 layout)
 * Policy side (the reference delegates these to torch.nn.LSTM / SB3's PPO, which are not in its tree):
 *   fdyn_policy_features, fdyn_lstm_cell_mfma, fdyn_policy_trunks, fdyn_policy_heads, fdyn_gaussian_head, fdyn_episode_flags
 *                          rollout: features extractor / LSTM cell / trunks / output heads of
 *                          learned_controllers/networks/lstm_policy.py:13-136 (+ sb3_contrib's actor / critic LSTMs)
 *   fdyn_lstm_cell_fwd/_bwd, fdyn_lstm_seq_fwd/_bwd(_bsum),      BPTT point-wise cell update and its gradient (bias sums folded in),
 *   fdyn_lstm_cell0_fwd/_bwd, fdyn_colsum_partials                the zero-state three-gate layout of the features extractor
 *   fdyn_gae, fdyn_ppo_loss, fdyn_colsum                         GAE(lambda), clipped-surrogate loss + gradient, bias gradients
 *                          (SB3 PPO.train semantics driven by learned_controllers/train_rate.py:128-147; parity unpinned --
 *                          SB3 is absent -- and checked against the same arithmetic in plain torch)
 * The reference-side binding a maintainer would add (ctypes) is shown in INTEGRATION.md.
 */
#ifndef FDYN_H
#define FDYN_H

#include <stdint.h>
#include "fdyn_layout.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FDYN_ABI_VERSION 3          /* 3: the two-cells-in-one-launch recurrent entry points removed (2: sharded episode-end records, fp32 env words in mixed) */

/* return codes: 0 ok; >0 a hipError_t from the launch; <0 argument errors */
#define FDYN_OK 0
#define FDYN_ERR_BAD_DT (-1)      /* the reference raises ValueError (simplified_6dof.py:241-245) */
#define FDYN_ERR_BAD_TYPES (-2)   /* n_types outside 1..8 */
#define FDYN_ERR_BAD_SIZE (-3)
#define FDYN_ERR_NULL (-4)

int fdyn_abi_version(void);
int fdyn_num_substeps(double dt, double dt_physics);
int fdyn_device_info(int* cu_count /*host*/, int* wave_size /*host*/, char* arch /*host*/, int arch_len);
/* smallest ev_cap with which fdyn_rate_env_step_* can never drop an episode-end record of an n-env fleet */
int64_t fdyn_event_capacity(int64_t n);

/* ---- physics ------------------------------------------------------------------------------------------------
 * x      [FD_NX][n]  state, updated in place
 * u      [FD_NU][n]  controls (elevator, aileron, rudder, throttle); clipped like set_controls
 * type   [n] uint8   aircraft-type index into params, or NULL (all type 0)
 * params [n_types][FD_NP] fp64 parameter blocks (FD_P_*), 1 <= n_types <= 8
 * advances n_sub RK4 steps of dt/n_sub each; derived_out [FD_ND][n] or NULL                                   */
int fdyn_sixdof_step_f64(double* x, const double* u, const uint8_t* type, const double* params, int n_types,
                         int64_t n, double dt, int n_sub, double* derived_out, void* stream);
int fdyn_sixdof_step_mixed(double* x, const double* u, const uint8_t* type, const double* params, int n_types,
                           int64_t n, double dt, int n_sub, double* derived_out, void* stream);
int fdyn_sixdof_step_f32(float* x, const float* u, const uint8_t* type, const double* params, int n_types,
                         int64_t n, double dt, int n_sub, float* derived_out, void* stream);
int fdyn_derived_f64(const double* x, int64_t n, double* out /*[FD_ND][n]*/, void* stream);
int fdyn_derived_f32(const float* x, int64_t n, float* out, void* stream);

/* ---- batched scalar PID --------------------------------------------------------------------------------------
 * cfg [FD_NPC] (cfg_per_lane = 0) or [n][FD_NPC] (1); state [FD_NPS][n] updated in place; out [n]             */
int fdyn_pid_compute_batch(const float* cfg, int cfg_per_lane, float* state, const float* setpoint,
                           const float* measurement, float dt, float* out, int64_t n, void* stream);

/* ---- cascade: n_steps x {mission update, waypoint->HSA->attitude->rate agents, one RK4 of dt} ---------------
 * pid_state [FD_NPID*FD_NPS][n] fp32 ; wp_idx [n] int32 (>= n_wp means mission complete)
 * pid_cfg [FD_NPID][FD_NPC] fp32 ; consts [FD_NC] fp64 (FD_C_*) ; wps [n_wp][FD_NWP] fp64, n_wp <= 16
 * surf_out [FD_NU][n] last commanded surfaces or NULL ; reached_total [n] int32 += waypoints reached, or NULL  */
int fdyn_cascade_step_f64(double* x, float* pid_state, int32_t* wp_idx, const uint8_t* type, const double* params,
                          int n_types, const float* pid_cfg, const double* consts, const double* wps, int n_wp,
                          int64_t n, double dt, int n_steps, double* surf_out, int32_t* reached_total, void* stream);
int fdyn_cascade_step_mixed(double* x, float* pid_state, int32_t* wp_idx, const uint8_t* type, const double* params,
                            int n_types, const float* pid_cfg, const double* consts, const double* wps, int n_wp,
                            int64_t n, double dt, int n_steps, double* surf_out, int32_t* reached_total, void* stream);
int fdyn_cascade_step_f32(float* x, float* pid_state, int32_t* wp_idx, const uint8_t* type, const double* params,
                          int n_types, const float* pid_cfg, const double* consts, const double* wps, int n_wp,
                          int64_t n, double dt, int n_steps, float* surf_out, int32_t* reached_total, void* stream);

/* ---- one cascade level commanded directly --------------------------------------------------------------------------
 * n_steps x {agent.compute_action(command, state, dt) -> set_controls -> one RK4 of dt}; n_steps == 0: compute_action only
 * (x untouched).  level = FD_LEVEL_* ; cmd [4][n]: RATE p, q, r, throttle | ATTITUDE roll, pitch, yaw (NaN = no yaw
 * command), throttle | HSA heading, speed, altitude, - | WAYPOINT north, east, altitude, speed (NaN = keep airspeed).
 * Replaces RateAgent / AttitudeAgent / HSAAgent / WaypointAgent.compute_action (controllers/rate_agent.py:65-124,
 * attitude_agent.py:86-154, hsa_agent.py:119-231, waypoint_agent.py:81-242) and the closed-loop helper the reference's tests
 * use (tests/test_control_integration.py:34-74).  pid_state / pid_cfg / consts as fdyn_cascade_step_*; cfg_per_lane != 0:
 * pid_cfg is [n][FD_NPID][FD_NPC], one gain set PER AIRCRAFT -- a whole gain sweep (examples/tune_pids.py tries five sets one
 * after the other) flies in one launch.                                                                                    */
int fdyn_agent_step_f64(int level, double* x, float* pid_state, const uint8_t* type, const double* params, int n_types,
                        const float* pid_cfg, int cfg_per_lane, const double* consts, const double* cmd, int64_t n, double dt,
                        int n_steps, double* surf_out, void* stream);
int fdyn_agent_step_mixed(int level, double* x, float* pid_state, const uint8_t* type, const double* params, int n_types,
                          const float* pid_cfg, int cfg_per_lane, const double* consts, const double* cmd, int64_t n, double dt,
                          int n_steps, double* surf_out, void* stream);
int fdyn_agent_step_f32(int level, float* x, float* pid_state, const uint8_t* type, const double* params, int n_types,
                        const float* pid_cfg, int cfg_per_lane, const double* consts, const float* cmd, int64_t n, double dt,
                        int n_steps, float* surf_out, void* stream);

/* ---- hybrid cascade: PID outer loops over a learned or PID rate loop, per aircraft -------------------------------------------
 * One control step per launch; the policy runs between launches on obs_out.
 *   1. apply (only if actions != NULL): learned lanes (learned[i] != 0, or learned == NULL) take actions [n][4] = [ail, elev, rud,
 *      thr], clipped to -1..1 (throttle 0..1) and stored to prev_action [n][4]; PID lanes take the surfaces the rate PID wrote
 *      to surf_out in the previous launch.  The throttle of a learned lane is the policy's (FD_HYBRID_THROTTLE_POLICY) or the
 *      outer loop's (FD_HYBRID_THROTTLE_OUTER, read back from surf_out).  Then one RK4 of dt (none for a frozen mission).
 *   2. the mission update (wps != NULL: level must be FD_LEVEL_WAYPOINT, 1 <= n_wp <= 16, cmd NULL; wp_idx / reached_total as
 *      fdyn_cascade_step_*) or the command cmd [4][n] (as fdyn_agent_step_* at `level`), then the waypoint / HSA / attitude agent
 *      on the new state, ending in a rate command p, q, r + throttle.
 *   3. PID lanes run the rate PID (its state rows advance only there) -> surf_out [4][n] for the next launch; learned lanes
 *      get the outer throttle in surf_out's throttle row and the surfaces applied in step 1 in the others.  Every lane: the
 *      policy observation obs_out [n][18] fp32 (rate_env.py:374-408 layout; command clipped to the max rates, differences
 *      and airspeed in the state's precision) and, if not NULL, rate_cmd_out [4][n] fp32 = p, q, r, throttle.
 * actions == NULL runs 2 and 3 only (x untouched): the priming call, and the single-aircraft agents' compute_action.
 * The fp32-evaluation variants rebuild their integrator trigonometry from the stored state every launch, so K launches
 * equal K one-step cascade launches bit for bit on PID lanes.                                                                 */
int fdyn_hybrid_step_f64(int level, double* x, float* pid_state, int32_t* wp_idx, const uint8_t* type, const double* params,
                         int n_types, const float* pid_cfg, const double* consts, const double* cmd, const double* wps, int n_wp,
                         const float* actions, const uint8_t* learned, int throttle_src, float* prev_action, float* obs_out,
                         float* rate_cmd_out, double* surf_out, int32_t* reached_total, int64_t n, double dt, void* stream);
int fdyn_hybrid_step_mixed(int level, double* x, float* pid_state, int32_t* wp_idx, const uint8_t* type, const double* params,
                           int n_types, const float* pid_cfg, const double* consts, const double* cmd, const double* wps, int n_wp,
                           const float* actions, const uint8_t* learned, int throttle_src, float* prev_action, float* obs_out,
                           float* rate_cmd_out, double* surf_out, int32_t* reached_total, int64_t n, double dt, void* stream);
int fdyn_hybrid_step_f32(int level, float* x, float* pid_state, int32_t* wp_idx, const uint8_t* type, const double* params,
                         int n_types, const float* pid_cfg, const double* consts, const float* cmd, const double* wps, int n_wp,
                         const float* actions, const uint8_t* learned, int throttle_src, float* prev_action, float* obs_out,
                         float* rate_cmd_out, float* surf_out, int32_t* reached_total, int64_t n, double dt, void* stream);

/* ---- rate-control env ------------------------------------------------------------------------------------------
 * x [FD_NX][n] ; e [FD_NE][n] (FD_E_*; fp64 in the f64 variant, fp32 in mixed and f32 -- there FD_E_SETTLE_TIMER counts settled
 *   steps and FD_E_TIME is step * dt) ; ei [FD_NEI][n] int32 ; env_consts [FD_NEC] fp64 (FD_EC_*)
 * pool [n][pool_depth][FD_NR] fp64 host-presampled reset records (parity mode), or NULL = in-kernel Philox draws
 *      keyed by (seed, env, episode) (throughput mode)
 * reset: mask [n] uint8 (NULL = all) ; pid_state [3*FD_NPS][n] zeroed for reset envs if non-NULL ; obs_out [n][18]
 * step : actions [n][4] fp32 (aileron, elevator, rudder, throttle), or NULL => the fused rate-PID demonstrator
 *        (needs pid_state, pid_cfg [>=3][FD_NPC], casc_consts [FD_NC]); actions_out [n][4] or NULL
 *        rw_delta [3][n] this step's random-walk deltas (parity mode) or NULL
 *        residual_scale > 0 (with actions, pid_state, pid_cfg, casc_consts): ResidualRateControlEnv
 *        (learned_controllers/envs/residual_rate_env.py:99-157): action = clip(PID + scale * actions), reward += bonus
 *        auto_reset != 0: envs that end are reset in-kernel and obs_out holds the post-reset observation
 *        reward_f32 [n] / reward_full [n] (either may be NULL) ; terminated, truncated [n] uint8
 *        ev_count [FD_EV_SHARDS] int32 (must be 0 on entry), ev_int [ev_cap][FD_EV_NI], ev_flt [ev_cap][FD_EV_NF]:
 *        compacted episode-end records (env id, length, terminated | return, terminal observation) in FD_EV_SHARDS
 *        segments of ev_cap / FD_EV_SHARDS records (fdyn_layout.h); NULL = no records.  ev_cap must be a positive
 *        multiple of FD_EV_SHARDS (FDYN_ERR_BAD_SIZE otherwise); fdyn_event_capacity(n) never drops a record.
 *        ev_count_next [FD_EV_SHARDS] or NULL: a second counter set this launch clears, so two sets can be
 *        ping-ponged across steps without a memset on the stream                                              */
int fdyn_rate_env_reset_f64(double* x, double* e, int32_t* ei, float* pid_state, const uint8_t* mask, const double* env_consts,
                            const double* pool, int pool_depth, uint64_t seed, float* obs_out, int64_t n, void* stream);
int fdyn_rate_env_step_f64(double* x, double* e, int32_t* ei, const uint8_t* type, const double* params, int n_types,
                           const double* env_consts, const float* actions, float* pid_state, const float* pid_cfg,
                           const double* casc_consts, float* actions_out, const double* rw_delta, const double* pool,
                           int pool_depth, uint64_t seed, int auto_reset, float residual_scale, float* obs_out,
                           float* reward_f32, double* reward_full, uint8_t* terminated, uint8_t* truncated, int32_t* ev_count,
                           int32_t* ev_count_next, int32_t* ev_int, float* ev_flt, int ev_cap, int64_t n, void* stream);
/* mixed: fp32 env words, see fdyn_layout.h, FD_E_* */
int fdyn_rate_env_reset_mixed(double* x, float* e, int32_t* ei, float* pid_state, const uint8_t* mask, const double* env_consts,
                              const double* pool, int pool_depth, uint64_t seed, float* obs_out, int64_t n, void* stream);
int fdyn_rate_env_step_mixed(double* x, float* e, int32_t* ei, const uint8_t* type, const double* params, int n_types,
                             const double* env_consts, const float* actions, float* pid_state, const float* pid_cfg,
                             const double* casc_consts, float* actions_out, const double* rw_delta, const double* pool,
                             int pool_depth, uint64_t seed, int auto_reset, float residual_scale, float* obs_out,
                             float* reward_f32, double* reward_full, uint8_t* terminated, uint8_t* truncated, int32_t* ev_count,
                             int32_t* ev_count_next, int32_t* ev_int, float* ev_flt, int ev_cap, int64_t n, void* stream);
int fdyn_rate_env_reset_f32(float* x, float* e, int32_t* ei, float* pid_state, const uint8_t* mask, const double* env_consts,
                            const double* pool, int pool_depth, uint64_t seed, float* obs_out, int64_t n, void* stream);
int fdyn_rate_env_step_f32(float* x, float* e, int32_t* ei, const uint8_t* type, const double* params, int n_types,
                           const double* env_consts, const float* actions, float* pid_state, const float* pid_cfg,
                           const double* casc_consts, float* actions_out, const float* rw_delta, const double* pool,
                           int pool_depth, uint64_t seed, int auto_reset, float residual_scale, float* obs_out,
                           float* reward_f32, float* reward_full, uint8_t* terminated, uint8_t* truncated, int32_t* ev_count,
                           int32_t* ev_count_next, int32_t* ev_int, float* ev_flt, int ev_cap, int64_t n, void* stream);

/* ---- rate-control env with domain randomisation (design_docs/06_RL_AGENT_TRAINING.md "Domain Randomization") ------------------
 * The two entry points above plus dr [FD_NDR][n] in the state dtype (FD_DR_* rows) and dr_consts [FD_NDC] fp64 (FD_DC_* ranges);
 * NULL for either => FDYN_ERR_NULL.  In the dynamics the aerodynamics see the air-relative body velocity v - R^T (W + g)
 * (W = steady wind, g = gust, NED, both read from dr and held over the step), kinematics keep the ground-relative one, and the
 * type's mass, inertias and air density are multiplied by the env's FD_DR_*_S rows.  After the physics the gust advances as
 * g <- A g + B n (n ~ N(0, 1) per axis, Philox keyed by seed, env, episode, step).  Observation airspeed, the airspeed
 * stability reward term and the stall test use the air-relative airspeed.  A reset with dr_consts[FD_DC_REDRAW] != 0 draws
 * every row from its range (A = exp(-dt V0 / L), B = sigma sqrt(1 - A^2), g0 ~ N(0, sigma^2), sigma = intensity V0, V0 = the
 * record's airspeed); with 0 it keeps the rows.  Either way the record's airspeed is air-relative: v = (V0, 0, 0) + R^T (W + g0).
 * IC and command draws are those of the plain entry points.  With neutral ranges (no wind, intensity 0, every scale 1) the
 * results equal the plain entry points' bit for bit.                                                                              */
int fdyn_rate_env_reset_dr_f64(double* x, double* e, int32_t* ei, float* pid_state, const uint8_t* mask, const double* env_consts,
                               const double* pool, int pool_depth, uint64_t seed, float* obs_out, int64_t n, double* dr,
                               const double* dr_consts, void* stream);
int fdyn_rate_env_step_dr_f64(double* x, double* e, int32_t* ei, const uint8_t* type, const double* params, int n_types,
                              const double* env_consts, const float* actions, float* pid_state, const float* pid_cfg,
                              const double* casc_consts, float* actions_out, const double* rw_delta, const double* pool,
                              int pool_depth, uint64_t seed, int auto_reset, float residual_scale, float* obs_out,
                              float* reward_f32, double* reward_full, uint8_t* terminated, uint8_t* truncated, int32_t* ev_count,
                              int32_t* ev_count_next, int32_t* ev_int, float* ev_flt, int ev_cap, int64_t n, double* dr,
                              const double* dr_consts, void* stream);
int fdyn_rate_env_reset_dr_mixed(double* x, float* e, int32_t* ei, float* pid_state, const uint8_t* mask, const double* env_consts,
                                 const double* pool, int pool_depth, uint64_t seed, float* obs_out, int64_t n, double* dr,
                                 const double* dr_consts, void* stream);
int fdyn_rate_env_step_dr_mixed(double* x, float* e, int32_t* ei, const uint8_t* type, const double* params, int n_types,
                                const double* env_consts, const float* actions, float* pid_state, const float* pid_cfg,
                                const double* casc_consts, float* actions_out, const double* rw_delta, const double* pool,
                                int pool_depth, uint64_t seed, int auto_reset, float residual_scale, float* obs_out,
                                float* reward_f32, double* reward_full, uint8_t* terminated, uint8_t* truncated, int32_t* ev_count,
                                int32_t* ev_count_next, int32_t* ev_int, float* ev_flt, int ev_cap, int64_t n, double* dr,
                                const double* dr_consts, void* stream);
int fdyn_rate_env_reset_dr_f32(float* x, float* e, int32_t* ei, float* pid_state, const uint8_t* mask, const double* env_consts,
                               const double* pool, int pool_depth, uint64_t seed, float* obs_out, int64_t n, float* dr,
                               const double* dr_consts, void* stream);
int fdyn_rate_env_step_dr_f32(float* x, float* e, int32_t* ei, const uint8_t* type, const double* params, int n_types,
                              const double* env_consts, const float* actions, float* pid_state, const float* pid_cfg,
                              const double* casc_consts, float* actions_out, const float* rw_delta, const double* pool,
                              int pool_depth, uint64_t seed, int auto_reset, float residual_scale, float* obs_out,
                              float* reward_f32, float* reward_full, uint8_t* terminated, uint8_t* truncated, int32_t* ev_count,
                              int32_t* ev_count_next, int32_t* ev_int, float* ev_flt, int ev_cap, int64_t n, float* dr,
                              const double* dr_consts, void* stream);

/* ---- rate-control env with a prepared launch image ---------------------------------------------------------------------------
 * A step derives a few words from the parameter table and env_consts alone: per aircraft type the reciprocals and the sin / cos /
 * tan of the limits in the staged block (FD_PD_*), and from env_consts the sub-step count and the settle-step count.  The entry
 * points above compute them in every workgroup of every launch; fdyn_rate_env_image computes them ONCE, with the same device
 * code, into image [FD_NIMG] fp64 (fdyn_layout.h, FD_IMG_*), and the _img entry points read them from there.  fp32_eval: 1 for
 * an image the mixed / f32 variants read, 0 for the f64 variant (it reads fewer derived words).  The _img entry points take the
 * argument list of their plain counterparts plus the image; `params` and `env_consts` are not read (the image holds both) and
 * may be NULL; n_types is the one the image was filled with.  Results equal the plain entry points' bit for bit.  Fill the image
 * again whenever params or env_consts change: it is a copy, not a view.                                                      */
int fdyn_rate_env_image(const double* params, int n_types, const double* env_consts, int fp32_eval, double* image, void* stream);
int fdyn_rate_env_step_img_f64(double* x, double* e, int32_t* ei, const uint8_t* type, const double* params, int n_types,
    const double* env_consts, const float* actions, float* pid_state, const float* pid_cfg, const double* casc_consts,
    float* actions_out, const double* rw_delta, const double* pool, int pool_depth, uint64_t seed, int auto_reset,
    float residual_scale, float* obs_out, float* reward_f32, double* reward_full, uint8_t* terminated, uint8_t* truncated,
    int32_t* ev_count, int32_t* ev_count_next, int32_t* ev_int, float* ev_flt, int ev_cap, int64_t n, const double* image,
    void* stream);
int fdyn_rate_env_step_dr_img_f64(double* x, double* e, int32_t* ei, const uint8_t* type, const double* params, int n_types,
    const double* env_consts, const float* actions, float* pid_state, const float* pid_cfg, const double* casc_consts,
    float* actions_out, const double* rw_delta, const double* pool, int pool_depth, uint64_t seed, int auto_reset,
    float residual_scale, float* obs_out, float* reward_f32, double* reward_full, uint8_t* terminated, uint8_t* truncated,
    int32_t* ev_count, int32_t* ev_count_next, int32_t* ev_int, float* ev_flt, int ev_cap, int64_t n, double* dr,
    const double* dr_consts, const double* image, void* stream);
int fdyn_rate_env_step_img_mixed(double* x, float* e, int32_t* ei, const uint8_t* type, const double* params, int n_types,
    const double* env_consts, const float* actions, float* pid_state, const float* pid_cfg, const double* casc_consts,
    float* actions_out, const double* rw_delta, const double* pool, int pool_depth, uint64_t seed, int auto_reset,
    float residual_scale, float* obs_out, float* reward_f32, double* reward_full, uint8_t* terminated, uint8_t* truncated,
    int32_t* ev_count, int32_t* ev_count_next, int32_t* ev_int, float* ev_flt, int ev_cap, int64_t n, const double* image,
    void* stream);
int fdyn_rate_env_step_dr_img_mixed(double* x, float* e, int32_t* ei, const uint8_t* type, const double* params, int n_types,
    const double* env_consts, const float* actions, float* pid_state, const float* pid_cfg, const double* casc_consts,
    float* actions_out, const double* rw_delta, const double* pool, int pool_depth, uint64_t seed, int auto_reset,
    float residual_scale, float* obs_out, float* reward_f32, double* reward_full, uint8_t* terminated, uint8_t* truncated,
    int32_t* ev_count, int32_t* ev_count_next, int32_t* ev_int, float* ev_flt, int ev_cap, int64_t n, double* dr,
    const double* dr_consts, const double* image, void* stream);
int fdyn_rate_env_step_img_f32(float* x, float* e, int32_t* ei, const uint8_t* type, const double* params, int n_types,
    const double* env_consts, const float* actions, float* pid_state, const float* pid_cfg, const double* casc_consts,
    float* actions_out, const float* rw_delta, const double* pool, int pool_depth, uint64_t seed, int auto_reset,
    float residual_scale, float* obs_out, float* reward_f32, float* reward_full, uint8_t* terminated, uint8_t* truncated,
    int32_t* ev_count, int32_t* ev_count_next, int32_t* ev_int, float* ev_flt, int ev_cap, int64_t n, const double* image,
    void* stream);
int fdyn_rate_env_step_dr_img_f32(float* x, float* e, int32_t* ei, const uint8_t* type, const double* params, int n_types,
    const double* env_consts, const float* actions, float* pid_state, const float* pid_cfg, const double* casc_consts,
    float* actions_out, const float* rw_delta, const double* pool, int pool_depth, uint64_t seed, int auto_reset,
    float residual_scale, float* obs_out, float* reward_f32, float* reward_full, uint8_t* terminated, uint8_t* truncated,
    int32_t* ev_count, int32_t* ev_count_next, int32_t* ev_int, float* ev_flt, int ev_cap, int64_t n, float* dr,
    const double* dr_consts, const double* image, void* stream);

/* ---- policy-side fused kernels (csrc/policy_kernels.hip) ------------------------------------------------------------
 * LSTM cell point-wise update from pre-activation gates [B][4H] (PyTorch order i,f,g,o; bias already added by the
 * GEMM): replaces the ~40 element-wise launches torch needs per cell (nn.LSTM arithmetic used by
 * learned_controllers/networks/lstm_policy.py:49-61 and sb3_contrib's actor/critic LSTMs).
 * gates_bf16: 1 = bf16 storage for gates/h_lp/act/dh/dgates, 0 = fp32.  c_prev NULL = zero state.  H % 8 == 0.
 * fwd: h_f32 [B][H] and/or h_lp [B][H] (either may be NULL), c_out [B][H] fp32, act_out [B][4H] activated gates or NULL.
 * bwd: from act, c_prev, c_new, dh (+ dc_next or NULL) -> dgates [B][4H], dc_prev [B][H] (or NULL).  A zero-state cell
 *      (c_prev NULL) may pass c_new NULL: c = i * g is then rebuilt from the saved gates (its forward need not keep c). */
int fdyn_lstm_cell_fwd(const void* gates, int gates_bf16, const float* c_prev, float* h_f32, void* h_lp, float* c_out,
                       void* act_out, int64_t B, int H, void* stream);
int fdyn_lstm_cell_bwd(const void* act, int bf16, const float* c_prev, const float* c_new, const void* dh,
                       const float* dc_next, void* dgates, float* dc_prev, int64_t B, int H, void* stream);
/* One step of an LSTM SEQUENCE (BPTT over T inside one autograd node): the same point-wise kernels with the episode-start
 * masks and the recurrent plumbing folded in, so a step costs two launches each way (the GEMM and this).
 * fwd: c_prev is multiplied by keep [B] (NULL = 1); besides h_lp [B][H] the kernel stores h * keep_next into h_next (row
 *      stride next_stride elements: the recurrent columns of the NEXT step's [x | h] input row), or h_next = NULL;
 *      bias [B / group_rows][4H] (gates dtype) or NULL is added to the gates of rows in group row / group_rows (a batched
 *      GEMM over several cells has no bias epilogue).
 * bwd: dh_total = dh + dh2_keep * dh2 (dh2 = the recurrent columns of step t+1's input gradient, row stride dh2_stride,
 *      or NULL), summed in fp32; dgates may alias act (in place); dc_prev comes out already multiplied by keep.        */
int fdyn_lstm_seq_fwd(const void* gates, int gates_bf16, const float* c_prev, const float* keep, void* h_lp, float* c_out,
                      void* act_out, void* h_next, int64_t next_stride, const float* keep_next, const void* bias,
                      int64_t group_rows, int64_t B, int H, void* stream);
int fdyn_lstm_seq_bwd(const void* act, int bf16, const float* c_prev, const float* keep, const float* c_new, const void* dh,
                      const void* dh2, int64_t dh2_stride, const float* dh2_keep, const float* dc_next, void* dgates,
                      float* dc_prev, int64_t B, int H, void* stream);
/* The same backward step with the BIAS GRADIENT folded in: every block owns rows_per_block consecutive rows, sums its dgates
 * (the rounded values it stores) per column and writes one partial row to bias_ws [ceil(B / rows_per_block)][4H]; the partial
 * rows of all steps of a BPTT pass are then reduced by fdyn_colsum_partials instead of a second pass over [T*B][4H].
 * Needs 256 % (H / 8) == 0 and (rows_per_block * H / 8) % 256 == 0. */
int fdyn_lstm_seq_bwd_bsum(const void* act, int bf16, const float* c_prev, const float* keep, const float* c_new, const void* dh,
                           const void* dh2, int64_t dh2_stride, const float* dh2_keep, const float* dc_next, void* dgates,
                           float* dc_prev, float* bias_ws, int64_t rows_per_block, int64_t B, int H, void* stream);
/* The same backward step when the forward kept the PRE-activations instead of the activated gates (the GEMM wrote them, the
 * forward point-wise pass never re-wrote them: 8 of its 28 bytes per hidden unit): `gates` [B][4H] + bias [B / group_rows][4H]
 * (gates dtype) are activated again here; everything else as fdyn_lstm_seq_bwd(_bsum) (bias_ws may be NULL). */
int fdyn_lstm_seq_bwd_pre(const void* gates, int bf16, const void* bias, int64_t group_rows, const float* c_prev, const float* keep,
                          const float* c_new, const void* dh, const void* dh2, int64_t dh2_stride, const float* dh2_keep,
                          const float* dc_next, void* dgates, float* dc_prev, float* bias_ws, int64_t rows_per_block, int64_t B, int H,
                          void* stream);
/* Zero-state cell in the THREE-gate layout (i, g, o along 3H): the features extractor's LSTM layers, which the reference runs
 * on a length-1 sequence without carried state (learned_controllers/networks/lstm_policy.py:75-92), so the forget gate
 * multiplies zero and neither its pre-activation nor its gradient exists.  fwd: gates [B][3H] (bias added by the GEMM) ->
 * h_out [B][H], act_out [B][3H] activated gates (NULL = not kept; may alias gates).  bwd: act, dh -> dgates [B][3H] (may alias
 * act); bias_ws as above with rows of 3H floats, or NULL. */
int fdyn_lstm_cell0_fwd(const void* gates, int bf16, void* h_out, void* act_out, int64_t B, int H, void* stream);
int fdyn_lstm_cell0_bwd(const void* act, int bf16, const void* dh, void* dgates, float* bias_ws, int64_t rows_per_block,
                        int64_t B, int H, void* stream);
/* The two trunks of the policy's mlp_extractor (pi and vf: Linear(256,128)+ReLU -> Linear(128,64)+ReLU; sb3_contrib MlpLstmPolicy
 * with the reference's net_arch, learned_controllers/networks/lstm_policy.py:107-136) as ONE MFMA launch (csrc/policy_trunk.hip):
 * h_pi, h_vf [B][256] bf16 -> lat_pi, lat_vf [B][64] bf16.  W1 [2][128][256] bf16 and b1 [2][128] fp32 (index 0 = pi, 1 = vf);
 * W2p [2][64][128] bf16 with the columns of every block of 16 in the order (0 1 2 3 8 9 10 11 4 5 6 7 12 13 14 15) -- the
 * first layer's output tile is the second layer's MFMA operand as it stands -- and b2 [2][64] fp32. */
int fdyn_policy_trunks(const void* h_pi, const void* h_vf, const void* W1, const float* b1, const void* W2p, const float* b2,
                       void* lat_pi, void* lat_vf, int64_t B, void* stream);
/* The same two trunks with the output heads and the sampling behind them in ONE launch (what fdyn_policy_trunks +
 * fdyn_policy_heads do in two, with lat_pi / lat_vf never leaving the registers): Wa [4][64], ba [4], wv [64], bv [1] bf16,
 * log_std [4] fp32, Philox key (seed, row, *step) as fdyn_policy_heads -> actions [B][4], logp [B], value [B] fp32.        */
int fdyn_policy_trunks_heads(const void* h_pi, const void* h_vf, const void* W1, const float* b1, const void* W2p, const float* b2,
                             const void* Wa, const void* ba, const void* wv, const void* bv, const float* log_std, uint64_t seed,
                             const uint32_t* step, int deterministic, float* actions, float* logp, float* value, int64_t B,
                             void* stream);
/* Rollout glue in one launch: episode_start [n] = (terminated | truncated) as fp32, keep [n] = 1 - episode_start (either may be
 * NULL), *counter += 1 (NULL = none: the device-side step counter of fdyn_policy_heads / fdyn_gaussian_head's action noise). */
int fdyn_episode_flags(const uint8_t* terminated, const uint8_t* truncated, float* episode_start, float* keep, int32_t* counter,
                       int64_t n, void* stream);
/* out [N] = column sums of nb partial rows [nb][N] fp32 (two stages, no atomics); ws_mid [ceil(nb / 64)][N]. */
int fdyn_colsum_partials(const float* partial, int64_t nb, int N, float* out, float* ws_mid, void* stream);
/* Reductions of the PPO update, self-contained so that a hipGraph replay recomputes them (accumulators are cleared by a
 * kernel of the same launch sequence).  fdyn_colsum: out [N] fp32 = column sums of x [M][N] (bf16 or fp32), two stages
 * through ws [fdyn_colsum_ws_floats(...)], no atomics: bias gradients.  n_groups > 1: rows come in segments of group_rows,
 * segment j belonging to group j % n_groups (the [T][G][B] row order of a multi-cell LSTM sequence); out [n_groups][N].
 * fdyn_ppo_loss: the clipped-surrogate loss of one slice of M samples and its gradient w.r.t. the policy outputs
 * (SB3 PPO.train semantics, which learned_controllers/train_rate.py:128-147 drives): mean, actions [M][4], log_std [4],
 * values, old_logp, adv, ret [M] (old_values [M] only if clip_range_vf > 0) -> dmean [M][4], dvalues [M],
 * stats [FDYN_PPO_NSTATS] = {policy loss, value loss, approx KL, clip fraction, policy + vf_coef * value,
 * d/dlog_std[4] of the log-prob part}; ws [2] scratch.  The entropy term is added by the caller.                         */
#define FDYN_PPO_NSTATS 9
int64_t fdyn_colsum_ws_floats(int64_t M, int N, int64_t group_rows, int n_groups);   /* size of ws (floats) */
int fdyn_colsum(const void* x, int bf16, int64_t M, int N, int64_t group_rows, int n_groups, float* out, float* ws, void* stream);
int fdyn_ppo_loss(const float* mean, const float* actions, const float* log_std, const float* values, const float* old_logp,
                  const float* adv, const float* ret, const float* old_values, int normalize_adv, float clip_range,
                  float clip_range_vf, float vf_coef, int64_t M, float* dmean, float* dvalues, float* stats, float* ws,
                  void* stream);
/* The whole LSTM cell step as ONE MFMA kernel (csrc/lstm_mfma.hip): gates = [x | keep*h_prev] W^T + bias on
 * v_mfma_f32_32x32x16_bf16 with the gate non-linearity and cell update fused on the accumulators (no [B][4H] tensor).
 * x [B][kx] bf16, h_prev [B][kh] bf16, c_prev [B][H] fp32, keep [B] fp32 or NULL (0 = episode start: zero the state),
 * W [4H][kx+kh] bf16 (= [W_ih | W_hh], gate order i,f,g,o), bias [4H] fp32 (= b_ih + b_hh).
 * kh == 0: zero-state layer (the reference's feature-extractor LSTM, lstm_policy.py:75-92): no h/c input.
 * Outputs h_out [B][H] bf16, c_out [B][H] fp32 (NULL allowed), h_out_f32 [B][H] or NULL.
 * Supported (kx, kh): (128,256) (128,0) (256,0) (128,128); H % 32 == 0.                                              */
int fdyn_lstm_cell_mfma(const void* x, int kx, const void* h_prev, int kh, const float* c_prev, const float* keep,
                        const void* W, const float* bias, void* h_out, float* c_out, float* h_out_f32,
                        int64_t B, int H, void* stream);
/* 1 = this shape may be stepped IN PLACE (h_out == h_prev, c_out == c_prev): half the state footprint, which at 65 536 rows
 * is what lets the two cells' state (201 MB) live in the 256 MB Infinity Cache from one rollout step to the next (measured:
 * rollout step 0.279 -> 0.261 ms).  Any other shape given aliased state is refused with FDYN_ERR_BAD_SIZE.                  */
int fdyn_lstm_cell_mfma_inplace_ok(int kx, int kh, int H, int64_t B);
/* Two cells of the same shape on the same x and keep -- MlpLstmPolicy's actor and critic LSTM
 * (learned_controllers/networks/lstm_policy.py:107-136, sb3_contrib's separate lstm_actor / lstm_critic) -- in ONE launch where
 * the one-wave-per-SIMD kernel applies (kx = 128, kh = H = 256, B a multiple of 256 and >= 32 768), otherwise as two calls of
 * fdyn_lstm_cell_mfma.  Operand meaning and the in-place rule as there; both cells need c_out.                               */
int fdyn_lstm_cell_mfma_pair(const void* x, int kx, const float* keep, int kh, int64_t B, int H,
                             const void* h_prev0, const float* c_prev0, const void* W0, const float* bias0, void* h_out0, float* c_out0,
                             const void* h_prev1, const float* c_prev1, const void* W1, const float* bias1, void* h_out1, float* c_out1,
                             void* stream);
/* BPTT forward of the same cell (csrc/lstm_mfma.hip, TRAIN instantiation): besides h_out / c_out it stores the ACTIVATED gates
 * act_out (bf16; kh > 0: [B][4H] = sigmoid(i), sigmoid(f), tanh(g), sigmoid(o); kh = 0, the zero-state layers of the features
 * extractor: [B][3H] = (i, g, o), c_out may be NULL) for fdyn_lstm_seq_bwd / fdyn_lstm_cell0_bwd, and -- h_next != NULL --
 * h' * keep_next into rows of stride next_stride (the recurrent columns of the next step's [x | h] row, which the weight-gradient
 * GEMM reads).  Replaces the training step's GEMM -> [B][4H] pre-activations in HBM -> fdyn_lstm_seq_fwd round trip. */
int fdyn_lstm_cell_mfma_train(const void* x, int kx, const void* h_prev, int kh, const float* c_prev, const float* keep,
                              const void* W, const float* bias, void* h_out, float* c_out, void* act_out,
                              void* h_next, int64_t next_stride, const float* keep_next, int64_t B, int H, void* stream);
/* The policy's features extractor as ONE kernel (csrc/policy_fe64.hip; learned_controllers/networks/lstm_policy.py:13-97):
 * obs [B][18] fp32 -> Linear(18,128)+ReLU -> two zero-state LSTM layers (128->256->256) -> Linear(256,128)+ReLU -> feats
 * [B][128] bf16, activations in registers between the layers.  weight_image: the four weight matrices as bf16 in the
 * kernel's streaming order and LDS layout (fdyn_policy_features_image_bytes() bytes; host packer: policy.pack_fe_weights),
 * bias [128 + 1024 + 1024 + 128] fp32 = embedding, b_ih + b_hh of layer 1 and 2, projection.  B % 256 == 0.               */
int fdyn_policy_features_image_bytes(void);
int fdyn_policy_features(const float* obs, const void* weight_image, const float* bias, void* feats, int64_t B, void* stream);
/* The same launch also doing the rollout glue of fdyn_episode_flags for its rows (terminated / truncated [B] uint8 of the
 * PREVIOUS env step -> episode_start [B], keep [B] fp32, either may be NULL; *counter += 1, NULL = none): the cells launched
 * behind it read keep, the heads read the counter -- one launch less per rollout step.                                      */
int fdyn_policy_features_flags(const float* obs, const void* weight_image, const float* bias, void* feats,
                               const uint8_t* terminated, const uint8_t* truncated, float* episode_start, float* keep,
                               int32_t* counter, int64_t B, void* stream);
/* Diagonal-Gaussian policy head: actions [B][4] = mean + exp(log_std) * N(0,1) (Philox keyed by seed, env, *step -- a
 * uint32 counter in DEVICE memory the caller increments on the stream, so graph replays draw fresh noise; or the mean
 * itself when deterministic), logp [B] = log-probability of the sampled action.  mean [B][4] bf16 (mean_bf16=1) or fp32. */
int fdyn_gaussian_head(const void* mean, int mean_bf16, const float* log_std, uint64_t seed, const uint32_t* step, int deterministic,
                       float* actions, float* logp, int64_t B, void* stream);
/* Both output heads + sampling in one launch: mean = pi_hidden [B][64] Wa^T + ba (action_net 64 -> 4), value = vf_hidden
 * [B][64] wv + bv (value_net 64 -> 1), then the Gaussian head.  All weights / hiddens bf16; actions [B][4], logp, value fp32. */
int fdyn_policy_heads(const void* pi_hidden, const void* vf_hidden, const void* Wa, const void* ba, const void* wv, const void* bv,
                      const float* log_std, uint64_t seed, const uint32_t* step, int deterministic, float* actions, float* logp,
                      float* value, int64_t B, void* stream);
/* GAE(lambda) over a [T][N] rollout (one lane per env): adv, ret [T][N].  episode_starts[t][n] = 1 if env n was reset
 * before step t; last_values / last_dones [N] describe the state after the final step.                              */
int fdyn_gae(const float* rewards, const float* values, const float* episode_starts, const float* last_values,
             const float* last_dones, float gamma, float lam, int T, int64_t N, float* adv, float* ret, void* stream);


/* ---- evaluation metrics (csrc/eval_kernels.hip) -----------------------------------------------------------------------
 * MetricsCalculator.compute_metrics (learned_controllers/eval/metrics.py:95-362) for n recorded episodes at once.
 * times [T] fp64 shared time base (times[t] = env time after step t+1, as eval_rate.py:104,219 records info["time"]);
 * rates, commands [T][3][n]; actions [T][n][4] fp32; rewards [T][n]; lengths [n] int32 = steps of each episode (<= T);
 * settle_steps = int(settling_duration / dt).  out [FD_NM][n] fp64 in RateControlMetrics field order (FD_M_*; success
 * as 0/1).  An axis whose |command| stays < 0.01 keeps zeros (metrics.py:144-145); a zero-length episode gives zeros. */
int fdyn_rate_metrics_f64(const double* times, const double* rates, const double* commands, const float* actions,
                          const double* rewards, const int32_t* lengths, double settling_threshold, int settle_steps,
                          int T, int64_t n, double* out, void* stream);
int fdyn_rate_metrics_f32(const double* times, const float* rates, const float* commands, const float* actions,
                          const float* rewards, const int32_t* lengths, double settling_threshold, int settle_steps,
                          int T, int64_t n, double* out, void* stream);


/* ---- rewards on recorded data (csrc/eval_kernels.hip) -----------------------------------------------------------------
 * RateTrackingReward.compute + SettlingTimeBonus.compute (learned_controllers/envs/rewards.py:48-137,168-221) over n
 * independent sequences of T steps, one sequence per lane -- the same arithmetic the fused env step applies
 * (rate_env.py:248-279), here with the reference's configurable weights and with the per-step components the env step
 * does not materialise.  errs [T][3][n]; actions [T][4][n] ([aileron, elevator, rudder, throttle]); prev0 [4][n] = the
 * action before step 0 (later steps use the previous row); flight [T][FD_NRF][n]; cmd [3][n]; params [FD_NRW] fp64;
 * rstate [FD_NRS][n] in/out (zeros = reset()).  Outputs (any may be NULL): tracking [T][n] (the RateTrackingReward total),
 * components [T][FD_NRC][n], settle [T][n] (the bonus of each step), settled [T][n] uint8 (is_settled after the step). */
int fdyn_rate_reward_seq_f64(const double* errs, const double* actions, const double* prev0, const double* flight,
                             const double* cmd, const double* params, double* rstate, double dt, int T, int64_t n,
                             double* tracking, double* components, double* settle, uint8_t* settled, void* stream);
int fdyn_rate_reward_seq_f32(const float* errs, const float* actions, const float* prev0, const float* flight,
                             const float* cmd, const double* params, float* rstate, float dt, int T, int64_t n,
                             float* tracking, float* components, float* settle, uint8_t* settled, void* stream);


/* ---- trajectory comparison, streamed (csrc/eval_kernels.hip) ----------------------------------------------------------
 * compare_trajectories (validation/metrics/trajectory_metrics.py:71-174) for n pairs of trajectories at once, with nothing
 * recorded: the launch consumes T steps of set A and set B in order and carries everything it needs in acc.
 * xa, xb [T][FD_NX][n] states, fp64 or (a_f32 / b_f32 != 0) fp32 -- with T = 1 a fleet's own x buffer; da, db
 * [T][FD_ND][n] derived rows in the same type as their side's states (airspeed and altitude are read), NULL = computed
 * from x as fdyn_derived_f64 does.  acc [FD_NTA][n] fp64 in/out (FD_TA_*; all zeros = a fresh comparison): a later launch
 * continues exactly where this one stopped, so any chunking of a trajectory gives bit-identical acc and metrics.
 * out [FD_NTM][n] fp64 (FD_TM_*) or NULL: the metrics finished from acc after the T steps; T = 0 finishes only.
 * All arithmetic is fp64; attitude and body rates are compared in degrees, yaw unwrapped as np.unwrap(period=360).
 * A correlation is 0 with fewer than two steps, NaN when either side is constant, and clamped to [-1, 1] otherwise;
 * no step at all gives zeros everywhere.                                                                                  */
int fdyn_traj_compare(const void* xa, int a_f32, const void* da, const void* xb, int b_f32, const void* db,
                      int T, int64_t n, double* acc, double* out, void* stream);


/* ---- steady flight and linearisation (csrc/trim_kernels.hip) ----------------------------------------------------------
 * fdyn_trim: the trim condition of docs/6dof_mathematical_formulation.tex:1380-1410 (x_dot = 0, "set controls to estimated
 * trim values" -- the reference states it and codes no solver), solved per aircraft.  spec [FD_NTS][n] fp64 (FD_TS_*):
 * airspeed V, flight-path angle gamma, turn rate psi_dot, altitude h, heading psi0.  type [n] uint8 or NULL (= 0);
 * scales [FD_NSC][n] fp64 multipliers on mass, Ixx, Iyy, Izz, air density, or NULL (= 1); params [n_types][FD_NP].
 * Unknowns z = (alpha, theta, phi, elevator, aileron, rudder, throttle), controls normalised as set_controls takes them and
 * NOT clipped while solving.  State from z: N = E = 0, D = -h, (u, v, w) = (V cos alpha, 0, V sin alpha), attitude
 * (phi, theta, psi0), (p, q, r) = psi_dot (-sin theta, sin phi cos theta, cos phi cos theta).  Residual
 * F = (u_dot, v_dot, w_dot, p_dot, q_dot, r_dot, D_dot + V sin gamma).  Newton from z0 = (0.05, 0.05 + gamma,
 * atan(V psi_dot / g), 0, 0, 0, 0.5): Jacobian by central differences with step 1e-6 (divided by the step actually taken),
 * full step from a 7 x 7 elimination with partial pivoting, a pivot below 1e-14 max|J| = singular, stop at
 * max|dz| < 1e-12, at most 20 steps.  Outputs, always the last iterate: x0 [FD_NX][n], u0 [FD_NU][n] fp64,
 * residual [n] = max|F| there (NaN for a BAD_SPEC lane), iters [n], status [n] int32 (FD_TRIM_* bits, 0 = flyable).     */
int fdyn_trim(const double* spec, const uint8_t* type, const double* scales, const double* params, int n_types, int64_t n,
              double* x0, double* u0, double* residual, int32_t* iters, int32_t* status, void* stream);
/* fdyn_linearize: the "linearised rate dynamics near trim" of docs/control_hierarchy_design.tex:282, which the reference
 * derives its PID structure from and never computes -- here for the full 12-state model at ANY state.  x [FD_NX][n] and
 * u [FD_NU][n], both fp64 or (xu_f32 != 0) both fp32; type, scales, params as above.  A [FD_NX * FD_NX][n] with
 * A[12 i + j] = d xdot_i / d x_j and B [FD_NX * FD_NU][n] with B[4 i + k] = d xdot_i / d u_k, fp64: central differences of
 * the unclipped equations of motion, state steps 1e-5 max(1, |x_j|), control steps 1e-5, each divided by
 * (x + s) - (x - s).  32 evaluations per aircraft in one launch.  Neither entry point synchronises or allocates.          */
int fdyn_linearize(const void* x, const void* u, int xu_f32, const uint8_t* type, const double* scales, const double* params,
                   int n_types, int64_t n, double* A, double* B, void* stream);


/* ---- gain-scheduled LQR (csrc/lqr_kernels.hip) ---------------------------------------------------------------------------
 * fdyn_lqr_design: the design step between fdyn_linearize and flight, one lane per aircraft, fp64.  A [FD_NX * FD_NX][n] and
 * B [FD_NX * FD_NU][n] exactly as fdyn_linearize writes them; weights [FD_NLQW] fp64 shared, or (weights_per_lane != 0)
 * [FD_NLQW][n]: a sweep of weight sets in one launch.  Per block -- longitudinal (u, w, q, theta | elevator, throttle) and
 * lateral (v, p, r, phi | aileron, rudder), (a, b) cut out of A, B -- the equation a^T X + X a - X G X + Q = 0 with
 * G = b R^-1 b^T is solved by the structure-preserving doubling algorithm: gamma = max(1, |a|_inf), a_g = a - gamma I,
 * W = a_g^T + Q a_g^-1 G, A_0 = I + 2 gamma W^-T, G_0 = 2 gamma a_g^-1 G W^-1, H_0 = 2 gamma W^-1 Q a_g^-1; then with
 * M = (I + G_k H_k)^-1: A_k+1 = A_k M A_k, G_k+1 = G_k + A_k M G_k A_k^T, H_k+1 = H_k + A_k^T H_k M A_k, until
 * max|H_k+1 - H_k| <= 1e-13 max(1, max|H_k+1|), at most 30 times.  X = (H + H^T) / 2, K = R^-1 b^T X.  Every 4 x 4 inverse
 * is an elimination with partial pivoting; a pivot below 1e-14 max|matrix| = singular.
 * Outputs: K [FD_NLQK][n] (FD_LQK_*), residual [n] = max|a^T X + X a - X G X + Q| / max(1, max|X|) of the worse block (NaN for
 * a BAD_INPUT lane), iters [n] (the larger of the two blocks), status [n] int32 (FD_LQR_* bits).  Status 0 is a certificate:
 * with Q > 0, X > 0 (an unrolled 4 x 4 L D L^T with every d > 0) and a residual <= 1e-8,
 * (a - b K)^T X + X (a - b K) = -Q - K^T R K < 0, so X is a Lyapunov function of the closed block and a - b K is Hurwitz --
 * proved per lane without computing an eigenvalue.  A lane with status != 0 gets K = 0 in all FD_NLQK words: flown, it
 * holds u0.  The words of A and B outside the two blocks are not read.  Neither entry point synchronises or allocates.   */
int fdyn_lqr_design(const double* A, const double* B, const double* weights, int weights_per_lane, int64_t n, double* K,
                    double* residual, int32_t* iters, int32_t* status, void* stream);
/* fdyn_lqr_step_*: n_steps x { u = u0 - K delta -> set_controls' clip -> one RK4 of dt } in one launch, the physics of
 * fdyn_agent_step_* to the bit.  delta = the eight words (u, w, q, theta | v, p, r, phi) of x - x0, formed in fp64, the two
 * angle differences wrapped to [-pi, pi); the feedback runs in fp64 (_f64) or fp32 (_mixed, _f32).  x [FD_NX][n] is updated
 * in place; x0 [FD_NX][n], u0 [FD_NU][n], K [FD_NLQK][n] fp64; type [n] uint8 or NULL, params [n_types][FD_NP].
 * surf_out [FD_NU][n] or NULL: the last applied, clipped controls.  sat_steps [n] int32 or NULL: += the number of steps in
 * which any control was clipped.  n_steps == 0 computes the controls only (x and sat_steps untouched).                    */
int fdyn_lqr_step_f64(double* x, const double* x0, const double* u0, const double* K, const uint8_t* type, const double* params,
                      int n_types, int64_t n, double dt, int n_steps, double* surf_out, int32_t* sat_steps, void* stream);
int fdyn_lqr_step_mixed(double* x, const double* x0, const double* u0, const double* K, const uint8_t* type, const double* params,
                        int n_types, int64_t n, double dt, int n_steps, double* surf_out, int32_t* sat_steps, void* stream);
int fdyn_lqr_step_f32(float* x, const double* x0, const double* u0, const double* K, const uint8_t* type, const double* params,
                      int n_types, int64_t n, double dt, int n_steps, float* surf_out, int32_t* sat_steps, void* stream);


/* ---- steady-state Kalman filter and the LQG loop (csrc/kf_kernels.hip) -----------------------------------------------------
 * fdyn_kf_design: the estimator's design, the dual of fdyn_lqr_design, one lane per aircraft, fp64.  A, B as fdyn_linearize
 * writes them; noise [FD_NKFN] shared or (noise_per_lane != 0) [FD_NKFN][n] (FD_KFN_*).  Per block (a, b) of fdyn_lqr_design,
 * every state measured (C = I), products summed left to right, every inverse the elimination with the 1e-14 relative pivot:
 *   discretise  ad = a dt; T_0 = S = I, T_k = (T_k-1 ad) / (k + 1), S += T_k for k = 1..17; Phi = I + ad S, Gamma = dt (S b).
 *               |a|_inf dt > 1.5 is BAD_INPUT: the first dropped term is then above 1e-14.
 *   solve       V = diag sigma^2, W = diag s^2 dt: P = Phi (P - P (P + V)^-1 P) Phi^T + W by the doubling loop of fdyn_lqr_design
 *               from A_0 = Phi^T, G_0 = V^-1, H_0 = W (same stopping rule, at most 30 steps); P = (H + H^T) / 2, L = P (P + V)^-1.
 * Outputs: F [FD_NKF][n] (FD_KF_*), residual [n] = max|Phi (P - L P) Phi^T + W - P| / max|P| of the worse block (NaN for a
 * BAD_INPUT lane), iters [n], status [n] int32 (FD_KF_* bits).  Status 0 is a certificate: P > 0 (L D L^T with every d > 0),
 * W > 0 and a residual <= 1e-8 make P a Lyapunov function of Phi (I - L), which is therefore Schur.  A lane
 * with status != 0 gets Phi = I, Gamma = 0, L = I: its estimate is the measurement.  Neither entry point synchronises or allocates. */
int fdyn_kf_design(const double* A, const double* B, double dt, const double* noise, int noise_per_lane, int64_t n, double* F,
                   double* residual, int32_t* iters, int32_t* status, void* stream);
/* fdyn_lqg_step_*: the output-feedback loop in one launch, the arguments of fdyn_lqr_step_* and the physics of it to the bit.
 * Each step s = 0, 1, ...:  d = the eight words of x - x0 as fdyn_lqr_step_* forms them;  y = d + sigma z_s;  per block in the
 * glue type (fp64 for _f64, fp32 for _mixed and _f32): pred = Phi xhat + Gamma du_prev, xhat = pred + L (y - pred), no angle wrap
 * of the innovation;  err_est += (xhat - d)^2, err_meas += (y - d)^2;  u = u0 - K f with f = xhat, y or d (feedback =
 * FD_LQG_*);  chatter += (clip(u) - (u0 + du_prev))^2, sat_steps counts the clipped steps, du_prev = clip(u) - u0;  set_controls
 * and one RK4 of dt.  F [FD_NKF][n], sigma [8] fp64; xhat [8][n] and du_prev [FD_NU][n] fp64, in and out.  z = NULL: the
 * normals are drawn in the kernel, Philox counter (row low, row high, *step + s + 1, FD_PHX_LQG + b), block b = 0 the
 * longitudinal four, b = 1 the lateral four, Box-Muller paired as the sensor layer pairs it (step = int32 in device memory,
 * NULL = 0; the caller advances it by n_steps after the launch).  z [n_steps][8][n] fp64: these normals instead.  The four
 * accumulators err_est [8][n], err_meas [8][n], chatter [FD_NU][n] (added to) and meas_out [8][n] (the last y, overwritten)
 * are fp64 and may each be NULL.  n_steps == 0 computes the controls from the stored xhat (from d when feedback is
 * FD_LQG_TRUTH) and changes nothing else.                                                                                      */
int fdyn_lqg_step_f64(double* x, const double* x0, const double* u0, const double* K, const uint8_t* type, const double* params,
                      int n_types, int64_t n, double dt, int n_steps, double* surf_out, int32_t* sat_steps, const double* F,
                      const double* sigma, double* xhat, double* du_prev, uint64_t seed, const int32_t* step, const double* z,
                      int feedback, double* err_est, double* err_meas, double* chatter, double* meas_out, void* stream);
int fdyn_lqg_step_mixed(double* x, const double* x0, const double* u0, const double* K, const uint8_t* type, const double* params,
                        int n_types, int64_t n, double dt, int n_steps, double* surf_out, int32_t* sat_steps, const double* F,
                        const double* sigma, double* xhat, double* du_prev, uint64_t seed, const int32_t* step, const double* z,
                        int feedback, double* err_est, double* err_meas, double* chatter, double* meas_out, void* stream);
int fdyn_lqg_step_f32(float* x, const double* x0, const double* u0, const double* K, const uint8_t* type, const double* params,
                      int n_types, int64_t n, double dt, int n_steps, float* surf_out, int32_t* sat_steps, const double* F,
                      const double* sigma, double* xhat, double* du_prev, uint64_t seed, const int32_t* step, const double* z,
                      int feedback, double* err_est, double* err_meas, double* chatter, double* meas_out, void* stream);


/* ---- loop margins (csrc/margin_kernels.hip) ---------------------------------------------------------------------------------
 * fdyn_loop_margins: how much robustness the loop has as fdyn_lqr_step_* / fdyn_lqg_step_* fly it -- sampled at dt, through the
 * estimator -- one lane per aircraft, fp64.  K [FD_NLQK][n] as fdyn_lqr_design writes it, F [FD_NKF][n] as fdyn_kf_design writes
 * it; feedback = FD_LQG_*; zre, zim [n_omega], 1 <= n_omega <= 256 (else FDYN_ERR_BAD_SIZE), shared by all lanes: the points
 * z = exp(j omega dt) of the unit circle, cos and sin taken by the caller (the kernel sees neither dt nor omega, and uses only
 * + - * / and sqrt).  Per block (Phi, Gamma, L of F; Kb = the block's 2 x 4 rows of K) and grid point:
 *   G = (z I - Phi)^-1 Gamma;  L_i = Kb G under measurement or truth feedback;  under estimate feedback
 *   L_i = z Kb (z I - F_c)^-1 L G with F_c = (I - L) (Phi - Gamma Kb), which is fdyn_lqg_step_*'s loop written out
 *   (xhat_k = (I - L) (Phi xhat_k-1 + Gamma du_k-1) + L y_k, du_k = -K xhat_k), opened at the plant input.
 *   Each solve is a complex 4 x 4 elimination with partial pivoting, pivot size |re| + |im|, a pivot below 1e-14 max|matrix| =
 *   singular.  M = I + L_i is 2 x 2: with F = |M|_F^2, D2 = |det M|^2, s_max^2 = (F + sqrt(max(F^2 - 4 D2, 0))) / 2,
 *   sigma_min(M) = sqrt(D2) / s_max;  1 / sigma_max(T) of T = L_i M^-1 = L_i adj(M) / det M = sqrt(D2) / s_max(L_i adj(M)).
 * Outputs, block-major [2][n]: alpha_s = min over the grid of sigma_min(I + L_i) and idx_s (int32) the first grid index attaining
 * it; alpha_t = min of 1 / sigma_max(T) (+inf where L_i = 0) and idx_t; curve [2][n_omega][n] or NULL: sigma_min(I + L_i) at
 * every point; status [n] int32 (FD_MRG_* bits).  Status 0 is a guarantee: the nominal loop is Schur (a power of its matrix has
 * |.|_inf < 1), and for every diagonal perturbation of the two control channels with gains in [1 / (1 + a), 1 / (1 - a)] or
 * phases up to 2 asin(a / 2), a <= alpha_s, I + L_i Delta stays nonsingular at the grid points, so no pole crosses the circle
 * there (between grid points: DESIGN.md 7h).  A lane with SINGULAR or BAD_INPUT gets NaN in every alpha and curve word and -1
 * in every index.  Neither synchronises nor allocates.                                                                        */
int fdyn_loop_margins(const double* K, const double* F, int feedback, const double* zre, const double* zim, int n_omega, int64_t n,
                      double* alpha_s, int32_t* idx_s, double* alpha_t, int32_t* idx_t, double* curve, int32_t* status, void* stream);


/* ---- sensor layer (csrc/sensor_kernels.hip) ---------------------------------------------------------------------------
 * NoisySensorInterface.update (interfaces/sensor.py:199-243) for n aircraft: meas [FD_NMS][n] = the 12 state words +
 * airspeed + altitude with Gaussian noise, body rates additionally offset by the gyro bias; bias [FD_NSB][n]
 * (gyro 3 | accel 3) random-walks in place (sensor.reset() = zero it).  x [FD_NX][n]; derived [FD_ND][n] (the backend's
 * airspeed / altitude rows) or NULL = computed from x; noise_cfg [FD_NSN] fp64 (FD_SN_*; FD_SN_ENABLED = 0 copies the
 * truth through).  z [FD_NSZ][n] = this update's standard normals in the reference's draw order (parity mode), or NULL =
 * in-kernel Philox keyed by (seed, aircraft, *step); step = uint32 in device memory (NULL = 0).                          */
int fdyn_sensor_update_f64(const double* x, const double* derived, double* bias, const double* noise_cfg, const double* z,
                           uint64_t seed, const uint32_t* step, double* meas, int64_t n, void* stream);
int fdyn_sensor_update_f32(const float* x, const float* derived, float* bias, const double* noise_cfg, const float* z,
                           uint64_t seed, const uint32_t* step, float* meas, int64_t n, void* stream);
/* The same model applied in place to rate-control observations obs [n][18] (rate_env.py:374-408): rates += noise + gyro
 * bias, rate errors recomputed from the measured rates, airspeed / altitude / attitude += noise; gyro_bias [3][n] fp32
 * walks in place and restarts from zero where reset_mask [n] (NULL = never) is set (first observation of an episode).  */
int fdyn_sensor_observe(float* obs, float* gyro_bias, const uint8_t* reset_mask, const double* noise_cfg, const float* z,
                        uint64_t seed, const uint32_t* step, int64_t n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FDYN_H */

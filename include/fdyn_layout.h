/* fdyn_layout.h -- flat-array layouts shared by the C-ABI (include/fdyn.h), the host mirror and the oracle.
 *
 * Everything that crosses the boundary is a plain array of scalars; these enums name the slots.
 * Reference sources the slots come from are cited per block (paths relative to the reference root).
 */
#ifndef FDYN_LAYOUT_H
#define FDYN_LAYOUT_H

/* ---- 12-word rigid-body state, simulation/simplified_6dof.py:172-173 ------------------------------- */
enum {
    FD_X_N = 0, FD_X_E, FD_X_D,        /* position NED (m)            */
    FD_X_U, FD_X_V, FD_X_W,            /* body velocity (m/s)         */
    FD_X_ROLL, FD_X_PITCH, FD_X_YAW,   /* Euler angles (rad)          */
    FD_X_P, FD_X_Q, FD_X_R,            /* body rates (rad/s)          */
    FD_NX = 12
};

/* ---- 4 control words, controllers/types.py:173-201 (ControlSurfaces.to_array order) ---------------- */
enum { FD_U_ELEVATOR = 0, FD_U_AILERON, FD_U_RUDDER, FD_U_THROTTLE, FD_NU = 4 };

/* ---- 4 derived words, simplified_6dof.py:295-331 (get_state) --------------------------------------- */
enum { FD_D_AIRSPEED = 0, FD_D_ALTITUDE, FD_D_GROUND_SPEED, FD_D_HEADING, FD_ND = 4 };

/* ---- aircraft parameter block (one per aircraft TYPE), simplified_6dof.py:31-117,181-187 ------------
 * The reference has no aero tables: this <=64-word block IS the "coefficient table"; the kernels stage
 * all n_types blocks in LDS and each lane picks its type's block.                                      */
enum {
    FD_P_MASS = 0, FD_P_IXX, FD_P_IYY, FD_P_IZZ,
    FD_P_WING_AREA, FD_P_WING_SPAN, FD_P_CHORD,
    FD_P_CL_0, FD_P_CL_ALPHA, FD_P_CD_0, FD_P_CD_ALPHA2,
    FD_P_CL_ELEVATOR, FD_P_CM_ELEVATOR, FD_P_CY_RUDDER, FD_P_CN_RUDDER, FD_P_CL_AILERON,
    FD_P_CM_ALPHA, FD_P_CN_BETA, FD_P_CL_BETA,
    FD_P_DAMPING_ROLL, FD_P_DAMPING_PITCH, FD_P_DAMPING_YAW,
    FD_P_MAX_THRUST, FD_P_AIR_DENSITY, FD_P_GRAVITY,
    FD_P_MIN_AIRSPEED_AERO, FD_P_MIN_U_VELOCITY,
    FD_P_MAX_ELEVATOR_RAD, FD_P_MAX_AILERON_RAD, FD_P_MAX_RUDDER_RAD,   /* np.radians(deg) done on host */
    FD_P_THRUST_ZERO_VELOCITY,
    FD_P_MAX_VELOCITY, FD_P_MAX_RATE_RAD, FD_P_MAX_PITCH_RAD, FD_P_MAX_ALPHA_RAD,
    FD_P_MAX_ACCELERATION, FD_P_MAX_ANGULAR_ACCELERATION,
    FD_P_MAX_TIMESTEP, FD_P_MIN_TIMESTEP,
    FD_NP_USED,
    FD_NP = 48,                        /* padded block stride (words) of the caller's array */
    /* derived words: exist only in the kernels' OWN staged (LDS) copy of a block, whose stride is FD_NP_STAGED; callers
     * never see them */
    FD_PD_INV_MASS = FD_NP_USED, FD_PD_INV_IXX, FD_PD_INV_IYY, FD_PD_INV_IZZ, FD_PD_SIN_MAX_ALPHA, FD_PD_COS_MAX_ALPHA,
    FD_PD_INV_THRUST_ZERO_V, FD_PD_TAN_ALPHA_FAST, FD_PD_ALPHA_NEEDS_ATAN2, FD_PD_SIN_MAX_PITCH, FD_PD_COS_MAX_PITCH,
    FD_NP_STAGED = 52
};

/* ---- scalar PID, cpp/include/pid_controller.h:22-49 and cpp/src/pid_controller.cpp:24-60 ----------- */
enum { FD_PC_KP = 0, FD_PC_KI, FD_PC_KD, FD_PC_OUT_MIN, FD_PC_OUT_MAX, FD_PC_INT_MIN, FD_PC_INT_MAX,
       FD_PC_ALPHA, FD_NPC = 8 };                      /* config: 8 x f32 */
enum { FD_PS_INTEGRAL = 0, FD_PS_ERR_PREV, FD_PS_DFILT, FD_NPS = 3 };   /* carried state: 3 x f32 */

/* the nine PIDs of the cascade, innermost first (rate_agent.py:41-50, attitude_agent.py:43-63,
 * hsa_agent.py:57-95)                                                                                  */
enum {
    FD_PID_RATE_ROLL = 0, FD_PID_RATE_PITCH, FD_PID_RATE_YAW,
    FD_PID_ATT_ROLL, FD_PID_ATT_PITCH, FD_PID_ATT_YAW,
    FD_PID_HEADING, FD_PID_ENERGY, FD_PID_BALANCE,
    FD_NPID = 9
};

/* ---- cascade glue constants (fp64 on the host; narrowed by the f32 kernels) -------------------------
 * rate_agent.py:52-55, attitude_agent.py:68-76, hsa_agent.py:101-109, waypoint_agent.py:50-65,
 * controllers/config_loader.py:40-85, controllers/mission_planner.py:173-184                           */
enum {
    FD_C_MAX_ROLL_RATE = 0, FD_C_MAX_PITCH_RATE, FD_C_MAX_YAW_RATE,   /* rad/s */
    FD_C_MAX_ROLL, FD_C_MAX_PITCH,                                    /* rad   */
    FD_C_MAX_BANK_RAD, FD_C_BASELINE_THROTTLE, FD_C_LOAD_FACTOR_GAIN, FD_C_MAX_PITCH_CMD_RAD,
    FD_C_GUIDANCE_TYPE,                                               /* 0 LOS, 1 PP, 2 default */
    FD_C_WP_MAX_BANK_RAD, FD_C_LOS_MAX_BANK_RAD, FD_C_LOS_LEAD_ANGLE_RAD,
    FD_C_LOOKAHEAD_TIME, FD_C_LOOKAHEAD_MIN, FD_C_LOOKAHEAD_MAX, FD_C_PROXIMITY_SCALE,
    FD_C_TURN_THRESHOLD_DIST, FD_C_TURN_THRESHOLD_ANGLE_RAD, FD_C_MAX_SPEED_REDUCTION, FD_C_MIN_SPEED,
    FD_C_ACCEPTANCE_RADIUS,
    FD_C_ON_COMPLETE,                                                 /* 0 freeze, 1 restart mission */
    /* fused rate-PID driver of the env kernels: throttle it holds (0.6 in pid_demonstrations.py:62 and
     * residual_rate_env.py:113, 0.5 in eval_rate.py:196) and the dt it hands the PIDs (0 = the env dt, as
     * pid_demonstrations.py:66; eval_rate.py:200 passes none => ControllerConfig.rate_loop_dt, types.py:342) */
    FD_C_PID_THROTTLE, FD_C_PID_DT,
    FD_NC = 28,
    /* derived, in the kernels' staged copy only: 1 / (g tan(bank limit)) of the two guidance laws (waypoint_agent.py:121,148) */
    FD_CD_WP_INV_G_TAN_BANK = FD_NC, FD_CD_LOS_INV_G_TAN_BANK,
    FD_NC_STAGED = 30
};
enum { FD_GUIDANCE_LOS = 0, FD_GUIDANCE_PP = 1, FD_GUIDANCE_DEFAULT = 2 };
/* control levels, numbered as the reference's ControlMode (controllers/types.py:13-24): the level a command enters at */
enum { FD_LEVEL_WAYPOINT = 1, FD_LEVEL_HSA = 2, FD_LEVEL_ATTITUDE = 3, FD_LEVEL_RATE = 4 };
enum { FD_WP_NORTH = 0, FD_WP_EAST, FD_WP_ALTITUDE, FD_WP_SPEED, FD_NWP = 4 };  /* waypoint row */
/* hybrid cascade (fdyn_hybrid_step_*): where a learned lane's throttle comes from -- the policy's fourth action word (what the
 * reference does with a LearnedRateAgent under an AttitudeAgent) or the outer loop's throttle (what a mission usually wants) */
enum { FD_HYBRID_THROTTLE_POLICY = 0, FD_HYBRID_THROTTLE_OUTER = 1 };
#define FD_MAX_WAYPOINTS 16

/* ---- rate-control env, learned_controllers/envs/rate_env.py ------------------------------------------ */
enum { FD_OBS_DIM = 18, FD_ACT_DIM = 4 };              /* rate_env.py:107-138, action = [ail, elev, rud, thr] */
enum { FD_CMD_STEP = 0, FD_CMD_RAMP = 1, FD_CMD_SINE = 2, FD_CMD_RANDOM_WALK = 3 };   /* rate_env.py:302-372 */

/* per-env carried words (one SoA row each, length N) */
enum {
    FD_E_CMD_P = 0, FD_E_CMD_Q, FD_E_CMD_R,            /* rate_command                         */
    FD_E_PREV_AIL, FD_E_PREV_ELEV, FD_E_PREV_RUD, FD_E_PREV_THR,   /* prev_action          */
    FD_E_PERR_P, FD_E_PERR_Q, FD_E_PERR_R,             /* RateTrackingReward.prev_errors       */
    FD_E_SIGN_P, FD_E_SIGN_Q, FD_E_SIGN_R,             /* RateTrackingReward.sign_changes      */
    FD_E_SETTLE_TIMER, FD_E_IS_SETTLED,                /* SettlingTimeBonus                    */
    FD_E_TIME,                                         /* current_time (+= dt each step)       */
    FD_E_SCHED0, FD_E_SCHED1, FD_E_SCHED2,             /* ramp end / sine amplitudes           */
    FD_E_SCHED3,                                       /* sine frequency                       */
    FD_E_EP_RETURN,                                    /* Monitor-style running episode return */
    FD_NE = 21
};
/* per-env integer words */
enum { FD_EI_STEP = 0, FD_EI_EPISODE, FD_NEI = 2 };

/* env constants (fp64) */
enum {
    FD_EC_DT = 0, FD_EC_DT_PHYSICS, FD_EC_MAX_STEPS, FD_EC_CMD_TYPE, FD_EC_DIFFICULTY_SCALE,
    FD_EC_MAX_RATE_P, FD_EC_MAX_RATE_Q, FD_EC_MAX_RATE_R,
    FD_NEC = 8
};

/* prepared launch image of the rate env (fdyn_rate_env_image, read by fdyn_rate_env_step_img_* / _dr_img_*), fp64 words: what
 * the step derives from env_consts and the parameter table alone, computed once instead of by every wave of every launch.
 *   [FD_IMG_EC ..]     the FD_NEC env constants, then the derived counts: RK4 sub-steps per env step (fdyn_num_substeps) and the
 *                      number of consecutive settled steps at which the settling bonus starts, then FD_ECD_SMALL_STEPS: 1.0 when,
 *                      for every type of the table, no Euler angle can move by more than 0.125 rad within one RK4 sub-step of
 *                      these env constants and the alpha limit lies inside the polynomial (fp32 evaluation only, else 0.0)
 *   [FD_IMG_PARAMS ..] FD_MAX_TYPES staged parameter blocks of FD_NP_STAGED words (FD_P_* then FD_PD_*)                     */
enum {
    FD_ECD_INTS = FD_NEC, FD_ECD_SMALL_STEPS = FD_NEC + 2,
    FD_IMG_EC = 0, FD_IMG_PARAMS = 16,
    FD_NIMG = FD_IMG_PARAMS + 8 * FD_NP_STAGED
};

/* one pre-sampled reset record (host NumPy pools in parity mode): 8 IC words + 7 command words        */
enum {
    FD_R_AIRSPEED = 0, FD_R_ALTITUDE, FD_R_ROLL, FD_R_PITCH, FD_R_YAW, FD_R_P, FD_R_Q, FD_R_R,
    FD_R_CMD0, FD_R_CMD1, FD_R_CMD2,                   /* step: command; ramp: end; sine: amplitudes */
    FD_R_CMD3,                                         /* sine: frequency                            */
    FD_NR = 12
};

/* one compacted episode-end record (written by the wave-ballot compaction)                            */
enum { FD_EV_ENV = 0, FD_EV_LENGTH, FD_EV_TERMINATED, FD_EV_NI = 3 };           /* int32 part      */
/* float part: [0] = episode return, [1..18] = terminal observation                                  */
#define FD_EV_NF (1 + FD_OBS_DIM)
/* The record list is kept in FD_EV_SHARDS segments, each with its own counter: workgroup b appends to shard b % FD_EV_SHARDS.
 * One counter for the whole fleet is ONE memory-side atomic word -- it saturates near 88 returning atomics per microsecond
 * on MI355X, and a step in which most waves hold a finished episode (random actions: ~1000 waves) spent 11 us of its 51 us
 * queueing on it (rocprofv3 SQ_WAIT_ANY, round 2).  Shard s owns records [s * cap_s, s * cap_s + count[s]) with
 * cap_s = ev_cap / FD_EV_SHARDS; size ev_cap with fdyn_event_capacity(n) to never lose a record.                  */
enum { FD_EV_SHARDS = 64 };

/* ---- domain randomisation of the rate env (fdyn_rate_env_{reset,step}_dr_*), design_docs/06_RL_AGENT_TRAINING.md ---------
 * per-env disturbance rows dr [FD_NDR][n] in the state dtype: steady wind and gust state in NED (m/s; the air-mass velocity is
 * their sum), the per-episode coefficients of the gust update g <- A g + B n (n ~ N(0, 1) per axis), and multipliers on the
 * type's mass, inertias and air density                                                                                      */
enum {
    FD_DR_WIND_N = 0, FD_DR_WIND_E, FD_DR_WIND_D,
    FD_DR_GUST_N, FD_DR_GUST_E, FD_DR_GUST_D,
    FD_DR_GUST_A, FD_DR_GUST_B,
    FD_DR_MASS_S, FD_DR_IXX_S, FD_DR_IYY_S, FD_DR_IZZ_S, FD_DR_RHO_S,
    FD_NDR = 13
};
/* ranges the resets draw the rows from (fp64, lo / hi pairs): wind speed (m/s) and direction (rad, the NED heading the air
 * moves toward), vertical wind (m/s, positive down), turbulence intensity (gust sigma as a fraction of the reset airspeed), gust
 * length scale L (m), the five multipliers; FD_DC_REDRAW = 1: every reset draws the rows, 0: resets keep what is there        */
enum {
    FD_DC_WIND_SPEED_LO = 0, FD_DC_WIND_SPEED_HI, FD_DC_WIND_DIR_LO, FD_DC_WIND_DIR_HI, FD_DC_WIND_VERT_LO, FD_DC_WIND_VERT_HI,
    FD_DC_TURB_LO, FD_DC_TURB_HI, FD_DC_GUST_L_LO, FD_DC_GUST_L_HI,
    FD_DC_MASS_LO, FD_DC_MASS_HI, FD_DC_IXX_LO, FD_DC_IXX_HI, FD_DC_IYY_LO, FD_DC_IYY_HI, FD_DC_IZZ_LO, FD_DC_IZZ_HI,
    FD_DC_RHO_LO, FD_DC_RHO_HI,
    FD_DC_REDRAW,
    FD_NDC = 21
};
/* Philox counter words: the fourth counter word names the consumer, the key is the 64-bit seed (DESIGN.md "Philox counter
 * layouts").  Env kernels, counter (env, episode, step, word): the IC and command record FD_PHX_RESET..+3, the random-walk command
 * increment FD_PHX_RANDOM_WALK, the randomisation rows FD_PHX_DR_RESET..+2, the initial gust FD_PHX_DR_GUST0, the gust update
 * FD_PHX_GUST.  Row kernels, counter (row low, row high, step, word): the policy's action noise FD_PHX_ACTION, the five blocks of
 * a sensor update FD_PHX_SENSOR..+4, the two blocks of an LQG step's measurement noise FD_PHX_LQG..+1.  The servo's own words
 * live in the headers of their entry points: FD_PHX_SERVO_GUST (fdyn_wind.h) and the three blocks FD_PHX_SERVO_LQG..+2
 * (fdyn_servo_lqg.h), of whose twelve normals fdyn_servo_lqg_step_* uses ten; words 10 and 11 are the north and east position
 * noise of fdyn_servo_lqg_mission_* (fdyn_servo_lqg_mission.h).                                                              */
enum {
    FD_PHX_RESET = 0, FD_PHX_RANDOM_WALK = 7, FD_PHX_DR_RESET = 16, FD_PHX_DR_GUST0 = 19, FD_PHX_GUST = 20,
    FD_PHX_ACTION = 0x51, FD_PHX_SENSOR = 0x60, FD_PHX_LQG = 0x70
};

/* ---- per-episode evaluation metrics, learned_controllers/eval/metrics.py:8-40 (field order of RateControlMetrics) */
enum {
    FD_M_SETTLE_ROLL = 0, FD_M_SETTLE_PITCH, FD_M_SETTLE_YAW,          /* s                           */
    FD_M_OVERSHOOT_ROLL, FD_M_OVERSHOOT_PITCH, FD_M_OVERSHOOT_YAW,     /* %                           */
    FD_M_SSERR_ROLL, FD_M_SSERR_PITCH, FD_M_SSERR_YAW,                 /* rad/s                       */
    FD_M_RISE_ROLL, FD_M_RISE_PITCH, FD_M_RISE_YAW,                    /* s                           */
    FD_M_SMOOTHNESS, FD_M_RMSE, FD_M_SUCCESS, FD_M_EPISODE_LENGTH, FD_M_TOTAL_REWARD,
    FD_NM = 17
};

/* ---- trajectory comparison (fdyn_traj_compare), validation/metrics/trajectory_metrics.py:71-174 --------------------- */
/* the 14 compared channels: the 12 state words with altitude and airspeed slotted in where the reference's columns have
 * them; attitude and body rates are compared in degrees (:136-137,150-151), yaw unwrapped (:140-142)                  */
enum {
    FD_TC_NORTH = 0, FD_TC_EAST, FD_TC_DOWN, FD_TC_ALTITUDE, FD_TC_U, FD_TC_V, FD_TC_W, FD_TC_AIRSPEED,
    FD_TC_ROLL, FD_TC_PITCH, FD_TC_YAW, FD_TC_P, FD_TC_Q, FD_TC_R,
    FD_NTC = 14
};
/* the metrics, in the insertion order of the dict compare_trajectories returns (:88-172)                               */
enum {
    FD_TM_POSITION_NORTH_RMSE = 0, FD_TM_POSITION_NORTH_CORRELATION, FD_TM_POSITION_NORTH_MAX_ERROR,
    FD_TM_POSITION_EAST_RMSE, FD_TM_POSITION_EAST_CORRELATION, FD_TM_POSITION_EAST_MAX_ERROR,
    FD_TM_POSITION_DOWN_RMSE, FD_TM_POSITION_DOWN_CORRELATION, FD_TM_POSITION_DOWN_MAX_ERROR,
    FD_TM_POSITION_3D_RMSE, FD_TM_POSITION_3D_MAX_ERROR,
    FD_TM_ALTITUDE_RMSE, FD_TM_ALTITUDE_CORRELATION,
    FD_TM_VELOCITY_U_RMSE, FD_TM_VELOCITY_V_RMSE, FD_TM_VELOCITY_W_RMSE, FD_TM_AIRSPEED_RMSE,
    FD_TM_ATTITUDE_ROLL_RMSE_DEG, FD_TM_ATTITUDE_ROLL_CORRELATION, FD_TM_ATTITUDE_ROLL_MAX_ERROR_DEG,
    FD_TM_ATTITUDE_PITCH_RMSE_DEG, FD_TM_ATTITUDE_PITCH_CORRELATION, FD_TM_ATTITUDE_PITCH_MAX_ERROR_DEG,
    FD_TM_ATTITUDE_YAW_RMSE_DEG, FD_TM_ATTITUDE_YAW_CORRELATION, FD_TM_ATTITUDE_YAW_MAX_ERROR_DEG,
    FD_TM_RATE_P_RMSE_DPS, FD_TM_RATE_P_CORRELATION, FD_TM_RATE_Q_RMSE_DPS, FD_TM_RATE_Q_CORRELATION,
    FD_TM_RATE_R_RMSE_DPS, FD_TM_RATE_R_CORRELATION,
    FD_TM_MEAN_POSITION_CORRELATION, FD_TM_MEAN_ATTITUDE_CORRELATION, FD_TM_OVERALL_CORRELATION,
    FD_NTM = 35
};
/* carried accumulator rows acc [FD_NTA][n], fp64; all zeros = a fresh comparison:
 *   COUNT              steps consumed so far (k)
 *   VARIED             bit 2j (side A) / 2j+1 (side B) set once a sample of correlated channel j differed from the first
 *                      one -- a side whose bit stays clear is constant, and its correlation is NaN
 *   YAW_PREV_*, _OFF_* np.unwrap(period=360) streamed: the previous RAW yaw sample (deg) and the running offset per side
 *   SSQ + c            sum of (a - b)^2 of channel c (FD_TC_*)
 *   POS3D_SSQ / _MAX   sum and maximum of the per-step 3-D position error
 *   MAX + m            running max |a - b| of north, east, down, roll, pitch, yaw (m = 0..5)
 *   CORR + 7 j + ...   correlated channel j (north, east, down, altitude, roll, pitch, yaw, p, q, r): the first sample of
 *                      each side (the pivots), then the co-moments about them: sum u, sum v, sum u^2, sum v^2, sum u v
 *                      with u = a - pivot_a, v = b - pivot_b                                                            */
enum {
    FD_TA_COUNT = 0, FD_TA_VARIED,
    FD_TA_YAW_PREV_A, FD_TA_YAW_PREV_B, FD_TA_YAW_OFF_A, FD_TA_YAW_OFF_B,
    FD_TA_SSQ = 6,
    FD_TA_POS3D_SSQ = FD_TA_SSQ + FD_NTC, FD_TA_POS3D_MAX,
    FD_TA_MAX = 22, FD_TA_NMAX = 6,
    FD_TA_CORR = FD_TA_MAX + FD_TA_NMAX, FD_TA_NCORR = 10,
    FD_TA_PIVOT_A = 0, FD_TA_PIVOT_B, FD_TA_SU, FD_TA_SV, FD_TA_SUU, FD_TA_SVV, FD_TA_SUV, FD_TA_CORR_WORDS = 7,
    FD_NTA = FD_TA_CORR + FD_TA_NCORR * FD_TA_CORR_WORDS
};

/* ---- steady-flight solver and linearisation (fdyn_trim / fdyn_linearize, csrc/trim_kernels.hip) ------------------------ */
/* flight condition per aircraft, spec [FD_NTS][n] fp64: airspeed (m/s), flight-path angle (rad, positive up), turn rate
 * (rad/s, positive to the right), altitude (m), heading (rad)                                                          */
enum { FD_TS_AIRSPEED = 0, FD_TS_CLIMB_ANGLE, FD_TS_TURN_RATE, FD_TS_ALTITUDE, FD_TS_HEADING, FD_NTS = 5 };
/* per-aircraft multipliers on the type's block, scales [FD_NSC][n] fp64 (the order of FD_DR_MASS_S .. FD_DR_RHO_S)       */
enum { FD_SC_MASS = 0, FD_SC_IXX, FD_SC_IYY, FD_SC_IZZ, FD_SC_RHO, FD_NSC = 5 };
/* status bits of a trim; 0 = a flyable equilibrium
 *   NOT_CONVERGED  the Newton iteration hit a singular Jacobian, a non-finite value or its iteration limit
 *   CONTROL_RANGE  a surface outside [-1, 1] or the throttle outside [0, 1]: the root needs more authority than there is
 *   ALPHA_LIMIT    |alpha| >= max_alpha: the aerodynamic alpha is clipped there, the root balances the forces with a frozen
 *                  lift coefficient and is not a flight condition
 *   PITCH_LIMIT    |theta| >= max_pitch (the Euler-rate clamp is active)
 *   BAD_SPEC       a spec word is not finite or the airspeed is not positive: nothing was solved                         */
enum {
    FD_TRIM_NOT_CONVERGED = 1, FD_TRIM_CONTROL_RANGE = 2, FD_TRIM_ALPHA_LIMIT = 4, FD_TRIM_PITCH_LIMIT = 8, FD_TRIM_BAD_SPEC = 16
};
/* the longitudinal (u, w, q, theta | elevator, throttle) and lateral (v, p, r, phi | aileron, rudder) sub-systems are read
 * out of A [FD_NX * FD_NX][n] and B [FD_NX * FD_NU][n] on the host (hcrl_amd.trim)                                       */

/* ---- gain-scheduled LQR (fdyn_lqr_design / fdyn_lqr_step_*, csrc/lqr_kernels.hip) ------------------------------------- */
/* weights [FD_NLQW] fp64, all diagonal penalties: q of (u, w, q, theta), q of (v, p, r, phi), r of (elevator, throttle),
 * r of (aileron, rudder)                                                                                                */
enum { FD_LQW_Q_LON = 0, FD_LQW_Q_LAT = 4, FD_LQW_R_LON = 8, FD_LQW_R_LAT = 10, FD_NLQW = 12 };
/* gains K [FD_NLQK][n] fp64: K_lon 2 x 4 row-major (rows elevator, throttle; columns u, w, q, theta), then K_lat 2 x 4
 * (rows aileron, rudder; columns v, p, r, phi)                                                                          */
enum { FD_LQK_LON = 0, FD_LQK_LAT = 8, FD_NLQK = 16 };
/* status bits of a design; 0 = a CERTIFIED stabilising gain
 *   NOT_CONVERGED   the doubling iteration hit its cap, a singular pivot or a non-finite value
 *   NO_CERTIFICATE  X is not positive definite or the Riccati residual exceeds 1e-8
 *   BAD_INPUT       a word of the two blocks of A, B is not finite, or a weight is not finite and > 0: nothing was solved   */
enum { FD_LQR_NOT_CONVERGED = 1, FD_LQR_NO_CERTIFICATE = 2, FD_LQR_BAD_INPUT = 4 };

/* ---- steady-state Kalman filter and the LQG loop (fdyn_kf_design / fdyn_lqg_step_*, csrc/kf_kernels.hip) -------------- */
/* noise [FD_NKFN] fp64: the measurement standard deviations sigma of (u, w, q, theta | v, p, r, phi), then the process-noise
 * rates s of the same eight words, in state units per sqrt(s)                                                           */
enum { FD_KFN_SIGMA = 0, FD_KFN_RATE = 8, FD_NKFN = 16 };
/* filter F [FD_NKF][n] fp64, every matrix row-major: the discretised blocks Phi 4 x 4 and Gamma 4 x 2 (columns elevator,
 * throttle | aileron, rudder) and the steady-state gains L 4 x 4                                                         */
enum { FD_KF_PHI_LON = 0, FD_KF_PHI_LAT = 16, FD_KF_GAMMA_LON = 32, FD_KF_GAMMA_LAT = 40, FD_KF_L_LON = 48, FD_KF_L_LAT = 64, FD_NKF = 80 };
/* status bits of a filter design; 0 = a CERTIFIED stable filter
 *   NOT_CONVERGED   the doubling iteration hit its cap, a singular pivot or a non-finite value
 *   NO_CERTIFICATE  P is not positive definite, P + V is singular or the residual of the filter equation exceeds 1e-8
 *   BAD_INPUT       a word of the two blocks of A, B is not finite, a sigma or a rate is not finite and > 0, dt is outside
 *                   (1e-6, 1] or |a|_inf dt > 1.5 (the series of the discretisation is cut where that bound holds)         */
enum { FD_KF_NOT_CONVERGED = 1, FD_KF_NO_CERTIFICATE = 2, FD_KF_BAD_INPUT = 4 };
/* what the LQG loop feeds back: the filter's estimate, the raw measurement, or the true state (= fdyn_lqr_step_*)         */
enum { FD_LQG_ESTIMATE = 0, FD_LQG_MEASUREMENT = 1, FD_LQG_TRUTH = 2 };

/* ---- loop margins (fdyn_loop_margins, csrc/margin_kernels.hip) -------------------------------------------------------- */
/* status bits of a margin report; 0 = the disk guarantee holds (include/fdyn.h)
 *   NOT_STABLE  the nominal closed loop has no certificate: no power M^(2^k), k <= 30, of Phi - Gamma Kb (under estimate
 *               feedback: nor of (I - L) Phi) has |.|_inf < 1, or a word of it stopped being finite.  alpha is still written
 *   SINGULAR    a solve met a pivot below 1e-14 max|matrix| or a grid point gave a non-finite value (a pole on the circle):
 *               every alpha and curve word of the lane is NaN, every index -1
 *   BAD_INPUT   a word of K or F that is read is not finite: nothing was computed, the outputs as for SINGULAR               */
enum { FD_MRG_NOT_STABLE = 1, FD_MRG_SINGULAR = 2, FD_MRG_BAD_INPUT = 4 };

/* ---- flight modes (fdyn_flight_modes / fdyn_block_modes, csrc/modes_kernels.hip, include/fdyn_modes.h) ---------------- */
/* summary [2][FD_NMO][n] fp64, per block over its four eigenvalues: max Re, max |.| (the spectral radius), min |.|, the
 * smallest damping ratio -Re / |.| (0 for an eigenvalue at 0; 1 = real and stable, -1 = real and unstable), the number with
 * Re > 0 and the number with Im != 0 (both as fp64)                                                                    */
enum { FD_MO_ABSCISSA = 0, FD_MO_RADIUS, FD_MO_MIN_ABS, FD_MO_MIN_ZETA, FD_MO_N_UNSTABLE, FD_MO_N_COMPLEX, FD_NMO = 6 };
/* status of a modes report (values, not bits); 0 = every eigenvalue of both blocks converged
 *   NOT_CONVERGED  a deflation hit its cap of 30 QR sweeps or a word stopped being finite
 *   BAD_INPUT      a word of a block that is read (A, and B and K where K is given; M) is not finite: nothing was solved
 * either way every eigenvalue and summary word of BOTH blocks of the lane is NaN                                          */
enum { FD_MO_NOT_CONVERGED = 1, FD_MO_BAD_INPUT = 2 };

/* ---- LQ servo (fdyn_servo_design / fdyn_servo_step_*, csrc/servo_kernels.hip, include/fdyn_servo.h) ------------------ */
/* the two augmented blocks: longitudinal (u, w, q, theta, z, i_V, i_h | elevator, throttle), 7 states, z the down-position word
 * and i_V, i_h the integrals of the airspeed and the altitude error; lateral (v, p, r, phi, psi, i_psi | aileron, rudder), 6 */
enum { FD_SV_NLON = 7, FD_SV_NLAT = 6 };
/* weights [FD_NSVW] fp64, all diagonal penalties: q of the seven longitudinal states, q of the six lateral states, r of
 * (elevator, throttle), r of (aileron, rudder)                                                                            */
enum { FD_SVW_Q_LON = 0, FD_SVW_Q_LAT = 7, FD_SVW_R_LON = 13, FD_SVW_R_LAT = 15, FD_NSVW = 17 };
/* gains K [FD_NSVK][n] fp64: K_lon 2 x 7 row-major (rows elevator, throttle), then K_lat 2 x 6 (rows aileron, rudder)      */
enum { FD_SVK_LON = 0, FD_SVK_LAT = 14, FD_NSVK = 26 };
/* reference ref [FD_NSVR][n] fp64: commanded airspeed (m/s), altitude (m) and heading (rad), and the rates the altitude and
 * heading commands move at by themselves (m/s, rad/s: the climb rate and the turn rate of the trim)                        */
enum { FD_SVR_SPEED = 0, FD_SVR_ALTITUDE, FD_SVR_HEADING, FD_SVR_CLIMB_RATE, FD_SVR_TURN_RATE, FD_NSVR = 5 };
/* integrators integ [FD_NSVI][n] fp64, error clips limits [FD_NSVI] fp64 and errors err_out [FD_NSVI][n]: airspeed, altitude,
 * heading                                                                                                                 */
enum { FD_SVI_SPEED = 0, FD_SVI_ALTITUDE, FD_SVI_HEADING, FD_NSVI = 3 };
/* status bits of a servo design, with the meaning of FD_LQR_*; 0 = a CERTIFIED stabilising gain
 *   NOT_CONVERGED   the doubling iteration hit its cap, a singular pivot or a non-finite value
 *   NO_CERTIFICATE  X is not positive definite or the Riccati residual exceeds 1e-8
 *   BAD_INPUT       a word of A, B or x0 that is read is not finite, a weight is not finite and > 0, or the trim's
 *                   sqrt(u0^2 + w0^2) is not > 0: nothing was solved                                                       */
enum { FD_SV_NOT_CONVERGED = 1, FD_SV_NO_CERTIFICATE = 2, FD_SV_BAD_INPUT = 4 };
/* mission statistics stats [FD_NMST][n] fp64 of fdyn_servo_mission_* (include/fdyn_mission.h), running extrema carried across
 * launches: the largest |altitude - the active waypoint's altitude| (m), the largest |roll| (rad), the smallest airspeed (m/s),
 * the largest horizontal distance from the leg that ends at the active waypoint (m).  The host starts them at 0, 0, +inf, 0.
 * (FD_MST_*, not FD_MS_*: that prefix and FD_NMS belong to the sensor's measurement block below.)                          */
enum { FD_MST_ALTITUDE_ERROR = 0, FD_MST_ROLL, FD_MST_MIN_AIRSPEED, FD_MST_CROSS_TRACK, FD_NMST = 4 };
/* gain schedule sched [n_nodes][FD_NSS][n] fp64 of fdyn_servo_sched_* (include/fdyn_servo_sched.h), per node: its airspeed
 * (m/s), the eight regulated trim words in the order the step kernel keeps them (u, w, q, theta, v, p, r, phi), the trim
 * controls (FD_U_* order) and the gains as fdyn_servo_design writes them (FD_SVK_*).  1 <= n_nodes <= FD_MAX_SCHED_NODES.
 * (FD_SS_*, FD_NSS, not FD_SC_*, FD_NSC: those belong to the per-aircraft scales above.)                                   */
enum { FD_SS_V = 0, FD_SS_X0 = 1, FD_SS_U0 = 9, FD_SS_K = 13, FD_NSS = 39 };
enum { FD_MAX_SCHED_NODES = 8 };
/* sched_on: what the table is entered with, the airspeed as step 1 of the law forms it or the commanded airspeed          */
enum { FD_SCHED_ON_AIRSPEED = 0, FD_SCHED_ON_COMMAND = 1 };

/* ---- stand-alone reward evaluation (fdyn_rate_reward_seq_*), learned_controllers/envs/rewards.py ------------------- */
/* parameters (fp64): RateTrackingReward weights :14-19, then SettlingTimeBonus :160-162                              */
enum {
    FD_RW_TRACKING = 0, FD_RW_SMOOTHNESS, FD_RW_STABILITY, FD_RW_OSCILLATION, FD_RW_SURVIVAL,
    FD_RW_SETTLE_THRESHOLD, FD_RW_MIN_SETTLE_TIME, FD_RW_BONUS_MULTIPLIER,
    FD_NRW = 8
};
/* carried state per sequence: RateTrackingReward.prev_errors / sign_changes (:37-38), SettlingTimeBonus timer / flag */
enum {
    FD_RS_PERR_P = 0, FD_RS_PERR_Q, FD_RS_PERR_R, FD_RS_SIGN_P, FD_RS_SIGN_Q, FD_RS_SIGN_R, FD_RS_SETTLE_TIMER, FD_RS_IS_SETTLED,
    FD_NRS = 8
};
/* reward components in the order of the reference's dict (:125-131); flight rows of the input                        */
enum { FD_RC_TRACKING = 0, FD_RC_SMOOTHNESS, FD_RC_STABILITY, FD_RC_OSCILLATION, FD_RC_SURVIVAL, FD_NRC = 5 };
enum { FD_RF_AIRSPEED = 0, FD_RF_ALTITUDE, FD_RF_ROLL, FD_RF_PITCH, FD_NRF = 4 };

/* ---- sensor layer, interfaces/sensor.py:137-243 (NoisySensorInterface) ------------------------------------------- */
/* noise configuration (fp64): standard deviations in the order the reference draws (:208-235), then the two bias
 * random-walk steps it hard-codes (:233-234) and the enabled flag (:203-205)                                        */
enum {
    FD_SN_GPS_POS = 0, FD_SN_GPS_VEL, FD_SN_ATTITUDE, FD_SN_GYRO, FD_SN_AIRSPEED, FD_SN_ALTITUDE,
    FD_SN_GYRO_BIAS_WALK, FD_SN_ACCEL_BIAS_WALK, FD_SN_ENABLED,
    FD_NSN = 12
};
/* one update consumes 20 standard normals, in the reference's call order                                           */
enum {
    FD_SZ_POS = 0, FD_SZ_VEL = 3, FD_SZ_ATT = 6, FD_SZ_GYRO = 9, FD_SZ_AIRSPEED = 12, FD_SZ_ALTITUDE = 13,
    FD_SZ_GYRO_BIAS = 14, FD_SZ_ACCEL_BIAS = 17, FD_NSZ = 20
};
/* measurement block: the 12 state words (FD_X_* order) + airspeed + altitude ; bias block: gyro(3) + accel(3)       */
enum { FD_MS_AIRSPEED = 12, FD_MS_ALTITUDE = 13, FD_NMS = 14, FD_NSB = 6 };

#endif /* FDYN_LAYOUT_H */

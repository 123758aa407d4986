"""Device-resident fleets: batched `Simplified6DOF` and the batched 5-level cascade.

`BatchedSixDOF` is the N-aircraft counterpart of the reference's `Simplified6DOF` + `SimulationAircraftBackend`
(simulation/simplified_6dof.py:148-331, simulation/simulation_backend.py:13-135): same reset / set_controls / step
semantics, state held structure-of-arrays in HBM as `x[12][N]`, every step one launch of the HIP kernel.
`BatchedCascade` adds the mission planner + Waypoint/HSA/Attitude/Rate agents of controllers/*.py fused in front of
the integrator (examples/03_waypoint_square_demo.py:148-209 per aircraft).
"""
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib, layout as L
from .config import (FlightControlConfig, cascade_consts, pid_table, waypoint_table)
from .flight_types import ControllerConfig, Waypoint
from .params import AircraftParams, param_table


class BatchedSixDOF:
    _trim = None                 # (TrimResult, scales) of the last .trim(): the point design_lqr designs at
    _lqr = _kalman = lqr_saturated_steps = None     # the last design_lqr() / design_kalman(); [N] int32 once an LQR / LQG step ran
    _servo = servo = None        # the last design_servo() and the ServoState it started
    servo_mission = None         # the last start_servo_mission()
    _servo_kalman = servo_lqg = None    # the last design_servo_kalman() and the ServoLqgState it started
    servo_position = servo_position_state = None    # the last start_servo_lqg_mission(): ServoPositionFilter, ServoLqgMissionState
    _servo_kalman_schedule = servo_sched_lqg = None # the last design_servo_kalman_schedule() and the ServoSchedLqgState it started

    def __init__(self, n: int, precision: str = "f64", types: Sequence = ("rc_plane",),
                 type_index: Optional[np.ndarray] = None, device=None):
        self.lib = _lib.load()
        self.device = device or _lib.require_gpu()
        self.n, self.precision = int(n), precision
        self.dtype = _lib.state_dtype(precision)
        self.params_host = param_table(types)
        self.n_types = len(self.params_host)
        self.params = torch.as_tensor(self.params_host, device=self.device).contiguous()
        self.type_index = None
        if type_index is not None:
            self.type_index = torch.as_tensor(np.asarray(type_index, np.uint8), device=self.device).contiguous()
        self.x = torch.zeros((L.FD_NX, self.n), dtype=self.dtype, device=self.device)
        self.u = torch.zeros((L.FD_NU, self.n), dtype=self.dtype, device=self.device)
        self.time = 0.0
        self._step_fn = getattr(self.lib, f"fdyn_sixdof_step_{precision}")
        self._derived_fn = getattr(self.lib, "fdyn_derived_f32" if precision == "f32" else "fdyn_derived_f64")
        self.reset()

    # Simplified6DOF.reset (simplified_6dof.py:189-212): default = level flight, 100 m, 20 m/s
    def reset(self, x0: Optional[np.ndarray] = None):
        if x0 is None:
            x0 = np.zeros((self.n, L.FD_NX))
            x0[:, L.FD_X_D] = -100.0
            x0[:, L.FD_X_U] = 20.0
        x0 = np.asarray(x0, dtype=np.float64).reshape(self.n, L.FD_NX)
        self.x.copy_(torch.as_tensor(np.ascontiguousarray(x0.T), device=self.device).to(self.dtype))
        self.time = 0.0

    # Simplified6DOF.set_controls (:214-226); rows = [elevator, aileron, rudder, throttle]; clip happens in-kernel
    def set_controls(self, u):
        if isinstance(u, torch.Tensor):
            self.u.copy_(u.to(self.dtype).reshape(L.FD_NU, self.n))
        else:
            u = np.asarray(u, dtype=np.float64).reshape(self.n, L.FD_NU)
            self.u.copy_(torch.as_tensor(np.ascontiguousarray(u.T), device=self.device).to(self.dtype))

    # SimulationAircraftBackend.step (simulation_backend.py:82-101) when dt_physics is given, else Simplified6DOF.step
    def step(self, dt: float, dt_physics: Optional[float] = None, derived_out: Optional[torch.Tensor] = None):
        n_sub = self.lib.fdyn_num_substeps(dt, dt_physics) if dt_physics else 1
        rc = self._step_fn(_lib.ptr(self.x), _lib.ptr(self.u), _lib.ptr(self.type_index), _lib.ptr(self.params),
                           self.n_types, self.n, float(dt), n_sub, _lib.ptr(derived_out), _lib.current_stream())
        _lib.check(rc, "Simplified6DOF.step")
        self.time += dt
        return n_sub

    def derived(self) -> torch.Tensor:
        """[4][N]: airspeed, altitude, ground_speed, heading (simplified_6dof.py:295-331)."""
        out = torch.empty((L.FD_ND, self.n), dtype=self.dtype, device=self.device)
        _lib.check(self._derived_fn(_lib.ptr(self.x), self.n, _lib.ptr(out), _lib.current_stream()), "get_state")
        return out

    def state_numpy(self) -> np.ndarray:
        """[N][12] float64 host copy."""
        return self.x.to(torch.float64).T.contiguous().cpu().numpy()

    # Steady flight (docs/6dof_mathematical_formulation.tex:1380-1410; the reference codes no solver): hcrl_amd.trim
    def trim(self, airspeed, climb_angle=0.0, turn_rate=0.0, altitude=100.0, heading=0.0, scales=None, strict: bool = True):
        """Solve every aircraft's equilibrium at the flight condition (scalars or length-N arrays) in fp64 for its own
        airframe (and `scales`: per-aircraft multipliers on mass, Ixx, Iyy, Izz, air density), then start the fleet there:
        `x` and `u` are overwritten in the fleet's storage type and the clock restarts.  Returns the TrimResult.  strict: raise
        ValueError, BEFORE anything of the fleet is touched, when an aircraft has no flyable equilibrium there."""
        from . import trim as T
        spec = torch.as_tensor(T.flight_condition(self.n, airspeed, climb_angle, turn_rate, altitude, heading), device=self.device)
        scale_rows = T.scale_rows(self.n, scales, self.device)
        res = T.trim_into(spec, self.params, self.type_index, scale_rows)
        if strict:
            T.require_ok(res, f"{type(self).__name__}.trim")
        self.x.copy_(res.x0)
        self.u.copy_(res.u0)
        self.time = 0.0
        self._trim = (res, scale_rows)
        return res

    def linearize(self, scales=None):
        """(A [12][12][N], B [12][4][N]) float64: d xdot / d x and d xdot / d u of every aircraft at its current `x` and `u`
        (any state, not only a trim), controls unclipped."""
        from . import trim as T
        return T.linearize_into(self.x, self.u, self.params, self.type_index, T.scale_rows(self.n, scales, self.device))

    # Gain-scheduled LQR (hcrl_amd.lqr): the design step between trim / linearize and flight
    def design_lqr(self, weights=None, scales=None, strict: bool = True):
        """An LQR gain for every aircraft at the fleet's current trim (the last `.trim(...)`), each designed on its own
        linear model: LqrDesign with K [16][N], status 0 = a certified stabilising gain.  weights: None (LqrWeights()), an
        LqrWeights, or penalties [12] / [12][N]; scales: None = the multipliers the trim was solved with.  strict: raise
        ValueError when an aircraft has no certified gain.  The fleet's state is not touched."""
        from . import lqr as Q
        res, trim_scales = self._need_trim("design_lqr")
        out = Q.design_lqr(res, self.params, self.type_index, trim_scales if scales is None else scales, weights)
        if strict:
            Q.require_ok(out, f"{type(self).__name__}.design_lqr")
        self._lqr = out                                  # the gains step_lqg feeds the estimate to
        return out

    def step_lqr(self, design, n_steps: int = 1, dt: Optional[float] = None):
        """n_steps x {u = u0 - K (x - x0), clipped as set_controls clips -> one RK4 of dt} in ONE launch (dt None: the fleet's
        own `dt` where it has one, else 0.01 s).  `u` receives the last applied controls; `lqr_saturated_steps` [N] int32
        counts, per aircraft, the steps in which a control was clipped.  The fleet integrates its airframes' own parameter
        blocks: a design made with `scales` belongs to an aircraft this fleet does not fly."""
        from . import lqr as Q
        if dt is None:
            dt = getattr(self, "dt", 0.01)
        Q.step_into(self.precision, self.x, design, self.params, self.type_index, dt, n_steps, self.u, self._saturated_steps())
        self.time += dt * n_steps

    # LQ servo (hcrl_amd.servo): LQR with integral action, flown to heading, speed and altitude commands
    def design_servo(self, weights=None, scales=None, strict: bool = True, dt: Optional[float] = None):
        """An LQ-servo gain for every aircraft at the fleet's current trim (the last `.trim(...)`): ServoDesign with K [26][N],
        status 0 = a certified stabilising gain.  weights: None (ServoWeights()), a ServoWeights, or penalties [17] / [17][N];
        scales: None = the multipliers the trim was solved with.  strict: raise ValueError when an aircraft has no certified
        gain.  Also starts the loop's state (`servo`: references at the trim's own airspeed, altitude and heading, moving at its
        climb rate and turn rate; integrators zero).  The fleet's state is not touched.
        dt: None = the continuous design, flown at any step; a control step = the sampled-data design for the loop as step_servo
        flies it at that step (hold and Euler integrators in the model).  It is then flown and analysed at that step only: another
        is a ValueError."""
        from . import servo as SV
        res, trim_scales = self._need_trim("design_servo")
        out = SV.design_servo(res, self.params, self.type_index, trim_scales if scales is None else scales, weights, dt)
        if strict:
            SV.require_ok(out, f"{type(self).__name__}.design_servo")
        self._servo = out
        self.servo = SV.ServoState.at_trim(res.x0)
        return out

    def command_servo(self, heading=None, speed=None, altitude=None):
        """New references for step_servo, each a scalar or N values (None: unchanged): heading (rad), speed (m/s), altitude (m).
        A heading or an altitude command stops that reference's own motion (the trim's turn or climb)."""
        self._need_servo("command_servo")
        self.servo.command(heading, speed, altitude)

    def design_servo_schedule(self, airspeeds, climb=0.0, turn=0.0, altitude=None, heading=None, weights=None, scales=None,
                              strict: bool = True, dt: Optional[float] = None):
        """A table of LQ-servo designs over airspeed for every aircraft (hcrl_amd.servo_sched): ServoSchedule with table
        [M][FD_NSS][N], for `step_servo(schedule=...)` and `fly_servo_mission(schedule=...)`.  airspeeds: M <= FD_MAX_SCHED_NODES
        strictly increasing values, or [M][N]; climb (rad), turn (rad/s), altitude and heading: the other words of the nodes' flight
        condition (altitude, heading None: those of the fleet's current trim, else 100 m and 0); weights and scales as design_servo
        takes them (scales None: the multipliers of the current trim, if any).  One trim, one linearise and one design launch over
        M N lanes.  ValueError for airspeeds that are not strictly increasing or for too many nodes; strict: also when a node has no
        trim or no certified gain.  The fleet's state, trim and design are not touched.  dt: as design_servo takes it; every node
        is then the sampled-data design for that control step, and the schedule is flown at that step only."""
        from . import servo_sched as SS
        trim_scales = None
        if self._trim is not None:
            res, trim_scales = self._trim
            altitude = -res.x0[L.FD_X_D] if altitude is None else altitude
            heading = res.x0[L.FD_X_YAW] if heading is None else heading
        out = SS.design_servo_schedule(airspeeds, self.n, self.params, self.type_index, climb, turn, 100.0 if altitude is None else altitude,
                                       0.0 if heading is None else heading, weights, trim_scales if scales is None else scales, strict=False,
                                       dt=dt)
        if strict:
            out.require_ok(f"{type(self).__name__}.design_servo_schedule")
        return out

    def step_servo(self, n_steps: int = 1, dt: Optional[float] = None, wind=None, schedule=None, on: str = "airspeed"):
        """n_steps x {errors against the references -> u = u0 - K d, clipped as set_controls clips -> integrators (held per block
        while one of its controls is clipped) -> one RK4 of dt -> the references move at their own rates} in ONE launch (dt None:
        the fleet's own `dt` where it has one, else 0.01 s).  Needs design_servo() first.  `u` receives the last applied
        controls, `lqr_saturated_steps` [N] int32 counts the steps in which a control was clipped, `servo.err` holds the last
        errors.  The fleet integrates its airframes' own parameter blocks; where they differ from the designed ones the
        integrators take up the difference.  wind: a servo.ServoWind, the air each aircraft flies in (None: still air).
        schedule: a ServoSchedule (design_servo_schedule): the trim point and the gains of each control step are interpolated from
        it at the measured airspeed (on="airspeed") or the commanded one (on="command"), and the design is not read: only the
        loop's state (`servo`), which design_servo() starts, is needed.  Not together with wind (NotImplementedError)."""
        from . import servo as SV
        if dt is None:
            dt = getattr(self, "dt", 0.01)
        if schedule is not None:
            self._need_servo_state("step_servo")
            SV.step_into(self.precision, self.x, self._servo, self.servo, self.params, self.type_index, dt, n_steps, self.u,
                         self._saturated_steps(), self.servo.err, wind=wind, schedule=schedule, on=on)
            self.time += dt * n_steps
            return
        design = self._need_servo("step_servo")
        if wind is not None:
            SV.step_into(self.precision, self.x, design, self.servo, self.params, self.type_index, dt, n_steps, self.u,
                         self._saturated_steps(), self.servo.err, wind=wind)
            self.time += dt * n_steps
            return
        SV.step_into(self.precision, self.x, design, self.servo, self.params, self.type_index, dt, n_steps, self.u,
                     self._saturated_steps(), self.servo.err)
        self.time += dt * n_steps

    # waypoint missions on the servo (include/fdyn_mission.h): the cascade's mission update and guidance in front of the servo law
    def start_servo_mission(self, waypoints, guidance_type: str = "PP", acceptance_radius: Optional[float] = None,
                            on_complete: str = "freeze", flight_config=None):
        """A waypoint mission for fly_servo_mission, the same one for every aircraft: ServoMission (also kept as `servo_mission`)
        with every aircraft at the first waypoint.  The arguments as BatchedCascade takes them.  Needs design_servo() first."""
        from . import servo as SV
        self._need_servo("start_servo_mission")
        self.servo_mission = SV.ServoMission.start(waypoints, self.n, self.device, guidance_type, acceptance_radius, on_complete, flight_config)
        return self.servo_mission

    def fly_servo_mission(self, n_steps: int = 1, dt: Optional[float] = None, wind=None, schedule=None, on: str = "airspeed"):
        """n_steps x {mission update -> guidance -> references -> the control step of step_servo} in ONE launch.  An aircraft whose
        mission is complete stops where it is.  `u`, `lqr_saturated_steps` and `servo.err` as step_servo leaves them; `time`
        advances by n_steps x dt (an aircraft's own flown time: servo_mission.mission_time(dt)).  wind: as step_servo takes it; the
        guidance then reads the air-relative speed, course and position stay ground quantities (no wind-correction angle).
        schedule, on: as step_servo takes them; on="command" enters the table with the speed command the guidance has just written."""
        from . import servo as SV
        if schedule is not None:
            self._need_servo_state("fly_servo_mission")
        design = self._servo if schedule is not None else self._need_servo("fly_servo_mission")
        if self.servo_mission is None:
            raise ValueError(f"{type(self).__name__}.fly_servo_mission: the fleet has no mission; call .start_servo_mission() first")
        if dt is None:
            dt = getattr(self, "dt", 0.01)
        if schedule is not None:
            SV.mission_into(self.precision, self.x, design, self.servo, self.servo_mission, self.params, self.type_index, dt, n_steps, self.u,
                            self._saturated_steps(), self.servo.err, wind=wind, schedule=schedule, on=on)
            self.time += dt * n_steps
            return
        if wind is not None:
            SV.mission_into(self.precision, self.x, design, self.servo, self.servo_mission, self.params, self.type_index, dt, n_steps, self.u,
                            self._saturated_steps(), self.servo.err, wind=wind)
            self.time += dt * n_steps
            return
        SV.mission_into(self.precision, self.x, design, self.servo, self.servo_mission, self.params, self.type_index, dt, n_steps, self.u,
                        self._saturated_steps(), self.servo.err)
        self.time += dt * n_steps

    def servo_mission_complete(self) -> torch.Tensor:
        """[N] bool on the device: the aircraft that have completed the mission."""
        self._need_servo("servo_mission_complete")
        if self.servo_mission is None:
            raise ValueError(f"{type(self).__name__}.servo_mission_complete: the fleet has no mission; call .start_servo_mission() first")
        return self.servo_mission.complete()

    def _need_servo_state(self, what: str):
        """Under a schedule the single design is never read; what the flight needs is the loop's state (`servo`: references, integrators
        and error clips), which design_servo() starts at the trim."""
        if self.servo is None:
            raise ValueError(f"{type(self).__name__}.{what}: the fleet has no servo state (references and integrators); "
                             "call .design_servo() first, which starts it at the trim")

    def _need_servo(self, what: str):
        if self._servo is None:
            raise ValueError(f"{type(self).__name__}.{what}: the fleet has no servo design; call .design_servo() first")
        return self._servo

    # the servo on noisy sensors (hcrl_amd.servo_lqg): the Kalman filter of the servo's ten physical words, and the servo flown on it
    def design_servo_kalman(self, dt: float, noise=None, scales=None, strict: bool = True):
        """A steady-state Kalman filter on (u, w, q, theta, z | v, p, r, phi, psi) for every aircraft at the fleet's current trim,
        discretised at `dt`: ServoKalmanDesign with F [120][N], status 0 = a certified stable filter.  noise: None (the sensor
        layer's default noise and the servo's default process-noise rates), a ServoKalmanNoise, or [20] / [20][N]; scales as
        design_servo.  strict: raise ValueError when an aircraft has no certified filter.  Also starts the estimator's state
        (`servo_lqg`: estimate at the trim, step word 0)."""
        from . import servo_lqg as SL
        res, trim_scales = self._need_trim("design_servo_kalman")
        out = SL.design_servo_kalman(res, self.params, self.type_index, trim_scales if scales is None else scales, dt, noise)
        if strict:
            SL.require_ok(out, f"{type(self).__name__}.design_servo_kalman")
        self._servo_kalman = out
        self.servo_lqg = SL.ServoLqgState.zeros(self.n, self.device, seed=getattr(self, "seed", 0) or 0)
        return out

    def design_servo_kalman_schedule(self, schedule, dt: float, noise=None, strict: bool = True):
        """A Kalman filter for every node of a ServoSchedule (design_servo_schedule), each on its own trim's model discretised at
        `dt` (hcrl_amd.servo_sched_lqg): ServoKalmanSchedule with table_f [M][120][N], for `step_servo_lqg(schedule=...)`.  noise as
        design_servo_kalman takes it.  One linearise and one design launch over M N lanes.  strict: ValueError when a node has no
        certified filter.  Also starts the scheduled estimator's state (`servo_sched_lqg`: estimate zero, no operating point yet,
        step word 0).  The fleet's state, trim, design and single filter are not touched."""
        from . import servo_sched_lqg as SQ
        out = SQ.design_servo_kalman_schedule(schedule, dt, noise, strict=False)
        if strict:
            out.require_ok(f"{type(self).__name__}.design_servo_kalman_schedule")
        self._servo_kalman_schedule = out
        self.servo_sched_lqg = SQ.ServoSchedLqgState.zeros(self.n, self.device, seed=getattr(self, "seed", 0) or 0)
        return out

    def step_servo_lqg(self, n_steps: int = 1, feedback: str = "estimate", z=None, schedule=None, on: str = "airspeed"):
        """n_steps x {measure the ten words with the sensor noise -> Kalman update, heading innovation wrapped -> the control step
        of step_servo on trim + f -> one RK4 of the filter's dt -> the references move} in ONE launch, f = the estimate, the raw
        measurement or the true state.  Needs design_servo() and design_servo_kalman() first.  z: None = in-kernel Philox draws
        keyed by `servo_lqg.seed` and `servo_lqg.step`, or [n_steps][10][N] float64 standard normals.  `u`, `lqr_saturated_steps`
        and `servo.err` (the errors of the TRUE state) as step_servo leaves them; `servo_lqg` carries the estimate and the
        accumulators (err_est, err_meas, chatter).
        schedule: a ServoSchedule whose filters design_servo_kalman_schedule() has made: the trim point, the gains and the filter of
        each control step are interpolated from the two tables at the airspeed of the law's input (on="airspeed") or at the commanded
        one (on="command"), the estimate is relative to the operating point and moves with it, and neither the single design nor
        the single filter is read: the loop's state (`servo`), the fleet's trim (the origin of the altitude and heading words) and
        `servo_sched_lqg` are.  A schedule without a filter schedule is a ValueError, and so is one whose filters were made at
        another dt than the fleet's single filter."""
        from . import servo_lqg as SL
        if schedule is not None:
            from . import servo_sched_lqg as SQ
            self._need_servo_state("step_servo_lqg")
            res, _ = self._need_trim("step_servo_lqg")
            kalman = self._servo_kalman_schedule
            if kalman is None or kalman.schedule is not schedule:
                raise ValueError(f"{type(self).__name__}.step_servo_lqg: the schedule has no filter schedule; call "
                                 ".design_servo_kalman_schedule(schedule, dt) first")
            dt = kalman.dt if self._servo_kalman is None else self._servo_kalman.dt
            SQ.sched_lqg_step_into(self.precision, self.x, schedule, kalman, SQ.origin_of(res.x0), self.servo, self.servo_sched_lqg, self.params,
                                   self.type_index, dt, n_steps, feedback, on, z, self.u, self._saturated_steps(), self.servo.err)
            self.time += dt * n_steps
            return
        design = self._need_servo("step_servo_lqg")
        if self._servo_kalman is None:
            raise ValueError(f"{type(self).__name__}.step_servo_lqg: the fleet has no servo filter; call .design_servo_kalman() first")
        kalman = self._servo_kalman
        SL.lqg_step_into(self.precision, self.x, design, kalman, self.servo, self.servo_lqg, self.params, self.type_index, kalman.dt,
                         n_steps, feedback, z, self.u, self._saturated_steps(), self.servo.err)
        self.time += kalman.dt * n_steps

    # waypoint missions on the servo's estimate (hcrl_amd.servo_lqg_mission): the mission's guidance fed by the filter and by a
    # filtered position measurement
    def start_servo_lqg_mission(self, waypoints, guidance_type: str = "PP", acceptance_radius: Optional[float] = None,
                                on_complete: str = "freeze", flight_config=None, sigma_pos: Optional[float] = None,
                                gain: Optional[float] = None, rate_pos: Optional[float] = None):
        """start_servo_mission, and the position filter of fly_servo_lqg_mission (`servo_position`: ServoPositionFilter at the
        sensor layer's position noise and position_gain's gain unless given; `servo_position_state`: phat at the fleet's north and
        east).  Needs design_servo() and design_servo_kalman() first.  Returns the ServoMission."""
        from . import servo_lqg_mission as SM
        if self._servo_kalman is None:
            raise ValueError(f"{type(self).__name__}.start_servo_lqg_mission: the fleet has no servo filter; call .design_servo_kalman() first")
        mission = self.start_servo_mission(waypoints, guidance_type, acceptance_radius, on_complete, flight_config)
        self.servo_position = SM.ServoPositionFilter.make(self.device, sigma_pos, gain, SM.DEFAULT_RATE_POS if rate_pos is None else rate_pos,
                                                          self._servo_kalman.dt)
        self.servo_position_state = SM.ServoLqgMissionState.start(self.x)
        return mission

    def fly_servo_lqg_mission(self, n_steps: int = 1, feedback: str = "estimate", z=None):
        """n_steps x {measure -> Kalman update -> position filter -> mission update -> guidance on the estimate -> the control step
        of step_servo_lqg -> one RK4 of the filter's dt} in ONE launch; feedback and the estimator's words as step_servo_lqg, z
        [n_steps][12][N] (the last two words: the north and east position normals).  `servo_mission.stats` are the TRUE state's."""
        from . import servo_lqg_mission as SM
        design = self._need_servo("fly_servo_lqg_mission")
        if self.servo_mission is None or self.servo_position is None:
            raise ValueError(f"{type(self).__name__}.fly_servo_lqg_mission: the fleet has no mission on the estimate; call .start_servo_lqg_mission() first")
        kalman = self._servo_kalman
        SM.lqg_mission_into(self.precision, self.x, design, kalman, self.servo, self.servo_lqg, self.servo_mission, self.servo_position,
                            self.servo_position_state, self.params, self.type_index, kalman.dt, n_steps, feedback, z, self.u,
                            self._saturated_steps(), self.servo.err)
        self.time += kalman.dt * n_steps

    # LQG (hcrl_amd.lqg): the estimator beside the LQR, and the output-feedback loop on noisy measurements
    def design_kalman(self, dt: float, noise=None, scales=None, strict: bool = True):
        """A steady-state Kalman filter for every aircraft at the fleet's current trim, discretised at `dt`: KalmanDesign with
        F [80][N], status 0 = a certified stable filter.  noise: None (the sensor layer's default noise and the default
        process-noise rates), a KalmanNoise, or [16] / [16][N]; scales as design_lqr.  strict: raise ValueError when an aircraft
        has no certified filter.  Also starts the loop's state (`lqg`: estimate at the trim, step word 0)."""
        from . import lqg as G
        res, trim_scales = self._need_trim("design_kalman")
        out = G.design_kalman(res, self.params, self.type_index, trim_scales if scales is None else scales, dt, noise)
        if strict:
            G.require_ok(out, f"{type(self).__name__}.design_kalman")
        self._kalman = out
        self.lqg = G.LqgState.zeros(self.n, self.device, seed=getattr(self, "seed", 0) or 0)
        return out

    def step_lqg(self, n_steps: int = 1, feedback: str = "estimate", z=None):
        """n_steps x {measure the eight regulated words with the sensor noise -> Kalman update -> u = u0 - K f, clipped -> one
        RK4 of the filter's dt} in ONE launch, f = the estimate, the raw measurement or the true state.  Needs design_lqr()
        and design_kalman() first.  z: None = in-kernel Philox draws keyed by `lqg.seed` and `lqg.step`, or [n_steps][8][N]
        float64 standard normals.  `u` receives the last applied controls, `lqr_saturated_steps` counts clipped steps, `lqg`
        carries the estimate and the accumulators (err_est, err_meas, chatter)."""
        from . import lqg as G
        lqr_design, kalman = self._need_designs("step_lqg")
        G.step_into(self.precision, self.x, lqr_design, kalman, self.lqg, self.params, self.type_index, kalman.dt, n_steps, feedback, z,
                    self.u, self._saturated_steps())
        self.time += kalman.dt * n_steps

    # Loop margins (hcrl_amd.margins): how robust the loop step_lqr / step_lqg fly is, sampled at dt and through the estimator
    def loop_margins(self, feedback: str = "estimate", omega=None, curve: bool = False):
        """LoopMargins of every aircraft's loop as `step_lqg(feedback=...)` flies it, at the filter's dt: alpha_s [2][N] (the
        smallest singular value of the return difference at the plant input, longitudinal | lateral), status 0 = the gain /
        phase disk it stands for is guaranteed.  Needs design_lqr() and design_kalman() first.  omega: None = 64 points,
        logarithmic from 0.01 rad/s to the Nyquist rate.  The fleet's state is not touched."""
        from . import margins as M
        return M.loop_margins(*self._need_designs("loop_margins"), feedback, omega, curve)

    def servo_loop_margins(self, feedback: str = "estimate", omega=None, curve: bool = False):
        """LoopMargins of every aircraft's servo loop as `step_servo_lqg(feedback=...)` flies it in its linear region, at the filter's
        dt: gain through a zero-order hold, integrators by forward Euler, and under "estimate" through the servo's filter.  Under
        "truth" or "measurement" it is the loop of `step_servo` at that dt.  Needs design_servo() and design_servo_kalman() first.
        omega: None = 64 points, logarithmic from 0.01 rad/s to the Nyquist rate.  The fleet's state is not touched."""
        from . import servo_margins as SM
        for design, lacks, call in ((self._servo, "stabilising servo gain", "design_servo()"), (self._servo_kalman, "stable servo filter", "design_servo_kalman(dt)")):
            if design is None:
                raise ValueError(f"{type(self).__name__}.servo_loop_margins: {self.n} of {self.n} aircraft have no certified {lacks} (call .{call} first)")
        return SM.servo_loop_margins(self._servo, self._servo_kalman, self._servo.x0, feedback, omega, curve)

    def servo_modes(self, loop: str = "continuous", scales=None):
        """ServoModes of every aircraft's servo loop: "continuous" = the seven longitudinal and six lateral poles of the augmented
        closed loop linearised at the fleet's current trim (scales: None = the multipliers the trim was solved with); "sampled" =
        the same loops as `step_servo` flies them at the filter's dt, integrators by forward Euler; "filter" = the five + five
        poles of the servo filter's error dynamics.  "continuous" needs design_servo(), "filter" design_servo_kalman(), "sampled"
        both.  The fleet's state is not touched."""
        from . import servo_modes as SMO
        if loop not in SMO.LOOPS:
            raise ValueError(f"loop must be one of {SMO.LOOPS}")
        needs = {"continuous": (True, False), "sampled": (True, True), "filter": (False, True)}[loop]
        for need, design, lacks, call in ((needs[0], self._servo, "stabilising servo gain", "design_servo()"),
                                          (needs[1], self._servo_kalman, "stable servo filter", "design_servo_kalman(dt)")):
            if need and design is None:
                raise ValueError(f"{type(self).__name__}.servo_modes: {self.n} of {self.n} aircraft have no certified {lacks} (call .{call} first)")
        if loop == "filter":
            return self._servo_kalman.filter_poles()
        if loop == "sampled":
            return SMO.sampled_poles(self._servo, self._servo_kalman, self._servo.x0)
        from . import trim as T
        res, trim_scales = self._need_trim("servo_modes")
        A, B = T.linearize_at_trim(res, self.params, self.type_index, trim_scales if scales is None else scales)
        return self._servo.modes(A, B)

    def servo_covariance(self, feedback: str = "estimate", sigma=None, process_rates=None):
        """ServoCovariance of every aircraft's servo loop as `step_servo_lqg(feedback=...)` flies it in its linear region, at the
        filter's dt: the predicted steady-state variances of the state, the estimate, the tracking errors, the integrators, the
        controls and their step-to-step change (rms_tracking(), chatter(), headroom(u0), ...).  sigma: None = the measurement noise
        `step_servo_lqg` applies (the filter design's `sigma`: the noise it was designed for when that is shared by the fleet, the
        sensor layer's defaults when it was designed on per-aircraft noise); process_rates: None = no process noise acts, as in the
        flights.  Needs design_servo() and
        design_servo_kalman() first.  The fleet's state is not touched."""
        from . import servo_covariance as SC
        for design, lacks, call in ((self._servo, "stabilising servo gain", "design_servo()"), (self._servo_kalman, "stable servo filter", "design_servo_kalman(dt)")):
            if design is None:
                raise ValueError(f"{type(self).__name__}.servo_covariance: {self.n} of {self.n} aircraft have no certified {lacks} (call .{call} first)")
        return SC.servo_covariance(self._servo, self._servo_kalman, self._servo.x0, None, sigma, process_rates, feedback)

    # Flight modes (hcrl_amd.modes): where the poles are
    def modes(self, design=None, scales=None):
        """FleetModes of every aircraft linearised at the fleet's current trim (the last `.trim(...)`): the open-loop poles, or
        with `design` (an LqrDesign) those of a - b K; eig [2][4][N] (longitudinal | lateral), summary [2][FD_NMO][N].  scales:
        None = the multipliers the trim was solved with.  The fleet's state is not touched."""
        from . import modes as MO
        res, trim_scales = self._need_trim("modes")
        return MO.fleet_modes(res, self.params, self.type_index, trim_scales if scales is None else scales, design)

    def _need_trim(self, what: str):
        if self._trim is None:
            raise ValueError(f"{type(self).__name__}.{what}: the fleet has no trim; call .trim(...) first")
        return self._trim

    def _need_designs(self, what: str):
        for design, lacks, call in ((self._lqr, "stabilising gain", "design_lqr()"), (self._kalman, "stable filter", "design_kalman(dt)")):
            if design is None:
                raise ValueError(f"{type(self).__name__}.{what}: {self.n} of {self.n} aircraft have no certified {lacks} (call .{call} first)")
        return self._lqr, self._kalman

    def _saturated_steps(self) -> torch.Tensor:
        if self.lqr_saturated_steps is None:
            self.lqr_saturated_steps = torch.zeros(self.n, dtype=torch.int32, device=self.device)
        return self.lqr_saturated_steps


class BatchedCascade(BatchedSixDOF):
    """N aircraft each flying the same waypoint mission under the 5-level cascaded PID stack."""

    def __init__(self, n: int, waypoints: Sequence[Waypoint], precision: str = "f64",
                 config: Optional[ControllerConfig] = None, flight_config: Optional[FlightControlConfig] = None,
                 guidance_type: str = "PP", acceptance_radius: Optional[float] = None, on_complete: str = "freeze",
                 **kw):
        super().__init__(n, precision, **kw)
        self.n_wp = len(waypoints)
        self.wps = torch.as_tensor(waypoint_table(waypoints), device=self.device)
        self.pid_cfg = torch.as_tensor(pid_table(config, flight_config), device=self.device)
        self.consts = torch.as_tensor(cascade_consts(config, flight_config, guidance_type, acceptance_radius,
                                                     on_complete), device=self.device)
        self.pid_state = torch.zeros((L.FD_NPID * L.FD_NPS, self.n), dtype=torch.float32, device=self.device)
        self.wp_idx = torch.zeros(self.n, dtype=torch.int32, device=self.device)
        self.reached_total = torch.zeros(self.n, dtype=torch.int32, device=self.device)
        self.surfaces = torch.zeros((L.FD_NU, self.n), dtype=self.dtype, device=self.device)
        self._cascade_fn = getattr(self.lib, f"fdyn_cascade_step_{precision}")

    def reset(self, x0=None):
        super().reset(x0)
        if hasattr(self, "pid_state"):
            self.pid_state.zero_(); self.wp_idx.zero_(); self.reached_total.zero_()

    def run(self, dt: float, n_steps: int):
        """n_steps control steps in ONE launch (mission update -> agents -> RK4), all state in registers."""
        rc = self._cascade_fn(_lib.ptr(self.x), _lib.ptr(self.pid_state), _lib.ptr(self.wp_idx),
                              _lib.ptr(self.type_index), _lib.ptr(self.params), self.n_types, _lib.ptr(self.pid_cfg),
                              _lib.ptr(self.consts), _lib.ptr(self.wps), self.n_wp, self.n, float(dt), int(n_steps),
                              _lib.ptr(self.surfaces), _lib.ptr(self.reached_total), _lib.current_stream())
        _lib.check(rc, "cascade step")
        self.time += dt * n_steps

    def mission_complete(self) -> torch.Tensor:
        return self.wp_idx >= self.n_wp

"""The LQ servo gain-scheduled over airspeed ON NOISY SENSORS: the schedule of `hcrl_amd.servo_sched` with a table of filters beside
the table of designs, flown by `fdyn_servo_sched_lqg_step_*` (include/fdyn_servo_sched_lqg.h).

`hcrl_amd.servo_lqg` flies one design through one filter, both made at one trim; `hcrl_amd.servo_sched` interpolates the design over
airspeed but reads the true state.  Here every node of a `ServoSchedule` also gets the steady-state Kalman filter of its own trim's
model (one `fdyn_linearize` and one `fdyn_servo_kf_design` launch over M x n lanes), and each control step reads the trim point, the
gains AND the filter from the two nodes that bracket the airspeed of the law's input (the default) or the commanded one.  The estimate
and the last control offset are moved to each new operating point, so neither jumps.

    fleet.trim(15.0)
    fleet.design_servo()
    sched = fleet.design_servo_schedule((15.0, 20.0, 25.0, 30.0))
    fleet.design_servo_kalman_schedule(sched, dt=0.01)              # ServoKalmanSchedule: table_f [M][120][n]
    fleet.command_servo(speed=30.0)
    fleet.step_servo_lqg(100, schedule=sched)                       # on="airspeed" | "command"

Still air only.  `sched_lqg_step_into` never synchronises with the device; the design does when `strict` reads the status back.
"""
from dataclasses import dataclass
from typing import Optional

import torch

from . import _lib, layout as L
from . import servo as SV
from . import servo_lqg as SL
from . import servo_sched as SS
from . import trim as T
from .lqg import FEEDBACK

NB, NX = L.FD_SK_NB, L.FD_NSKX


@dataclass
class ServoKalmanSchedule:
    table_f: torch.Tensor                   # [M][FD_NSKF][n] float64: node k's filter, what fdyn_servo_sched_lqg_step_* read
    status: torch.Tensor                    # [M][n] int32: FD_KF_* bits of each node's filter (pass-through words where not 0)
    dt: float                               # the step every node's model was discretised at
    noise: torch.Tensor                     # [FD_NSKN] or [FD_NSKN][n] float64: what the filters were designed for
    sigma: Optional[torch.Tensor] = None    # [10] float64: the measurement noise the loop applies
    schedule: Optional[SS.ServoSchedule] = None   # the designs these filters belong to

    @property
    def n(self) -> int:
        return int(self.table_f.shape[2])

    @property
    def n_nodes(self) -> int:
        return int(self.table_f.shape[0])

    @property
    def ok(self) -> torch.Tensor:
        """[n] bool: every node of the aircraft has a certified stable filter."""
        return (self.status == 0).all(dim=0)

    def count_not_ok(self) -> int:
        return int((~self.ok).sum())

    def require_ok(self, what: str = "design_servo_kalman_schedule"):
        bad = self.count_not_ok()
        if bad:
            first = int(torch.nonzero(~self.ok)[0])
            node = int(torch.nonzero(self.status[:, first] != 0)[0])
            raise ValueError(f"{what}: {bad} of {self.n} aircraft have a node without a certified stable filter (first: aircraft "
                             f"{first}, node {node}: {SL.describe_status(int(self.status[node, first]))})")

    def interpolated(self, position: torch.Tensor) -> torch.Tensor:
        """[FD_NSKF][n]: the filter at the table positions k + t [n] (0 <= position <= M - 1), as step 3 forms it, with torch ops."""
        k = position.floor().clamp(0, max(self.n_nodes - 2, 0)).to(torch.int64)
        t = position - k.to(torch.float64)
        lo = torch.gather(self.table_f, 0, k[None, None].expand(1, L.FD_NSKF, self.n))[0]
        hi = torch.gather(self.table_f, 0, (k + 1).clamp(max=self.n_nodes - 1)[None, None].expand(1, L.FD_NSKF, self.n))[0]
        return lo + t * (hi - lo)

    def frozen_point_report(self, points_per_interval: int = 1) -> dict:
        """The frozen-point check of the filter schedule, through existing entry points only: between every two nodes, at
        `points_per_interval` evenly spaced table positions, P = (M - 1) x points_per_interval points in all, lane p n + i = point p
        of aircraft i.  Returns dict(
          airspeeds [P][n],
          poles: (longitudinal, lateral) ServoModes over P n lanes of Phi_t (I - L_t), the interpolated filter's error dynamics in
                 ServoKalmanDesign.filter_matrix's form (two launches of fdyn_square_modes at N = 5); spectral_radius() < 1 at a
                 point: the interpolated filter is stable on its own interpolated model there,
          dphi [P][n], dgamma [P][n]: |Phi_t - Phi*|_inf and |Gamma_t - Gamma*|_inf (largest absolute entry, both blocks) against
                 the filter designed AT that point (one launch each of fdyn_trim, fdyn_linearize and fdyn_servo_kf_design),
          status [P][n]: FD_KF_* bits of the filter designed at the point)."""
        from . import servo_modes as SMO
        s = self.schedule
        if s is None or s.context is None:
            raise ValueError("the filter schedule carries no flight condition to trim at (it was not made by design_servo_kalman_schedule)")
        if self.n_nodes < 2 or points_per_interval < 1:
            raise ValueError("frozen_point_report needs at least two nodes and one point per interval")
        c, n, dev = s.context, self.n, self.table_f.device
        pos = torch.tensor([k + (j + 1) / (points_per_interval + 1) for k in range(self.n_nodes - 1) for j in range(points_per_interval)],
                           dtype=torch.float64, device=dev)
        P = int(pos.shape[0])
        V = torch.stack([s.interpolated(p.expand(n))[L.FD_SS_V] for p in pos])                    # [P][n]
        Ft = torch.stack([self.interpolated(p.expand(n)) for p in pos]).permute(1, 0, 2).reshape(L.FD_NSKF, P * n).contiguous()
        spec = torch.stack([V.reshape(-1)] + [c["spec"][k].repeat(P) for k in range(1, L.FD_NTS)]).contiguous()
        rep = lambda t: None if t is None else t.repeat(*([1] * (t.dim() - 1)), P).contiguous()    # noqa: E731
        tr = T.trim_into(spec, c["params"], rep(c["type_index"]), rep(c["scales"]))
        A, B = T.linearize_into(tr.x0, tr.u0, c["params"], rep(c["type_index"]), rep(c["scales"]))
        star = SL.servo_kalman_into(A, B, self.dt, rep(self.noise) if self.noise.dim() == 2 else self.noise)
        interp = SL.ServoKalmanDesign(Ft, star.residual, star.iters, star.status, self.dt)
        fm = interp.filter_matrix()                                                                # [2][5][5][P n]
        poles = tuple(SMO.square_modes_into(fm[b].contiguous()) for b in range(2))
        dphi = (interp.phi() - star.phi()).abs().amax(dim=(0, 1, 2)).reshape(P, n)
        dgamma = (interp.gamma() - star.gamma()).abs().amax(dim=(0, 1, 2)).reshape(P, n)
        return dict(airspeeds=V, poles=poles, dphi=dphi, dgamma=dgamma, status=star.status.reshape(P, n))


def pack_f(F: torch.Tensor, M: int) -> torch.Tensor:
    """F [FD_NSKF][M n] (lane k n + i = node k of aircraft i) -> table_f [M][FD_NSKF][n]."""
    n = int(F.shape[1]) // M
    return F.reshape(L.FD_NSKF, M, n).permute(1, 0, 2).contiguous()


def design_servo_kalman_schedule(schedule: SS.ServoSchedule, dt: float, noise=None, strict: bool = True) -> ServoKalmanSchedule:
    """A filter for every node of `schedule`: linearise at the node trims the schedule keeps (its `x0`, the table's trim controls,
    and the params, types and scales of its record), then ONE fdyn_linearize and ONE fdyn_servo_kf_design launch over M n lanes, and
    a reshape.  noise as `servo_lqg.noise_tensor` takes it (per aircraft: shared by its nodes).  A node without a certified filter
    carries its FD_KF_* bits and the pass-through words; strict: ValueError when there is one."""
    if schedule.x0 is None or schedule.context is None:
        raise ValueError("the schedule carries no node trims to linearise at (it was not made by design_servo_schedule)")
    c, M, n, dev = schedule.context, schedule.n_nodes, schedule.n, schedule.table.device
    u0 = schedule.table[:, L.FD_SS_U0:L.FD_SS_K].permute(1, 0, 2).reshape(L.FD_NU, M * n).contiguous()
    tile = lambda t: None if t is None else t.repeat(*([1] * (t.dim() - 1)), M).contiguous()       # noqa: E731
    A, B = T.linearize_into(schedule.x0, u0, c["params"], tile(c["type_index"]), tile(c["scales"]))
    nz = SL.noise_tensor(noise, n, dev)
    kf = SL.servo_kalman_into(A, B, dt, tile(nz) if nz.dim() == 2 else nz)
    sigma = nz[:NX].clone() if nz.dim() == 1 else torch.as_tensor(SL.servo_sensor_sigma(), device=dev)
    out = ServoKalmanSchedule(pack_f(kf.F, M), kf.status.reshape(M, n), float(dt), nz, sigma, schedule)
    if strict:
        out.require_ok()
    return out


@dataclass
class ServoSchedLqgState(SL.ServoLqgState):
    """A ServoLqgState plus the operating point its estimate is relative to."""
    sched_state: Optional[torch.Tensor] = None      # [2][n] float64: sigma and the table position; position < 0: none yet

    @classmethod
    def zeros(cls, n: int, device, seed: int = 0) -> "ServoSchedLqgState":
        z = lambda rows: torch.zeros((rows, n), dtype=torch.float64, device=device)   # noqa: E731
        out = cls(z(NX), z(L.FD_NU), torch.zeros(1, dtype=torch.int32, device=device), z(NX), z(NX), z(L.FD_NU), z(NX), int(seed))
        out.sched_state = torch.stack([torch.zeros(n, dtype=torch.float64, device=device), -torch.ones(n, dtype=torch.float64, device=device)])
        return out

    def reset(self, seed: Optional[int] = None):
        """Back to no operating point (position -1), then ServoLqgState.reset."""
        super().reset(seed)
        self.sched_state[0].zero_()
        self.sched_state[1].fill_(-1.0)


def origin_of(x0: torch.Tensor) -> torch.Tensor:
    """[2][n] float64: z0 and psi0 of a trim x0 [12][n]."""
    return torch.stack([x0[L.FD_X_D], x0[L.FD_X_YAW]]).to(torch.float64).contiguous()


def sched_lqg_step_into(precision: str, x: torch.Tensor, schedule: SS.ServoSchedule, kalman: Optional[ServoKalmanSchedule], origin: torch.Tensor,
                        state: SV.ServoState, lqg_state: ServoSchedLqgState, params: torch.Tensor, type_index: Optional[torch.Tensor],
                        dt: float, n_steps: int, feedback="estimate", on: str = "airspeed", z: Optional[torch.Tensor] = None,
                        surf_out: Optional[torch.Tensor] = None, sat_steps: Optional[torch.Tensor] = None,
                        err_out: Optional[torch.Tensor] = None, accumulate: bool = True):
    """One launch of fdyn_servo_sched_lqg_step_<precision>: lqg_step_into with the design AND the filter read from the two schedules;
    origin [2][n] float64 (z0, psi0: `origin_of` a trim).  The estimator's words, the operating point (`lqg_state.sched_state`) and
    the step word advance.  n_steps = 0 writes surf_out alone.  ValueError for a missing filter schedule, or one made for another
    schedule or at another dt."""
    if kalman is None:
        raise ValueError("the schedule has no filter schedule; call design_servo_kalman_schedule(schedule, dt) first")
    if kalman.dt != float(dt):
        raise ValueError(f"the filter schedule was designed at dt = {kalman.dt}, the flight asks for dt = {float(dt)}")
    if kalman.sigma is None:
        raise ValueError("the filter schedule carries no measurement noise (sigma)")
    SV.check_step(schedule, dt, "sched_lqg_step_into")
    n = SS._check(precision, x, schedule, state, None)
    if (kalman.n_nodes, kalman.n) != (schedule.n_nodes, n) or tuple(kalman.table_f.shape[1:]) != (L.FD_NSKF, n) or kalman.table_f.dtype != torch.float64:
        raise ValueError(f"the filter schedule must be [{schedule.n_nodes}][{L.FD_NSKF}][{n}] float64 beside the schedule's table, got "
                         f"{tuple(kalman.table_f.shape)} {kalman.table_f.dtype}")
    if tuple(origin.shape) != (2, n) or origin.dtype != torch.float64:
        raise ValueError(f"origin must be [2][{n}] float64, got {tuple(origin.shape)} {origin.dtype}")
    ss = lqg_state.sched_state
    if int(lqg_state.xhat.shape[1]) != n or ss is None or tuple(ss.shape) != (2, n) or ss.dtype != torch.float64:
        raise ValueError(f"the estimator's state must be that of the fleet, with sched_state [2][{n}] float64")
    fb = FEEDBACK[feedback] if isinstance(feedback, str) else int(feedback)
    if z is not None and (tuple(z.shape) != (int(n_steps), NX, n) or z.dtype != torch.float64 or not z.is_contiguous()):
        raise ValueError(f"z must be contiguous float64 [{int(n_steps)}][{NX}][{n}]")
    acc = (lqg_state.err_est, lqg_state.err_meas, lqg_state.chatter, lqg_state.meas) if accumulate else (None, None, None, None)
    rc = getattr(_lib.load(), f"fdyn_servo_sched_lqg_step_{precision}")(
        _lib.ptr(x), _lib.ptr(schedule.table), _lib.ptr(kalman.table_f), schedule.n_nodes, SS.sched_on(on), _lib.ptr(origin), _lib.ptr(state.ref),
        _lib.ptr(state.integ), _lib.ptr(state.limits), _lib.ptr(type_index), _lib.ptr(params), int(params.shape[0]), n, float(dt), int(n_steps),
        _lib.ptr(surf_out), _lib.ptr(sat_steps), _lib.ptr(err_out), _lib.ptr(kalman.sigma), _lib.ptr(lqg_state.xhat), _lib.ptr(lqg_state.du_prev),
        _lib.ptr(ss), int(lqg_state.seed) & 0xFFFFFFFFFFFFFFFF, _lib.ptr(lqg_state.step), _lib.ptr(z), fb, *(_lib.ptr(t) for t in acc),
        _lib.current_stream())
    _lib.check(rc, "fdyn_servo_sched_lqg_step")
    if n_steps > 0:
        if lqg_state.step is not None:
            lqg_state.step.add_(int(n_steps))
        lqg_state.steps_accumulated += int(n_steps)

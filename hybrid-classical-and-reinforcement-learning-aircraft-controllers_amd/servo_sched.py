"""The LQ servo gain-scheduled over airspeed in flight: trim -> linearise -> design at M airspeeds -> fly on the interpolated design.

`hcrl_amd.servo` flies one design per aircraft; a speed command far from that trim leaves the new trim's pitch, elevator and
throttle to the integrators.  Here every aircraft carries a table of M <= FD_MAX_SCHED_NODES designs over airspeed
(include/fdyn_servo_sched.h), and each control step of `fdyn_servo_sched_step_*` / `fdyn_servo_sched_mission_*` reads its trim point
and its gains from the two nodes that bracket the measured airspeed (the default) or the commanded one.  The M trims of n aircraft
are one trim, one linearise and one `fdyn_servo_design` launch over M x n lanes.

    fleet.trim(15.0)
    sched = fleet.design_servo_schedule((15.0, 20.0, 25.0, 30.0))   # ServoSchedule: table [M][FD_NSS][n]
    fleet.command_servo(speed=30.0)
    fleet.step_servo(n_steps=100, dt=0.01, schedule=sched)          # on="airspeed" | "command"
    sched.frozen_point_modes()                                      # the poles of A - B K between the nodes
    fleet.design_servo_schedule((15.0, 20.0, 25.0, 30.0), dt=0.02)  # every node the sampled-data design for that step (servo.servo_dt_into)

Still air and the true state only.  The flight entry points (`sched_step_into`, `sched_mission_into`) never synchronise with the
device.  The design does, before anything is launched: `strict` reads the status back, and node airspeeds or flight-condition
words given as device tensors are brought to the host to be checked and broadcast -- `BatchedSixDOF.design_servo_schedule` passes
the current trim's altitude and heading that way when they are not given.
"""
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _lib, layout as L
from . import servo as SV
from . import trim as T

ON = {"airspeed": L.FD_SCHED_ON_AIRSPEED, "command": L.FD_SCHED_ON_COMMAND}
# the rows of x0 a node keeps, in the order the step kernel keeps them: u, w, q, theta, v, p, r, phi
X0_WORDS = (L.FD_X_U, L.FD_X_W, L.FD_X_Q, L.FD_X_PITCH, L.FD_X_V, L.FD_X_P, L.FD_X_R, L.FD_X_ROLL)


def sched_on(on: str) -> int:
    if on not in ON:
        raise ValueError(f"on must be one of {tuple(ON)}, got {on!r}")
    return ON[on]


def node_airspeeds(airspeeds, n: int) -> np.ndarray:
    """M scalars, or [M][n] -> float64 [M][n]; ValueError unless 1 <= M <= FD_MAX_SCHED_NODES and every aircraft's airspeeds are
    finite and strictly increasing."""
    if isinstance(airspeeds, torch.Tensor):
        airspeeds = airspeeds.detach().cpu().numpy()
    a = np.asarray(airspeeds, np.float64)
    if a.ndim == 1:
        a = np.repeat(a[:, None], n, axis=1)
    if a.ndim != 2 or a.shape[1] != n:
        raise ValueError(f"node airspeeds: expected M values or [M][{n}], got shape {a.shape}")
    if not 1 <= a.shape[0] <= L.FD_MAX_SCHED_NODES:
        raise ValueError(f"a schedule has 1 to {L.FD_MAX_SCHED_NODES} nodes, got {a.shape[0]}")
    if not np.isfinite(a).all() or not (np.diff(a, axis=0) > 0.0).all():
        raise ValueError("node airspeeds must be finite and strictly increasing")
    return np.ascontiguousarray(a)


def pack(airspeeds: torch.Tensor, x0: torch.Tensor, u0: torch.Tensor, K: torch.Tensor) -> torch.Tensor:
    """airspeeds [M][n], x0 [12][M n], u0 [4][M n], K [26][M n] (lane k n + i = node k of aircraft i) -> table [M][FD_NSS][n], with
    torch ops on the device."""
    M, n = (int(v) for v in airspeeds.shape)
    table = torch.empty((M, L.FD_NSS, n), dtype=torch.float64, device=airspeeds.device)
    table[:, L.FD_SS_V] = airspeeds
    table[:, L.FD_SS_X0:L.FD_SS_U0] = x0[list(X0_WORDS)].reshape(len(X0_WORDS), M, n).permute(1, 0, 2)
    table[:, L.FD_SS_U0:L.FD_SS_K] = u0.reshape(L.FD_NU, M, n).permute(1, 0, 2)
    table[:, L.FD_SS_K:] = K.reshape(L.FD_NSVK, M, n).permute(1, 0, 2)
    return table


@dataclass
class ServoSchedule:
    table: torch.Tensor                     # [M][FD_NSS][n] float64 (FD_SS_*): what fdyn_servo_sched_* read
    airspeeds: torch.Tensor                 # [M][n] float64: the node airspeeds, strictly increasing per aircraft
    status: torch.Tensor                    # [M][n] int32: FD_SV_* bits of each node's design (FD_SV_BAD_INPUT also: no trim there)
    x0: Optional[torch.Tensor] = None       # [12][M n] float64: the nodes' trims, lane k n + i = node k of aircraft i
    context: Optional[dict] = None          # what frozen_point_modes trims and linearises with
    dt: Optional[float] = None              # the control step sampled-data nodes were designed for (None: continuous designs)

    @property
    def n(self) -> int:
        return int(self.table.shape[2])

    @property
    def n_nodes(self) -> int:
        return int(self.table.shape[0])

    @property
    def ok(self) -> torch.Tensor:
        """[n] bool: every node of the aircraft has a certified stabilising gain."""
        return (self.status == 0).all(dim=0)

    def count_not_ok(self) -> int:
        return int((~self.ok).sum())

    def require_ok(self, what: str = "design_servo_schedule"):
        bad = self.count_not_ok()
        if bad:
            first = int(torch.nonzero(~self.ok)[0])
            node = int(torch.nonzero(self.status[:, first] != 0)[0])
            raise ValueError(f"{what}: {bad} of {self.n} aircraft have a node without a certified stabilising servo gain (first: aircraft "
                             f"{first}, node {node}: {SV.describe_status(int(self.status[node, first]))})")

    @classmethod
    def from_design(cls, design: SV.ServoDesign) -> "ServoSchedule":
        """The one-node schedule of a ServoDesign: flown, it is that design bit for bit."""
        if design.x0 is None or design.u0 is None:
            raise ValueError("the design carries no trim point (x0, u0)")
        u, w = design.x0[L.FD_X_U], design.x0[L.FD_X_W]
        V = torch.sqrt(u * u + w * w)[None]
        return cls(pack(V, design.x0, design.u0, design.K), V, design.status[None].clone(), design.x0, dt=design.dt)

    def interpolated(self, position: torch.Tensor) -> torch.Tensor:
        """[FD_NSS][n]: the words at the table positions k + t [n] (0 <= position <= M - 1), as step 0b forms them, with torch ops."""
        k = position.floor().clamp(0, max(self.n_nodes - 2, 0)).to(torch.int64)
        t = position - k.to(torch.float64)
        lo = torch.gather(self.table, 0, k[None, None].expand(1, L.FD_NSS, self.n))[0]
        hi = torch.gather(self.table, 0, (k + 1).clamp(max=self.n_nodes - 1)[None, None].expand(1, L.FD_NSS, self.n))[0]
        return lo + t * (hi - lo)

    def frozen_point_modes(self, points_per_interval: int = 1):
        """The frozen-point check of the schedule: between every two nodes, at `points_per_interval` evenly spaced airspeeds, trim and
        linearise each aircraft there, interpolate K there, and report the poles of the continuous augmented closed loops
        A - B K (one launch each of fdyn_trim, fdyn_linearize and fdyn_servo_flight_modes over P n lanes, P = (M - 1) x
        points_per_interval).  Returns (ServoModes over P n lanes, lane p n + i = point p of aircraft i; airspeeds [P][n]).
        abscissa() < 0 at a point: the interpolated gain stabilises the airframe's own model there."""
        from . import servo_modes as SMO
        if self.context is None:
            raise ValueError("the schedule carries no flight condition to trim at (it was not made by design_servo_schedule)")
        if self.n_nodes < 2 or points_per_interval < 1:
            raise ValueError("frozen_point_modes needs at least two nodes and one point per interval")
        c, n, dev = self.context, self.n, self.table.device
        pos = torch.tensor([k + (j + 1) / (points_per_interval + 1) for k in range(self.n_nodes - 1) for j in range(points_per_interval)],
                           dtype=torch.float64, device=dev)
        P = int(pos.shape[0])
        words = torch.stack([self.interpolated(p.expand(n)) for p in pos])                         # [P][FD_NSS][n]
        V = words[:, L.FD_SS_V]
        spec = torch.stack([V.reshape(-1)] + [c["spec"][k].repeat(P) for k in range(1, L.FD_NTS)]).contiguous()
        rep = lambda t: None if t is None else t.repeat(*([1] * (t.dim() - 1)), P).contiguous()    # noqa: E731
        tr = T.trim_into(spec, c["params"], rep(c["type_index"]), rep(c["scales"]))
        A, B = T.linearize_into(tr.x0, tr.u0, c["params"], rep(c["type_index"]), rep(c["scales"]))
        K = words[:, L.FD_SS_K:].permute(1, 0, 2).reshape(L.FD_NSVK, P * n).contiguous()
        return SMO.flight_modes_into(A, B, tr.x0, K), V


def design_servo_schedule(airspeeds, n: int, params: torch.Tensor, type_index=None, climb=0.0, turn=0.0, altitude=100.0, heading=0.0,
                          weights=None, scales=None, strict: bool = True, dt: Optional[float] = None) -> ServoSchedule:
    """Trim, linearise and design n aircraft at M airspeeds each: one launch of fdyn_trim, fdyn_linearize and fdyn_servo_design (dt
    None) or fdyn_servo_design_dt (the sampled-data design for the control step dt; the schedule then carries that `dt`) over
    M n lanes, then a torch pack.  airspeeds: M values for the whole fleet, or [M][n]; the other flight-condition words, weights
    and scales as trim_fleet and design_servo take them (per aircraft: shared by its nodes).  ValueError for airspeeds that are not
    strictly increasing or for M > FD_MAX_SCHED_NODES; strict: ValueError when a node has no trim or no certified gain."""
    dev = params.device
    V = node_airspeeds(airspeeds, n)
    M = V.shape[0]
    rows = T.flight_condition(n, V[0], climb, turn, altitude, heading)                             # [5][n]; row 0 replaced per node
    spec = np.tile(rows, (1, M))
    spec[L.FD_TS_AIRSPEED] = V.reshape(-1)
    spec_d = torch.as_tensor(spec, device=dev)
    tidx = T._type_tensor(n, type_index, dev)
    sc = T.scale_rows(n, scales, dev)
    tile = lambda t: None if t is None else t.repeat(*([1] * (t.dim() - 1)), M).contiguous()       # noqa: E731
    tr = T.trim_into(spec_d, params, tile(tidx), tile(sc))
    A, B = T.linearize_into(tr.x0, tr.u0, params, tile(tidx), tile(sc))
    w = SV.weights_tensor(weights, n, dev)
    w = tile(w) if w.dim() == 2 else w
    d = SV.servo_into(A, B, tr.x0, w) if dt is None else SV.servo_dt_into(A, B, tr.x0, w, dt)
    status = (d.status | (tr.status != 0).to(torch.int32) * L.FD_SV_BAD_INPUT).reshape(M, n)
    V_d = torch.as_tensor(V, device=dev)
    out = ServoSchedule(pack(V_d, tr.x0, tr.u0, d.K), V_d, status, tr.x0,
                        dict(spec=torch.as_tensor(rows, device=dev), params=params, type_index=tidx, scales=sc), d.dt)
    if strict:
        out.require_ok()
    return out


def sched_step_into(precision: str, x: torch.Tensor, schedule: ServoSchedule, state: SV.ServoState, params: torch.Tensor,
                    type_index: Optional[torch.Tensor], dt: float, n_steps: int, on: str = "airspeed", surf_out: Optional[torch.Tensor] = None,
                    sat_steps: Optional[torch.Tensor] = None, err_out: Optional[torch.Tensor] = None, sigma_out: Optional[torch.Tensor] = None):
    """One launch of fdyn_servo_sched_step_<precision>: step_into with the design read from the schedule; sigma_out [2][n] float64
    receives sigma and the table position of the last control step.  n_steps = 0 writes surf_out and sigma_out alone."""
    n = _check(precision, x, schedule, state, sigma_out)
    SV.check_step(schedule, dt, "sched_step_into")
    rc = getattr(_lib.load(), f"fdyn_servo_sched_step_{precision}")(
        _lib.ptr(x), _lib.ptr(schedule.table), schedule.n_nodes, sched_on(on), _lib.ptr(state.ref), _lib.ptr(state.integ), _lib.ptr(state.limits),
        _lib.ptr(type_index), _lib.ptr(params), int(params.shape[0]), n, float(dt), int(n_steps), _lib.ptr(surf_out), _lib.ptr(sat_steps),
        _lib.ptr(err_out), _lib.ptr(sigma_out), _lib.current_stream())
    _lib.check(rc, "fdyn_servo_sched_step")


def sched_mission_into(precision: str, x: torch.Tensor, schedule: ServoSchedule, state: SV.ServoState, mission: SV.ServoMission,
                       params: torch.Tensor, type_index: Optional[torch.Tensor], dt: float, n_steps: int, on: str = "airspeed",
                       surf_out: Optional[torch.Tensor] = None, sat_steps: Optional[torch.Tensor] = None, err_out: Optional[torch.Tensor] = None,
                       sigma_out: Optional[torch.Tensor] = None):
    """One launch of fdyn_servo_sched_mission_<precision>: mission_into with the design read from the schedule."""
    n = _check(precision, x, schedule, state, sigma_out)
    SV.check_step(schedule, dt, "sched_mission_into")
    if mission.n != n:
        raise ValueError(f"the mission holds {mission.n} aircraft, the fleet {n}")
    rc = getattr(_lib.load(), f"fdyn_servo_sched_mission_{precision}")(
        _lib.ptr(x), _lib.ptr(schedule.table), schedule.n_nodes, sched_on(on), _lib.ptr(state.ref), _lib.ptr(state.integ), _lib.ptr(state.limits),
        _lib.ptr(mission.wp_idx), _lib.ptr(mission.consts), _lib.ptr(mission.wps), mission.n_wp, _lib.ptr(type_index), _lib.ptr(params),
        int(params.shape[0]), n, float(dt), int(n_steps), _lib.ptr(surf_out), _lib.ptr(sat_steps), _lib.ptr(err_out),
        _lib.ptr(mission.reached_total), _lib.ptr(mission.steps_flown), _lib.ptr(mission.stats), _lib.ptr(sigma_out), _lib.current_stream())
    _lib.check(rc, "fdyn_servo_sched_mission")


def _check(precision, x, schedule, state, sigma_out) -> int:
    n = int(x.shape[1])
    if x.dtype != _lib.state_dtype(precision) or schedule.n != n or state.n != n:
        raise ValueError(f"x must be [12][{schedule.n}] {_lib.state_dtype(precision)}, and the servo state of that fleet")
    if tuple(schedule.table.shape[1:]) != (L.FD_NSS, n) or schedule.table.dtype != torch.float64:
        raise ValueError(f"the schedule's table must be [M][{L.FD_NSS}][{n}] float64, got {tuple(schedule.table.shape)} {schedule.table.dtype}")
    if sigma_out is not None and (tuple(sigma_out.shape) != (2, n) or sigma_out.dtype != torch.float64):
        raise ValueError(f"sigma_out must be [2][{n}] float64, got {tuple(sigma_out.shape)} {sigma_out.dtype}")
    return n

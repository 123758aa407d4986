"""Hybrid cascade fleets: the PID outer loops (mission, waypoint, HSA, attitude) over a learned or a PID rate loop, chosen per
aircraft and switched live.

The reference composes the two by duck typing: `AttitudeAgent` holds its inner loop as `self.rate_agent`
(controllers/attitude_agent.py:67,152), `LearnedRateAgent.compute_action` (controllers/learned_rate_agent.py:128-198) has the
PID `RateAgent`'s signature, and the GUI worker swaps one for the other, resetting both (gui/simulation_worker_learned.py:51-118).
`HybridFleet` is that composition for N aircraft on the device: per control step one policy step on the observations the
previous launch assembled, then one `fdyn_hybrid_step_*` launch (apply the surfaces, RK4, outer loops on the new state, rate
PID on PID lanes, next observation).
"""
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib, layout as L
from .config import FlightControlConfig, cascade_consts, pid_table, waypoint_table
from .fleet import BatchedSixDOF
from .flight_types import ControllerConfig, Waypoint
from .policy import RNNStates

LEVEL_NAMES = {"waypoint": L.FD_LEVEL_WAYPOINT, "hsa": L.FD_LEVEL_HSA, "attitude": L.FD_LEVEL_ATTITUDE}
THROTTLE_SOURCES = {"policy": L.FD_HYBRID_THROTTLE_POLICY, "outer": L.FD_HYBRID_THROTTLE_OUTER}
PREV_ACTION_RESET = (0.0, 0.0, 0.0, 0.5)                     # learned_rate_agent.py:120 / rate_env.py reset
RATE_PID_ROWS = slice(0, 3 * L.FD_NPS)                       # FD_PID_RATE_ROLL..YAW, three state words each


def hybrid_step(fn, level, x, pid_state, wp_idx, type_index, params, n_types, pid_cfg, consts, cmd, wps, n_wp, actions,
                learned, throttle_src, prev_action, obs, rate_cmd, surfaces, reached_total, n, dt):
    """One `fdyn_hybrid_step_*` launch on the current stream (tensors or None)."""
    p = _lib.ptr
    rc = fn(int(level), p(x), p(pid_state), p(wp_idx), p(type_index), p(params), int(n_types), p(pid_cfg), p(consts), p(cmd),
            p(wps), int(n_wp), p(actions), p(learned), int(throttle_src), p(prev_action), p(obs), p(rate_cmd), p(surfaces),
            p(reached_total), int(n), float(dt), _lib.current_stream())
    _lib.check(rc, "hybrid step")


class HybridFleet(BatchedSixDOF):
    """N aircraft under the PID outer loops of `level`; the rate loop of each aircraft is the policy (learned lane) or the PID
    rate agent.  `waypoints` given: every aircraft flies that mission (level "waypoint", wp_idx / reached_total as
    BatchedCascade).  Otherwise the level is commanded per aircraft with `set_command` ([4][N] rows as fdyn_agent_step_*).
    `throttle`: a learned lane flies the policy's throttle ("policy", the reference's LearnedRateAgent under an AttitudeAgent)
    or the outer loop's ("outer").  `dt` is the control step the priming launch of reset() hands the PIDs; run() takes its own."""

    def __init__(self, n: int, policy, level: str = "waypoint", waypoints: Optional[Sequence[Waypoint]] = None,
                 precision: str = "mixed", config: Optional[ControllerConfig] = None,
                 flight_config: Optional[FlightControlConfig] = None, guidance_type: str = "PP",
                 acceptance_radius: Optional[float] = None, on_complete: str = "freeze", throttle: str = "policy",
                 learned=True, types=("rc_plane",), type_index=None, use_graph: bool = False, dt: float = 0.01):
        super().__init__(n, precision, types=types, type_index=type_index)
        if level not in LEVEL_NAMES:
            raise ValueError(f"level must be one of {tuple(LEVEL_NAMES)}")
        if waypoints is not None and level != "waypoint":
            raise ValueError("a waypoint mission needs level='waypoint'")
        if throttle not in THROTTLE_SOURCES:
            raise ValueError(f"throttle must be one of {tuple(THROTTLE_SOURCES)}")
        self.policy, self.level, self.level_id = policy, level, LEVEL_NAMES[level]
        self.throttle_src, self.use_graph, self.dt = THROTTLE_SOURCES[throttle], bool(use_graph), float(dt)
        self.config = config or ControllerConfig()
        dev, n = self.device, self.n
        self.pid_cfg = torch.as_tensor(pid_table(self.config, flight_config), device=dev)
        self.consts = torch.as_tensor(cascade_consts(self.config, flight_config, guidance_type, acceptance_radius, on_complete),
                                      device=dev)
        self.restart = on_complete == "restart"
        if waypoints is not None:
            self.n_wp = len(waypoints)
            self.wps = torch.as_tensor(waypoint_table(waypoints), device=dev)
            self.cmd = None
        else:
            self.n_wp, self.wps = 0, None
            self.cmd = torch.zeros((4, n), dtype=self.dtype, device=dev)
        self.pid_state = torch.zeros((L.FD_NPID * L.FD_NPS, n), dtype=torch.float32, device=dev)
        self.wp_idx = torch.zeros(n, dtype=torch.int32, device=dev)
        self.reached_total = torch.zeros(n, dtype=torch.int32, device=dev)
        self.surfaces = torch.zeros((L.FD_NU, n), dtype=self.dtype, device=dev)
        self.obs = torch.zeros((n, L.FD_OBS_DIM), dtype=torch.float32, device=dev)
        self.rate_cmd = torch.zeros((4, n), dtype=torch.float32, device=dev)
        self.prev_action = torch.zeros((n, L.FD_ACT_DIM), dtype=torch.float32, device=dev)
        self.actions = torch.zeros((n, L.FD_ACT_DIM), dtype=torch.float32, device=dev)   # last raw policy output
        self.learned = torch.ones(n, dtype=torch.uint8, device=dev)
        self.states = policy.initial_state(n, dev)
        with torch.no_grad():
            fused = hasattr(policy, "_fused_ok") and bool(policy._fused_ok(self.obs))
        if fused:
            # the fused path's own dtypes (h bf16, c fp32): its cells read them without a conversion and may update them in place
            self.states = RNNStates(self.states.pi_h.to(torch.bfloat16), self.states.pi_c, self.states.vf_h.to(torch.bfloat16),
                                    self.states.vf_c)
        self._inplace = fused and bool(policy.recurrent_inplace_ok(n, dev))
        self.start = torch.ones(n, dtype=torch.float32, device=dev)
        self.keep = torch.zeros(n, dtype=torch.float32, device=dev)          # 1 - start
        self._fn = getattr(self.lib, f"fdyn_hybrid_step_{precision}")
        self._agent_fn = getattr(self.lib, f"fdyn_agent_step_{precision}")
        self._graph, self._graph_dt = None, None
        self.set_learned(learned, _initial=True)
        self.reset()

    # ---- state ------------------------------------------------------------------------------------------------------------
    def reset(self, x0=None, dt: Optional[float] = None):
        """Aircraft to x0 (default: level flight, 100 m, 20 m/s); PID states, mission progress and the policy state zeroed,
        prev_action = [0, 0, 0, 0.5]; then one priming launch (outer loops + observation, no physics) at `dt`."""
        super().reset(x0)
        if not hasattr(self, "obs"):
            return                                            # BatchedSixDOF.__init__'s own reset
        if dt is not None:
            self.dt = float(dt)
        self.pid_state.zero_(); self.wp_idx.zero_(); self.reached_total.zero_(); self.surfaces.zero_()
        self.prev_action.copy_(torch.tensor(PREV_ACTION_RESET, device=self.device).expand(self.n, 4))
        for t in self.states:
            t.zero_()
        self.start.fill_(1.0); self.keep.zero_()
        self._launch(None, self.dt)

    def set_command(self, cmd):
        """Per-aircraft command of the level ([4] for all, or [4][N]): ATTITUDE roll, pitch, yaw (NaN = none), throttle | HSA
        heading, speed, altitude, - | WAYPOINT north, east, altitude, speed.  The outer loops read it in the next launch (the
        observation in hand was built from the previous command): set it before reset() for the first control step."""
        if self.cmd is None:
            raise ValueError("this fleet flies a waypoint mission; set_command applies to commanded levels")
        c = torch.as_tensor(cmd, dtype=self.dtype, device=self.device)
        if c.ndim == 1:
            c = c[:, None].expand(4, self.n)
        assert c.shape == (4, self.n), "command rows are [4][N]"
        self.cmd.copy_(c)

    def _mask(self, learned) -> torch.Tensor:
        if isinstance(learned, (bool, np.bool_)):
            return torch.full((self.n,), int(learned), dtype=torch.uint8, device=self.device)
        m = torch.as_tensor(learned, device=self.device).reshape(self.n)
        return (m != 0).to(torch.uint8)

    def set_learned(self, learned, _initial: bool = False):
        """Live switch of the rate loop, per aircraft (True / False / mask [N]), with the reference's reset on toggle: lanes that
        become learned start a new policy episode (recurrent state zeroed at the next step, prev_action = [0, 0, 0, 0.5],
        also in the observation in hand); lanes that become PID get zeroed rate-PID states, and the surfaces of the next step are
        recomputed by the rate PID from the rate command in hand.  Outer-loop PID states are kept."""
        new = self._mask(learned)
        if _initial:
            self.learned.copy_(new)
            return
        old = self.learned.bool()
        to_learned, to_pid = new.bool() & ~old, ~new.bool() & old
        self.learned.copy_(new)
        if bool(to_learned.any()):
            pa = torch.tensor(PREV_ACTION_RESET, device=self.device)
            self.start[to_learned] = 1.0
            self.keep[to_learned] = 0.0
            self.prev_action[to_learned] = pa
            self.obs[to_learned, 14:18] = pa
        idx = torch.nonzero(to_pid).flatten()
        if idx.numel():
            self.pid_state[RATE_PID_ROWS, idx] = 0.0
            self._rate_pid_fixup(idx)

    def _rate_pid_fixup(self, idx):
        """The rate PID of lanes `idx` (zeroed state) on the rate command in hand: the surfaces the next launch applies there --
        what the hybrid launch would have written had the lanes been PID lanes when it ran."""
        m = idx.numel()
        xs = self.x[:, idx].contiguous()
        ps = torch.zeros((L.FD_NPID * L.FD_NPS, m), dtype=torch.float32, device=self.device)
        cmd = torch.cat([self.rate_cmd[0:3, idx].to(self.dtype), self.surfaces[L.FD_U_THROTTLE:, idx]]).contiguous()
        surf = torch.empty((L.FD_NU, m), dtype=self.dtype, device=self.device)
        tix = self.type_index[idx].contiguous() if self.type_index is not None else None
        rc = self._agent_fn(L.FD_LEVEL_RATE, _lib.ptr(xs), _lib.ptr(ps), _lib.ptr(tix), _lib.ptr(self.params), self.n_types,
                            _lib.ptr(self.pid_cfg), 0, _lib.ptr(self.consts), _lib.ptr(cmd), m, float(self.dt), 0, _lib.ptr(surf),
                            _lib.current_stream())
        _lib.check(rc, "hybrid rate-PID switch")
        if self.wps is not None and not self.restart:     # a frozen aircraft keeps zero surfaces (as the cascade's surf_out)
            surf = surf * (self.wp_idx[idx] < self.n_wp).to(surf.dtype)
        self.surfaces[:, idx] = surf
        self.pid_state[RATE_PID_ROWS, idx] = ps[RATE_PID_ROWS]

    # ---- stepping -----------------------------------------------------------------------------------------------------------
    def _launch(self, actions, dt):
        hybrid_step(self._fn, self.level_id, self.x, self.pid_state, self.wp_idx, self.type_index, self.params, self.n_types,
                    self.pid_cfg, self.consts, self.cmd, self.wps, self.n_wp, actions, self.learned, self.throttle_src,
                    self.prev_action, self.obs, self.rate_cmd, self.surfaces, self.reached_total if self.wps is not None else None,
                    self.n, dt)

    def _step(self, dt):
        """One control step, device ops only (eager or under graph capture): all state stays in fixed buffers."""
        act, _, _, new_states = self.policy.step(self.obs, self.states, self.start, deterministic=True, keep=self.keep,
                                                 out_states=self.states if self._inplace else None)
        for dst, src in zip(self.states, new_states):
            if dst.data_ptr() != src.data_ptr():
                dst.copy_(src)                                # un-fused policy paths return fresh tensors
        self.start.zero_(); self.keep.fill_(1.0)
        self.actions.copy_(act)
        self._launch(self.actions, dt)

    def apply(self, actions: torch.Tensor, dt: float):
        """One control step with the caller's actions [N, 4] (ail, elev, rud, thr) instead of the policy's: what a learned lane
        applies is this (clipped); PID lanes ignore it."""
        a = torch.as_tensor(actions, dtype=torch.float32, device=self.device)
        assert a.shape == (self.n, L.FD_ACT_DIM)
        self.actions.copy_(a)
        self.dt = float(dt)
        self._launch(self.actions, self.dt)
        self.time += dt

    @torch.no_grad()
    def fused(self) -> bool:
        """True where the policy runs its fused MFMA path on this fleet's observations (inside run(), which needs no gradient)."""
        return bool(self.policy._fused_ok(self.obs))

    @torch.no_grad()
    def run(self, dt: float, n_steps: int):
        """n_steps x {policy step on obs -> hybrid launch}.  use_graph: one control step is captured (after one eager step)
        and replayed."""
        self.dt = float(dt)
        k = 0
        if self.use_graph and n_steps > 0 and (self._graph is None or self._graph_dt != self.dt):
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                self._step(self.dt)                           # warm-up on a side stream: a real control step
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            self._graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self._graph, capture_error_mode="thread_local"):
                self._step(self.dt)
            self._graph_dt = self.dt
            k = 1
        for _ in range(k, n_steps):
            if self.use_graph:
                self._graph.replay()
            else:
                self._step(self.dt)
        self.time += dt * n_steps

    def mission_complete(self) -> torch.Tensor:
        if self.wps is None:
            raise ValueError("no mission: this fleet is commanded with set_command")
        return self.wp_idx >= self.n_wp

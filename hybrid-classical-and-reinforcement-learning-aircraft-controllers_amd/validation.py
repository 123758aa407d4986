"""Physics validation for whole fleets: trajectory-comparison metrics streamed on the device.

Host mirror of the reference's validation suite -- validation/metrics/trajectory_metrics.py:9-208 (the metrics and their
printed summary), validation/scenarios/{base_scenario.py:12-153, level_flight.py:10-94} (scenarios) and
validation/run_validation.py:16-99 (the runner).  The reference flies ONE aircraft on two backends, records both
trajectories in DataFrames and reduces them with NumPy / scipy.  Here the two "backends" are two fleets -- two precisions,
two airframes, two sets of gains -- of up to 65 536 aircraft each, nothing is recorded, and `fdyn_traj_compare`
(csrc/eval_kernels.hip) updates a block of accumulators per aircraft pair from the fleets' own state buffers after every step.
pandas and scipy are not needed; `compare_trajectories` keeps the reference's one-pair signature and runs on the device too.
"""
from abc import ABC, abstractmethod
from typing import Any, Callable, Dict, Optional

import numpy as np
import torch

from . import _lib, layout as L
from .flight_types import AircraftState, ControlSurfaces

# the reference's column names of the compared channels, in FD_TC_* order, and its metric keys in FD_TM_* order
CHANNELS = ("north", "east", "down", "altitude", "u", "v", "w", "airspeed", "roll", "pitch", "yaw", "p", "q", "r")
METRIC_KEYS = tuple(name[len("FD_TM_"):].lower() for name, _ in
                    sorted(((k, v) for k, v in vars(L).items() if k.startswith("FD_TM_")), key=lambda kv: kv[1]))
assert len(CHANNELS) == L.FD_NTC and len(METRIC_KEYS) == L.FD_NTM
_STATE_COLUMNS = ("north", "east", "down", "u", "v", "w", "roll", "pitch", "yaw", "p", "q", "r")       # FD_X_* order
DEFAULT_CHUNK = 16         # steps per launch of TrajectoryComparison: measured faster than 1 at 65 536 pairs


# ---- batched single-channel metrics (trajectory_metrics.py:9-68) on [T][n] tensors, reduced over T -----------------------
def compute_rmse(data1: torch.Tensor, data2: torch.Tensor) -> torch.Tensor:
    return torch.sqrt(torch.mean((data1 - data2) ** 2, dim=0))


def compute_nrmse(data1: torch.Tensor, data2: torch.Tensor) -> torch.Tensor:
    """RMSE as a percentage of the range of data1; 0 where data1 is constant."""
    span = data1.amax(dim=0) - data1.amin(dim=0)
    rmse = compute_rmse(data1, data2)
    return torch.where(span == 0, torch.zeros_like(rmse), rmse / torch.where(span == 0, torch.ones_like(span), span) * 100.0)


def compute_correlation(data1: torch.Tensor, data2: torch.Tensor) -> torch.Tensor:
    """Pearson r per column: 0 with fewer than two samples, NaN where either side is constant, clamped to [-1, 1]."""
    if data1.shape[0] < 2:
        return torch.zeros(data1.shape[1:], dtype=data1.dtype, device=data1.device)
    a, b = data1 - data1.mean(dim=0), data2 - data2.mean(dim=0)
    r = ((a / torch.linalg.vector_norm(a, dim=0)) * (b / torch.linalg.vector_norm(b, dim=0))).sum(dim=0).clamp(-1.0, 1.0)
    constant = (data1 == data1[:1]).all(dim=0) | (data2 == data2[:1]).all(dim=0)
    return torch.where(constant, torch.full_like(r, float("nan")), r)


def compute_max_error(data1: torch.Tensor, data2: torch.Tensor) -> torch.Tensor:
    return (data1 - data2).abs().amax(dim=0)


# ---- the streamed comparison -----------------------------------------------------------------------------------------------
class TrajectoryComparison:
    """All 35 metrics of `compare_trajectories` for n pairs of aircraft, accumulated step by step on the device.

    `update` consumes one step ([12][n]) or a block of steps ([T][12][n]) of both sides; `metrics` finishes [FD_NTM][n].
    With chunk > 1 single steps are staged into a device ring of `chunk` steps that one launch consumes -- the accumulator
    block (FD_NTA words per pair) is then read and written once per `chunk` steps instead of once per step.  Either way the
    result is bit-identical: the kernel adds the steps of a pair in order, one lane per pair."""

    def __init__(self, n: int, device=None, chunk: int = DEFAULT_CHUNK):
        self.lib = _lib.load()
        self.device = device or _lib.require_gpu()
        self.n, self.chunk = int(n), max(1, int(chunk))
        self.acc = torch.zeros((L.FD_NTA, self.n), dtype=torch.float64, device=self.device)
        self._ring, self._sig, self._fill = None, None, 0

    def reset(self):
        self.acc.zero_()
        self._fill = 0

    def _launch(self, xa, da, xb, db, T, out=None):
        rc = self.lib.fdyn_traj_compare(_lib.ptr(xa), int(xa is not None and xa.dtype == torch.float32), _lib.ptr(da),
                                        _lib.ptr(xb), int(xb is not None and xb.dtype == torch.float32), _lib.ptr(db),
                                        int(T), self.n, _lib.ptr(self.acc), _lib.ptr(out), _lib.current_stream())
        _lib.check(rc, "TrajectoryComparison")

    def _side(self, x, d):
        """-> (x [T][12][n], d [T][4][n] or None), contiguous on the device, in the side's own storage type."""
        x = torch.as_tensor(x, device=self.device)
        if x.dtype not in (torch.float32, torch.float64):
            x = x.to(torch.float64)
        x = x.reshape(-1, L.FD_NX, self.n).contiguous()
        if d is not None:
            d = torch.as_tensor(d, device=self.device).to(x.dtype).reshape(x.shape[0], L.FD_ND, self.n).contiguous()
        return x, d

    def update(self, xa, xb, derived_a=None, derived_b=None):
        single = getattr(xa, "ndim", 3) == 2
        xa, da = self._side(xa, derived_a)
        xb, db = self._side(xb, derived_b)
        if xa.shape[0] != xb.shape[0]:
            raise ValueError("both sides must hold the same number of steps")
        if self.chunk == 1 or not single:
            self.flush()
            self._launch(xa, da, xb, db, xa.shape[0])
            return self
        sig = (xa.dtype, xb.dtype, da is not None, db is not None)
        if sig != self._sig:                                    # first use, or the callers changed what they pass
            self.flush()
            new = lambda rows, dt, on: torch.empty((self.chunk, rows, self.n), dtype=dt, device=self.device) if on else None  # noqa: E731
            self._ring = (new(L.FD_NX, xa.dtype, True), new(L.FD_ND, xa.dtype, da is not None),
                          new(L.FD_NX, xb.dtype, True), new(L.FD_ND, xb.dtype, db is not None))
            self._sig = sig
        for ring, src in zip(self._ring, (xa, da, xb, db)):
            if ring is not None:
                ring[self._fill].copy_(src[0])
        self._fill += 1
        if self._fill == self.chunk:
            self.flush()
        return self

    def update_fleets(self, fleet_a, fleet_b):
        """One step of two fleets (BatchedSixDOF, BatchedCascade, HybridFleet; any two precisions): their `x` is read in
        place (chunk = 1) or copied into the ring, airspeed and altitude are derived in the kernel."""
        if fleet_a.n != self.n or fleet_b.n != self.n:
            raise ValueError("fleets and comparison must have the same number of aircraft")
        return self.update(fleet_a.x, fleet_b.x)

    def flush(self):
        if self._fill:
            fill, self._fill = self._fill, 0
            self._launch(*self._ring, fill)

    def metrics(self) -> torch.Tensor:
        """[FD_NTM][n] float64, rows in METRIC_KEYS order."""
        self.flush()
        out = torch.empty((L.FD_NTM, self.n), dtype=torch.float64, device=self.device)
        self._launch(None, None, None, None, 0, out)
        return out

    def as_dict(self, i: int = 0, metrics: Optional[torch.Tensor] = None) -> Dict[str, float]:
        m = (self.metrics() if metrics is None else metrics)[:, i].cpu().tolist()
        return dict(zip(METRIC_KEYS, m))


def _column(traj, name) -> np.ndarray:
    col = traj[name]
    return np.asarray(getattr(col, "values", col), dtype=np.float64)


def compare_trajectories(df_a, df_b) -> Dict[str, Any]:
    """trajectory_metrics.py:71-174 for one pair.  `df_a`, `df_b`: anything indexable by the reference's column names
    (a DataFrame, a dict of arrays); unequal lengths are cut to the shorter.  Returns the same 35 keys as Python floats."""
    dev = _lib.require_gpu()
    a = np.stack([_column(df_a, c) for c in _STATE_COLUMNS + ("airspeed", "altitude")])
    b = np.stack([_column(df_b, c) for c in _STATE_COLUMNS + ("airspeed", "altitude")])
    T = min(a.shape[1], b.shape[1])
    cmp_ = TrajectoryComparison(1, dev)

    def split(m):                                               # -> x [T][12][1], derived [T][FD_ND][1]
        m = torch.as_tensor(np.ascontiguousarray(m[:, :T].T), device=dev)
        d = torch.zeros((T, L.FD_ND, 1), dtype=torch.float64, device=dev)
        d[:, L.FD_D_AIRSPEED, 0], d[:, L.FD_D_ALTITUDE, 0] = m[:, 12], m[:, 13]
        return m[:, :12].reshape(T, L.FD_NX, 1), d
    (xa, da), (xb, db) = split(a), split(b)
    if T:
        cmp_.update(xa, xb, da, db)
    return cmp_.as_dict(0)


_SUMMARY = (("\nPosition Errors:", (("  3D RMSE:      {:8.3f} m", "position_3d_rmse"),
                                    ("  3D Max Error: {:8.3f} m", "position_3d_max_error"),
                                    ("  Altitude RMSE: {:7.3f} m", "altitude_rmse"),
                                    ("  Mean Correlation: {:5.3f}", "mean_position_correlation"))),
            ("\nAttitude Errors:", (("  Roll RMSE:    {:8.3f} deg", "attitude_roll_rmse_deg"),
                                    ("  Pitch RMSE:   {:8.3f} deg", "attitude_pitch_rmse_deg"),
                                    ("  Yaw RMSE:     {:8.3f} deg", "attitude_yaw_rmse_deg"),
                                    ("  Mean Correlation: {:5.3f}", "mean_attitude_correlation"))),
            ("\nOverall:", (("  Overall Correlation: {:5.3f}", "overall_correlation"),)))


def format_metrics_summary(metrics: Dict[str, Any]) -> str:
    """The text block the reference prints for one metrics dict (trajectory_metrics.py:177-208)."""
    bar = "=" * 60
    lines = [bar, "TRAJECTORY COMPARISON METRICS", bar]
    for title, rows in _SUMMARY:
        lines.append(title)
        lines.extend(fmt.format(metrics[key]) for fmt, key in rows)
    lines.append(bar)
    return "\n".join(lines)


# ---- scenarios (validation/scenarios) ---------------------------------------------------------------------------------------
class ValidationScenario(ABC):
    """Initial conditions + a control sequence over time + duration and step (base_scenario.py:12-153)."""

    DT_PHYSICS = 0.001          # the sub-step SimulationAircraftBackend integrates with (its `dt_physics` default)

    def __init__(self, config: Optional[Dict[str, Any]] = None):
        self.config = config or {}
        self.duration = self.config.get("duration", 10.0)
        self.dt = self.config.get("dt", 0.01)

    @abstractmethod
    def get_name(self) -> str: ...

    @abstractmethod
    def get_description(self) -> str: ...

    @abstractmethod
    def get_initial_conditions(self) -> AircraftState: ...

    @abstractmethod
    def get_control_function(self) -> Callable[[float], ControlSurfaces]: ...

    @property
    def num_steps(self) -> int:
        return int(self.duration / self.dt)

    def run_simulation(self, backend):
        """Fly the scenario on one `SimulationAircraftBackend` and return its time series: a DataFrame where pandas is
        installed, else a dict of arrays with the same 19 columns."""
        backend.reset(self.get_initial_conditions())
        control_fn = self.get_control_function()
        cols = ("time",) + CHANNELS + ("elevator", "aileron", "rudder", "throttle")
        rows = np.zeros((self.num_steps, len(cols)))
        for k in range(self.num_steps):
            controls = control_fn(k * self.dt)
            backend.set_controls(controls)
            s = backend.step(self.dt)
            rows[k] = (s.time, *s.position, s.altitude, *s.velocity, s.airspeed, *s.attitude, *s.angular_rate,
                       controls.elevator, controls.aileron, controls.rudder, controls.throttle)
        data = {c: rows[:, j].copy() for j, c in enumerate(cols)}
        try:
            import pandas as pd
        except ImportError:
            return data
        return pd.DataFrame(data)

    def run_fleets(self, fleet_a, fleet_b, comparison: Optional[TrajectoryComparison] = None, x0=None):
        """Fly the scenario on two fleets of equal size side by side and compare them after every step.  Both start from the
        scenario's initial conditions, or from per-aircraft rows x0 [n][12]; fleets without controllers get the scenario's
        controls and the backend's sub-stepping, fleets with a `run` method (cascade, hybrid) fly their own control loop."""
        n = fleet_a.n
        if fleet_b.n != n:
            raise ValueError("both fleets must have the same number of aircraft")
        cmp_ = comparison if comparison is not None else TrajectoryComparison(n, fleet_a.device)
        if x0 is None:
            x0 = np.tile(self.get_initial_conditions().to_vector(), (n, 1))
        control_fn = self.get_control_function()
        for f in (fleet_a, fleet_b):
            f.reset(x0)
        last = None
        for k in range(self.num_steps):
            u = control_fn(k * self.dt).to_array()
            for f in (fleet_a, fleet_b):
                if hasattr(f, "run"):
                    f.run(self.dt, 1)
                    continue
                if last is None or not np.array_equal(u, last):
                    f.set_controls(np.tile(u, (n, 1)))
                f.step(self.dt, self.DT_PHYSICS)
            last = u
            cmp_.update_fleets(fleet_a, fleet_b)
        return cmp_

    def get_expected_metrics(self) -> Dict[str, Any]:
        return {"position_rmse_threshold": 20.0, "attitude_rmse_threshold": 10.0, "min_correlation": 0.80}

    def __repr__(self) -> str:
        return f"{self.get_name()} (duration={self.duration}s, dt={self.dt}s)"


class LevelFlightScenario(ValidationScenario):
    """Trimmed level flight: 100 m, 20 m/s, level attitude, fixed elevator and throttle, no aileron or rudder, 30 s
    (level_flight.py:10-94)."""

    def __init__(self, config: Optional[Dict[str, Any]] = None):
        config = {} if config is None else config
        config.setdefault("duration", 30.0)
        config.setdefault("dt", 0.01)
        super().__init__(config)
        self.trim_elevator = self.config.get("trim_elevator", 0.0)
        self.trim_throttle = self.config.get("trim_throttle", 0.5)

    def get_name(self) -> str:
        return "Level Flight"

    def get_description(self) -> str:
        return "Trimmed level flight at 100m altitude, 20 m/s airspeed. Tests basic aerodynamic equilibrium."

    def get_initial_conditions(self) -> AircraftState:
        return AircraftState(time=0.0, position=np.array([0.0, 0.0, -100.0]), velocity=np.array([20.0, 0.0, 0.0]),
                             attitude=np.zeros(3), angular_rate=np.zeros(3), airspeed=20.0, altitude=100.0,
                             ground_speed=20.0, heading=0.0)

    def get_control_function(self) -> Callable[[float], ControlSurfaces]:
        trim = ControlSurfaces(elevator=self.trim_elevator, aileron=0.0, rudder=0.0, throttle=self.trim_throttle)
        return lambda t: trim

    def get_expected_metrics(self) -> Dict[str, Any]:
        return {"position_rmse_threshold": 5.0, "attitude_rmse_threshold": 2.0, "min_correlation": 0.98}


class TrimmedFlightScenario(ValidationScenario):
    """Steady flight that IS an equilibrium: every fleet is trimmed on the device for its own airframe at `airspeed` (m/s),
    `climb_deg` (flight-path angle, degrees) and `turn_rate` (rad/s) and holds its own trim controls for the whole run
    (hcrl_amd.trim; the reference states the condition in docs/6dof_mathematical_formulation.tex:1380-1410 and codes no
    solver -- its LevelFlightScenario flies hand-picked controls and starts with a transient).  30 s by default."""

    def __init__(self, config: Optional[Dict[str, Any]] = None):
        config = {} if config is None else config
        config.setdefault("duration", 30.0)
        config.setdefault("dt", 0.01)
        super().__init__(config)
        self.airspeed = float(self.config.get("airspeed", 20.0))
        self.climb_deg = float(self.config.get("climb_deg", 0.0))
        self.turn_rate = float(self.config.get("turn_rate", 0.0))
        self.altitude = float(self.config.get("altitude", 100.0))
        self.heading = float(self.config.get("heading", 0.0))
        self.aircraft_type = self.config.get("aircraft_type", "rc_plane")      # the single-aircraft methods' airframe
        self._single = None

    def get_name(self) -> str:
        return "Trimmed Flight"

    def get_description(self) -> str:
        return (f"Steady flight at {self.airspeed:g} m/s, flight-path angle {self.climb_deg:g} deg, turn rate "
                f"{self.turn_rate:g} rad/s from {self.altitude:g} m, each aircraft trimmed for its own airframe.")

    def _condition(self):
        return dict(airspeed=self.airspeed, climb_angle=float(np.radians(self.climb_deg)), turn_rate=self.turn_rate,
                    altitude=self.altitude, heading=self.heading)

    def _solve_single(self):
        if self._single is None:
            from .trim import require_ok, trim_fleet
            res = trim_fleet(1, types=(self.aircraft_type,), **self._condition())
            require_ok(res, "TrimmedFlightScenario")
            self._single = (res.x0[:, 0].cpu().numpy(), res.surfaces(0))
        return self._single

    def get_initial_conditions(self) -> AircraftState:
        x0, _ = self._solve_single()
        return AircraftState.from_vector(x0.copy(), time=0.0)

    def get_control_function(self) -> Callable[[float], ControlSurfaces]:
        _, trim = self._solve_single()
        return lambda t: trim

    def run_fleets(self, fleet_a, fleet_b, comparison: Optional[TrajectoryComparison] = None, x0=None):
        """Trim each fleet for ITS airframe(s), then fly both side by side holding their own controls and compare after every
        step.  Fleets with a `run` method (cascade, hybrid) start from their trim and fly their own control loop.  x0 is not
        accepted: the initial state is the solver's."""
        if x0 is not None:
            raise ValueError("TrimmedFlightScenario computes the initial state of every aircraft itself")
        n = fleet_a.n
        if fleet_b.n != n:
            raise ValueError("both fleets must have the same number of aircraft")
        cmp_ = comparison if comparison is not None else TrajectoryComparison(n, fleet_a.device)
        self.trims = tuple(f.trim(strict=True, **self._condition()) for f in (fleet_a, fleet_b))
        for f in (fleet_a, fleet_b):
            if hasattr(f, "pid_state"):                          # a cascade starts its loops fresh from the trim state
                f.pid_state.zero_(); f.wp_idx.zero_(); f.reached_total.zero_()
        for _ in range(self.num_steps):
            for f in (fleet_a, fleet_b):
                if hasattr(f, "run"):
                    f.run(self.dt, 1)
                else:
                    f.step(self.dt, self.DT_PHYSICS)
            cmp_.update_fleets(fleet_a, fleet_b)
        return cmp_

    def get_expected_metrics(self) -> Dict[str, Any]:
        """Level flight's position and attitude thresholds; no correlation threshold: in steady flight most channels are
        constant, and the correlation of a constant channel is NaN (scipy's pearsonr, and fdyn_traj_compare after it)."""
        return {"position_rmse_threshold": 5.0, "attitude_rmse_threshold": 2.0, "min_correlation": None}


# ---- the runner (validation/run_validation.py:16-99), fleet-wide --------------------------------------------------------------
def spread_initial_conditions(n: int, seed: int = 20261004) -> np.ndarray:
    """Per-aircraft initial states [n][12] drawn over the flight envelope: airspeed 15-30 m/s, altitude 50-200 m, roll and
    pitch within 15 deg, any heading, body rates within 0.1 rad/s."""
    rs = np.random.RandomState(seed)
    x0 = np.zeros((n, L.FD_NX))
    x0[:, L.FD_X_U] = rs.uniform(15.0, 30.0, n)
    x0[:, L.FD_X_D] = -rs.uniform(50.0, 200.0, n)
    x0[:, L.FD_X_ROLL] = rs.uniform(-np.radians(15), np.radians(15), n)
    x0[:, L.FD_X_PITCH] = rs.uniform(-np.radians(15), np.radians(15), n)
    x0[:, L.FD_X_YAW] = rs.uniform(0.0, 2 * np.pi, n)
    x0[:, L.FD_X_P:L.FD_X_R + 1] = rs.uniform(-0.1, 0.1, (n, 3))
    return x0


def run_validation(scenario: ValidationScenario, a: str = "f64", b: str = "mixed", n: int = 65536, type_a: str = "rc_plane",
                   type_b: str = "rc_plane", spread: bool = False, seed: int = 20261004, out=print) -> Dict[str, Any]:
    """Fly `scenario` on a fleet of n `type_a` aircraft in precision `a` and n `type_b` aircraft in precision `b`, compare every
    pair on the device and score the fleet against the scenario's thresholds.  Returns the metrics [FD_NTM][n], the number
    of aircraft passing each criterion and `all_pass`."""
    from .fleet import BatchedSixDOF
    fleet_a, fleet_b = BatchedSixDOF(n, a, types=(type_a,)), BatchedSixDOF(n, b, types=(type_b,))
    bar = "=" * 70
    out(f"{bar}\nPHYSICS VALIDATION: {type_a} [{a}] vs {type_b} [{b}], {n} aircraft\n{bar}")
    out(f"\n   Scenario: {scenario.get_name()}\n   Description: {scenario.get_description()}")
    out(f"   Duration: {scenario.duration}s at {1 / scenario.dt} Hz")
    if spread and isinstance(scenario, TrimmedFlightScenario):
        raise ValueError("spread initial conditions do not apply to a trimmed scenario: every aircraft starts at its trim")
    cmp_ = scenario.run_fleets(fleet_a, fleet_b, x0=spread_initial_conditions(n, seed) if spread else None)
    m = cmp_.metrics()
    row = {k: m[j] for j, k in enumerate(METRIC_KEYS)}
    order = torch.argsort(row["position_3d_rmse"])
    for label, i in (("median", int(order[(n - 1) // 2])), ("worst", int(order[-1]))):
        out(f"\nAircraft {i} ({label} position_3d_rmse):")
        out(format_metrics_summary(cmp_.as_dict(i, m)))
    expected = scenario.get_expected_metrics()
    passing = {"position": row["position_3d_rmse"] < expected["position_rmse_threshold"],
               "attitude": row["attitude_roll_rmse_deg"] < expected["attitude_rmse_threshold"]}
    if expected["min_correlation"] is None:                  # a scenario whose channels are constant by design has no correlation
        passing["correlation"] = torch.ones_like(passing["position"])
    else:
        passing["correlation"] = row["overall_correlation"] > expected["min_correlation"]          # NaN fails, as in the reference
    counts = {k: int(v.sum()) for k, v in passing.items()}
    verdict = lambda k: "PASS" if counts[k] == n else "FAIL"                                      # noqa: E731
    out("\nValidating against expected criteria...")
    out(f"   Position RMSE: {float(row['position_3d_rmse'].max()):.2f}m (threshold: {expected['position_rmse_threshold']}m) "
        f"{verdict('position')} ({counts['position']} of {n})")
    out(f"   Attitude RMSE: {float(row['attitude_roll_rmse_deg'].max()):.2f}° (threshold: {expected['attitude_rmse_threshold']}°) "
        f"{verdict('attitude')} ({counts['attitude']} of {n})")
    if expected["min_correlation"] is None:
        out("   Correlation: not scored (steady flight: constant channels have no correlation)")
    else:
        out(f"   Correlation: {float(row['overall_correlation'].min()):.3f} "
            f"(threshold: {expected['min_correlation']}) {verdict('correlation')} ({counts['correlation']} of {n})")
    all_pass = all(c == n for c in counts.values())
    out(f"\n{bar}\n" + ("VALIDATION PASSED - the two fleets agree within the scenario's thresholds" if all_pass else
                        "Warning: VALIDATION INCOMPLETE - Some metrics outside expected range") + f"\n{bar}")
    return {"metrics": m, "passing": counts, "all_pass": all_pass, "comparison": cmp_}


def main(argv=None) -> int:
    import argparse
    ap = argparse.ArgumentParser(description="Fly one scenario on two fleets and compare every pair of aircraft on the device.")
    ap.add_argument("--a", default="f64", choices=_lib.PRECISIONS)
    ap.add_argument("--b", default="mixed", choices=_lib.PRECISIONS)
    ap.add_argument("--type-a", default="rc_plane")
    ap.add_argument("--type-b", default="rc_plane")
    ap.add_argument("--aircraft", type=int, default=65536)
    ap.add_argument("--duration", type=float, default=None, help="seconds (default: the scenario's 30 s)")
    ap.add_argument("--spread", action="store_true", help="per-aircraft initial conditions over the flight envelope")
    ap.add_argument("--scenario", default="level", choices=("level", "trimmed"),
                    help="level: the reference's fixed controls; trimmed: every fleet solved for its own equilibrium")
    ap.add_argument("--airspeed", type=float, default=20.0, help="trimmed: airspeed (m/s)")
    ap.add_argument("--climb-deg", type=float, default=0.0, help="trimmed: flight-path angle (degrees)")
    ap.add_argument("--turn-rate", type=float, default=0.0, help="trimmed: turn rate (rad/s)")
    args = ap.parse_args(argv)
    config = {} if args.duration is None else {"duration": args.duration}
    if args.scenario == "trimmed":
        scenario = TrimmedFlightScenario(dict(config, airspeed=args.airspeed, climb_deg=args.climb_deg, turn_rate=args.turn_rate))
    else:
        scenario = LevelFlightScenario(config)
    res = run_validation(scenario, args.a, args.b, args.aircraft, args.type_a, args.type_b, args.spread)
    return 0 if res["all_pass"] else 1

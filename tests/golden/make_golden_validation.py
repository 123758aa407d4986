#!/usr/bin/env python3
"""Trajectory-comparison fixtures, from the reference itself: ten pairs of 500-step trajectories flown by the reference's
SimulationAircraftBackend through the reference's ValidationScenario.run_simulation, and the 35 metrics the reference's
compare_trajectories (pandas + scipy) returns for each pair -- for the fp64 trajectories and for the same trajectories
rounded to fp32 and widened again.

Runs only in the build container (needs /root/reference and `make -C oracle ref`); about a minute.
Writes tests/golden/validation_pairs.npz and tests/golden/validation_reference.json.  DATA only (inputs + expected outputs).

The pairs (index, 0-based):
  0      LevelFlightScenario(duration 5), rc_plane against cessna: the lateral channels are exactly constant, so five
         correlations (east, roll, yaw, p, r) and the three means are NaN
  1      the rc_plane trajectory of pair 0 against itself
  2..6   open-loop flights from distinct envelope initial conditions (the draw of tests/test_gpu_parity_scale.py::_cfg2_inputs)
         with constant controls, rc_plane against cessna: every channel varies
  7, 8   sustained aileron and rudder at dt = 0.05: yaw crosses +-180 deg several times, the two sides at different steps
  9      side A of pair 2 against the same flight integrated with dt_physics = 0.002: tiny differences, correlations near 1

Conditioning: every stored pair is also reduced by `streamed_metrics` below -- plain sequential fp64 NumPy in the order the
device kernel accumulates (pivot = first sample, streamed unwrap) -- and must agree with the reference within 1e-13 absolute
for correlations and 1e-13 relative to max(|value|, 1) for everything else, 10x inside the gate of the GPU test.  A draw that
fails is replaced by the next one, never loosened.
"""
import importlib
import json
import os
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = os.environ.get("REFERENCE_ROOT", "/root/reference")
SEED, STEPS = 20261018, 500
CHANNELS = ("north", "east", "down", "altitude", "u", "v", "w", "airspeed", "roll", "pitch", "yaw", "p", "q", "r")
CORRELATED = ("north", "east", "down", "altitude", "roll", "pitch", "yaw", "p", "q", "r")
IN_DEGREES = ("roll", "pitch", "yaw", "p", "q", "r")


def load_reference():
    """The reference's scenario and metric modules by file path: `import validation` would pull in the JSBSim backend."""
    sys.dont_write_bytecode = True
    sys.path.insert(0, os.path.join(REPO, "oracle", "_ref"))
    sys.path.insert(0, REF)
    pkg = types.ModuleType("_ref_scenarios")
    pkg.__path__ = [os.path.join(REF, "validation", "scenarios")]
    sys.modules["_ref_scenarios"] = pkg
    base = importlib.import_module("_ref_scenarios.base_scenario")
    level = importlib.import_module("_ref_scenarios.level_flight")
    spec = importlib.util.spec_from_file_location("_ref_trajectory_metrics",
                                                  os.path.join(REF, "validation", "metrics", "trajectory_metrics.py"))
    metrics = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(metrics)
    return base, level, metrics


def streamed_metrics(a, b):
    """a, b [T][14] (CHANNELS order, radians) -> the 35 metrics, accumulated one step at a time in fp64."""
    ch = {c: j for j, c in enumerate(CHANNELS)}
    deg = np.array([180.0 / np.pi if c in IN_DEGREES else 1.0 for c in CHANNELS])
    ci = np.array([ch[c] for c in CORRELATED])
    k = 0
    ssq, mx = np.zeros(14), np.zeros(14)
    p3_ssq = p3_max = 0.0
    for t in range(len(a)):
        sa, sb = a[t] * deg, b[t] * deg
        if k == 0:
            prev, off = np.array([sa[ch["yaw"]], sb[ch["yaw"]]]), np.zeros(2)
        cur = np.array([sa[ch["yaw"]], sb[ch["yaw"]]])
        dd = cur - prev
        ddmod = np.mod(dd + 180.0, 360.0) - 180.0
        ddmod[(ddmod == -180.0) & (dd > 0)] = 180.0
        corr = ddmod - dd
        corr[np.abs(dd) < 180.0] = 0.0
        off, prev = off + corr, cur
        sa[ch["yaw"]], sb[ch["yaw"]] = cur[0] + off[0], cur[1] + off[1]
        if k == 0:
            piv_a, piv_b = sa[ci].copy(), sb[ci].copy()
            var_a, var_b = np.zeros(10, bool), np.zeros(10, bool)
            su, sv, suu, svv, suv = (np.zeros(10) for _ in range(5))
        e = sa - sb
        ssq += e * e
        mx = np.maximum(mx, np.abs(e))
        pos = np.sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2])
        p3_ssq += pos * pos
        p3_max = max(p3_max, pos)
        u, v = sa[ci] - piv_a, sb[ci] - piv_b
        var_a |= u != 0
        var_b |= v != 0
        su += u; sv += v; suu += u * u; svv += v * v; suv += u * v
        k += 1
    with np.errstate(all="ignore"):
        r = (suv - su * sv / k) / (np.sqrt(suu - su * su / k) * np.sqrt(svv - sv * sv / k))
    r = np.clip(r, -1.0, 1.0)
    r[~(var_a & var_b)] = np.nan
    if k < 2:
        r[:] = 0.0
    rm = np.sqrt(ssq / k)
    cor = dict(zip(CORRELATED, r))
    m = {}
    for ax in ("north", "east", "down"):
        m[f"position_{ax}_rmse"], m[f"position_{ax}_correlation"], m[f"position_{ax}_max_error"] = rm[ch[ax]], cor[ax], mx[ch[ax]]
    m["position_3d_rmse"], m["position_3d_max_error"] = np.sqrt(p3_ssq / k), p3_max
    m["altitude_rmse"], m["altitude_correlation"] = rm[ch["altitude"]], cor["altitude"]
    for ax in ("u", "v", "w"):
        m[f"velocity_{ax}_rmse"] = rm[ch[ax]]
    m["airspeed_rmse"] = rm[ch["airspeed"]]
    for ax in ("roll", "pitch", "yaw"):
        m[f"attitude_{ax}_rmse_deg"], m[f"attitude_{ax}_correlation"], m[f"attitude_{ax}_max_error_deg"] = rm[ch[ax]], cor[ax], mx[ch[ax]]
    for ax in ("p", "q", "r"):
        m[f"rate_{ax}_rmse_dps"], m[f"rate_{ax}_correlation"] = rm[ch[ax]], cor[ax]
    m["mean_position_correlation"] = (cor["north"] + cor["east"] + cor["down"]) / 3.0
    m["mean_attitude_correlation"] = (cor["roll"] + cor["pitch"] + cor["yaw"]) / 3.0
    m["overall_correlation"] = (m["mean_position_correlation"] + m["mean_attitude_correlation"]) / 2.0
    return m


def well_conditioned(want, got):
    """The conditioning gate of the module docstring; also requires the same NaN pattern."""
    worst = 0.0
    for key, w in want.items():
        g = got[key]
        if np.isnan(w) or np.isnan(g):
            if not (np.isnan(w) and np.isnan(g)):
                return False, np.inf
            continue
        err = abs(g - w) if key.endswith("correlation") else abs(g - w) / max(abs(w), 1.0)
        worst = max(worst, err)
    return worst <= 1e-13, worst


def envelope_draw(rs):
    """One row of tests/test_gpu_parity_scale.py::_cfg2_inputs' distribution: initial state and constant controls."""
    x0 = np.zeros(12)
    x0[3] = rs.uniform(15.0, 30.0)
    x0[2] = -rs.uniform(50.0, 200.0)
    x0[6:8] = rs.uniform(-np.radians(15), np.radians(15), 2)
    x0[8] = rs.uniform(0.0, 2 * np.pi)
    x0[9:12] = rs.uniform(-0.1, 0.1, 3)
    u = np.concatenate([rs.uniform(-0.3, 0.3, 3), rs.uniform(0.3, 0.9, 1)])          # elevator, aileron, rudder, throttle
    return x0, u


def main():
    base, level, refm = load_reference()
    import pandas as pd
    from controllers.types import AircraftState, ControlSurfaces
    from simulation import SimulationAircraftBackend

    class OpenLoop(base.ValidationScenario):
        def __init__(self, x0, u, dt=0.01):
            super().__init__({"duration": STEPS * dt + 0.5 * dt, "dt": dt})
            self.x0, self.u = x0, u

        def get_name(self):
            return "Open loop"

        def get_description(self):
            return "constant controls from a drawn initial state"

        def get_initial_conditions(self):
            x = self.x0
            return AircraftState(time=0.0, position=np.array(x[0:3]), velocity=np.array(x[3:6]), attitude=np.array(x[6:9]),
                                 angular_rate=np.array(x[9:12]), airspeed=float(np.linalg.norm(x[3:6])), altitude=float(-x[2]))

        def get_control_function(self):
            c = ControlSurfaces(elevator=self.u[0], aileron=self.u[1], rudder=self.u[2], throttle=self.u[3])
            return lambda t: c

    def fly(scenario, aircraft_type, **cfg):
        df = scenario.run_simulation(SimulationAircraftBackend({"aircraft_type": aircraft_type, **cfg}))
        assert len(df) == STEPS, len(df)
        return df[list(CHANNELS)].values.astype(np.float64)

    def frame(t):
        return pd.DataFrame({c: t[:, j] for j, c in enumerate(CHANNELS)})

    def reference_metrics(a, b):
        with np.errstate(all="ignore"):
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")                                   # scipy's constant-input warning
                return {k: float(v) for k, v in refm.compare_trajectories(frame(a), frame(b)).items()}

    def rounded(t):
        return t.astype(np.float32).astype(np.float64)

    def accept(a, b):
        """-> (metrics of the pair, metrics of the rounded pair, worst conditioning figure) or None."""
        m64, m32 = reference_metrics(a, b), reference_metrics(rounded(a), rounded(b))
        ok64, w64 = well_conditioned(m64, streamed_metrics(a, b))
        ok32, w32 = well_conditioned(m32, streamed_metrics(rounded(a), rounded(b)))
        return (m64, m32, max(w64, w32)) if ok64 and ok32 else None

    def wraps(t):
        return np.flatnonzero(np.abs(np.diff(t[:, CHANNELS.index("yaw")])) > np.pi)

    rs = np.random.RandomState(SEED)
    pairs, draws, notes = [], [], []
    lf = level.LevelFlightScenario({"duration": 5})
    lf_rc, lf_cessna = fly(lf, "rc_plane"), fly(lf, "cessna")
    pairs += [(lf_rc, lf_cessna), (lf_rc, lf_rc.copy())]
    while len(pairs) < 7:                                                         # open loop, every channel varies
        x0, u = envelope_draw(rs)
        a, b = fly(OpenLoop(x0, u), "rc_plane"), fly(OpenLoop(x0, u), "cessna")
        if accept(a, b) is not None and all(np.ptp(t[:, j]) > 0 for t in (a, b) for j in range(14)):
            pairs.append((a, b))
            draws.append((x0, u))
    while len(pairs) < 9:                                                         # spiral: yaw wraps on both sides
        x0, u = envelope_draw(rs)
        x0[8], x0[2] = rs.uniform(2.6, 3.1), -rs.uniform(1500.0, 2000.0)            # room to descend: no ground contact
        u[1], u[2] = rs.uniform(0.5, 0.9), rs.uniform(0.5, 0.9)
        a, b = fly(OpenLoop(x0, u, dt=0.05), "rc_plane"), fly(OpenLoop(x0, u, dt=0.05), "cessna")
        wa, wb = wraps(a), wraps(b)
        if min(a[:, 3].min(), b[:, 3].min()) > 10.0 and len(wa) >= 3 and len(wb) >= 3 and not np.array_equal(wa, wb) and accept(a, b) is not None:
            pairs.append((a, b))
            notes.append(f"pair {len(pairs) - 1}: yaw wraps after steps {wa.tolist()} (A) and {wb.tolist()} (B)")
    for j, (x0, u) in enumerate(draws):                                           # coarser physics step on side B
        a, b = pairs[2 + j][0], fly(OpenLoop(x0, u), "rc_plane", dt_physics=0.002)
        if accept(a, b) is not None:
            pairs.append((a, b))
            notes.append(f"pair 9: side A of pair {2 + j} against dt_physics = 0.002")
            break
    assert len(pairs) == 10

    a = np.stack([p[0] for p in pairs])
    b = np.stack([p[1] for p in pairs])
    res = [accept(p, q) for p, q in zip(a, b)]
    assert all(r is not None for r in res)
    keys = list(res[0][0])
    m64 = np.array([[r[0][k] for k in keys] for r in res])
    m32 = np.array([[r[1][k] for k in keys] for r in res])
    assert np.isnan(m64[0]).sum() == 8 and not np.isnan(m64[2:]).any()
    # Stored compactly: altitude is the negated down column, so 13 channels are kept, as [side][pair][channel][step]; the
    # doubles are split into their eight byte planes (plane p = byte p of every value), which deflate far better than the
    # interleaved bytes.  tests/test_gpu_validation.py::_load_pairs puts them together again.
    assert np.array_equal(a[:, :, 3], -a[:, :, 2]) and np.array_equal(b[:, :, 3], -b[:, :, 2])
    stored = [c for c in CHANNELS if c != "altitude"]
    ab = np.stack([a, b])[:, :, :, [CHANNELS.index(c) for c in stored]].transpose(0, 1, 3, 2)
    planes = np.ascontiguousarray(np.ascontiguousarray(ab).reshape(-1).view(np.uint8).reshape(-1, 8).T)
    path = os.path.join(REPO, "tests", "golden", "validation_pairs.npz")
    np.savez_compressed(path, byte_planes=planes, shape=np.array(ab.shape), channels=np.array(stored), metrics=m64,
                        metrics_rounded=m32, seed=SEED)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.1f} KiB; conditioning worst {max(r[2] for r in res):.2e}")
    for line in notes:
        print(" ", line)

    class Default(OpenLoop):
        def __init__(self):
            base.ValidationScenario.__init__(self)

    def constants(s):
        return {"name": s.get_name(), "description": s.get_description(), "duration": s.duration, "dt": s.dt,
                "expected_metrics": s.get_expected_metrics()}
    lf30 = level.LevelFlightScenario()
    doc = {"METRIC_KEYS": keys, "channels": list(CHANNELS),
           "summary_text": {"2": refm.format_metrics_summary(dict(zip(keys, m64[2]))),
                            "7": refm.format_metrics_summary(dict(zip(keys, m64[7])))},
           "scenarios": {"ValidationScenario": {k: v for k, v in constants(Default()).items() if k not in ("name", "description")},
                         "LevelFlightScenario": dict(constants(lf30), trim_elevator=lf30.trim_elevator,
                                                     trim_throttle=lf30.trim_throttle)},
           "notes": notes}
    jpath = os.path.join(REPO, "tests", "golden", "validation_reference.json")
    with open(jpath, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"wrote {jpath}")


if __name__ == "__main__":
    main()

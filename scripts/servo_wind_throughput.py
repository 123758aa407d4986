#!/usr/bin/env python3
"""What wind and gusts cost the LQ servo and its waypoint missions on the device: the six fdyn_*_wind_* entries beside the still-air
ones, timed in the same run.

65 536 aircraft of both airframes (alternating), the fleet of scripts/servo_throughput.py, trimmed, linearised and designed once;
each aircraft in air of its own (ServoWind.from_disturbances: 0..8 m/s from any direction, +-1 m/s vertical, turbulence 2..8 % of
its airspeed over 100..300 m), started in trim relative to that air.  Then per precision `--steps` control steps in one launch of
  * fdyn_servo_step_*  and  fdyn_servo_step_wind_*        (servo law, RK4) toward the trim's own references,
  * fdyn_servo_mission_*  and  fdyn_servo_mission_wind_*  (mission update, guidance, servo law, RK4) through the project's 300 m square,
the wind entries with the gust normals drawn in the kernel (Philox + Box-Muller, once per control step) and with them replayed
from memory, each timed with device events, eager and as a captured graph, over back-to-back launches after a warm-up of 3; every
carried word is put back to its start before each timed series.

    python scripts/servo_wind_throughput.py [--aircraft 65536] [--steps 100] [--json profiles/servo_wind_throughput_65536.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import hcrl_amd  # noqa: E402,F401
from hcrl_amd import _lib, layout as L  # noqa: E402
from hcrl_amd import servo as SV  # noqa: E402
from hcrl_amd import trim as T  # noqa: E402
from hcrl_amd.config import square_mission  # noqa: E402
from hcrl_amd.disturbances import Disturbances  # noqa: E402
from hcrl_amd.fleet import BatchedSixDOF  # noqa: E402
from servo_throughput import TYPES, graphed, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--aircraft", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--dt", type=float, default=0.01)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    n, dev = args.aircraft, _lib.require_gpu()
    rs = np.random.RandomState(0)
    ty = (np.arange(n) % 2).astype(np.uint8)
    cond = (rs.uniform(15.0, 30.0, n), np.radians(rs.uniform(0.0, 5.0, n)), rs.uniform(-0.1, 0.3, n), rs.uniform(50.0, 200.0, n),
            rs.uniform(0.0, 6.28, n))
    wps = square_mission(300.0, 100.0, 20.0)

    fleet = BatchedSixDOF(n, "f64", types=TYPES, type_index=ty)
    trim = fleet.trim(*cond, strict=False)
    A, B = T.linearize_into(trim.x0, trim.u0, fleet.params, fleet.type_index, None)
    servo = SV.servo_into(A, B, trim.x0, SV.weights_tensor(None, n, dev))
    servo.x0, servo.u0 = trim.x0, trim.u0
    state0 = SV.ServoState.at_trim(trim.x0)
    air = Disturbances(wind_speed=(0.0, 8.0), wind_direction=(0.0, 6.28), wind_vertical=(-1.0, 1.0), turbulence_intensity=(0.02, 0.08),
                       gust_length=(100.0, 300.0))
    wind = SV.ServoWind.from_disturbances(air, n, cond[0], args.dt, dev, np.random.default_rng(0), seed=1)
    rows0, x_air = wind.rows.clone(), wind.ground_state(trim.x0)
    z = torch.randn((args.steps, 3, n), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    res = {"aircraft": n, "steps": args.steps, "dt": args.dt, "repeats": args.repeats, "warmup": 3, "trim_not_ok": trim.count_not_ok(),
           "servo_design_not_ok": servo.count_not_ok()}

    for precision in _lib.PRECISIONS:
        f = BatchedSixDOF(n, precision, types=TYPES, type_index=ty)
        surf = torch.zeros((L.FD_NU, n), dtype=f.dtype, device=dev)
        sat = torch.zeros(n, dtype=torch.int32, device=dev)
        state = SV.ServoState(state0.ref.clone(), state0.integ.clone(), state0.limits, state0.err.clone())
        mission = SV.ServoMission.start(wps, n, dev)
        stats0 = mission.stats.clone()

        def put_back(windy, f=f, state=state, mission=mission, stats0=stats0):
            f.x.copy_(x_air if windy else trim.x0)
            state.ref.copy_(state0.ref)
            state.integ.zero_()
            mission.wp_idx.zero_(); mission.reached_total.zero_(); mission.steps_flown.zero_()
            mission.stats.copy_(stats0)
            wind.rows.copy_(rows0)
            wind.step.zero_()

        def entry(kind, w, zz, f=f, state=state, mission=mission, surf=surf, sat=sat):
            if kind == "mission":
                return lambda: SV.mission_into(f.precision, f.x, servo, state, mission, f.params, f.type_index, args.dt, args.steps, surf, sat,
                                               state.err, wind=w, z=zz)
            return lambda: SV.step_into(f.precision, f.x, servo, state, f.params, f.type_index, args.dt, args.steps, surf, sat, state.err, wind=w, z=zz)

        for kind in ("step", "mission"):
            for tag, w, zz in (("", None, None), ("_wind", wind, None), ("_wind_replayed", wind, z)):
                call, back = entry(kind, w, zz), (lambda w=w: put_back(w is not None))
                res[f"servo_{kind}{tag}_{precision}_us_eager"] = timed(call, args.repeats, back)
                res[f"servo_{kind}{tag}_{precision}_us_graph"] = timed(graphed(call), args.repeats, back)
            for tag in ("_wind", "_wind_replayed"):
                res[f"{kind}{tag}_over_still_{precision}"] = res[f"servo_{kind}{tag}_{precision}_us_graph"] / res[f"servo_{kind}_{precision}_us_graph"]
            res[f"servo_{kind}_wind_{precision}_aircraft_steps_per_s"] = n * args.steps / (res[f"servo_{kind}_wind_{precision}_us_graph"] * 1e-6)
        put_back(True)
        entry("mission", wind, None)()
        torch.cuda.synchronize()
        res[f"servo_mission_wind_{precision}_steps_flown_mean"] = float(mission.steps_flown.double().mean())
        res[f"servo_mission_wind_{precision}_gust_rms"] = float(wind.rows[L.FD_SW_GUST_N:L.FD_SW_GUST_N + 3].pow(2).mean().sqrt())

    print(f"{n} aircraft, {TYPES}, {args.steps} control steps per launch, {args.repeats} launches per figure after 3: "
          f"trim not ok {res['trim_not_ok']}, design not ok {res['servo_design_not_ok']}")
    for p in _lib.PRECISIONS:
        for kind in ("step", "mission"):
            for tag in ("", "_wind", "_wind_replayed"):
                k = f"servo_{kind}{tag}_{p}"
                print(f"  {k:36s} eager {res[k + '_us_eager']:10.1f} us   graph {res[k + '_us_graph']:10.1f} us")
            print(f"  {p} {kind}: wind / still {res[f'{kind}_wind_over_still_{p}']:.3f}, with replayed normals {res[f'{kind}_wind_replayed_over_still_{p}']:.3f}, "
                  f"{res[f'servo_{kind}_wind_{p}_aircraft_steps_per_s']:.3e} aircraft-steps/s")
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()

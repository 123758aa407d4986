#!/usr/bin/env python3
"""What a waypoint mission on the LQ servo costs on the device, beside the plain servo step and the PID cascade timed in the same run.

65 536 aircraft of both airframes (alternating), the fleet of scripts/servo_throughput.py (flight conditions spread over
V = 15..30 m/s, flight-path angle 0..5 deg, turn rate -0.1..0.3 rad/s, altitude 50..200 m), trimmed, linearised and designed
once.  Then per precision `--steps` control steps in one launch of
  * fdyn_servo_mission_*  (mission update, guidance, servo law, RK4) through the project's 300 m square, pure pursuit,
  * fdyn_servo_step_*     (servo law, RK4) toward the trim's own references,
  * fdyn_cascade_step_*   (mission update, guidance, nine PIDs, RK4) through the same square,
each timed with device events, eager and as a captured graph, over back-to-back launches after a warm-up of 3; every carried word
is put back to its start before each timed series.

    python scripts/servo_mission_throughput.py [--aircraft 65536] [--steps 100] [--json profiles/servo_mission_throughput_65536.json]
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
from hcrl_amd.fleet import BatchedCascade, BatchedSixDOF  # noqa: E402
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

        def put_back(f=f, state=state, mission=mission, stats0=stats0):
            f.x.copy_(trim.x0)
            state.ref.copy_(state0.ref)
            state.integ.zero_()
            mission.wp_idx.zero_(); mission.reached_total.zero_(); mission.steps_flown.zero_()
            mission.stats.copy_(stats0)

        fly = lambda f=f, state=state, mission=mission, surf=surf, sat=sat: SV.mission_into(   # noqa: E731
            f.precision, f.x, servo, state, mission, f.params, f.type_index, args.dt, args.steps, surf, sat, state.err)
        step = lambda f=f, state=state, surf=surf, sat=sat: SV.step_into(   # noqa: E731
            f.precision, f.x, servo, state, f.params, f.type_index, args.dt, args.steps, surf, sat, state.err)
        res[f"servo_mission_{precision}_us_eager"] = timed(fly, args.repeats, put_back)
        res[f"servo_mission_{precision}_us_graph"] = timed(graphed(fly), args.repeats, put_back)
        put_back()
        fly()
        torch.cuda.synchronize()
        res[f"servo_mission_{precision}_steps_flown_mean"] = float(mission.steps_flown.double().mean())
        res[f"servo_mission_{precision}_reached_mean"] = float(mission.reached_total.double().mean())
        res[f"servo_step_{precision}_us_eager"] = timed(step, args.repeats, put_back)
        res[f"servo_step_{precision}_us_graph"] = timed(graphed(step), args.repeats, put_back)

        pid = BatchedCascade(n, wps, precision, guidance_type="PP", types=TYPES, type_index=ty)

        def put_back_pid(pid=pid):
            pid.x.copy_(trim.x0)
            pid.pid_state.zero_(); pid.wp_idx.zero_(); pid.reached_total.zero_()

        run = lambda pid=pid: pid.run(args.dt, args.steps)   # noqa: E731
        res[f"cascade_step_{precision}_us_eager"] = timed(run, args.repeats, put_back_pid)
        res[f"cascade_step_{precision}_us_graph"] = timed(graphed(run), args.repeats, put_back_pid)
        res[f"mission_over_servo_step_{precision}"] = res[f"servo_mission_{precision}_us_graph"] / res[f"servo_step_{precision}_us_graph"]
        res[f"mission_over_cascade_step_{precision}"] = res[f"servo_mission_{precision}_us_graph"] / res[f"cascade_step_{precision}_us_graph"]
        res[f"servo_mission_{precision}_aircraft_steps_per_s"] = n * args.steps / (res[f"servo_mission_{precision}_us_graph"] * 1e-6)

    print(f"{n} aircraft, {TYPES}, {args.steps} control steps per launch, {args.repeats} launches per figure after 3: "
          f"trim not ok {res['trim_not_ok']}, design not ok {res['servo_design_not_ok']}")
    for p in _lib.PRECISIONS:
        for k in ("servo_mission", "servo_step", "cascade_step"):
            print(f"  {k + '_' + p:24s} eager {res[f'{k}_{p}_us_eager']:10.1f} us   graph {res[f'{k}_{p}_us_graph']:10.1f} us")
        print(f"  {p}: mission / servo step {res[f'mission_over_servo_step_{p}']:.3f}, mission / cascade step {res[f'mission_over_cascade_step_{p}']:.3f}, "
              f"{res[f'servo_mission_{p}_aircraft_steps_per_s']:.3e} aircraft-steps/s; steps flown per aircraft "
              f"{res[f'servo_mission_{p}_steps_flown_mean']:.1f}, waypoints reached {res[f'servo_mission_{p}_reached_mean']:.2f}")
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What flying a waypoint mission on the servo's ESTIMATE costs on the device, beside the mission on the true state
(fdyn_servo_mission_*) and the servo on noisy sensors without a mission (fdyn_servo_lqg_step_*), timed in the same run.

65 536 aircraft of both airframes (alternating), level trims spread over V = 15..30 m/s and all headings at 100 m: trimmed,
linearised, servo gain and servo filter designed, then one launch of `--steps` control steps of
  * fdyn_servo_lqg_mission_* on the estimate, in-kernel draws, every accumulator, the 300 m square at 100 m;
  * fdyn_servo_mission_* of the same fleet and mission;
  * fdyn_servo_lqg_step_* of the same fleet holding its trim references;
in each precision, eager and as a captured graph, timed with device events over back-to-back launches after a warm-up; every
carried word is put back to its start before each timed series.  No target is set: the figures are reported and written.

    python scripts/servo_lqg_mission_throughput.py [--aircraft 65536] [--steps 100] [--json profiles/servo_lqg_mission_throughput_65536.json]
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
from hcrl_amd import servo_lqg as SL  # noqa: E402
from hcrl_amd import servo_lqg_mission as SM  # noqa: E402
from hcrl_amd import trim as T  # noqa: E402
from hcrl_amd.config import square_mission  # noqa: E402
from hcrl_amd.fleet import BatchedSixDOF  # noqa: E402
from servo_throughput import TYPES, graphed, timed  # noqa: E402

# LDS per 64-lane workgroup of fdyn_servo_lqg_mission_*: CONSTANTS of this script, copied from the code-object metadata for gfx950
# when it was written, not found by the run
LDS_BYTES = {"f64": 45552, "mixed": 63352, "f32": 63352}


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
    fleet = BatchedSixDOF(n, "f64", types=TYPES, type_index=ty)
    trim = fleet.trim(rs.uniform(15.0, 30.0, n), altitude=100.0, heading=rs.uniform(0.0, 6.28, n), strict=False)
    A, B = T.linearize_into(trim.x0, trim.u0, fleet.params, fleet.type_index, None)
    nz = SL.noise_tensor(None, n, dev)
    servo = SV.servo_into(A, B, trim.x0, SV.weights_tensor(None, n, dev))
    servo.x0, servo.u0 = trim.x0, trim.u0
    kalman = SL.servo_kalman_into(A, B, args.dt, nz)
    kalman.sigma = nz[:L.FD_NSKX].clone()
    state0 = SV.ServoState.at_trim(trim.x0)
    pos = SM.ServoPositionFilter.make(dev, dt=args.dt)
    torch.cuda.synchronize()
    res = {"aircraft": n, "steps": args.steps, "dt": args.dt, "trim_not_ok": trim.count_not_ok(), "servo_design_not_ok": servo.count_not_ok(),
           "servo_kf_design_not_ok": kalman.count_not_ok(), "position_gain": pos.gain, "lds_bytes_per_workgroup_script_constants": LDS_BYTES,
           "workgroups_per_cu_by_lds_from_those_constants": {p: 163840 // b for p, b in LDS_BYTES.items()}}
    for precision in _lib.PRECISIONS:
        f = BatchedSixDOF(n, precision, types=TYPES, type_index=ty)
        surf = torch.zeros((L.FD_NU, n), dtype=f.dtype, device=dev)
        sat = torch.zeros(n, dtype=torch.int32, device=dev)
        state = SV.ServoState(state0.ref.clone(), state0.integ.clone(), state0.limits, state0.err.clone())
        q = SL.ServoLqgState.zeros(n, dev, seed=1)
        mission = SV.ServoMission.start(square_mission(300.0, 100.0, 20.0), n, dev)
        m0 = [t.clone() for t in (mission.wp_idx, mission.reached_total, mission.steps_flown, mission.stats)]
        f.x.copy_(trim.x0)
        ps = SM.ServoLqgMissionState.start(f.x)

        def put_back(f=f, state=state, q=q, mission=mission, m0=m0, ps=ps):
            f.x.copy_(trim.x0)
            state.ref.copy_(state0.ref)
            state.integ.zero_()
            q.reset()
            for t, v in zip((mission.wp_idx, mission.reached_total, mission.steps_flown, mission.stats), m0):
                t.copy_(v)
            ps.reset(f.x)

        fly_lm = lambda f=f, state=state, q=q, mission=mission, ps=ps, surf=surf, sat=sat: SM.lqg_mission_into(                # noqa: E731
            f.precision, f.x, servo, kalman, state, q, mission, pos, ps, f.params, f.type_index, args.dt, args.steps, "estimate", None, surf, sat,
            state.err)
        fly_m = lambda f=f, state=state, mission=mission, surf=surf, sat=sat: SV.mission_into(                                  # noqa: E731
            f.precision, f.x, servo, state, mission, f.params, f.type_index, args.dt, args.steps, surf, sat, state.err)
        fly_lqg = lambda f=f, state=state, q=q, surf=surf, sat=sat: SL.lqg_step_into(                                           # noqa: E731
            f.precision, f.x, servo, kalman, state, q, f.params, f.type_index, args.dt, args.steps, "estimate", None, surf, sat, state.err)
        for name, fn in (("servo_lqg_mission", fly_lm), ("servo_mission", fly_m), ("servo_lqg_step", fly_lqg)):
            res[f"{name}_{precision}_us_eager"] = timed(fn, args.repeats, put_back)
            res[f"{name}_{precision}_us_graph"] = timed(graphed(fn), args.repeats, put_back)
        g = lambda name: res[f"{name}_{precision}_us_graph"]   # noqa: E731
        res[f"servo_lqg_mission_over_servo_mission_{precision}"] = g("servo_lqg_mission") / g("servo_mission")
        res[f"servo_lqg_mission_over_servo_lqg_step_{precision}"] = g("servo_lqg_mission") / g("servo_lqg_step")
        res[f"servo_lqg_mission_aircraft_steps_per_s_{precision}"] = n * args.steps / (g("servo_lqg_mission") * 1e-6)
        if precision != "f32":                                  # what the timed flight does: 30 s of the square on the estimate
            put_back()
            for _ in range(int(round(30.0 / (args.dt * args.steps)))):
                fly_lm()
            good = trim.ok & servo.ok & kalman.ok
            res[f"{precision}_first_waypoints_reached_after_30s_median"] = float(mission.reached_total[good].to(torch.float64).median())
            res[f"{precision}_err_pos_ratio_median"] = float(ps.error_ratio()[good].median())
            res[f"{precision}_cross_track_p99_m"] = float(torch.quantile(mission.stats[L.FD_MST_CROSS_TRACK][good], 0.99))

    print(f"{n} aircraft, {TYPES}: trim not ok {res['trim_not_ok']}, servo gain not ok {res['servo_design_not_ok']}, servo filter not ok "
          f"{res['servo_kf_design_not_ok']}; position gain {pos.gain:.4f}")
    for p in _lib.PRECISIONS:
        for k in (f"servo_lqg_mission_{p}", f"servo_mission_{p}", f"servo_lqg_step_{p}"):
            print(f"  {k + '_us':34s} eager {res[k + '_us_eager']:10.1f}   graph {res[k + '_us_graph']:10.1f}   ({args.steps} control steps)")
        print(f"  mission on the estimate / mission on the truth, {p}: {res[f'servo_lqg_mission_over_servo_mission_{p}']:.3f}; / servo LQG step: "
              f"{res[f'servo_lqg_mission_over_servo_lqg_step_{p}']:.3f}; {res[f'servo_lqg_mission_aircraft_steps_per_s_{p}']:.3e} aircraft-steps/s; "
              f"{LDS_BYTES[p]} B of LDS per workgroup, {163840 // LDS_BYTES[p]} workgroups per CU")
    for p in ("f64", "mixed"):
        print(f"  30 s of the square on the estimate ({p}): waypoints reached, median {res[f'{p}_first_waypoints_reached_after_30s_median']:.0f}; "
              f"err_pos[0] / err_pos[1] median {res[f'{p}_err_pos_ratio_median']:.3f}; true cross-track p99 {res[f'{p}_cross_track_p99_m']:.2f} m")
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()

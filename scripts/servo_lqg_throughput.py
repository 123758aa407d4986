#!/usr/bin/env python3
"""What designing and flying the LQ servo on noisy sensors costs on the device, beside the servo on the true state and the
4-state Kalman design timed in the same run.

65 536 aircraft of both airframes (alternating), flight conditions spread over V = 15..30 m/s, flight-path angle 0..5 deg and turn
rate -0.1..0.3 rad/s (scripts/servo_throughput.py's fleet): trimmed, linearised, then
  * one launch of fdyn_servo_kf_design (two 5 x 5 filter Riccati equations per aircraft) beside one launch of fdyn_kf_design (two
    4 x 4) and one of fdyn_servo_design (a 7 x 7 and a 6 x 6) on the same linearisations;
  * one launch of fdyn_servo_lqg_step_* flying `--steps` control steps toward per-aircraft climb, turn and speed commands on the
    estimate with in-kernel draws and all four accumulators, in each precision, beside one launch of fdyn_servo_step_* of the same
    fleet, commands and step count.
Every launch is timed with device events, eager and as a captured graph, over back-to-back launches after a warm-up; the state,
the references, the integrators and the estimator's words are put back to their start before each timed series.

    python scripts/servo_lqg_throughput.py [--aircraft 65536] [--steps 100] [--json profiles/servo_lqg_throughput_65536.json]
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
from hcrl_amd import lqg as G  # noqa: E402
from hcrl_amd import servo as SV  # noqa: E402
from hcrl_amd import servo_lqg as SL  # noqa: E402
from hcrl_amd import trim as T  # noqa: E402
from hcrl_amd.fleet import BatchedSixDOF  # noqa: E402
from servo_throughput import TYPES, graphed, timed  # noqa: E402

# LDS per 64-lane workgroup of fdyn_servo_lqg_step_* and the 160 KB a CU has.  CONSTANTS of this script, copied from the code-object
# metadata for gfx950 when it was written, not found by the run; f64_lds = 41 728 static + 61 440 dynamic
LDS_BYTES = {"f64": 41728, "mixed": 59904, "f32": 59904, "f64_lds": 41728 + 61440}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--aircraft", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--dt", type=float, default=0.01)
    ap.add_argument("--design-repeats", type=int, default=50)
    ap.add_argument("--step-repeats", type=int, default=20)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    n, dev = args.aircraft, _lib.require_gpu()
    rs = np.random.RandomState(0)
    ty = (np.arange(n) % 2).astype(np.uint8)
    cond = (rs.uniform(15.0, 30.0, n), np.radians(rs.uniform(0.0, 5.0, n)), rs.uniform(-0.1, 0.3, n), rs.uniform(50.0, 200.0, n),
            rs.uniform(0.0, 6.28, n))
    commands = dict(heading=rs.uniform(-1.0, 1.0, n), speed=rs.uniform(-3.0, 3.0, n), altitude=rs.uniform(-20.0, 20.0, n))

    fleet = BatchedSixDOF(n, "f64", types=TYPES, type_index=ty)
    trim = fleet.trim(*cond, strict=False)
    A, B = T.linearize_into(trim.x0, trim.u0, fleet.params, fleet.type_index, None)
    w_servo, nz_servo, nz_kf = SV.weights_tensor(None, n, dev), SL.noise_tensor(None, n, dev), G.noise_tensor(None, n, dev)
    servo = SV.servo_into(A, B, trim.x0, w_servo)
    servo.x0, servo.u0 = trim.x0, trim.u0
    kalman = SL.servo_kalman_into(A, B, args.dt, nz_servo)
    kalman.sigma = nz_servo[:L.FD_NSKX].clone()
    kf4 = G.kalman_into(A, B, args.dt, nz_kf)
    torch.cuda.synchronize()
    it = kalman.iters.to(torch.float64)
    res = {"aircraft": n, "steps": args.steps, "dt": args.dt, "trim_not_ok": trim.count_not_ok(), "servo_design_not_ok": servo.count_not_ok(),
           "servo_kf_design_not_ok": kalman.count_not_ok(), "kf_design_not_ok": kf4.count_not_ok(), "servo_kf_iterations_mean": float(it.mean()),
           "servo_kf_iterations_max": int(it.max()), "servo_kf_residual_worst": float(kalman.residual[kalman.ok].max()),
           "lds_bytes_per_workgroup_script_constants": LDS_BYTES,
           "workgroups_per_cu_by_lds_from_those_constants": {p: 163840 // b for p, b in LDS_BYTES.items()}}
    for name, fn in (("servo_kf_design", lambda: SL.servo_kalman_into(A, B, args.dt, nz_servo, kalman)),
                     ("kf_design", lambda: G.kalman_into(A, B, args.dt, nz_kf, kf4)),
                     ("servo_design", lambda: SV.servo_into(A, B, trim.x0, w_servo, servo))):
        res[f"{name}_us_eager"] = timed(fn, args.design_repeats)
        res[f"{name}_us_graph"] = timed(graphed(fn), args.design_repeats)
    res["servo_kf_over_kf_design"] = res["servo_kf_design_us_graph"] / res["kf_design_us_graph"]
    res["servo_kf_design_aircraft_per_s"] = n / (res["servo_kf_design_us_graph"] * 1e-6)

    state0 = SV.ServoState.at_trim(trim.x0)
    state0.command(heading=state0.ref[L.FD_SVR_HEADING].cpu().numpy() + commands["heading"],
                   speed=state0.ref[L.FD_SVR_SPEED].cpu().numpy() + commands["speed"],
                   altitude=state0.ref[L.FD_SVR_ALTITUDE].cpu().numpy() + commands["altitude"])
    for precision in _lib.PRECISIONS:
        f = BatchedSixDOF(n, precision, types=TYPES, type_index=ty)
        surf = torch.zeros((L.FD_NU, n), dtype=f.dtype, device=dev)
        sat = torch.zeros(n, dtype=torch.int32, device=dev)
        state = SV.ServoState(state0.ref.clone(), state0.integ.clone(), state0.limits, state0.err.clone())
        q = SL.ServoLqgState.zeros(n, dev, seed=1)

        def put_back(f=f, state=state, q=q):
            f.x.copy_(trim.x0)
            state.ref.copy_(state0.ref)
            state.integ.zero_()
            q.reset()

        fly = lambda f=f, state=state, surf=surf, sat=sat: SV.step_into(f.precision, f.x, servo, state, f.params, f.type_index, args.dt,   # noqa: E731
                                                                        args.steps, surf, sat, state.err)
        fly_lqg = lambda f=f, state=state, q=q, surf=surf, sat=sat: SL.lqg_step_into(                                                      # noqa: E731
            f.precision, f.x, servo, kalman, state, q, f.params, f.type_index, args.dt, args.steps, "estimate", None, surf, sat, state.err)
        res[f"servo_lqg_step_{precision}_us_eager"] = timed(fly_lqg, args.step_repeats, put_back)
        res[f"servo_lqg_step_{precision}_us_graph"] = timed(graphed(fly_lqg), args.step_repeats, put_back)
        if precision == "f64":                                  # the other placement of the f64 filter: dynamic LDS, same run, same fleet
            fly_lds = lambda f=f, state=state, q=q, surf=surf, sat=sat: SL.lqg_step_into(                                                  # noqa: E731
                f.precision, f.x, servo, kalman, state, q, f.params, f.type_index, args.dt, args.steps, "estimate", None, surf, sat, state.err,
                filter_in_lds=True)
            res["servo_lqg_step_f64_lds_us_eager"] = timed(fly_lds, args.step_repeats, put_back)
            res["servo_lqg_step_f64_lds_us_graph"] = timed(graphed(fly_lds), args.step_repeats, put_back)
            res["f64_filter_placement_faster"] = ("read from the caller's F rows every step (fdyn_servo_lqg_step_f64)"
                                                  if res["servo_lqg_step_f64_us_graph"] <= res["servo_lqg_step_f64_lds_us_graph"]
                                                  else "dynamic LDS (fdyn_servo_lqg_step_f64_lds)")
        if precision != "f32":                                  # what the timed flight does: 40 s toward the commands on the estimate
            put_back(); sat.zero_()
            for _ in range(int(round(40.0 / (args.dt * args.steps)))):
                fly_lqg()
            good = trim.ok & servo.ok & kalman.ok
            e = state.err[:, good].abs()
            for k, name in enumerate(("speed", "altitude", "heading")):
                res[f"{precision}_error_{name}_after_40s_median"] = float(e[k].median())
                res[f"{precision}_error_{name}_after_40s_p99"] = float(torch.quantile(e[k], 0.99))
            ratio = (q.err_est / q.err_meas)[:, good]
            res[f"{precision}_err_est_over_err_meas_median"] = [float(v) for v in ratio.median(dim=1).values]
            res[f"{precision}_err_est_over_err_meas_worst_word_p99"] = float(torch.quantile(ratio.max(dim=0).values, 0.99))
        res[f"servo_step_{precision}_us_eager"] = timed(fly, args.step_repeats, put_back)
        res[f"servo_step_{precision}_us_graph"] = timed(graphed(fly), args.step_repeats, put_back)
        res[f"servo_lqg_over_servo_step_{precision}"] = res[f"servo_lqg_step_{precision}_us_graph"] / res[f"servo_step_{precision}_us_graph"]
        res[f"servo_lqg_aircraft_steps_per_s_{precision}"] = n * args.steps / (res[f"servo_lqg_step_{precision}_us_graph"] * 1e-6)

    print(f"{n} aircraft, {TYPES}: trim not ok {res['trim_not_ok']}, servo filter not ok {res['servo_kf_design_not_ok']} (4-state filter "
          f"{res['kf_design_not_ok']}, servo gain {res['servo_design_not_ok']}), iterations mean {res['servo_kf_iterations_mean']:.2f} max "
          f"{res['servo_kf_iterations_max']}, worst residual {res['servo_kf_residual_worst']:.2e}")
    for k in ("servo_kf_design", "kf_design", "servo_design"):
        print(f"  {k + '_us':34s} eager {res[k + '_us_eager']:10.1f}   graph {res[k + '_us_graph']:10.1f}")
    print(f"  servo filter design / 4-state filter design: {res['servo_kf_over_kf_design']:.2f}; {res['servo_kf_design_aircraft_per_s']:.3e} aircraft/s")
    for p in _lib.PRECISIONS:
        for k in (f"servo_lqg_step_{p}", f"servo_step_{p}"):
            print(f"  {k + '_us':34s} eager {res[k + '_us_eager']:10.1f}   graph {res[k + '_us_graph']:10.1f}   ({args.steps} control steps)")
        print(f"  servo LQG step / servo step, {p}: {res[f'servo_lqg_over_servo_step_{p}']:.3f}; {res[f'servo_lqg_aircraft_steps_per_s_{p}']:.3e} "
              f"aircraft-steps/s; {LDS_BYTES[p]} B of LDS per workgroup, {163840 // LDS_BYTES[p]} workgroups per CU")
    print(f"  f64 filter placement: F rows {res['servo_lqg_step_f64_us_graph']:.1f} us, dynamic LDS {res['servo_lqg_step_f64_lds_us_graph']:.1f} us "
          f"(graph; eager {res['servo_lqg_step_f64_us_eager']:.1f}, {res['servo_lqg_step_f64_lds_us_eager']:.1f}); faster: {res['f64_filter_placement_faster']}")
    for p in ("f64", "mixed"):
        print(f"  40 s toward the commands on the estimate ({p}): " + ", ".join(
            f"|e_{k}| median {res[f'{p}_error_{k}_after_40s_median']:.2e} p99 {res[f'{p}_error_{k}_after_40s_p99']:.2e}"
            for k in ("speed", "altitude", "heading")) + f"; err_est / err_meas, worst word, p99 {res[f'{p}_err_est_over_err_meas_worst_word_p99']:.3f}")
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()

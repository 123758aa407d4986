#!/usr/bin/env python3
"""What designing and flying the LQ servo costs on the device, beside the LQR timed in the same run.

65 536 aircraft of both airframes (alternating), flight conditions spread over V = 15..30 m/s, flight-path angle 0..5 deg and turn
rate -0.1..0.3 rad/s: trimmed, linearised, then
  * one launch of fdyn_servo_design (a 7 x 7 and a 6 x 6 Riccati equation per aircraft) beside one launch of fdyn_lqr_design (two
    4 x 4) on the same linearisations;
  * one launch of fdyn_servo_step_* flying `--steps` control steps toward per-aircraft climb, turn and speed commands, in each
    precision, beside one launch of fdyn_lqr_step_* of the same fleet size and step count from a perturbed start.
Every launch is timed with device events, eager and as a captured graph, over back-to-back launches after a warm-up; the state,
the references and the integrators are put back to their start before each timed series.

    python scripts/servo_throughput.py [--aircraft 65536] [--steps 100] [--json profiles/servo_throughput_65536.json]
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
from hcrl_amd import lqr as Q  # noqa: E402
from hcrl_amd import servo as SV  # noqa: E402
from hcrl_amd import trim as T  # noqa: E402
from hcrl_amd.fleet import BatchedSixDOF  # noqa: E402

TYPES = ("rc_plane", "cessna")
PERTURBATION = {L.FD_X_U: 2.0, L.FD_X_V: 1.0, L.FD_X_W: -1.0, L.FD_X_ROLL: 0.15, L.FD_X_PITCH: 0.08, L.FD_X_P: 0.3, L.FD_X_Q: -0.2,
                L.FD_X_R: 0.1}


def timed(fn, repeats, before=None):
    """Device time of one call in microseconds: `repeats` calls between two events, after a warm-up of 3."""
    for _ in range(3):
        fn()
    if before is not None:
        before()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(repeats):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / repeats


def graphed(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g.replay


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
    w_servo, w_lqr = SV.weights_tensor(None, n, dev), Q.weights_tensor(None, n, dev)
    servo = SV.servo_into(A, B, trim.x0, w_servo)
    lqr = Q.lqr_into(A, B, w_lqr)
    servo.x0 = lqr.x0 = trim.x0
    servo.u0 = lqr.u0 = trim.u0
    torch.cuda.synchronize()
    it = servo.iterations.to(torch.float64)
    res = {"aircraft": n, "steps": args.steps, "dt": args.dt, "trim_not_ok": trim.count_not_ok(), "servo_design_not_ok": servo.count_not_ok(),
           "lqr_design_not_ok": lqr.count_not_ok(), "servo_iterations_mean": float(it.mean()), "servo_iterations_max": int(it.max()),
           "servo_residual_worst": float(servo.residual[servo.ok].max())}
    for name, fn in (("servo_design", lambda: SV.servo_into(A, B, trim.x0, w_servo, servo)), ("lqr_design", lambda: Q.lqr_into(A, B, w_lqr, lqr))):
        res[f"{name}_us_eager"] = timed(fn, args.design_repeats)
        res[f"{name}_us_graph"] = timed(graphed(fn), args.design_repeats)
    res["servo_over_lqr_design"] = res["servo_design_us_graph"] / res["lqr_design_us_graph"]
    res["servo_design_aircraft_per_s"] = n / (res["servo_design_us_graph"] * 1e-6)

    state0 = SV.ServoState.at_trim(trim.x0)
    state0.command(heading=state0.ref[L.FD_SVR_HEADING].cpu().numpy() + commands["heading"],
                   speed=state0.ref[L.FD_SVR_SPEED].cpu().numpy() + commands["speed"],
                   altitude=state0.ref[L.FD_SVR_ALTITUDE].cpu().numpy() + commands["altitude"])
    perturbed = trim.x0.clone()
    for k, v in PERTURBATION.items():
        perturbed[k] += v
    for precision in _lib.PRECISIONS:
        f = BatchedSixDOF(n, precision, types=TYPES, type_index=ty)
        surf = torch.zeros((L.FD_NU, n), dtype=f.dtype, device=dev)
        sat = torch.zeros(n, dtype=torch.int32, device=dev)
        state = SV.ServoState(state0.ref.clone(), state0.integ.clone(), state0.limits, state0.err.clone())

        def put_back(f=f, state=state):
            f.x.copy_(trim.x0)
            state.ref.copy_(state0.ref)
            state.integ.zero_()

        fly = lambda f=f, state=state, surf=surf, sat=sat: SV.step_into(f.precision, f.x, servo, state, f.params, f.type_index, args.dt,   # noqa: E731
                                                                        args.steps, surf, sat, state.err)
        res[f"servo_step_{precision}_us_eager"] = timed(fly, args.step_repeats, put_back)
        res[f"servo_step_{precision}_us_graph"] = timed(graphed(fly), args.step_repeats, put_back)
        if precision == "f64":                                  # what the timed flight does: 40 s toward the commands
            put_back(); sat.zero_()
            for _ in range(int(round(40.0 / (args.dt * args.steps)))):
                fly()
            good = trim.ok & servo.ok
            e = state.err[:, good].abs()
            for k, name in enumerate(("speed", "altitude", "heading")):
                res[f"error_{name}_after_40s_median"] = float(e[k].median())
                res[f"error_{name}_after_40s_p99"] = float(torch.quantile(e[k], 0.99))
            res["saturated_steps_mean"] = float(sat[good].to(torch.float64).mean())
        put_back_lqr = lambda f=f: f.x.copy_(perturbed)                                           # noqa: E731
        fly_lqr = lambda f=f, surf=surf, sat=sat: Q.step_into(f.precision, f.x, lqr, f.params, f.type_index, args.dt, args.steps, surf, sat)  # noqa: E731
        res[f"lqr_step_{precision}_us_eager"] = timed(fly_lqr, args.step_repeats, put_back_lqr)
        res[f"lqr_step_{precision}_us_graph"] = timed(graphed(fly_lqr), args.step_repeats, put_back_lqr)
        res[f"servo_over_lqr_step_{precision}"] = res[f"servo_step_{precision}_us_graph"] / res[f"lqr_step_{precision}_us_graph"]

    print(f"{n} aircraft, {TYPES}: trim not ok {res['trim_not_ok']}, servo design not ok {res['servo_design_not_ok']} (LQR {res['lqr_design_not_ok']}), "
          f"iterations mean {res['servo_iterations_mean']:.2f} max {res['servo_iterations_max']}, worst residual {res['servo_residual_worst']:.2e}")
    for k in ("servo_design_us_eager", "servo_design_us_graph", "lqr_design_us_eager", "lqr_design_us_graph"):
        print(f"  {k:34s} {res[k]:10.1f} us")
    print(f"  servo design / LQR design: {res['servo_over_lqr_design']:.2f}; {res['servo_design_aircraft_per_s']:.3e} aircraft/s")
    for p in _lib.PRECISIONS:
        for k in (f"servo_step_{p}_us_eager", f"servo_step_{p}_us_graph", f"lqr_step_{p}_us_eager", f"lqr_step_{p}_us_graph"):
            print(f"  {k:34s} {res[k]:10.1f} us   ({args.steps} control steps)")
        print(f"  servo step / LQR step, {p}: {res[f'servo_over_lqr_step_{p}']:.3f}")
    print("  40 s toward the commands (f64): " + ", ".join(
        f"|e_{k}| median {res[f'error_{k}_after_40s_median']:.2e} p99 {res[f'error_{k}_after_40s_p99']:.2e}" for k in ("speed", "altitude", "heading"))
        + f"; {res['saturated_steps_mean']:.1f} saturated steps per aircraft")
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()

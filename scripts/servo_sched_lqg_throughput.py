#!/usr/bin/env python3
"""What the scheduled filter costs on the device, beside its two parents' launches timed in the same run.

65 536 aircraft of both airframes (alternating), level trims spread over V = 15..30 m/s, each given a speed command of up to +-3 m/s,
on the default sensor noise under estimate feedback with in-kernel draws:
  * one launch of fdyn_servo_sched_lqg_step_mixed flying `--steps` control steps on a 4-node and on an 8-node pair of tables, entered
    with the estimated airspeed (both tables are read every step) and with the command (read at launch entry only), beside one launch
    of fdyn_servo_lqg_step_mixed (one design, one filter) and one of fdyn_servo_sched_step_mixed (the 4-node table, measured airspeed,
    true state) of the same fleet, ALTERNATING over `--rounds` rounds, every launch a captured graph timed with device events;
  * the M n-lane design of the filter tables (linearise, filter design, reshape) beside the one filter design of the single loop.
The state, the references, the integrators and the estimator's words are put back to their start before each timed series.
Nothing else is measured: no counters, no memory traffic.

    python scripts/servo_sched_lqg_throughput.py [--aircraft 65536] [--steps 100] [--out profiles/servo_sched_lqg_throughput.txt]
"""
import argparse
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
from hcrl_amd import servo_sched as SS  # noqa: E402
from hcrl_amd import servo_sched_lqg as SQ  # noqa: E402
from hcrl_amd.fleet import BatchedSixDOF  # noqa: E402

sys.path.insert(0, os.path.join(REPO, "scripts"))
from servo_throughput import TYPES, graphed, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--aircraft", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--dt", type=float, default=0.01)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--precision", default="mixed")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n, dev, p = args.aircraft, _lib.require_gpu(), args.precision
    rs = np.random.RandomState(0)
    ty = (np.arange(n) % 2).astype(np.uint8)
    V, dV = rs.uniform(15.0, 30.0, n), rs.uniform(-3.0, 3.0, n)
    fleet = BatchedSixDOF(n, p, types=TYPES, type_index=ty)
    trim = fleet.trim(V, strict=False)
    design = fleet.design_servo(strict=False)
    kalman = fleet.design_servo_kalman(args.dt, strict=False)
    x_start, origin = fleet.x.clone(), SQ.origin_of(trim.x0)
    tables = {4: (15.0, 20.0, 25.0, 30.0), 8: tuple(np.linspace(14.0, 31.5, 8))}
    lines, design_us = [], {}

    def design_timed(fn):
        fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(3):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / 3

    design_us[1] = design_timed(lambda: fleet.design_servo_kalman(args.dt, strict=False))
    fleet._servo_kalman = kalman
    scheds, filters = {}, {}
    for M, speeds in tables.items():
        scheds[M] = fleet.design_servo_schedule(speeds, altitude=100.0, heading=0.0, strict=False)
        design_us[M] = design_timed(lambda M=M: SQ.design_servo_kalman_schedule(scheds[M], args.dt, strict=False))
        filters[M] = SQ.design_servo_kalman_schedule(scheds[M], args.dt, strict=False)
    torch.cuda.synchronize()
    lines.append(f"{n} aircraft, {TYPES}, {p}, {args.steps} control steps per launch, dt {args.dt}, estimate feedback, in-kernel draws; trims not ok "
                 f"{trim.count_not_ok()}, designs not ok {design.count_not_ok()}, filters not ok {kalman.count_not_ok()}, filter schedules not ok " +
                 ", ".join(f"M={M}: {f.count_not_ok()}" for M, f in filters.items()))
    for M in (1, 4, 8):
        lines.append(f"  filter design of {M} node(s) per aircraft (linearise + filter design + reshape, eager): {design_us[M]:10.1f} us   "
                     f"x{design_us[M] / design_us[1]:.2f}")

    state0 = SV.ServoState.at_trim(trim.x0)
    state0.command(speed=state0.ref[L.FD_SVR_SPEED].cpu().numpy() + dV)
    state = SV.ServoState(state0.ref.clone(), state0.integ.clone(), state0.limits, state0.err.clone())
    est = SQ.ServoSchedLqgState.zeros(n, dev, seed=1)
    surf, sat = torch.zeros_like(fleet.u), torch.zeros(n, dtype=torch.int32, device=dev)

    def put_back():
        fleet.x.copy_(x_start)
        state.ref.copy_(state0.ref)
        state.integ.zero_()
        est.reset()

    series = {"servo_lqg_step": graphed(lambda: SL.lqg_step_into(p, fleet.x, design, kalman, state, est, fleet.params, fleet.type_index, args.dt,
                                                                 args.steps, "estimate", None, surf, sat, state.err)),
              "servo_sched_step_4_airspeed": graphed(lambda: SS.sched_step_into(p, fleet.x, scheds[4], state, fleet.params, fleet.type_index, args.dt,
                                                                                args.steps, "airspeed", surf, sat, state.err))}
    for M in tables:
        for on in ("airspeed", "command"):
            series[f"sched_lqg_{M}_{on}"] = graphed(lambda M=M, on=on: SQ.sched_lqg_step_into(
                p, fleet.x, scheds[M], filters[M], origin, state, est, fleet.params, fleet.type_index, args.dt, args.steps, "estimate", on, None,
                surf, sat, state.err))
    times = {k: [] for k in series}
    for _ in range(args.rounds):                                 # alternating: every series once per round
        for k, fn in series.items():
            times[k].append(timed(fn, args.repeats, put_back))
    base = float(np.mean(times["servo_lqg_step"]))
    for k, v in times.items():
        lines.append(f"  {k:28s} {np.mean(v):10.1f} us  (rounds {', '.join(f'{t:.1f}' for t in v)})   x{np.mean(v) / base:.3f}")
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

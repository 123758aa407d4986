#!/usr/bin/env python3
"""What the sampled-data servo design costs on the device, beside the continuous design timed in the same run.

65 536 aircraft of both airframes (alternating), level trims spread over V = 15..30 m/s, linearised once; then one launch of
fdyn_servo_design_dt at dt 0.02 and at dt 0.01 beside one launch of fdyn_servo_design on the same A, B, x0 and weights, ALTERNATING
over `--rounds` rounds, every launch a captured graph timed with device events.  There is no target: the figure of merit is the ratio
to fdyn_servo_design, reported as measured.  Nothing else is measured: no counters, no memory traffic.

    python scripts/servo_dt_throughput.py [--aircraft 65536] [--out profiles/servo_dt_throughput.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import hcrl_amd  # noqa: E402,F401
from hcrl_amd import _lib  # noqa: E402
from hcrl_amd import servo as SV  # noqa: E402
from hcrl_amd import trim as T  # noqa: E402
from hcrl_amd.fleet import BatchedSixDOF  # noqa: E402

sys.path.insert(0, os.path.join(REPO, "scripts"))
from servo_throughput import TYPES, graphed, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--aircraft", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n = args.aircraft
    _lib.require_gpu()
    rs = np.random.RandomState(0)
    fleet = BatchedSixDOF(n, "f64", types=TYPES, type_index=(np.arange(n) % 2).astype(np.uint8))
    trim = fleet.trim(rs.uniform(15.0, 30.0, n), strict=False)
    A, B = T.linearize_at_trim(trim, fleet.params, fleet.type_index, None)
    w = SV.weights_tensor(None, n, A.device)
    outs = {"servo_design": SV.servo_into(A, B, trim.x0, w), "servo_design_dt_0.02": SV.servo_dt_into(A, B, trim.x0, w, 0.02),
            "servo_design_dt_0.01": SV.servo_dt_into(A, B, trim.x0, w, 0.01)}
    torch.cuda.synchronize()
    series = {"servo_design": graphed(lambda: SV.servo_into(A, B, trim.x0, w, outs["servo_design"])),
              "servo_design_dt_0.02": graphed(lambda: SV.servo_dt_into(A, B, trim.x0, w, 0.02, outs["servo_design_dt_0.02"])),
              "servo_design_dt_0.01": graphed(lambda: SV.servo_dt_into(A, B, trim.x0, w, 0.01, outs["servo_design_dt_0.01"]))}
    times = {k: [] for k in series}
    for _ in range(args.rounds):                                 # alternating: every series once per round
        for k, fn in series.items():
            times[k].append(timed(fn, args.repeats))
    lines = [f"{n} aircraft, {TYPES}, fp64, default weights, one design launch per call; trims not ok {trim.count_not_ok()}, designs not ok " +
             ", ".join(f"{k}: {d.count_not_ok()}" for k, d in outs.items()) + "; doubling steps at most " +
             ", ".join(f"{k}: {int(d.iterations.max())}" for k, d in outs.items())]
    base = float(np.mean(times["servo_design"]))
    for k, v in times.items():
        lines.append(f"  {k:24s} {np.mean(v):10.1f} us  (rounds {', '.join(f'{t:.1f}' for t in v)})   x{np.mean(v) / base:.3f}")
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

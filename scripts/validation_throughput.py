#!/usr/bin/env python3
"""What the streamed trajectory comparison (hcrl_amd.validation.TrajectoryComparison) costs next to the fleets it watches, and
the closed-loop drift of the mixed-precision cascade from the fp64 one.

Two cascade fleets (f64 and mixed) fly the cfg-3 square mission one control step per launch, three ways: without comparison,
compared after every step with chunk = 1 (the accumulators are read and written every step) and with chunk = 16 (states staged
into a ring, one comparison launch per 16 steps).  Prints the three times per control step, the comparison kernel's traffic per
aircraft and step, and the mixed-against-f64 metrics over the whole flight.

    python scripts/validation_throughput.py [--aircraft 65536] [--steps 1000] [--json out.json]
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
from hcrl_amd import config as cfgmod, layout as L  # noqa: E402
from hcrl_amd.fleet import BatchedCascade  # noqa: E402
from hcrl_amd.flight_types import ControllerConfig  # noqa: E402
from hcrl_amd.validation import METRIC_KEYS, TrajectoryComparison  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--aircraft", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    n, steps, dt = args.aircraft, args.steps, 0.01
    fc = cfgmod.load_controller_config("cascaded_pid.yaml")
    mc = cfgmod.load_mission_config("square_pattern.yaml")
    wps = cfgmod.square_mission(mc.pattern_size, mc.altitude, mc.speed)
    rs = np.random.RandomState(0)
    x0 = np.zeros((n, 12))
    x0[:, 2], x0[:, 3] = -mc.altitude, mc.speed
    x0[:, 0:2] = rs.uniform(-20, 20, (n, 2))
    x0[:, 8] = rs.uniform(-0.1745, 0.1745, n)
    fleets = [BatchedCascade(n, wps, p, ControllerConfig(), fc, guidance_type=mc.guidance, on_complete="restart")
              for p in ("f64", "mixed")]

    def fly(cmp_):
        """Device time of `steps` control steps of both fleets (+ the comparison), in ms per control step."""
        for f in fleets:
            f.reset(x0)
            f.run(dt, 1)
        if cmp_ is not None:
            cmp_.update_fleets(*fleets)                           # warm-up; the measured flight starts fresh
            cmp_.metrics()
            cmp_.reset()
        for f in fleets:
            f.reset(x0)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            for f in fleets:
                f.run(dt, 1)
            if cmp_ is not None:
                cmp_.update_fleets(*fleets)
        if cmp_ is not None:
            cmp_.flush()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / steps

    res = {"aircraft": n, "steps": steps, "dt": dt}
    res["ms_per_step_no_comparison"] = fly(None)
    comparisons = {c: TrajectoryComparison(n, chunk=c) for c in (1, 16)}
    for c, cmp_ in comparisons.items():
        res[f"ms_per_step_chunk_{c}"] = fly(cmp_)
    state_bytes = L.FD_NX * (8 + 8)                               # both fleets keep fp64 state
    res["kernel_bytes_per_aircraft_step"] = {
        "chunk_1": state_bytes + 2 * 8 * L.FD_NTA,
        "chunk_16": state_bytes + 2 * 8 * L.FD_NTA / 16,
        "chunk_16_with_staging": 3 * state_bytes + 2 * 8 * L.FD_NTA / 16}
    m1, m16 = comparisons[1].metrics(), comparisons[16].metrics()
    res["chunked_bit_identical"] = bool(torch.equal(m1.view(torch.int64), m16.view(torch.int64)))
    row = {k: m1[j] for j, k in enumerate(METRIC_KEYS)}
    rmse = row["position_3d_rmse"]
    res["mixed_against_f64"] = {
        "position_3d_rmse_median_m": float(rmse.median()), "position_3d_rmse_worst_m": float(rmse.max()),
        **{f"attitude_{ax}_max_error_deg_worst": float(row[f"attitude_{ax}_max_error_deg"].max()) for ax in ("roll", "pitch", "yaw")},
        "overall_correlation_min": float(row["overall_correlation"].min()), "seconds_flown": steps * dt}
    print(f"{n} aircraft x 2 fleets (f64, mixed), {steps} control steps of {dt} s")
    for key in ("ms_per_step_no_comparison", "ms_per_step_chunk_1", "ms_per_step_chunk_16"):
        print(f"  {key:28s} {res[key] * 1e3:9.1f} us")
    print("  bytes / aircraft / step:", res["kernel_bytes_per_aircraft_step"], " chunked bit-identical:", res["chunked_bit_identical"])
    print("  mixed against f64:", json.dumps(res["mixed_against_f64"]))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()

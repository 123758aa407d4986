#!/usr/bin/env python3
"""Aircraft-control-steps/s of the hybrid cascade (hcrl_amd.hybrid.HybridFleet) on the cfg-3 square mission: PID-only,
all-learned and half/half fleets, eager and graphed, plus the split of one learned control step between the policy's
kernels and the hybrid kernel (each timed alone on the same buffers).

    python scripts/hybrid_throughput.py [--aircraft 65536] [--steps 200] [--precision mixed] [--json out.json]
The policy is a freshly initialised bf16 RateLSTMPolicy: its cost does not depend on its weights.
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
from hcrl_amd import config as cfgmod  # noqa: E402
from hcrl_amd.flight_types import ControllerConfig  # noqa: E402
from hcrl_amd.hybrid import HybridFleet  # noqa: E402
from hcrl_amd.policy import RateLSTMPolicy  # noqa: E402


def timed(fn, steps):
    """Mean device time per call of fn over `steps` calls (events around the whole loop), in ms."""
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--aircraft", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--precision", default="mixed", choices=["f64", "mixed", "f32"])
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    n, dt = args.aircraft, 0.01
    torch.manual_seed(0)
    pol = RateLSTMPolicy(compute_dtype=torch.bfloat16).cuda()
    pol.prepare_inference()
    fc = cfgmod.load_controller_config("cascaded_pid.yaml")
    mc = cfgmod.load_mission_config("square_pattern.yaml")
    wps = cfgmod.square_mission(mc.pattern_size, mc.altitude, mc.speed)
    x0 = np.zeros((n, 12))
    x0[:, 2], x0[:, 3] = -mc.altitude, mc.speed
    rs = np.random.RandomState(0)
    x0[1:, 0:2] = rs.uniform(-20, 20, (n - 1, 2))
    x0[1:, 8] = rs.uniform(-0.1745, 0.1745, n - 1)
    results = {"aircraft": n, "precision": args.precision, "steps": args.steps}
    masks = {"pid_only": False, "all_learned": True, "half_half": np.arange(n) % 2 == 0}
    print(f"{n} aircraft, {args.precision}, {args.steps} control steps per figure")
    for name, learned in masks.items():
        for graph in (False, True):
            f = HybridFleet(n, pol, "waypoint", wps, args.precision, ControllerConfig(), fc, guidance_type=mc.guidance,
                            throttle="outer", learned=learned, use_graph=graph, dt=dt)
            f.reset(x0)
            f.run(dt, 2)                                          # capture (graph) / warm-up
            ms = timed(lambda: f.run(dt, 1), args.steps)
            key = f"{name}_{'graph' if graph else 'eager'}"
            results[key] = {"ms_per_step": ms, "aircraft_steps_per_s": n / (ms * 1e-3), "fused_policy": f.fused()}
            print(f"  {key:20s} {ms * 1e3:8.1f} us / control step   {n / (ms * 1e-3):.3e} aircraft-control-steps/s")
    # the split of one learned control step (all-learned fleet, eager): policy kernels alone, hybrid kernel alone
    f = HybridFleet(n, pol, "waypoint", wps, args.precision, ControllerConfig(), fc, guidance_type=mc.guidance,
                    throttle="outer", learned=True, dt=dt)
    f.reset(x0)
    f.run(dt, 2)
    with torch.no_grad():
        pol_ms = timed(lambda: pol.step(f.obs, f.states, f.start, deterministic=True), args.steps)
    hyb_ms = timed(lambda: f._launch(f.actions, dt), args.steps)
    results["split_all_learned"] = {"policy_ms": pol_ms, "hybrid_kernel_ms": hyb_ms,
                                    "hybrid_share": hyb_ms / (pol_ms + hyb_ms)}
    print(f"  split of a learned control step: policy {pol_ms * 1e3:.1f} us, hybrid kernel {hyb_ms * 1e3:.1f} us "
          f"({100 * hyb_ms / (pol_ms + hyb_ms):.1f} % of the two)")
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()

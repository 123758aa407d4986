#!/usr/bin/env python3
"""Cost of domain randomisation on the rate-env step: the plain entry points against the _dr ones (design-doc ranges) at
65 536 envs, random actions, auto-reset on, device sampling -- `steps` warm-up steps, then one timed region of `steps` steps
(events around the loop), as bench.py's headline does.  Actions are drawn on the device before the timed region.

    python scripts/disturbance_throughput.py [--envs 65536] [--steps 200] [--json profiles/dr_throughput_65536.json]
"""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import hcrl_amd  # noqa: E402,F401
from hcrl_amd.disturbances import Disturbances  # noqa: E402
from hcrl_amd.rate_env import GpuRateVecEnv  # noqa: E402


def run(n, precision, dr, steps):
    env = GpuRateVecEnv(n, "medium", 10.0, 0.02, "step", seed=0, precision=precision,
                        disturbances=Disturbances.design_doc() if dr else None)
    env.reset()
    g = torch.Generator(device=env.device).manual_seed(0)
    acts = (torch.rand((16, n, 4), device=env.device, generator=g) * 2 - 1).contiguous()
    acts[..., 3] = acts[..., 3].abs()
    for k in range(steps):
        env.step_device(acts[k % 16])
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for k in range(steps):
        env.step_device(acts[k % 16])
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    res = {"envs": args.envs, "steps": args.steps, "ranges": Disturbances.design_doc().to_config()}
    for precision in ("mixed", "f64"):
        plain = run(args.envs, precision, False, args.steps)
        dr = run(args.envs, precision, True, args.steps)
        res[precision] = {"plain_ms_per_step": plain, "dr_ms_per_step": dr, "dr_over_plain": dr / plain,
                          "dr_env_steps_per_s": args.envs / (dr * 1e-3)}
        print(f"{precision:6s} plain {plain * 1e3:8.1f} us/step   dr {dr * 1e3:8.1f} us/step   ratio {dr / plain:.3f}")
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()

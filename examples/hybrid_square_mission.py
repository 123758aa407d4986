#!/usr/bin/env python3
"""The cfg-3 square mission (examples/03_waypoint_square_demo.py: pure pursuit, 15 m/s, 100 m, acceptance radius from the
mission file, dt 0.01) flown by ONE fleet in which half the aircraft have the learned rate loop under the PID outer loops and
half the PID rate loop -- the reference's `attitude_agent.rate_agent = LearnedRateAgent(...)` composition, side by side with
the all-PID cascade.  Initial conditions: the SURVEY 8d cfg-3 offsets (N, E ~ U(+-20) m, yaw ~ U(+-10 deg), seed 0).

    python examples/hybrid_square_mission.py --model <model_save_dir>/final_model.pt --aircraft 65536 --precision mixed
Without --model a freshly initialised policy flies (a loud warning says so).  Per group it prints the completion rate, the mean
time to each waypoint, the RMS cross-track error, the RMS surface rate and the crashes (altitude < 0).
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import hcrl_amd  # noqa: E402,F401
from hcrl_amd import config as cfgmod, layout as L  # noqa: E402
from hcrl_amd.flight_types import ControllerConfig  # noqa: E402
from hcrl_amd.hybrid import HybridFleet  # noqa: E402
from hcrl_amd.policy import RateLSTMPolicy  # noqa: E402


def initial_conditions(n, altitude, speed, seed=0):
    """SURVEY 8d cfg 3 (as examples/03_waypoint_square_demo.py): level flight, per-aircraft offsets around the start."""
    x0 = np.zeros((n, L.FD_NX))
    x0[:, L.FD_X_D], x0[:, L.FD_X_U] = -altitude, speed
    if n > 1:
        rs = np.random.RandomState(seed)
        x0[1:, 0:2] = rs.uniform(-20, 20, (n - 1, 2))
        x0[1:, L.FD_X_YAW] = rs.uniform(-0.1745, 0.1745, n - 1)
    return x0


def cross_track(x, wps, idx):
    """Distance of each aircraft from the leg it flies (previous waypoint -> current one), horizontal."""
    w = torch.as_tensor(np.array([[p.north, p.east] for p in wps]), device=x.device, dtype=torch.float64)
    cur = idx.clamp(max=len(wps) - 1).long()
    prev = (cur - 1).clamp(min=0)
    a, b = w[prev], w[cur]
    p = torch.stack([x[L.FD_X_N].double(), x[L.FD_X_E].double()], 1)
    d = b - a
    ln = d.norm(dim=1)
    t = ((p - a) * d).sum(1) / ln.clamp(min=1e-9)
    along = a + d * (t / ln.clamp(min=1e-9)).clamp(0, 1)[:, None]
    return torch.where(ln > 1e-9, (p - along).norm(dim=1), (p - a).norm(dim=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default=None)
    ap.add_argument("--aircraft", type=int, default=65536)
    ap.add_argument("--precision", default="mixed", choices=["f64", "mixed", "f32"])
    ap.add_argument("--max-steps", type=int, default=8000)
    ap.add_argument("--throttle", default="outer", choices=["policy", "outer"])
    args = ap.parse_args()
    n, dt = args.aircraft, 0.01
    if args.model:
        from hcrl_amd.eval_rate import load_policy
        pol = load_policy(args.model)
    else:
        print("#" * 100 + "\n# WARNING: no --model given: the learned half of the fleet flies a FRESHLY INITIALISED (untrained) policy.\n"
              "# Its numbers say nothing about a trained controller.\n" + "#" * 100)
        torch.manual_seed(0)
        pol = RateLSTMPolicy(compute_dtype=torch.bfloat16).cuda()
    pol.prepare_inference()
    fc = cfgmod.load_controller_config("cascaded_pid.yaml")
    mc = cfgmod.load_mission_config("square_pattern.yaml")
    wps = cfgmod.square_mission(mc.pattern_size, mc.altitude, mc.speed)
    learned = np.arange(n) % 2 == 0                                  # interleaved halves: every wave holds both kinds
    fleet = HybridFleet(n, pol, "waypoint", wps, args.precision, ControllerConfig(), fc, guidance_type=mc.guidance,
                        throttle=args.throttle, learned=learned, use_graph=True, dt=dt)
    fleet.reset(initial_conditions(n, mc.altitude, mc.speed))
    dev = fleet.device
    groups = {"learned": torch.as_tensor(learned, device=dev), "pid": torch.as_tensor(~learned, device=dev)}
    n_wp = len(wps)
    arrive = torch.full((n, n_wp), float("nan"), dtype=torch.float64, device=dev)
    xt_sq = torch.zeros(n, dtype=torch.float64, device=dev)
    sr_sq = torch.zeros(n, dtype=torch.float64, device=dev)
    samples = torch.zeros(n, dtype=torch.float64, device=dev)
    crashed = torch.zeros(n, dtype=torch.bool, device=dev)
    arrive[fleet.wp_idx > 0, 0] = 0.0                                  # reached in the priming launch of reset()
    prev_surf = None
    t0 = time.time()
    for k in range(args.max_steps):
        idx_before = fleet.wp_idx.clone()
        fleet.run(dt, 1)
        surf = torch.where(groups["learned"][None], fleet.prev_action.T[[1, 0, 2, 3]].double(), fleet.surfaces.double())
        active = ~fleet.mission_complete()
        if prev_surf is not None:
            rate = ((surf[:3] - prev_surf[:3]) / dt).square().sum(0) / 3
            sr_sq += torch.where(active, rate, torch.zeros_like(rate))
        prev_surf = surf
        xt_sq += torch.where(active, cross_track(fleet.x, wps, fleet.wp_idx).square(), torch.zeros_like(xt_sq))
        samples += active.double()
        crashed |= fleet.x[L.FD_X_D] > 0
        hit = fleet.wp_idx != idx_before
        if bool(hit.any()):
            j = idx_before.clamp(max=n_wp - 1).long()
            arrive[hit, j[hit]] = (k + 1) * dt
        if k % 500 == 0 and bool(fleet.mission_complete().all()):
            break
    torch.cuda.synchronize()
    wall = time.time() - t0
    print(f"{n} aircraft ({int(learned.sum())} learned / {int((~learned).sum())} PID), precision {args.precision}, "
          f"throttle from {args.throttle}, {k + 1} control steps in {wall:.1f} s")
    for name, m in groups.items():
        done = fleet.mission_complete()[m].double().mean().item()
        times = [float(torch.nanmean(arrive[m, j]).item()) for j in range(n_wp)]
        xt = float((xt_sq[m].sum() / samples[m].sum().clamp(min=1)).sqrt())
        sr = float((sr_sq[m].sum() / samples[m].sum().clamp(min=1)).sqrt())
        print(f"  {name:8s} completion {100 * done:6.2f} %   mean time to waypoint [s] "
              + " ".join("   -  " if np.isnan(t) else f"{t:6.2f}" for t in times)
              + f"   RMS cross-track {xt:7.2f} m   RMS surface rate {sr:7.3f} /s   crashes {int(crashed[m].sum())}")


if __name__ == "__main__":
    main()

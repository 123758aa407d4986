#!/usr/bin/env python3
"""What the gain schedule still buys on noisy sensors: the four 15 <-> 30 m/s flights of examples/servo_schedule.py on the sensor
layer's default noise under estimate feedback, flown by
  * the single design at the start speed with its single filter (fdyn_servo_lqg_step_*),
  * the scheduled gains and filters entered with the commanded speed,
  * the scheduled gains and filters entered with the ESTIMATED airspeed
(nodes at 15 / 20 / 25 / 30 m/s, level trims, default weights and noise, dt 0.01, 40 s, the command at t = 1 s, in-kernel draws of
one seed).  All flights of a way are one fleet; everything runs on the device.

    python examples/servo_schedule_noise.py
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hcrl_amd  # noqa: E402,F401
from hcrl_amd import layout as L  # noqa: E402
from hcrl_amd.fleet import BatchedSixDOF  # noqa: E402

FLIGHTS = (("rc_plane", 15.0, 30.0), ("rc_plane", 30.0, 15.0), ("cessna", 15.0, 30.0), ("cessna", 30.0, 15.0))
NODES, DT, PER_LAUNCH = (15.0, 20.0, 25.0, 30.0), 0.01, 10


def fly(how):
    types = ("rc_plane", "cessna")
    fleet = BatchedSixDOF(len(FLIGHTS), "f64", types=types, type_index=[types.index(f[0]) for f in FLIGHTS])
    fleet.trim([f[1] for f in FLIGHTS])
    fleet.design_servo()
    sched = None
    if how == "single":
        fleet.design_servo_kalman(DT)
    else:
        sched = fleet.design_servo_schedule(NODES)
        fleet.design_servo_kalman_schedule(sched, DT)
    est = fleet.servo_lqg if sched is None else fleet.servo_sched_lqg
    on = "command" if how == "command" else "airspeed"
    peak = torch.zeros(fleet.n, dtype=torch.float64, device=fleet.device)
    area = torch.zeros_like(peak)
    for k in range(int(round(40.0 / (DT * PER_LAUNCH)))):
        if k == int(round(1.0 / (DT * PER_LAUNCH))):
            fleet.command_servo(speed=[f[2] for f in FLIGHTS])
        fleet.step_servo_lqg(PER_LAUNCH, "estimate", schedule=sched, on=on)
        e_h = (-fleet.x[L.FD_X_D] - fleet.servo.ref[L.FD_SVR_ALTITUDE]).abs()
        peak, area = torch.maximum(peak, e_h), area + e_h * (DT * PER_LAUNCH)
    return dict(peak=peak.cpu().numpy(), area=area.cpu().numpy(), chatter=est.chatter.sum(dim=0).cpu().numpy(),
                err_est=est.err_est.sum(dim=0).cpu().numpy())


def main():
    ways = ("single", "command", "airspeed")
    out = {how: fly(how) for how in ways}
    print("peak |e_h| (m), the integral of |e_h| (m s), the chatter sum and the err_est sum over 40 s; |e_h| sampled every 10 steps")
    print(f"{'airframe, command':20s}" + "".join(f"{how:>40s}" for how in ways))
    for i, (name, a, b) in enumerate(FLIGHTS):
        print(f"{name + f' {a:.0f} -> {b:.0f}':20s}" + "".join(
            f"{out[how]['peak'][i]:10.3f} {out[how]['area'][i]:8.2f} {out[how]['chatter'][i]:9.3f} {out[how]['err_est'][i]:10.1f}" for how in ways))
    for how in ways[1:]:
        print(f"peak |e_h|, {how} / single: " + ", ".join(f"{v:.3f}" for v in out[how]["peak"] / out["single"]["peak"]) +
              "; chatter: " + ", ".join(f"{v:.3f}" for v in out[how]["chatter"] / out["single"]["chatter"]))
    fleet = BatchedSixDOF(2, "f64", types=("rc_plane", "cessna"), type_index=[0, 1])
    fleet.trim(20.0)
    rep = fleet.design_servo_kalman_schedule(fleet.design_servo_schedule(NODES), DT).frozen_point_report()
    radius = torch.stack([m.spectral_radius().max(dim=0).values for m in rep["poles"]]).max(dim=0).values.reshape(rep["airspeeds"].shape)
    print("frozen-point check of the filters between the nodes (spectral radius of Phi_t (I - L_t); |Phi_t - Phi*|, |Gamma_t - Gamma*| against "
          "the filter designed there):")
    for j, name in enumerate(("rc_plane", "cessna")):
        print(f"  {name}: " + ", ".join(f"{rep['airspeeds'][p, j]:.1f} m/s {radius[p, j]:.4f} {rep['dphi'][p, j]:.1e} {rep['dgamma'][p, j]:.1e}"
                                        for p in range(radius.shape[0])))


if __name__ == "__main__":
    main()

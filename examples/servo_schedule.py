#!/usr/bin/env python3
"""What a gain schedule over airspeed buys on a large speed change: 15 <-> 30 m/s on both airframes, flown by the single design at the
start speed, by the schedule entered with the commanded speed, and by the schedule entered with the measured airspeed (nodes at
15 / 20 / 25 / 30 m/s, level trims, default weights, dt 0.01, 40 s, the command at t = 1 s).  All twelve flights are one fleet per
way; everything runs on the device.

    python examples/servo_schedule.py
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hcrl_amd  # noqa: E402,F401
from hcrl_amd import layout as L  # noqa: E402
from hcrl_amd import servo_sched as SS  # noqa: E402
from hcrl_amd.fleet import BatchedSixDOF  # noqa: E402

FLIGHTS = (("rc_plane", 15.0, 30.0), ("rc_plane", 30.0, 15.0), ("cessna", 15.0, 30.0), ("cessna", 30.0, 15.0))
NODES, DT, PER_LAUNCH = (15.0, 20.0, 25.0, 30.0), 0.01, 10


def fly(how):
    types = ("rc_plane", "cessna")
    fleet = BatchedSixDOF(len(FLIGHTS), "f64", types=types, type_index=[types.index(f[0]) for f in FLIGHTS])
    fleet.trim([f[1] for f in FLIGHTS])
    design = fleet.design_servo()
    sched = SS.ServoSchedule.from_design(design) if how == "single" else fleet.design_servo_schedule(NODES)
    on = "command" if how == "command" else "airspeed"
    peak = torch.zeros(fleet.n, dtype=torch.float64, device=fleet.device)
    area = torch.zeros_like(peak)
    for k in range(int(round(40.0 / (DT * PER_LAUNCH)))):
        if k == int(round(1.0 / (DT * PER_LAUNCH))):
            fleet.command_servo(speed=[f[2] for f in FLIGHTS])
        fleet.step_servo(PER_LAUNCH, DT, schedule=sched, on=on)
        e_h = (-fleet.x[L.FD_X_D] - fleet.servo.ref[L.FD_SVR_ALTITUDE]).abs()
        peak, area = torch.maximum(peak, e_h), area + e_h * (DT * PER_LAUNCH)
    return peak.cpu().numpy(), area.cpu().numpy(), fleet.servo.err.abs().cpu().numpy()


def main():
    ways = ("single", "command", "airspeed")
    out = {how: fly(how) for how in ways}
    print("peak |e_h| (m) and the integral of |e_h| (m s) over 40 s, sampled every 10 steps")
    print(f"{'airframe, command':24s}" + "".join(f"{how:>22s}" for how in ways))
    for i, (name, a, b) in enumerate(FLIGHTS):
        print(f"{name + f' {a:.0f} -> {b:.0f}':24s}" + "".join(f"{out[how][0][i]:12.3f} {out[how][1][i]:9.2f}" for how in ways))
    end = np.max([out[how][2] for how in ways], axis=(0, 2))
    print(f"largest end errors over all flights: |e_V| {end[0]:.3f} m/s, |e_h| {end[1]:.3f} m, |e_psi| {end[2]:.2e} rad")
    modes, V = fleet_modes()
    print("frozen-point check between the nodes (largest real part of the thirteen poles of A - B K, K interpolated):")
    for j, name in enumerate(("rc_plane", "cessna")):
        print(f"  {name}: " + ", ".join(f"{V[p, j]:.1f} m/s {modes[p, j]:+.3f}" for p in range(V.shape[0])))


def fleet_modes():
    fleet = BatchedSixDOF(2, "f64", types=("rc_plane", "cessna"), type_index=[0, 1])
    fleet.trim(20.0)
    m, V = fleet.design_servo_schedule(NODES).frozen_point_modes()
    return m.abscissa().max(dim=0).values.reshape(V.shape).cpu().numpy(), V.cpu().numpy()


if __name__ == "__main__":
    main()

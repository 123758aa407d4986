#!/usr/bin/env python3
"""A fleet under the LQ servo given per-aircraft climb, turn and speed commands: trim -> design_servo -> command_servo -> step_servo.

Sixteen aircraft of both airframes are trimmed level at their own airspeeds; after one second each is told to climb, to turn and
to change speed by its own amounts.  Prints the worst airspeed, altitude and heading errors of the fleet over time, then each
aircraft's command and its errors at the end.  The first aircraft is told to descend 20 m and to slow down at once: it holds zero
throttle, trades the height for speed and waits for drag, so it is the last to arrive -- the servo has no energy management.

    python examples/servo_commands.py [--precision f64] [--seconds 40] [--dt 0.01]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hcrl_amd  # noqa: E402,F401
from hcrl_amd import layout as L  # noqa: E402
from hcrl_amd.fleet import BatchedSixDOF  # noqa: E402

TYPES = ("rc_plane", "cessna")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="f64", choices=("f64", "mixed", "f32"))
    ap.add_argument("--seconds", type=float, default=40.0)
    ap.add_argument("--dt", type=float, default=0.01)
    args = ap.parse_args()
    n = 16
    ty = (np.arange(n) % 2).astype(np.uint8)
    V = np.linspace(16.0, 26.0, n)
    climb = np.linspace(-20.0, 30.0, n)                       # m
    turn = np.radians(np.linspace(-90.0, 90.0, n))            # rad
    faster = np.linspace(-2.0, 4.0, n)                        # m/s

    fleet = BatchedSixDOF(n, args.precision, types=TYPES, type_index=ty)
    fleet.trim(V, altitude=100.0, heading=0.3)
    design = fleet.design_servo()
    print(f"{n} aircraft designed: {int(design.iterations.max())} doubling steps at most, worst residual {float(design.residual.max()):.1e}")
    per_second = int(round(1.0 / args.dt))
    fleet.step_servo(per_second, args.dt)
    fleet.command_servo(heading=0.3 + turn, speed=V + faster, altitude=100.0 + climb)
    print("   t (s)   worst |e_V| (m/s)   worst |e_h| (m)   worst |e_psi| (rad)   saturated steps (mean)")
    for second in range(2, int(round(args.seconds)) + 1):
        fleet.step_servo(per_second, args.dt)
        if second in (2, 3, 5, 8, 12, 16, 20, 25, 30) or second == int(round(args.seconds)):
            e = fleet.servo.err.abs().max(dim=1).values.cpu().numpy()
            print(f"  {second:6d}   {e[L.FD_SVI_SPEED]:17.3e}   {e[L.FD_SVI_ALTITUDE]:15.3e}   {e[L.FD_SVI_HEADING]:19.3e}"
                  f"   {float(fleet.lqr_saturated_steps.double().mean()):22.1f}")
    e = fleet.servo.err.T.cpu().numpy()
    print("\n  aircraft    airframe    dV (m/s)   dh (m)   dpsi (deg)      e_V (m/s)       e_h (m)     e_psi (rad)")
    for i in range(n):
        print(f"  {i:8d}   {TYPES[ty[i]]:>9s}   {faster[i]:9.2f}  {climb[i]:7.1f}  {np.degrees(turn[i]):11.1f}   {e[i, 0]:12.3e}  {e[i, 1]:12.3e}  {e[i, 2]:14.3e}")


if __name__ == "__main__":
    main()

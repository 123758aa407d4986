#!/usr/bin/env python3
"""The LQ servo designed for the loop as it is flown: one fleet, the continuous design and the sampled-data design at dt 0.02, side
by side.

`design_servo()` solves a continuous Riccati equation; every flight kernel then applies that gain through a zero-order hold at dt
with forward-Euler integrators, and at 50 Hz the hold eats most of the margin.  `design_servo(dt=0.02)` puts the hold and the Euler
integrators into the model and solves the discrete Riccati equation instead (include/fdyn_servo_dt.h).  Prints, per (airframe,
airspeed), alpha_s = min sigma_min(I + L_i) of both blocks and the gain margins of the worse one for both designs under truth
feedback at dt 0.02, then flies one command step (+4 m/s, +30 m, +60 deg) for 10 s on each and prints the errors left.

    python examples/servo_sampled_design.py [--dt 0.02]
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
    ap.add_argument("--dt", type=float, default=0.02, help="the control step the loop is flown at")
    args = ap.parse_args()
    speeds = np.array([12.0, 15.0, 18.0, 20.0, 25.0, 30.0])
    ty = np.repeat(np.arange(len(TYPES), dtype=np.uint8), len(speeds))
    V = np.tile(speeds, len(TYPES))
    rows = {}
    for name, dt in (("continuous", None), ("sampled", args.dt)):
        fleet = BatchedSixDOF(len(V), "f64", types=TYPES, type_index=ty)
        fleet.trim(V, 0.0, 0.0)
        design = fleet.design_servo(dt=dt)
        fleet.design_servo_kalman(args.dt)                       # supplies Phi and Gamma at the flown step to the margins
        m = fleet.servo_loop_margins("truth")
        low, high = (v.cpu().numpy() for v in m.gain_margin_db())
        ref = fleet.servo.ref
        fleet.command_servo(heading=ref[L.FD_SVR_HEADING] + np.radians(60.0), speed=ref[L.FD_SVR_SPEED] + 4.0, altitude=ref[L.FD_SVR_ALTITUDE] + 30.0)
        fleet.step_servo(int(round(10.0 / args.dt)), args.dt)
        rows[name] = (m.alpha_s.cpu().numpy(), low, high, fleet.servo.err.abs().cpu().numpy(), int(design.iterations.max()))
    print(f"truth feedback at dt {args.dt}: alpha_s lon / lat [gain margin of the worse block, dB low / high]; then |e_V| m/s, |e_h| m, |e_psi| rad at 10 s")
    print("airframe     V   " + "   ".join(f"{name:62s}" for name in rows))
    for k in range(len(V)):
        cells = []
        for a, low, high, err, _ in rows.values():
            b = int(np.argmin(a[:, k]))
            cells.append(f"{a[0, k]:.3f} / {a[1, k]:.3f} [{low[b, k]:5.2f} / {high[b, k]:4.2f}]   {err[0, k]:.3f} {err[1, k]:.3f} {err[2, k]:.4f}")
        print(f"{TYPES[ty[k]]:9s} {V[k]:5.1f}   " + "   ".join(f"{c:62s}" for c in cells))
    print("doubling steps at most: " + ", ".join(f"{name} {r[4]}" for name, r in rows.items()))


if __name__ == "__main__":
    main()

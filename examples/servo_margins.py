#!/usr/bin/env python3
"""Loop margins of the LQ servo as it is flown: trim -> linearise -> design (servo gain and servo Kalman filter) -> margins, one
aircraft per (airframe, airspeed).

Prints one table over airframe x V: alpha_s = min sigma_min(I + L_i) of the worse block and the gain / phase margins it stands for,
for the servo on the true state (feedback = truth) and on its estimate (feedback = estimate) at dt 0.01 and 0.02.  Then loop recovery
in ONE launch: the first aircraft's filter designed for process-noise rates x 0.1 ... 1e4, one lane per value; as the rates grow the
Kalman gain goes to I (every state is measured) and the estimate loop's alpha_s returns to the true-state loop's.

    python examples/servo_margins.py [--sweep 11]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hcrl_amd  # noqa: E402,F401
from hcrl_amd.fleet import BatchedSixDOF  # noqa: E402
from hcrl_amd.margins import describe_status  # noqa: E402
from hcrl_amd.servo_lqg import DEFAULT_RATES, ServoKalmanNoise  # noqa: E402

TYPES = ("rc_plane", "cessna")


def worse_block(m):
    """-> per aircraft: (alpha_s, gain margin low / high in dB, phase margin in degrees, omega of the minimum, status) of the worse block"""
    a = m.alpha_s.cpu().numpy()
    b = np.nanargmin(np.where(np.isnan(a), np.inf, a), axis=0)
    k = np.arange(a.shape[1])
    low, high = (v.cpu().numpy()[b, k] for v in m.gain_margin_db())
    return a[b, k], low, high, m.phase_margin_deg().cpu().numpy()[b, k], m.omega_s.cpu().numpy()[b, k], m.status.cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweep", type=int, default=11, help="values of the process-noise multiplier between 0.1 and 1e4")
    args = ap.parse_args()
    speeds = np.array([12.0, 15.0, 18.0, 20.0, 25.0, 30.0])
    ty = np.repeat(np.arange(len(TYPES), dtype=np.uint8), len(speeds))
    V = np.tile(speeds, len(TYPES))
    fleet = BatchedSixDOF(len(V), "f64", types=TYPES, type_index=ty)
    fleet.trim(V, 0.0, 0.0, strict=False)
    fleet.design_servo(strict=False)
    print("alpha_s of the worse block [gain margin dB low / high, phase margin deg] @ rad/s")
    print("airframe     V   " + "   ".join(f"{name} dt {dt:<21g}" for dt in (0.01, 0.02) for name in ("truth", "estimate")))
    cells = []
    for dt in (0.01, 0.02):
        fleet.design_servo_kalman(dt, strict=False)
        for fb in ("truth", "estimate"):
            cells.append(worse_block(fleet.servo_loop_margins(fb)))
    for k in range(len(V)):
        row = []
        for a, low, high, pm, w, st in cells:
            row.append(f"{a[k]:.3f} [{low[k]:5.1f} / {high[k]:4.1f}, {pm[k]:4.1f}] @ {w[k]:6.1f}" if st[k] in (0,) else f"{describe_status(st[k]):33s}")
        print(f"{TYPES[ty[k]]:9s} {V[k]:5.1f}   " + "   ".join(row))

    # loop recovery: one aircraft, one lane per process-noise multiplier, one launch of each kernel
    mult = np.geomspace(0.1, 1.0e4, args.sweep)
    one = BatchedSixDOF(len(mult), "f64", types=TYPES[:1])
    one.trim(20.0, 0.0, 0.0)
    one.design_servo()
    one.design_servo_kalman(0.01, ServoKalmanNoise(rates=tuple(r * mult for r in DEFAULT_RATES)), strict=False)
    est, tru = one.servo_loop_margins("estimate"), one.servo_loop_margins("truth")
    a_e, a_t = est.alpha_s.cpu().numpy(), tru.alpha_s.cpu().numpy()
    print(f"\nloop recovery, {TYPES[0]} at 20 m/s, dt 0.01: process-noise rates x m")
    print("        m   alpha_s estimate lon / lat   truth lon / lat          difference              status")
    for k, m in enumerate(mult):
        print(f"{m:9.3g}   {a_e[0, k]:.6f} / {a_e[1, k]:.6f}      {a_t[0, k]:.6f} / {a_t[1, k]:.6f}      {abs(a_e[0, k] - a_t[0, k]):.1e} / {abs(a_e[1, k] - a_t[1, k]):.1e}"
              f"      {describe_status(int(est.status[k]))}")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Trim table and modes of an airframe: the steady-flight solver and the linearisation on a handful of aircraft.

Prints, for V x flight-path angle, the angle of attack, elevator and throttle that hold the aircraft there (and why not where
nothing does), then the eigenvalues of the longitudinal (u, w, q, theta) and lateral (v, p, r, phi) blocks of the linear model
at each level-flight trim -- short period, phugoid, roll, spiral and Dutch roll -- computed by NumPy on the host.

    python examples/trim_envelope.py [--type rc_plane] [--turn-rate 0.0]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hcrl_amd  # noqa: E402,F401
from hcrl_amd import layout as L  # noqa: E402
from hcrl_amd.fleet import BatchedSixDOF  # noqa: E402
from hcrl_amd.trim import describe_status, lateral_block, longitudinal_block  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--type", default="rc_plane")
    ap.add_argument("--turn-rate", type=float, default=0.0)
    args = ap.parse_args()
    speeds, climbs = np.array([10.0, 12.0, 15.0, 20.0, 25.0, 30.0, 35.0, 40.0]), np.array([-5.0, 0.0, 3.0, 5.0, 8.0])
    V, G = (a.reshape(-1) for a in np.meshgrid(speeds, climbs, indexing="ij"))
    fleet = BatchedSixDOF(len(V), "f64", types=(args.type,))
    res = fleet.trim(V, np.radians(G), args.turn_rate, strict=False)
    alpha, u0, status = np.degrees(res.alpha.cpu().numpy()), res.u0.cpu().numpy(), res.status.cpu().numpy()
    print(f"{args.type}, turn rate {args.turn_rate:g} rad/s: alpha (deg) / elevator / throttle")
    print("  V \\ gamma " + "".join(f"{g:>22.0f} deg" for g in climbs))
    for i, v in enumerate(speeds):
        cells = []
        for j in range(len(climbs)):
            k = i * len(climbs) + j
            cells.append(f"{alpha[k]:6.2f} {u0[L.FD_U_ELEVATOR, k]:6.3f} {u0[L.FD_U_THROTTLE, k]:6.3f} {'  ok ' if status[k] == 0 else ' [' + str(status[k]) + '] '}")
        print(f"  {v:5.1f} m/s  " + " ".join(cells))
    for s in sorted(set(status.tolist()) - {0}):
        print(f"  [{s}] = {describe_status(s)}")
    A, B = fleet.linearize()
    (Al, _), (Ad, _) = longitudinal_block(A, B), lateral_block(A, B)
    Al, Ad = Al.permute(2, 0, 1).cpu().numpy(), Ad.permute(2, 0, 1).cpu().numpy()
    np.set_printoptions(precision=3, suppress=True, linewidth=160)
    print("\neigenvalues at the level-flight trims (1/s):")
    for i, v in enumerate(speeds):
        k = i * len(climbs) + int(np.flatnonzero(climbs == 0.0)[0])
        if status[k] & (L.FD_TRIM_NOT_CONVERGED | L.FD_TRIM_BAD_SPEC):
            continue
        print(f"  {v:5.1f} m/s  longitudinal {np.linalg.eigvals(Al[k])}   lateral {np.linalg.eigvals(Ad[k])}")


if __name__ == "__main__":
    main()

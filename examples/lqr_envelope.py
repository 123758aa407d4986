#!/usr/bin/env python3
"""Gain schedule of an LQR over the flight envelope: trim -> linearise -> design, one aircraft per (airframe, airspeed).

Prints, per airframe and airspeed, the certified gains of the longitudinal block (elevator and throttle from u, w, q, theta)
and of the lateral block (aileron and rudder from v, p, r, phi) with the open- and closed-loop poles of each block and of the
coupled 8-state model -- the eigenvalues are NumPy's, on the host, for the table only: the design certifies stability per
aircraft without them (status 0).

    python examples/lqr_envelope.py [--turn-rate 0.0] [--theta-max 0.1]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hcrl_amd  # noqa: E402,F401
from hcrl_amd import layout as L  # noqa: E402
from hcrl_amd.fleet import BatchedSixDOF  # noqa: E402
from hcrl_amd.lqr import LqrWeights, describe_status  # noqa: E402
from hcrl_amd.trim import (LATERAL_STATES, LONGITUDINAL_STATES, lateral_block, longitudinal_block)  # noqa: E402

TYPES = ("rc_plane", "cessna")


def worst(ev):
    return float(np.max(ev.real))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--turn-rate", type=float, default=0.0)
    ap.add_argument("--theta-max", type=float, default=0.1, help="Bryson maximum of the pitch excursion (rad)")
    args = ap.parse_args()
    speeds = np.array([12.0, 15.0, 18.0, 20.0, 25.0, 30.0])
    ty = np.repeat(np.arange(len(TYPES), dtype=np.uint8), len(speeds))
    V = np.tile(speeds, len(TYPES))
    fleet = BatchedSixDOF(len(V), "f64", types=TYPES, type_index=ty)
    trim = fleet.trim(V, 0.0, args.turn_rate, strict=False)
    design = fleet.design_lqr(LqrWeights(theta=args.theta_max), strict=False)
    A, B = fleet.linearize()
    closed = design.closed_loop(A, B).permute(2, 0, 1).cpu().numpy()
    (Al, _), (Ad, _) = longitudinal_block(A, B), lateral_block(A, B)
    Al, Ad = Al.permute(2, 0, 1).cpu().numpy(), Ad.permute(2, 0, 1).cpu().numpy()
    K, status, tstatus = design.K.T.cpu().numpy(), design.status.cpu().numpy(), trim.status.cpu().numpy()
    iters, res = design.iterations.cpu().numpy(), design.residual.cpu().numpy()
    lon, lat = list(LONGITUDINAL_STATES), list(LATERAL_STATES)
    np.set_printoptions(precision=3, suppress=True, linewidth=170)
    for t, name in enumerate(TYPES):
        print(f"\n{name}, turn rate {args.turn_rate:g} rad/s, level flight")
        for k in np.flatnonzero(ty == t):
            if tstatus[k] & (L.FD_TRIM_NOT_CONVERGED | L.FD_TRIM_BAD_SPEC) or status[k]:
                print(f"  {V[k]:5.1f} m/s  no gain: {describe_status(status[k])}")
                continue
            cl = closed[k]
            print(f"  {V[k]:5.1f} m/s  {iters[k]} doubling steps, residual {res[k]:.1e}")
            print(f"      elevator <- u w q theta {K[k, 0:4]}   throttle <- {K[k, 4:8]}")
            print(f"      aileron  <- v p r phi   {K[k, 8:12]}   rudder   <- {K[k, 12:16]}")
            print(f"      worst pole (1/s): longitudinal {worst(np.linalg.eigvals(Al[k])):7.3f} -> {worst(np.linalg.eigvals(cl[np.ix_(lon, lon)])):7.3f}"
                  f"   lateral {worst(np.linalg.eigvals(Ad[k])):7.3f} -> {worst(np.linalg.eigvals(cl[np.ix_(lat, lat)])):7.3f}"
                  f"   coupled 8-state -> {worst(np.linalg.eigvals(cl[np.ix_(lon + lat, lon + lat)])):7.3f}")


if __name__ == "__main__":
    main()

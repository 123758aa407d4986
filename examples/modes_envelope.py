#!/usr/bin/env python3
"""Flight modes over the flight envelope, every pole taken on the device: trim -> linearise -> design -> MODES.

Part 1, one aircraft per (airframe, airspeed), the table of examples/lqr_envelope.py: per block the open-loop poles, the poles under
the default LQR, and the sampled loop Phi - Gamma K at dt 0.01 and 0.02 brought back to the s-plane (ln z / dt) -- frequency,
damping ratio and time to double (or time constant) per mode.  The report is generic: these airframes have no yaw stiffness and
so no dutch roll, and most of their phugoids are unstable; nothing here is a slot named after a classical mode.

Part 2, a weight sweep, the use the report exists for: N weight sets on one flight condition, one launch each of design -> modes
-> margins; the sets whose closed loop has min_damping >= 0.6 in both blocks, ranked by the disk margin alpha of the LQG loop.

    python examples/modes_envelope.py [--turn-rate 0.0] [--sets 4096] [--airspeed 20] [--top 8]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hcrl_amd  # noqa: E402,F401
from hcrl_amd import lqr as Q  # noqa: E402
from hcrl_amd.fleet import BatchedSixDOF  # noqa: E402
from hcrl_amd.lqr import LqrWeights  # noqa: E402

TYPES = ("rc_plane", "cessna")
BLOCKS = ("longitudinal", "lateral")


def mode_lines(re, im, wn, zeta, tau, t2):
    """One block of one aircraft (host arrays [4]) -> a line per mode: a pair is printed once."""
    out, k = [], 0
    while k < 4:
        pair = k < 3 and im[k] != 0.0 and im[k + 1] == -im[k]
        lone = f"{re[k]:9.4f} +  {im[k]:8.4f}j" if im[k] != 0.0 else f"{re[k]:9.4f}              "     # ln of a negative real z: at the Nyquist rate
        pole = f"{re[k]:9.4f} +- {im[k]:8.4f}j" if pair else lone
        speed = f"doubles in {t2[k]:7.2f} s" if re[k] > 0.0 else f"tau {tau[k]:7.3f} s"
        out.append(f"{pole}  wn {wn[k]:8.4f} rad/s  zeta {zeta[k]:7.4f}  {speed}")
        k += 2 if pair else 1
    return out


def host_views(m, eig=None):
    """FleetModes -> (re, im, wn, zeta, tau, t2) as host arrays [n][2][4], of `eig` [2][4][n] complex instead of the report's own."""
    if eig is None:
        views = (m.re, m.im, m.natural_frequency(), m.damping_ratio(), m.time_constant(), m.time_to_double())
    else:                                                        # the same formulas on poles mapped to the s-plane
        re, im, wn = eig.real, eig.imag, eig.abs()
        inf = torch.full_like(re, float("inf"))
        views = (re, im, wn, -re / wn, -1.0 / re, torch.where(re > 0.0, float(np.log(2.0)) / re, inf))
    return tuple(v.permute(2, 0, 1).cpu().numpy() for v in views)


def envelope(args):
    speeds = np.array([12.0, 15.0, 18.0, 20.0, 25.0, 30.0])
    ty = np.repeat(np.arange(len(TYPES), dtype=np.uint8), len(speeds))
    V = np.tile(speeds, len(TYPES))
    fleet = BatchedSixDOF(len(V), "f64", types=TYPES, type_index=ty)
    trim = fleet.trim(V, 0.0, args.turn_rate, strict=False)
    design = fleet.design_lqr(strict=False)
    reports = [("open loop", host_views(fleet.modes())), ("closed loop", host_views(fleet.modes(design)))]
    for dt in (0.01, 0.02):
        sampled = Q.sampled_poles(design, fleet.design_kalman(dt, strict=False))
        reports.append((f"sampled at dt {dt}: ln z / dt (radius {float(sampled.spectral_radius().max()):.5f})", host_views(sampled, sampled.to_s_plane(dt))))
    ok = (trim.ok & design.ok).cpu().numpy()
    for t, name in enumerate(TYPES):
        print(f"\n{name}, turn rate {args.turn_rate:g} rad/s, level flight")
        for k in np.flatnonzero(ty == t):
            if not ok[k]:
                print(f"  {V[k]:5.1f} m/s  no certified design")
                continue
            print(f"  {V[k]:5.1f} m/s")
            for title, views in reports:
                for b, block in enumerate(BLOCKS):
                    print(f"      {title}, {block}")
                    for line in mode_lines(*(v[k, b] for v in views)):
                        print(f"          {line}")


def sweep(args):
    n = args.sets
    rs = np.random.RandomState(0)
    logu = lambda lo, hi: np.exp(rs.uniform(np.log(lo), np.log(hi), n))          # noqa: E731
    weights = LqrWeights(u=logu(0.5, 8.0), w=logu(0.5, 8.0), q=logu(0.1, 2.0), theta=logu(0.02, 0.5), v=logu(0.5, 8.0), p=logu(0.2, 4.0),
                         r=logu(0.1, 2.0), phi=logu(0.05, 1.0), elevator=logu(0.1, 1.0), throttle=logu(0.1, 1.0), aileron=logu(0.1, 1.0),
                         rudder=logu(0.1, 1.0))
    fleet = BatchedSixDOF(n, "f64", types=(args.airframe,))
    fleet.trim(args.airspeed, 0.0, args.turn_rate)
    design = fleet.design_lqr(weights, strict=False)             # one launch: N Riccati problems on one model
    modes = fleet.modes(design)                                  # one launch: the poles of every closed loop
    fleet.design_kalman(args.dt, strict=False)
    margins = fleet.loop_margins("estimate")                     # one launch: the disk margin of every LQG loop
    zeta = modes.min_damping().min(dim=0).values                 # [n]: the worse block
    alpha = margins.alpha_s.min(dim=0).values
    keep = design.ok & modes.ok & margins.ok & (zeta >= 0.6)
    score = torch.where(keep, alpha, torch.full_like(alpha, -1.0))
    order = torch.argsort(score, descending=True)[:args.top].cpu().numpy()
    print(f"\nweight sweep: {n} Bryson sets on {args.airframe} at {args.airspeed:g} m/s, LQG at dt {args.dt}: {int(design.ok.sum())} certified, "
          f"{int(keep.sum())} with min damping >= 0.6 in both blocks; the best {len(order)} by alpha")
    zeta, alpha, absc = zeta.cpu().numpy(), alpha.cpu().numpy(), modes.abscissa().max(dim=0).values.cpu().numpy()
    kept, maxima = keep.cpu().numpy(), np.array(weights.maxima()).T
    print("     set   alpha  min zeta  slowest pole   maxima (u w q theta | v p r phi | elevator throttle aileron rudder)")
    for i in order:
        if kept[i]:
            print(f"  {i:6d}  {alpha[i]:6.4f}  {zeta[i]:8.4f}  {absc[i]:12.4f}   {np.array2string(maxima[i], precision=2, suppress_small=True, max_line_width=200)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--turn-rate", type=float, default=0.0)
    ap.add_argument("--sets", type=int, default=4096)
    ap.add_argument("--airframe", default="rc_plane", choices=TYPES)
    ap.add_argument("--airspeed", type=float, default=20.0)
    ap.add_argument("--dt", type=float, default=0.02)
    ap.add_argument("--top", type=int, default=8)
    args = ap.parse_args()
    envelope(args)
    sweep(args)


if __name__ == "__main__":
    main()

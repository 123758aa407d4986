#!/usr/bin/env python3
"""Flight modes of the LQ servo, every pole taken on the device: trim -> linearise -> design (servo gain and servo Kalman filter) ->
MODES, one aircraft per (airframe, airspeed).

Part 1, one table over airframe x V: the slowest pole's time constant and the least damping of both blocks for the continuous
augmented loop (7 longitudinal + 6 lateral poles) and for the loop as it is flown at dt 0.01 and 0.02 (zero-order hold, forward-Euler
integrators) brought back to the s-plane (ln z / dt); and the shift: how far the slowest pole of each block -- the integrators and the
modes the weights shape -- moved between the continuous design and the loop that is flown.  Then the filter's ten poles' radius.

Part 2, a weight sweep, the use the report exists for: N ServoWeights sets on one flight condition, ONE launch each of servo design
-> continuous modes -> sampled modes -> servo margins (plus one filter design): the sets ranked by the least damping of the flown
loop, then those with min damping >= 0.5 ranked by the servo margin alpha.

    python examples/servo_modes.py [--sets 4096] [--airframe rc_plane] [--airspeed 20] [--dt 0.02] [--top 8]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hcrl_amd  # noqa: E402,F401
from hcrl_amd.fleet import BatchedSixDOF  # noqa: E402
from hcrl_amd.servo import ServoWeights  # noqa: E402

TYPES = ("rc_plane", "cessna")


def s_plane_summary(m, dt=None):
    """ServoModes -> per block (slowest time constant [n], least damping [n], slowest pole [n] complex) of its poles, mapped to the
    s-plane first when dt is given."""
    out = []
    for b in range(2):
        lam = m.eig(b) if dt is None else m.to_s_plane(b, dt)
        slow = lam.real.argmax(dim=0)
        pole = lam.gather(0, slow[None])[0]
        out.append((-1.0 / pole.real, (-lam.real / lam.abs()).min(dim=0).values, pole))
    return out


def envelope():
    speeds = np.array([12.0, 15.0, 18.0, 20.0, 25.0, 30.0])
    ty = np.repeat(np.arange(len(TYPES), dtype=np.uint8), len(speeds))
    V = np.tile(speeds, len(TYPES))
    fleet = BatchedSixDOF(len(V), "f64", types=TYPES, type_index=ty)
    trim = fleet.trim(V, 0.0, 0.0, strict=False)
    design = fleet.design_servo(strict=False)
    cont = fleet.servo_modes("continuous")
    rows = [("continuous", s_plane_summary(cont), None)]
    radius = {}
    for dt in (0.01, 0.02):
        kalman = fleet.design_servo_kalman(dt, strict=False)
        rows.append((f"flown at dt {dt}", s_plane_summary(fleet.servo_modes("sampled"), dt), dt))
        radius[dt] = (fleet.servo_modes("sampled").spectral_radius().max(dim=0).values.cpu().numpy(),
                      fleet.servo_modes("filter").spectral_radius().max(dim=0).values.cpu().numpy(), kalman.ok.cpu().numpy())
    ok = (trim.ok & design.ok & cont.ok).cpu().numpy()
    print("slowest pole: time constant (s) lon / lat; least damping lon / lat; |shift of the slowest pole against the continuous design| (rad/s) lon / lat")
    for k in range(len(V)):
        if not ok[k]:
            print(f"{TYPES[ty[k]]:9s} {V[k]:5.1f}   no certified design")
            continue
        print(f"{TYPES[ty[k]]:9s} {V[k]:5.1f}")
        base = rows[0][1]
        for title, blocks, dt in rows:
            tau, zeta = [float(b[0][k]) for b in blocks], [float(b[1][k]) for b in blocks]
            shift = "" if dt is None else "   shift {:.2e} / {:.2e}".format(*(float((blocks[b][2][k] - base[b][2][k]).abs()) for b in range(2)))
            tail = "" if dt is None else f"   radius loop {radius[dt][0][k]:.6f}, filter {radius[dt][1][k]:.6f}"
            print(f"    {title:18s} tau {tau[0]:7.3f} / {tau[1]:7.3f}   zeta {zeta[0]:6.4f} / {zeta[1]:6.4f}{shift}{tail}")


def sweep(args):
    n = args.sets
    rs = np.random.RandomState(0)
    logu = lambda lo, hi: np.exp(rs.uniform(np.log(lo), np.log(hi), n))          # noqa: E731
    d = ServoWeights()
    spread = {f: logu(0.25 * getattr(d, f), 4.0 * getattr(d, f)) for f in ServoWeights.__dataclass_fields__}
    weights = ServoWeights(**spread)
    fleet = BatchedSixDOF(n, "f64", types=(args.airframe,))
    fleet.trim(args.airspeed, 0.0, 0.0)
    design = fleet.design_servo(weights, strict=False)           # one launch: N pairs of Riccati problems on one model
    kalman = fleet.design_servo_kalman(args.dt, strict=False)    # one launch: the model at dt (and the filter)
    cont = fleet.servo_modes("continuous")                       # one launch: 13 poles of every continuous loop
    flown = fleet.servo_modes("sampled")                         # one launch: 13 poles of every loop as it is flown
    margins = fleet.servo_loop_margins("truth")                  # one launch: the disk margin of every flown loop
    zeta = torch.stack([s[1] for s in s_plane_summary(flown, args.dt)]).min(dim=0).values
    tau = torch.stack([s[0] for s in s_plane_summary(flown, args.dt)]).max(dim=0).values
    alpha = margins.alpha_s.min(dim=0).values
    good = design.ok & kalman.ok & cont.ok & flown.ok & margins.ok & (flown.spectral_radius().max(dim=0).values < 1.0)
    print(f"\nweight sweep: {n} ServoWeights sets on {args.airframe} at {args.airspeed:g} m/s, flown at dt {args.dt}: {int(design.ok.sum())} certified, "
          f"{int(good.sum())} with every report ok; five launches")
    maxima = np.array([np.broadcast_to(v, n) for v in weights.maxima()]).T
    zeta_h, tau_h, alpha_h, zc = zeta.cpu().numpy(), tau.cpu().numpy(), alpha.cpu().numpy(), cont.min_damping().min(dim=0).values.cpu().numpy()
    for title, score in (("by the least damping of the flown loop", torch.where(good, zeta, torch.full_like(zeta, -2.0))),
                         ("with min damping >= 0.5, by the servo margin alpha", torch.where(good & (zeta >= 0.5), alpha, torch.full_like(alpha, -2.0)))):
        order = torch.argsort(score, descending=True)[:args.top].cpu().numpy()
        print(f"  the best {len(order)} {title}")
        print("     set   min zeta flown (continuous)   slowest tau   alpha   maxima (u w q theta z i_V i_h | v p r phi psi i_psi | controls)")
        for i in order:
            if float(score[i]) > -2.0:
                print(f"  {i:6d}   {zeta_h[i]:8.4f} ({zc[i]:8.4f})        {tau_h[i]:9.3f} s   {alpha_h[i]:6.4f}   "
                      f"{np.array2string(maxima[i], precision=2, suppress_small=True, max_line_width=220)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", type=int, default=4096)
    ap.add_argument("--airframe", default="rc_plane", choices=TYPES)
    ap.add_argument("--airspeed", type=float, default=20.0)
    ap.add_argument("--dt", type=float, default=0.02)
    ap.add_argument("--top", type=int, default=8)
    args = ap.parse_args()
    envelope()
    sweep(args)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Predicted RMS errors and chatter of the LQ servo, every figure taken on the device without a flight: trim -> linearise -> design
(servo gain and servo Kalman filter) -> margins -> PREDICTED PERFORMANCE, one aircraft per (airframe, airspeed).

Part 1, one table over airframe x V under estimate and under measurement feedback: predicted RMS altitude, airspeed and heading
error, RMS of the altitude estimate's error, the throttle's and the elevator's chatter, and the throttle's headroom to its limits in
predicted sigma (below about 3 the loop clips and the prediction does not hold).

Part 2, a weight sweep, the use the report exists for: N ServoWeights sets on one flight condition, ONE launch each of servo design
-> filter design -> servo margins -> predicted covariance: the sets ranked by predicted altitude RMS among those with throttle headroom
>= 3 sigma and a margin alpha >= the floor.  Launches only.

Part 3, the confirmation: the top and the bottom candidates of that ranking flown for 40 s on in-kernel sensor noise (10 s
discarded), their flown err_est and chatter per step against the prediction.

    python examples/servo_predicted_performance.py [--sets 4096] [--airframe rc_plane] [--airspeed 20] [--dt 0.01] [--top 4]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hcrl_amd  # noqa: E402,F401
from hcrl_amd import layout as L  # noqa: E402
from hcrl_amd.fleet import BatchedSixDOF  # noqa: E402
from hcrl_amd.servo import ServoWeights  # noqa: E402

TYPES = ("rc_plane", "cessna")


def envelope(dt):
    speeds = np.array([15.0, 18.0, 20.0, 25.0, 30.0])
    ty = np.repeat(np.arange(len(TYPES), dtype=np.uint8), len(speeds))
    V = np.tile(speeds, len(TYPES))
    fleet = BatchedSixDOF(len(V), "f64", types=TYPES, type_index=ty)
    trim = fleet.trim(V, 0.0, 0.0, strict=False)
    design = fleet.design_servo(strict=False)
    kalman = fleet.design_servo_kalman(dt, strict=False)
    print(f"predicted at dt {dt}: RMS errors h (m) / V (m/s) / psi (mrad); RMS altitude estimate error (m); chatter sigma throttle / elevator; "
          "throttle headroom (sigma)")
    for fb in ("estimate", "measurement"):
        c = fleet.servo_covariance(fb)
        ok = (trim.ok & design.ok & kalman.ok & c.ok).cpu().numpy()
        rms, est = c.rms_tracking().cpu().numpy(), c.rms_estimate_error().cpu().numpy()
        ch, room = torch.sqrt(c.chatter()).cpu().numpy(), c.headroom(design.u0).cpu().numpy()
        print(f"  feedback = {fb}")
        for k in range(len(V)):
            if not ok[k]:
                print(f"    {TYPES[ty[k]]:9s} {V[k]:5.1f}   no report ({c.describe_status(int(c.status[k]))})")
                continue
            flag = "" if room[L.FD_U_THROTTLE, k] >= 3.0 else "   <- the throttle will clip: not to be trusted"
            print(f"    {TYPES[ty[k]]:9s} {V[k]:5.1f}   h {rms[1, k]:7.4f}  V {rms[0, k]:7.4f}  psi {1e3 * rms[2, k]:7.3f}   est h {est[4, k]:7.4f}   "
                  f"chatter {ch[L.FD_U_THROTTLE, k]:.5f} / {ch[L.FD_U_ELEVATOR, k]:.5f}   headroom {room[L.FD_U_THROTTLE, k]:6.1f}{flag}")


def sweep(args):
    n = args.sets
    rs = np.random.RandomState(0)
    logu = lambda lo, hi: np.exp(rs.uniform(np.log(lo), np.log(hi), n))          # noqa: E731
    d = ServoWeights()
    weights = ServoWeights(**{f: logu(0.25 * getattr(d, f), 4.0 * getattr(d, f)) for f in ServoWeights.__dataclass_fields__})
    fleet = BatchedSixDOF(n, "mixed", types=(args.airframe,))
    fleet.trim(args.airspeed, 0.0, 0.0)
    design = fleet.design_servo(weights, strict=False)           # one launch: N pairs of Riccati problems on one model
    kalman = fleet.design_servo_kalman(args.dt, strict=False)    # one launch: the model at dt and the filter
    margins = fleet.servo_loop_margins("estimate")               # one launch: the disk margin of every loop on its estimate
    pred = fleet.servo_covariance("estimate")                    # one launch: what every loop will hold on its sensors
    alpha = margins.alpha_s.min(dim=0).values
    room = pred.headroom(design.u0).min(dim=0).values
    h_rms = pred.rms_tracking()[1]
    good = design.ok & kalman.ok & margins.ok & pred.ok
    admitted = good & (room >= 3.0) & (alpha >= args.alpha_floor)
    print(f"\nweight sweep: {n} ServoWeights sets on {args.airframe} at {args.airspeed:g} m/s, dt {args.dt}: {int(good.sum())} with every report ok, "
          f"{int(admitted.sum())} with headroom >= 3 sigma and alpha >= {args.alpha_floor}; four launches, no flight")
    score = torch.where(admitted, h_rms, torch.full_like(h_rms, float("inf")))
    order = torch.argsort(score)
    best = order[:args.top]
    worst = order[:int(admitted.sum())][-args.top:]
    picks = torch.cat([best, worst])
    maxima = np.array([np.broadcast_to(v, n) for v in weights.maxima()]).T
    ch = pred.chatter()
    for title, idx in (("best", best), ("worst admitted", worst)):
        print(f"  the {len(idx)} {title} by predicted altitude RMS")
        for i in idx.cpu().numpy():
            print(f"  {i:6d}   h {float(h_rms[i]):7.4f} m   alpha {float(alpha[i]):6.4f}   headroom {float(room[i]):6.1f}   throttle chatter "
                  f"{float(ch[L.FD_U_THROTTLE, i]):.3e}   maxima {np.array2string(maxima[i], precision=2, suppress_small=True, max_line_width=220)}")

    # the confirmation: every set flies (one launch flies them all), the picks are read
    n_discard, n_acc = int(round(10.0 / args.dt)), int(round(30.0 / args.dt))
    fleet.step_servo_lqg(n_discard, "estimate")
    for t in (fleet.servo_lqg.err_est, fleet.servo_lqg.err_meas, fleet.servo_lqg.chatter):
        t.zero_()
    fleet.step_servo_lqg(n_acc, "estimate")
    want_est, want_ch = pred.expected_accumulators(n_acc)
    r_est, r_ch = fleet.servo_lqg.err_est / want_est, fleet.servo_lqg.chatter / want_ch
    sat = fleet.lqr_saturated_steps
    print(f"  flown {n_discard} + {n_acc} steps, one noise row per set: flown / predicted of one 30 s sample")
    for i in picks.cpu().numpy():
        print(f"  {i:6d}   err_est z {float(r_est[4, i]):.3f}  u {float(r_est[0, i]):.3f}   chatter throttle {float(r_ch[L.FD_U_THROTTLE, i]):.3f}  elevator "
              f"{float(r_ch[L.FD_U_ELEVATOR, i]):.3f}   saturated steps {int(sat[i])}")
    adm = admitted.cpu().numpy()
    print(f"  over the {int(adm.sum())} admitted sets: chatter flown / predicted median {float(r_ch[:, admitted].median()):.3f}, "
          f"5 % .. 95 % {float(torch.quantile(r_ch[:, admitted].flatten(), 0.05)):.3f} .. {float(torch.quantile(r_ch[:, admitted].flatten(), 0.95)):.3f}; "
          f"sets with a saturated step {int((sat[admitted] > 0).sum())}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", type=int, default=4096)
    ap.add_argument("--airframe", default="rc_plane", choices=TYPES)
    ap.add_argument("--airspeed", type=float, default=20.0)
    ap.add_argument("--dt", type=float, default=0.01)
    ap.add_argument("--top", type=int, default=4)
    ap.add_argument("--alpha-floor", type=float, default=0.5)
    args = ap.parse_args()
    envelope(args.dt)
    sweep(args)


if __name__ == "__main__":
    main()

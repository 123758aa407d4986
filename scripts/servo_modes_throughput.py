#!/usr/bin/env python3
"""What the flight-mode reports of the LQ servo of a whole fleet cost on the device, beside the 4 x 4 report, the servo design and the
servo's loop margins timed in the same run.

65 536 aircraft of both airframes (alternating), flight conditions spread over V = 15..30 m/s, flight-path angle 0..5 deg and turn
rate -0.1..0.3 rad/s (scripts/servo_throughput.py's fleet): trimmed, linearised, designed (servo gain and servo filter; LQR gain for
the 4 x 4 report); then one launch each of fdyn_servo_flight_modes, fdyn_servo_sampled_modes, fdyn_servo_filter_modes and
fdyn_square_modes (N = 7, on the longitudinal loop torch composes), beside fdyn_flight_modes (closed loop), fdyn_servo_design and
fdyn_servo_loop_margins (truth feedback, 64 points).  Every launch is timed with device events, eager and as a captured graph, over
back-to-back launches after a warm-up.

    python scripts/servo_modes_throughput.py [--aircraft 65536] [--json profiles/servo_modes_throughput_65536.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hcrl_amd  # noqa: E402,F401
from hcrl_amd import _lib, layout as L  # noqa: E402
from hcrl_amd import lqr as Q  # noqa: E402
from hcrl_amd import margins as M  # noqa: E402
from hcrl_amd import modes as MO  # noqa: E402
from hcrl_amd import servo as SV  # noqa: E402
from hcrl_amd import servo_lqg as SL  # noqa: E402
from hcrl_amd import servo_margins as SM  # noqa: E402
from hcrl_amd import servo_modes as SMO  # noqa: E402
from hcrl_amd import trim as T  # noqa: E402
from hcrl_amd.fleet import BatchedSixDOF  # noqa: E402
from margin_throughput import TYPES, graphed, timed  # noqa: E402

# Per 64-lane workgroup of the servo-modes kernels and the 160 KB a CU has.  CONSTANTS of this script, copied from the compiler's
# resource report for gfx950 when it was written, not found by the run
LDS_BYTES = {"servo_modes": 25088, "filter_modes": 12800, "square_modes_7": 25088}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--aircraft", type=int, default=65536)
    ap.add_argument("--dt", type=float, default=0.02)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--json", default=None, help="default for the default fleet: profiles/servo_modes_throughput_65536.json")
    args = ap.parse_args()
    if args.json is None and args.aircraft == 65536:
        args.json = os.path.join(REPO, "profiles", "servo_modes_throughput_65536.json")
    n, dev = args.aircraft, _lib.require_gpu()
    rs = np.random.RandomState(0)
    ty = (np.arange(n) % 2).astype(np.uint8)
    cond = (rs.uniform(15.0, 30.0, n), np.radians(rs.uniform(0.0, 5.0, n)), rs.uniform(-0.1, 0.3, n), rs.uniform(50.0, 200.0, n),
            rs.uniform(0.0, 6.28, n))
    fleet = BatchedSixDOF(n, "f64", types=TYPES, type_index=ty)
    trim = fleet.trim(*cond, strict=False)
    A, B = T.linearize_into(trim.x0, trim.u0, fleet.params, fleet.type_index, None)
    w_servo = SV.weights_tensor(None, n, dev)
    servo = SV.servo_into(A, B, trim.x0, w_servo)
    servo.x0 = trim.x0
    kalman = SL.servo_kalman_into(A, B, args.dt, SL.noise_tensor(None, n, dev))
    lqr = Q.lqr_into(A, B, Q.weights_tensor(None, n, dev))
    zre, zim = (torch.as_tensor(v, device=dev) for v in M.unit_circle(M.default_grid(args.dt, 64), args.dt))
    m_lon = servo.closed_loop(A, B)[0].contiguous()
    good = trim.ok & servo.ok & kalman.ok
    torch.cuda.synchronize()

    outs = {"servo_flight_modes": SMO.empty(n, dev), "servo_sampled_modes": SMO.empty(n, dev), "servo_filter_modes": SMO.empty(n, dev, (5, 5)),
            "square_modes_7": SMO.empty(n, dev, (7,))}
    old, mrg = MO.modes_into(A, B, lqr.K), SM.servo_margins_into(servo.K, kalman.F, trim.x0, args.dt, zre, zim, "truth")
    calls = {"servo_flight_modes": lambda: SMO.flight_modes_into(A, B, trim.x0, servo.K, outs["servo_flight_modes"]),
             "servo_sampled_modes": lambda: SMO.sampled_modes_into(servo.K, kalman.F, trim.x0, args.dt, outs["servo_sampled_modes"]),
             "servo_filter_modes": lambda: SMO.filter_modes_into(kalman.F, outs["servo_filter_modes"]),
             "square_modes_7": lambda: SMO.square_modes_into(m_lon, outs["square_modes_7"]),
             "flight_modes_4x4": lambda: MO.modes_into(A, B, lqr.K, old),
             "servo_design": lambda: SV.servo_into(A, B, trim.x0, w_servo, servo),
             "servo_margins_truth": lambda: SM.servo_margins_into(servo.K, kalman.F, trim.x0, args.dt, zre, zim, "truth", mrg)}
    res = {"aircraft": n, "dt": args.dt, "designs_not_ok": int((~good).sum()), "lds_bytes_per_workgroup_script_constants": LDS_BYTES,
           "workgroups_per_cu_by_lds_from_those_constants": {k: 163840 // b for k, b in LDS_BYTES.items()}}
    for name, fn in calls.items():
        res[f"{name}_us_eager"] = timed(fn, args.repeats)
        res[f"{name}_us_graph"] = timed(graphed(fn), args.repeats)
    torch.cuda.synchronize()
    for name in ("servo_flight_modes", "servo_sampled_modes", "servo_filter_modes"):
        r = outs[name]
        res[f"{name}_over_flight_modes_4x4"] = res[f"{name}_us_graph"] / res["flight_modes_4x4_us_graph"]
        res[f"{name}_over_servo_design"] = res[f"{name}_us_graph"] / res["servo_design_us_graph"]
        res[f"{name}_over_servo_margins_truth"] = res[f"{name}_us_graph"] / res["servo_margins_truth_us_graph"]
        res[f"{name}_ns_per_aircraft"] = res[f"{name}_us_graph"] * 1e3 / n
        res[f"{name}_not_ok_of_good_designs"] = int((r.status[good] != 0).sum())
        res[f"{name}_not_converged_of_good_designs"] = int((r.status[good] == L.FD_MO_NOT_CONVERGED).sum())
        it = r.iterations[good].double()
        res[f"{name}_sweeps_mean_max"] = [float(it.mean()), int(it.max())]
    # a lane at the sweep cap reports FD_MO_NOT_CONVERGED and NaN words: the extremes are over the lanes that have a report
    have = {name: good & outs[name].ok for name in outs}
    res["continuous_abscissa_max_of_good_designs"] = float(outs["servo_flight_modes"].abscissa()[:, have["servo_flight_modes"]].max())
    res["sampled_radius_max_of_good_designs"] = float(outs["servo_sampled_modes"].spectral_radius()[:, have["servo_sampled_modes"]].max())
    res["filter_radius_max_of_good_designs"] = float(outs["servo_filter_modes"].spectral_radius()[:, have["servo_filter_modes"]].max())
    both = have["square_modes_7"] & have["servo_flight_modes"]
    res["square_modes_7_equals_fused_lon_within"] = float((outs["square_modes_7"].eig_re - outs["servo_flight_modes"].eig_re[:7])[:, both].abs().max())

    print(f"{n} aircraft, {TYPES}, dt {args.dt}: designs not ok {res['designs_not_ok']}")
    for k in sorted(k for k in res if k.endswith(("_us_eager", "_us_graph"))):
        print(f"  {k:40s} {res[k]:10.1f} us")
    for name in ("servo_flight_modes", "servo_sampled_modes", "servo_filter_modes"):
        print(f"  {name}: {res[f'{name}_over_flight_modes_4x4']:.2f} x the 4 x 4 report, {res[f'{name}_over_servo_design']:.3f} x the servo design, "
              f"{res[f'{name}_over_servo_margins_truth']:.3f} x the servo margins; {res[f'{name}_ns_per_aircraft']:.2f} ns per aircraft; sweeps mean / max "
              f"{res[f'{name}_sweeps_mean_max']}; not ok among good designs {res[f'{name}_not_ok_of_good_designs']}")
    print(f"  abscissa max {res['continuous_abscissa_max_of_good_designs']:.4f}, sampled radius max {res['sampled_radius_max_of_good_designs']:.6f}, "
          f"filter radius max {res['filter_radius_max_of_good_designs']:.6f}")
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()

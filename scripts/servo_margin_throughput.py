#!/usr/bin/env python3
"""What the loop-margin report of the LQ servo of a whole fleet costs on the device, beside the regulators' report and the servo's
Kalman design timed in the same run.

65 536 aircraft of both airframes (alternating), flight conditions spread over V = 15..30 m/s, flight-path angle 0..5 deg and turn
rate -0.1..0.3 rad/s (scripts/servo_throughput.py's fleet): trimmed, linearised, designed (servo gain and servo filter; LQR gain and
4-state filter for the comparison); then one launch of fdyn_servo_loop_margins on `--points` grid points under estimate and under
truth feedback, with and without the curve, beside one launch of fdyn_loop_margins on the same grid and one of
fdyn_servo_kf_design.  Every launch is timed with device events, eager and as a captured graph, over back-to-back launches after a
warm-up.

--alt-lib PATH: a shared library holding another build of fdyn_servo_loop_margins alone (csrc/servo_margin_kernels.hip compiled with
-DFDYN_SERVO_MARGIN_COLUMNS: all 115 block words of a lane parked in LDS instead of Phi, Gamma, L and Kx re-read through L2); it is
timed on the same tensors in the same run and its outputs are compared with the library's bit for bit:
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -DFDYN_SERVO_MARGIN_COLUMNS <pkg>/csrc/servo_margin_kernels.hip -o alt.so

Also the table of DESIGN.md 7n, on the device: the 288 linearisations of tests/golden/trim_reference.npz designed with the default
servo weights and servo Kalman noise at dt 0.01 and 0.02, alpha_s under truth and under estimate feedback.

    python scripts/servo_margin_throughput.py [--aircraft 65536] [--points 64] [--json profiles/servo_margin_throughput_65536.json]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hcrl_amd  # noqa: E402,F401
from hcrl_amd import _lib  # noqa: E402
from hcrl_amd import lqg as G  # noqa: E402
from hcrl_amd import lqr as Q  # noqa: E402
from hcrl_amd import margins as M  # noqa: E402
from hcrl_amd import servo as SV  # noqa: E402
from hcrl_amd import servo_lqg as SL  # noqa: E402
from hcrl_amd import servo_margins as SM  # noqa: E402
from hcrl_amd import trim as T  # noqa: E402
from hcrl_amd.fleet import BatchedSixDOF  # noqa: E402
from margin_throughput import TYPES, graphed, timed  # noqa: E402

# Per 64-lane workgroup of servo_loop_margins_kernel and the 160 KB a CU has.  CONSTANTS of this script, copied from the code-object
# metadata for gfx950 when it was written, not found by the run
LDS_BYTES = {"rows": 23040, "columns": 58880}


def golden_table(dev):
    """alpha_s over the 288 golden linearisations, designed and analysed on the device -> {"truth_dt0.01": [[lon min, median, max], [lat ...]], ...}"""
    g = np.load(os.path.join(REPO, "tests", "golden", "trim_reference.npz"))
    A = torch.as_tensor(np.ascontiguousarray(np.transpose(g["A"], (1, 2, 0))), device=dev)
    B = torch.as_tensor(np.ascontiguousarray(np.transpose(g["B"], (1, 2, 0))), device=dev)
    x0 = torch.as_tensor(np.ascontiguousarray(g["x0"].T), device=dev)
    n = A.shape[-1]
    servo = SV.servo_into(A, B, x0, SV.weights_tensor(None, n, dev))
    servo.x0 = x0
    out = {"servo_design_not_ok": servo.count_not_ok()}
    for dt in (0.01, 0.02):
        kal = SL.servo_kalman_into(A, B, dt, SL.noise_tensor(None, n, dev))
        for fb in ("truth", "estimate"):
            m = SM.servo_loop_margins(servo, kal, x0, fb)
            a = m.alpha_s.cpu().numpy()
            out[f"{fb}_dt{dt}"] = [[float(a[b].min()), float(np.median(a[b])), float(a[b].max())] for b in range(2)]
            out[f"{fb}_dt{dt}_not_ok"] = m.count_not_ok() + kal.count_not_ok()
            out[f"{fb}_dt{dt}_minimum_at_nyquist"] = int((m.idx_s == 63).all(dim=0).sum())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--aircraft", type=int, default=65536)
    ap.add_argument("--points", type=int, default=64)
    ap.add_argument("--dt", type=float, default=0.01)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--alt-lib", default=None, help="another build of fdyn_servo_loop_margins to time beside the library's")
    ap.add_argument("--json", default=None, help="default for the default fleet and grid: profiles/servo_margin_throughput_65536.json")
    args = ap.parse_args()
    if args.json is None and (args.aircraft, args.points) == (65536, 64):
        args.json = os.path.join(REPO, "profiles", "servo_margin_throughput_65536.json")
    n, dev = args.aircraft, _lib.require_gpu()
    rs = np.random.RandomState(0)
    ty = (np.arange(n) % 2).astype(np.uint8)
    cond = (rs.uniform(15.0, 30.0, n), np.radians(rs.uniform(0.0, 5.0, n)), rs.uniform(-0.1, 0.3, n), rs.uniform(50.0, 200.0, n),
            rs.uniform(0.0, 6.28, n))

    fleet = BatchedSixDOF(n, "f64", types=TYPES, type_index=ty)
    trim = fleet.trim(*cond, strict=False)
    A, B = T.linearize_into(trim.x0, trim.u0, fleet.params, fleet.type_index, None)
    nz_servo = SL.noise_tensor(None, n, dev)
    servo = SV.servo_into(A, B, trim.x0, SV.weights_tensor(None, n, dev))
    kalman = SL.servo_kalman_into(A, B, args.dt, nz_servo)
    lqr, kf4 = Q.lqr_into(A, B, Q.weights_tensor(None, n, dev)), G.kalman_into(A, B, args.dt, G.noise_tensor(None, n, dev))
    zre, zim = (torch.as_tensor(v, device=dev) for v in M.unit_circle(M.default_grid(args.dt, args.points), args.dt))
    good = trim.ok & servo.ok & kalman.ok
    torch.cuda.synchronize()
    res = {"aircraft": n, "points": args.points, "dt": args.dt, "designs_not_ok": int((~good).sum()),
           "lds_bytes_per_workgroup_script_constants": LDS_BYTES,
           "workgroups_per_cu_by_lds_from_those_constants": {k: 163840 // b for k, b in LDS_BYTES.items()}}
    res["servo_kf_design_us_eager"] = timed(lambda: SL.servo_kalman_into(A, B, args.dt, nz_servo, kalman), args.repeats)
    res["servo_kf_design_us_graph"] = timed(graphed(lambda: SL.servo_kalman_into(A, B, args.dt, nz_servo, kalman)), args.repeats)

    alt = None
    if args.alt_lib:
        alt = getattr(ctypes.CDLL(os.path.abspath(args.alt_lib)), "fdyn_servo_loop_margins")
        alt.restype, alt.argtypes = _lib.SERVO_MARGIN_SIGNATURES["fdyn_servo_loop_margins"]

    def alt_into(fb, out):
        rc = alt(_lib.ptr(servo.K), _lib.ptr(kalman.F), _lib.ptr(trim.x0), args.dt, G.FEEDBACK[fb], _lib.ptr(zre), _lib.ptr(zim), args.points, n,
                 _lib.ptr(out.alpha_s), _lib.ptr(out.idx_s), _lib.ptr(out.alpha_t), _lib.ptr(out.idx_t), _lib.ptr(out.curve), _lib.ptr(out.status),
                 _lib.current_stream())
        _lib.check(rc, "fdyn_servo_loop_margins (alt)")

    for fb in ("estimate", "truth"):
        for curve in (False, True):
            out = SM.servo_margins_into(servo.K, kalman.F, trim.x0, args.dt, zre, zim, fb, None, curve)
            fn = lambda fb=fb, out=out: SM.servo_margins_into(servo.K, kalman.F, trim.x0, args.dt, zre, zim, fb, out)  # noqa: E731
            key = f"servo_margins_{fb}{'_curve' if curve else ''}"
            res[f"{key}_us_eager"] = timed(fn, args.repeats)
            res[f"{key}_us_graph"] = timed(graphed(fn), args.repeats)
            old = M.margins_into(lqr.K, kf4.F, zre, zim, fb, None, curve)
            fo = lambda fb=fb, old=old: M.margins_into(lqr.K, kf4.F, zre, zim, fb, old)  # noqa: E731
            key4 = f"margins_{fb}{'_curve' if curve else ''}"
            res[f"{key4}_us_eager"] = timed(fo, args.repeats)
            res[f"{key4}_us_graph"] = timed(graphed(fo), args.repeats)
            if alt is not None:
                other = SM.servo_margins_into(servo.K, kalman.F, trim.x0, args.dt, zre, zim, fb, None, curve)
                for t in (other.alpha_s, other.alpha_t):
                    t.fill_(-1.0)
                fa = lambda fb=fb, other=other: alt_into(fb, other)  # noqa: E731
                res[f"{key}_columns_us_eager"] = timed(fa, args.repeats)
                res[f"{key}_columns_us_graph"] = timed(graphed(fa), args.repeats)
                torch.cuda.synchronize()
                same = all(torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a, b.view(torch.int64) if b.dtype == torch.float64 else b)
                           for a, b in ((out.alpha_s, other.alpha_s), (out.alpha_t, other.alpha_t), (out.idx_s, other.idx_s), (out.idx_t, other.idx_t),
                                        (out.status, other.status)) + (((out.curve, other.curve),) if curve else ()))
                res[f"{key}_columns_bit_equal"] = bool(same)
        a = out.alpha_s[:, good]
        res[f"servo_margins_{fb}_not_ok_of_good_designs"] = int((out.status[good] != 0).sum())
        res[f"alpha_s_{fb}"] = [[float(a[b].min()), float(a[b].median()), float(a[b].max())] for b in range(2)]
        res[f"servo_margins_{fb}_over_margins"] = res[f"servo_margins_{fb}_us_graph"] / res[f"margins_{fb}_us_graph"]
        res[f"servo_margins_{fb}_over_servo_kf_design"] = res[f"servo_margins_{fb}_us_graph"] / res["servo_kf_design_us_graph"]
        res[f"servo_margins_{fb}_ns_per_aircraft_point"] = res[f"servo_margins_{fb}_us_graph"] * 1e3 / (n * 2 * args.points)
    res["golden_table"] = golden_table(dev)

    print(f"{n} aircraft, {TYPES}, {args.points} grid points, dt {args.dt}: designs not ok {res['designs_not_ok']}")
    for k in sorted(k for k in res if k.endswith(("_us_eager", "_us_graph"))):
        print(f"  {k:48s} {res[k]:10.1f} us")
    for fb in ("estimate", "truth"):
        print(f"  {fb}: servo margins / margins {res[f'servo_margins_{fb}_over_margins']:.2f}, / servo Kalman design "
              f"{res[f'servo_margins_{fb}_over_servo_kf_design']:.2f}; {res[f'servo_margins_{fb}_ns_per_aircraft_point']:.3f} ns per aircraft, block "
              f"and point; alpha_s (min, median, max) lon {res[f'alpha_s_{fb}'][0]}, lat {res[f'alpha_s_{fb}'][1]}; not ok among good designs "
              f"{res[f'servo_margins_{fb}_not_ok_of_good_designs']}")
    for k in sorted(k for k in res if k.endswith("_bit_equal")):
        print(f"  {k}: {res[k]}")
    print("  golden table:", json.dumps(res["golden_table"]))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()

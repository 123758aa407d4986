#!/usr/bin/env python3
"""What the predicted-performance report of the LQ servo of a whole fleet costs on the device, beside the filter design, the loop
margins and the flight it replaces, timed in the same run.

65 536 aircraft of both airframes (alternating), flight conditions spread over V = 15..30 m/s, flight-path angle 0..5 deg and turn
rate -0.1..0.3 rad/s (scripts/servo_throughput.py's fleet): trimmed, linearised, designed (servo gain and servo filter); then one
launch each of fdyn_servo_covariance under the three feedbacks (with and without the 200 covariance rows) and of fdyn_stein_solve
(7 x 7 on the longitudinal loop), beside fdyn_servo_kf_design and fdyn_servo_loop_margins (estimate feedback, 64 points), each timed
with device events, eager and as a captured graph, over back-to-back launches after a warm-up; and ONE flight of 3000 steps of
fdyn_servo_lqg_step_mixed on in-kernel draws, the experiment the report stands in for, timed once after a 100-step warm-up.

    python scripts/servo_covariance_throughput.py [--aircraft 65536] [--json profiles/servo_covariance_throughput_65536.json]
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
from hcrl_amd import margins as M  # noqa: E402
from hcrl_amd import servo_covariance as SC  # noqa: E402
from hcrl_amd import servo_lqg as SL  # noqa: E402
from hcrl_amd import servo_margins as SM  # noqa: E402
from hcrl_amd import trim as T  # noqa: E402
from hcrl_amd.fleet import BatchedSixDOF  # noqa: E402
from margin_throughput import TYPES, graphed, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--aircraft", type=int, default=65536)
    ap.add_argument("--dt", type=float, default=0.01)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--flight-steps", type=int, default=3000)
    ap.add_argument("--json", default=None, help="default for the default fleet: profiles/servo_covariance_throughput_65536.json")
    args = ap.parse_args()
    if args.json is None and args.aircraft == 65536:
        args.json = os.path.join(REPO, "profiles", "servo_covariance_throughput_65536.json")
    n, dev = args.aircraft, _lib.require_gpu()
    rs = np.random.RandomState(0)
    ty = (np.arange(n) % 2).astype(np.uint8)
    cond = (rs.uniform(15.0, 30.0, n), np.radians(rs.uniform(0.0, 5.0, n)), rs.uniform(-0.1, 0.3, n), rs.uniform(50.0, 200.0, n),
            rs.uniform(0.0, 6.28, n))
    fleet = BatchedSixDOF(n, "mixed", types=TYPES, type_index=ty)
    trim = fleet.trim(*cond, strict=False)
    servo = fleet.design_servo(strict=False)
    kalman = fleet.design_servo_kalman(args.dt, strict=False)
    A, B = T.linearize_into(trim.x0, trim.u0, fleet.params, fleet.type_index, None)
    noise = SL.noise_tensor(None, n, dev)
    sigma, rates = noise[:L.FD_NSKX].clone(), noise[L.FD_NSKX:].clone()
    zre, zim = (torch.as_tensor(v, device=dev) for v in M.unit_circle(M.default_grid(args.dt, 64), args.dt))
    good = trim.ok & servo.ok & kalman.ok
    torch.cuda.synchronize()

    full = {fb: SC.empty(n, dev) for fb in ("estimate", "measurement", "truth")}
    lean = SC.empty(n, dev, cov=False)
    with_w = SC.empty(n, dev)
    kf_out = SL.servo_kalman_into(A, B, args.dt, noise)
    mrg = SM.servo_margins_into(servo.K, kalman.F, trim.x0, args.dt, zre, zim, "estimate")
    calls = {f"servo_covariance_{fb}": (lambda fb=fb: SC.servo_covariance_into(servo.K, kalman.F, trim.x0, args.dt, sigma, None, fb, full[fb]))
             for fb in full}
    calls["servo_covariance_estimate_no_cov"] = lambda: SC.servo_covariance_into(servo.K, kalman.F, trim.x0, args.dt, sigma, None, "estimate", lean)
    calls["servo_covariance_estimate_with_w"] = lambda: SC.servo_covariance_into(servo.K, kalman.F, trim.x0, args.dt, sigma, rates, "estimate", with_w)
    calls["servo_kf_design"] = lambda: SL.servo_kalman_into(A, B, args.dt, noise, kf_out)
    calls["servo_margins_estimate"] = lambda: SM.servo_margins_into(servo.K, kalman.F, trim.x0, args.dt, zre, zim, "estimate", mrg)
    res = {"aircraft": n, "dt": args.dt, "designs_not_ok": int((~good).sum())}
    for name, fn in calls.items():
        res[f"{name}_us_eager"] = timed(fn, args.repeats)
        res[f"{name}_us_graph"] = timed(graphed(fn), args.repeats)
    torch.cuda.synchronize()
    # the 7 x 7 of the longitudinal loop through the general door: torch composes Acl, and Q = Sx - Acl Sx Acl^T of the fused entry's
    # Sx, so that the solve has to give Sx back
    pred = full["measurement"]
    have = good & pred.ok
    sx = pred.matrices(0)[2]
    phi, gam, kb = kalman.phi()[0], kalman.gamma()[0], servo.K[:14].view(2, 7, n)
    Acl = torch.zeros((7, 7, n), dtype=torch.float64, device=dev)
    Acl[:5] = -torch.einsum("rjn,jcn->rcn", gam, kb)
    Acl[:5, :5] += phi
    u0, w0 = trim.x0[L.FD_X_U], trim.x0[L.FD_X_W]
    V0 = torch.sqrt(u0 * u0 + w0 * w0)
    Acl[5, 0], Acl[5, 1], Acl[6, 4] = args.dt * u0 / V0, args.dt * w0 / V0, -args.dt
    Acl[5, 5] = Acl[6, 6] = 1.0
    Q = (sx - torch.einsum("rjn,jkn,ckn->rcn", Acl, sx, Acl)).contiguous()
    sol = SC.stein_solve(Acl, Acl, Q)
    res["stein_solve_7x7_us_eager"] = timed(lambda: SC.stein_solve(Acl, Acl, Q, sol), args.repeats)
    res["stein_solve_7x7_us_graph"] = timed(graphed(lambda: SC.stein_solve(Acl, Acl, Q, sol)), args.repeats)
    torch.cuda.synchronize()
    both = have & sol.ok
    res["stein_solve_7x7_lanes_compared"] = int(both.sum())
    res["stein_solve_7x7_equals_fused_within_relative"] = float(((sol.X - sx)[:, :, both].abs().amax(dim=(0, 1)) / sx[:, :, both].abs().amax(dim=(0, 1))).max())

    # the flight the report replaces: 3000 steps of every aircraft on in-kernel draws, once
    fleet.step_servo_lqg(100, "estimate")
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fleet.step_servo_lqg(args.flight_steps, "estimate")
    b.record()
    torch.cuda.synchronize()
    res["flight_steps"] = args.flight_steps
    res["flight_mixed_estimate_us"] = a.elapsed_time(b) * 1e3

    est = full["estimate"]
    ok = good & est.ok
    res["report_not_ok_of_good_designs"] = {fb: int((full[fb].status[good] != 0).sum()) for fb in full}
    res["report_status_counts_estimate"] = {str(int(s)): int((est.status == s).sum()) for s in torch.unique(est.status)}
    it = est.iterations[ok].double()
    res["doublings_mean_max_estimate"] = [float(it.mean()), int(it.max())]
    res["residual_max_estimate"] = float(est.residual[ok].max())
    res["predicted_altitude_rms_m_min_median_max"] = [float(v) for v in torch.quantile(est.rms_tracking()[1][ok], torch.tensor([0.0, 0.5, 1.0], dtype=torch.float64, device=dev))]
    room = est.headroom(servo.u0)[L.FD_U_THROTTLE][ok]
    res["throttle_headroom_min_median"] = [float(room.min()), float(room.median())]
    res["throttle_headroom_below_3"] = int((room < 3.0).sum())
    for fb in full:
        res[f"servo_covariance_{fb}_over_kf_design"] = res[f"servo_covariance_{fb}_us_graph"] / res["servo_kf_design_us_graph"]
        res[f"servo_covariance_{fb}_over_margins_estimate"] = res[f"servo_covariance_{fb}_us_graph"] / res["servo_margins_estimate_us_graph"]
        res[f"flight_over_servo_covariance_{fb}"] = res["flight_mixed_estimate_us"] / res[f"servo_covariance_{fb}_us_graph"]
        res[f"servo_covariance_{fb}_ns_per_aircraft"] = res[f"servo_covariance_{fb}_us_graph"] * 1e3 / n

    print(f"{n} aircraft, {TYPES}, dt {args.dt}: designs not ok {res['designs_not_ok']}")
    for k in sorted(k for k in res if k.endswith(("_us_eager", "_us_graph", "_us"))):
        print(f"  {k:48s} {res[k]:12.1f} us")
    print(f"  estimate: {res['servo_covariance_estimate_over_kf_design']:.2f} x the filter design, {res['servo_covariance_estimate_over_margins_estimate']:.3f} x "
          f"the margins, the {args.flight_steps}-step flight is {res['flight_over_servo_covariance_estimate']:.0f} x the report; doublings mean / max "
          f"{res['doublings_mean_max_estimate']}; status counts {res['report_status_counts_estimate']}; throttle headroom below 3 sigma: "
          f"{res['throttle_headroom_below_3']}")
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()

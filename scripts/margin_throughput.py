#!/usr/bin/env python3
"""What the loop-margin report of a whole fleet costs on the device, beside the Kalman design it analyses.

The fleet of scripts/lqg_throughput.py: 65 536 aircraft of both airframes (alternating), flight conditions spread over
V = 15..30 m/s, flight-path angle 0..5 deg and turn rate -0.1..0.3 rad/s, +-20 % mass, trimmed, linearised and designed (gain and
filter); then in the same run one launch of fdyn_loop_margins on `--points` grid points under estimate and under truth feedback,
with and without the curve, beside one launch of fdyn_kf_design.  Every launch is timed with device events, eager and as a captured
graph, over back-to-back launches after a warm-up.

Also the table of DESIGN.md 7h, on the device: the 288 linearisations of tests/golden/trim_reference.npz designed with the default
weights and noise at dt 0.01 and 0.02, alpha_s of the sampled LQR (truth feedback) and of the LQG loop (estimate feedback).

    python scripts/margin_throughput.py [--aircraft 65536] [--points 64] [--json profiles/margin_throughput_65536.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import hcrl_amd  # noqa: E402,F401
from hcrl_amd import _lib  # noqa: E402
from hcrl_amd import lqg as G  # noqa: E402
from hcrl_amd import lqr as Q  # noqa: E402
from hcrl_amd import margins as M  # noqa: E402
from hcrl_amd import trim as T  # noqa: E402
from hcrl_amd.fleet import BatchedSixDOF  # noqa: E402

TYPES = ("rc_plane", "cessna")


def timed(fn, repeats):
    """Device time of one call in microseconds: `repeats` calls between two events, after a warm-up of 3."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(repeats):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / repeats


def graphed(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g.replay


def golden_table(dev):
    """alpha_s over the 288 golden linearisations, designed and analysed on the device -> {"lqr_dt0.01": [[lon min, lon max], [lat ...]], ...}"""
    g = np.load(os.path.join(REPO, "tests", "golden", "trim_reference.npz"))
    A = torch.as_tensor(np.ascontiguousarray(np.transpose(g["A"], (1, 2, 0))), device=dev)
    B = torch.as_tensor(np.ascontiguousarray(np.transpose(g["B"], (1, 2, 0))), device=dev)
    n = A.shape[-1]
    lqr = Q.lqr_into(A, B, Q.weights_tensor(None, n, dev))
    out = {"lqr_design_not_ok": lqr.count_not_ok()}
    for dt in (0.01, 0.02):
        kal = G.kalman_into(A, B, dt, G.noise_tensor(None, n, dev))
        for name, fb in (("lqr", "truth"), ("lqg", "estimate")):
            m = M.loop_margins(lqr, kal, fb)
            a = m.alpha_s.cpu().numpy()
            out[f"{name}_dt{dt}"] = [[float(a[b].min()), float(a[b].max())] for b in range(2)]
            out[f"{name}_dt{dt}_not_ok"] = m.count_not_ok() + kal.count_not_ok()
            out[f"{name}_dt{dt}_worst_at_nyquist"] = bool(int(m.idx_s.reshape(-1)[int(m.alpha_s.reshape(-1).argmin())]) == 63)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--aircraft", type=int, default=65536)
    ap.add_argument("--points", type=int, default=64)
    ap.add_argument("--dt", type=float, default=0.01)
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--json", default=None, help="default for the default fleet and grid: profiles/margin_throughput_65536.json")
    args = ap.parse_args()
    if args.json is None and (args.aircraft, args.points) == (65536, 64):
        args.json = os.path.join(REPO, "profiles", "margin_throughput_65536.json")
    n, dev = args.aircraft, _lib.require_gpu()
    rs = np.random.RandomState(0)
    ty = (np.arange(n) % 2).astype(np.uint8)
    cond = (rs.uniform(15.0, 30.0, n), np.radians(rs.uniform(0.0, 5.0, n)), rs.uniform(-0.1, 0.3, n), rs.uniform(50.0, 200.0, n),
            rs.uniform(0.0, 6.28, n))
    scales = (rs.uniform(0.8, 1.2, n), 1.0, 1.0, 1.0, 1.0)

    fleet = BatchedSixDOF(n, "f64", types=TYPES, type_index=ty)
    trim = fleet.trim(*cond, scales=scales, strict=False)
    AB = T.linearize_into(trim.x0, trim.u0, fleet.params, fleet.type_index, T.scale_rows(n, scales, dev))
    w, nz = Q.weights_tensor(None, n, dev), G.noise_tensor(None, n, dev)
    lqr, kal = Q.lqr_into(AB[0], AB[1], w), G.kalman_into(AB[0], AB[1], args.dt, nz)
    zre, zim = (torch.as_tensor(v, device=dev) for v in M.unit_circle(M.default_grid(args.dt, args.points), args.dt))
    good = trim.ok & lqr.ok & kal.ok
    torch.cuda.synchronize()
    res = {"aircraft": n, "points": args.points, "dt": args.dt, "designs_not_ok": int((~good).sum())}
    res["kf_design_us_eager"] = timed(lambda: G.kalman_into(AB[0], AB[1], args.dt, nz, kal), args.repeats)
    res["kf_design_us_graph"] = timed(graphed(lambda: G.kalman_into(AB[0], AB[1], args.dt, nz, kal)), args.repeats)
    for fb in ("estimate", "truth"):
        for curve in (False, True):
            out = M.margins_into(lqr.K, kal.F, zre, zim, fb, None, curve)
            fn = lambda fb=fb, out=out: M.margins_into(lqr.K, kal.F, zre, zim, fb, out)  # noqa: E731
            key = f"margins_{fb}{'_curve' if curve else ''}"
            res[f"{key}_us_eager"] = timed(fn, args.repeats)
            res[f"{key}_us_graph"] = timed(graphed(fn), args.repeats)
        a = out.alpha_s[:, good]
        res[f"margins_{fb}_not_ok_of_good_designs"] = int((out.status[good] != 0).sum())
        res[f"alpha_s_{fb}"] = [[float(a[b].min()), float(a[b].median()), float(a[b].max())] for b in range(2)]
        res[f"margins_{fb}_over_kf_design"] = res[f"margins_{fb}_us_graph"] / res["kf_design_us_graph"]
        res[f"margins_{fb}_ns_per_aircraft_point"] = res[f"margins_{fb}_us_graph"] * 1e3 / (n * 2 * args.points)
    res["golden_table"] = golden_table(dev)

    print(f"{n} aircraft, {TYPES}, {args.points} grid points, dt {args.dt}: designs not ok {res['designs_not_ok']}")
    for k in sorted(k for k in res if k.endswith(("_us_eager", "_us_graph"))):
        print(f"  {k:40s} {res[k]:10.1f} us")
    for fb in ("estimate", "truth"):
        print(f"  {fb}: margins / Kalman design {res[f'margins_{fb}_over_kf_design']:.2f}; {res[f'margins_{fb}_ns_per_aircraft_point']:.3f} ns per "
              f"aircraft, block and point; alpha_s (min, median, max) lon {res[f'alpha_s_{fb}'][0]}, lat {res[f'alpha_s_{fb}'][1]}; "
              f"not ok among good designs {res[f'margins_{fb}_not_ok_of_good_designs']}")
    print("  golden table:", json.dumps(res["golden_table"]))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()

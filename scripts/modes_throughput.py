#!/usr/bin/env python3
"""What the flight-mode report of a whole fleet costs on the device, beside the LQR design whose loop it describes.

The fleet of scripts/lqr_throughput.py: 65 536 aircraft of both airframes (alternating), flight conditions spread over
V = 15..30 m/s, flight-path angle 0..5 deg and turn rate -0.1..0.3 rad/s, +-20 % mass, trimmed, linearised and designed (gain and
filter); then in the same run one launch of fdyn_flight_modes open loop and closed loop and one of fdyn_block_modes on the filter
matrix Phi (I - L), beside one launch of fdyn_lqr_design.  Every launch is timed with device events, eager and as a captured graph,
over back-to-back launches after a warm-up.  Also the census of the fleet's modes, taken from the summary words on the device.

    python scripts/modes_throughput.py [--aircraft 65536] [--json profiles/modes_throughput_65536.json]
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
from hcrl_amd import _lib, layout as L  # noqa: E402
from hcrl_amd import lqg as G  # noqa: E402
from hcrl_amd import lqr as Q  # noqa: E402
from hcrl_amd import modes as MO  # noqa: E402
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


def census(m, good):
    """Per block over the lanes `good`: how many aircraft have 0, 2, 4 complex poles and 0..4 unstable ones; the ranges of the
    abscissa, the radius and the smallest damping ratio; the sweeps."""
    out = {"not_ok": int((m.status[good] != 0).sum()), "max_sweeps": int(m.iterations[good].max()),
           "mean_sweeps": float(m.iterations[good].double().mean())}
    for b, name in enumerate(("lon", "lat")):
        s = m.summary[b][:, good]
        out[name] = {"n_complex": torch.bincount(s[L.FD_MO_N_COMPLEX].long(), minlength=5).tolist(),
                     "n_unstable": torch.bincount(s[L.FD_MO_N_UNSTABLE].long(), minlength=5).tolist(),
                     "abscissa": [float(s[L.FD_MO_ABSCISSA].min()), float(s[L.FD_MO_ABSCISSA].max())],
                     "radius": [float(s[L.FD_MO_RADIUS].min()), float(s[L.FD_MO_RADIUS].max())],
                     "min_damping": [float(s[L.FD_MO_MIN_ZETA].min()), float(s[L.FD_MO_MIN_ZETA].max())]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--aircraft", type=int, default=65536)
    ap.add_argument("--dt", type=float, default=0.01)
    ap.add_argument("--repeats", type=int, default=500)
    ap.add_argument("--json", default=None, help="default for the default fleet: profiles/modes_throughput_65536.json")
    args = ap.parse_args()
    if args.json is None and args.aircraft == 65536:
        args.json = os.path.join(REPO, "profiles", "modes_throughput_65536.json")
    n, dev = args.aircraft, _lib.require_gpu()
    rs = np.random.RandomState(0)
    ty = (np.arange(n) % 2).astype(np.uint8)
    cond = (rs.uniform(15.0, 30.0, n), np.radians(rs.uniform(0.0, 5.0, n)), rs.uniform(-0.1, 0.3, n), rs.uniform(50.0, 200.0, n),
            rs.uniform(0.0, 6.28, n))
    scales = (rs.uniform(0.8, 1.2, n), 1.0, 1.0, 1.0, 1.0)

    fleet = BatchedSixDOF(n, "f64", types=TYPES, type_index=ty)
    trim = fleet.trim(*cond, scales=scales, strict=False)
    A, B = T.linearize_into(trim.x0, trim.u0, fleet.params, fleet.type_index, T.scale_rows(n, scales, dev))
    w, nz = Q.weights_tensor(None, n, dev), G.noise_tensor(None, n, dev)
    lqr, kal = Q.lqr_into(A, B, w), G.kalman_into(A, B, args.dt, nz)
    Mf = kal.filter_matrix().contiguous()
    good = trim.ok & lqr.ok & kal.ok
    torch.cuda.synchronize()
    res = {"aircraft": n, "dt": args.dt, "designs_not_ok": int((~good).sum())}
    res["lqr_design_us_eager"] = timed(lambda: Q.lqr_into(A, B, w, lqr), args.repeats)
    res["lqr_design_us_graph"] = timed(graphed(lambda: Q.lqr_into(A, B, w, lqr)), args.repeats)
    reports = {}
    for key, launch in (("modes_open", lambda out: MO.modes_into(A, B, None, out)), ("modes_closed", lambda out: MO.modes_into(A, B, lqr.K, out)),
                        ("block_modes_filter", lambda out: MO.block_modes_into(Mf, out))):
        out = launch(None)
        fn = lambda launch=launch, out=out: launch(out)  # noqa: E731
        res[f"{key}_us_eager"] = timed(fn, args.repeats)
        res[f"{key}_us_graph"] = timed(graphed(fn), args.repeats)
        res[f"{key}_over_lqr_design"] = res[f"{key}_us_graph"] / res["lqr_design_us_graph"]
        res[f"{key}_ns_per_aircraft"] = res[f"{key}_us_graph"] * 1e3 / n
        res[f"{key}_census"] = census(out, good)
        reports[key] = out

    print(f"{n} aircraft, {TYPES}, dt {args.dt}: designs not ok {res['designs_not_ok']}")
    for k in sorted(k for k in res if k.endswith(("_us_eager", "_us_graph"))):
        print(f"  {k:40s} {res[k]:10.1f} us")
    for key in reports:
        print(f"  {key}: / LQR design {res[f'{key}_over_lqr_design']:.2f}; {res[f'{key}_ns_per_aircraft']:.3f} ns per aircraft; "
              f"{json.dumps(res[f'{key}_census'])}")
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()

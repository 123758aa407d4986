#!/usr/bin/env python3
"""What trimming and linearising a whole fleet costs on the device.

65 536 aircraft of both airframes (alternating) with a per-aircraft mass spread of +-20 %, flight conditions spread over
V = 15..30 m/s, flight-path angle 0..5 deg and turn rate -0.1..0.3 rad/s.  One launch of fdyn_trim and one of fdyn_linearize
are timed with device events, eager and as a captured graph, over `--repeats` back-to-back launches after a warm-up.  For
context the script also times the NumPy restatement of the solver over the CPU oracle on the 288 aircraft of the test grid.

    python scripts/trim_throughput.py [--aircraft 65536] [--repeats 50] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import hcrl_amd  # noqa: E402,F401
from hcrl_amd import _lib, layout as L  # noqa: E402
from hcrl_amd import trim as T  # noqa: E402
from hcrl_amd.params import param_table  # noqa: E402

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--aircraft", type=int, default=65536)
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--no-cpu", action="store_true", help="skip the NumPy-over-oracle context timing")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    n, dev = args.aircraft, _lib.require_gpu()
    rs = np.random.RandomState(0)
    spec = torch.as_tensor(T.flight_condition(n, rs.uniform(15.0, 30.0, n), np.radians(rs.uniform(0.0, 5.0, n)),
                                              rs.uniform(-0.1, 0.3, n), rs.uniform(50.0, 200.0, n), rs.uniform(0.0, 6.28, n)), device=dev)
    ty = torch.as_tensor((np.arange(n) % 2).astype(np.uint8), device=dev)
    scales = T.scale_rows(n, (rs.uniform(0.8, 1.2, n), 1.0, 1.0, 1.0, 1.0), dev)
    params = torch.as_tensor(param_table(TYPES), device=dev)
    out = T.trim_into(spec, params, ty, scales)
    AB = T.linearize_into(out.x0, out.u0, params, ty, scales)
    torch.cuda.synchronize()
    iters = out.iterations.to(torch.float64)
    res = {"aircraft": n, "repeats": args.repeats, "not_ok": out.count_not_ok(), "iterations_mean": float(iters.mean()),
           "iterations_max": int(iters.max()), "residual_worst": float(out.residual.max()),
           "evaluations_per_trim_mean": float((iters * 15 + 1).mean()), "evaluations_per_linearize": 32}
    do_trim = lambda: T.trim_into(spec, params, ty, scales, out)                       # noqa: E731
    do_lin = lambda: T.linearize_into(out.x0, out.u0, params, ty, scales, AB)          # noqa: E731
    res["trim_us_eager"], res["linearize_us_eager"] = timed(do_trim, args.repeats), timed(do_lin, args.repeats)
    res["trim_us_graph"], res["linearize_us_graph"] = timed(graphed(do_trim), args.repeats), timed(graphed(do_lin), args.repeats)
    res["trim_aircraft_per_s"] = n / (res["trim_us_graph"] * 1e-6)
    res["linearize_aircraft_per_s"] = n / (res["linearize_us_graph"] * 1e-6)
    res["linearize_output_bytes"] = n * 8 * (L.FD_NX * L.FD_NX + L.FD_NX * L.FD_NU)
    if not args.no_cpu:
        sys.path.insert(0, os.path.join(REPO, "tests"))
        import trim_numpy as tn
        ty_h, spec_h, scales_h = tn.feasible_grid()
        t0 = time.perf_counter()
        tn.oracle_solve(ty_h, spec_h, scales_h, with_ab=False)
        res["numpy_over_oracle_288_trims_s"] = time.perf_counter() - t0
    print(f"{n} aircraft, {TYPES}, mass spread +-20 %: {res['not_ok']} not ok, iterations mean {res['iterations_mean']:.2f} "
          f"max {res['iterations_max']}, worst residual {res['residual_worst']:.2e}")
    for k in ("trim_us_eager", "trim_us_graph", "linearize_us_eager", "linearize_us_graph"):
        print(f"  {k:22s} {res[k]:10.1f} us")
    print(f"  trim {res['trim_aircraft_per_s']:.3e} aircraft/s, linearise {res['linearize_aircraft_per_s']:.3e} aircraft/s "
          f"({res['linearize_output_bytes'] / 2**20:.0f} MiB of A and B per launch)")
    if "numpy_over_oracle_288_trims_s" in res:
        print(f"  context: NumPy Newton over the CPU oracle, 288 aircraft: {res['numpy_over_oracle_288_trims_s']:.2f} s")
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What designing a Kalman filter for every aircraft and flying the LQG loop costs on the device, beside the LQR.

The fleet of scripts/lqr_throughput.py: 65 536 aircraft of both airframes (alternating), flight conditions spread over
V = 15..30 m/s, flight-path angle 0..5 deg and turn rate -0.1..0.3 rad/s, trimmed and linearised; then in the same run
  * one launch of fdyn_kf_design beside one launch of fdyn_lqr_design (on the linearisation with the +-20 % mass spread);
  * one launch of fdyn_lqg_step_* flying `--steps` control steps from trim with in-kernel draws and all accumulators, in each
    precision, beside one launch of fdyn_lqr_step_* of the same fleet and step count.
Every launch is timed with device events, eager and as a captured graph, over back-to-back launches after a warm-up; the state
is put back to its start before each timed series.

    python scripts/lqg_throughput.py [--aircraft 65536] [--steps 100] [--json profiles/lqg_throughput_65536.json]
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
from hcrl_amd import trim as T  # noqa: E402
from hcrl_amd.fleet import BatchedSixDOF  # noqa: E402

TYPES = ("rc_plane", "cessna")


def timed(fn, repeats, before=None):
    """Device time of one call in microseconds: `repeats` calls between two events, after a warm-up of 3."""
    for _ in range(3):
        fn()
    if before is not None:
        before()
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
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--dt", type=float, default=0.01)
    ap.add_argument("--design-repeats", type=int, default=200)
    ap.add_argument("--step-repeats", type=int, default=20)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
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
    torch.cuda.synchronize()
    res = {"aircraft": n, "steps": args.steps, "dt": args.dt, "trim_not_ok": trim.count_not_ok(), "lqr_design_not_ok": lqr.count_not_ok(),
           "kf_design_not_ok": kal.count_not_ok(), "kf_iterations_mean": float(kal.iters.to(torch.float64).mean()),
           "kf_iterations_max": int(kal.iters.max()), "kf_residual_worst": float(kal.residual[kal.ok].max())}
    for name, fn in (("lqr_design", lambda: Q.lqr_into(AB[0], AB[1], w, lqr)), ("kf_design", lambda: G.kalman_into(AB[0], AB[1], args.dt, nz, kal))):
        res[f"{name}_us_eager"] = timed(fn, args.design_repeats)
        res[f"{name}_us_graph"] = timed(graphed(fn), args.design_repeats)
    res["kf_over_lqr_design"] = res["kf_design_us_graph"] / res["lqr_design_us_graph"]

    # the fleets integrate their airframes' nominal blocks (no per-aircraft mass), so what is FLOWN is designed without the spread
    trim = fleet.trim(*cond, strict=False)
    lqr = fleet.design_lqr(strict=False)
    kal = fleet.design_kalman(args.dt, strict=False)
    start = trim.x0.clone()
    for precision in _lib.PRECISIONS:
        f = BatchedSixDOF(n, precision, types=TYPES, type_index=ty)
        surf = torch.zeros((L.FD_NU, n), dtype=f.dtype, device=dev)
        sat = torch.zeros(n, dtype=torch.int32, device=dev)
        state = G.LqgState.zeros(n, dev, seed=1)

        def put_back(f=f, state=state):
            f.x.copy_(start)
            state.reset()

        fly_lqr = lambda f=f, surf=surf, sat=sat: Q.step_into(f.precision, f.x, lqr, f.params, f.type_index, args.dt, args.steps, surf, sat)  # noqa: E731
        fly_lqg = lambda f=f, surf=surf, sat=sat, state=state: G.step_into(f.precision, f.x, lqr, kal, state, f.params, f.type_index,  # noqa: E731
                                                                            args.dt, args.steps, "estimate", None, surf, sat)
        for name, fn in (("lqr_step", fly_lqr), ("lqg_step", fly_lqg)):
            res[f"{name}_{precision}_us_eager"] = timed(fn, args.step_repeats, put_back)
            res[f"{name}_{precision}_us_graph"] = timed(graphed(fn), args.step_repeats, put_back)
        res[f"lqg_over_lqr_step_{precision}"] = res[f"lqg_step_{precision}_us_graph"] / res[f"lqr_step_{precision}_us_graph"]
        # what the timed flight does: 10 s from trim on the default sensor noise, under the estimate and under the measurement
        good = trim.ok & lqr.ok & kal.ok
        out = {}
        for fb in ("estimate", "measurement"):
            put_back()
            for _ in range(int(round(10.0 / (args.dt * args.steps)))):
                G.step_into(f.precision, f.x, lqr, kal, state, f.params, f.type_index, args.dt, args.steps, fb, None, surf, sat)
            out[fb] = (state.err_est[:, good].clone(), state.err_meas[:, good].clone(), state.chatter[:, good].clone())
        res[f"err_est_over_err_meas_worst_{precision}"] = float((out["estimate"][0] / out["estimate"][1]).max())
        res[f"chatter_ratio_worst_{precision}"] = float((out["estimate"][2] / out["measurement"][2]).max())
        res[f"chatter_ratio_median_{precision}"] = float((out["estimate"][2] / out["measurement"][2]).median())

    print(f"{n} aircraft, {TYPES}: trim not ok {res['trim_not_ok']}, LQR design not ok {res['lqr_design_not_ok']}, Kalman design not ok "
          f"{res['kf_design_not_ok']}, iterations mean {res['kf_iterations_mean']:.2f} max {res['kf_iterations_max']}, "
          f"worst residual {res['kf_residual_worst']:.2e}")
    for k in ("lqr_design_us_eager", "lqr_design_us_graph", "kf_design_us_eager", "kf_design_us_graph"):
        print(f"  {k:34s} {res[k]:10.1f} us")
    print(f"  Kalman design / LQR design: {res['kf_over_lqr_design']:.3f}")
    for p in _lib.PRECISIONS:
        for k in (f"lqr_step_{p}_us_eager", f"lqr_step_{p}_us_graph", f"lqg_step_{p}_us_eager", f"lqg_step_{p}_us_graph"):
            print(f"  {k:34s} {res[k]:10.1f} us")
        print(f"  LQG / LQR step, {p}: {res[f'lqg_over_lqr_step_{p}']:.3f}; 10 s from trim: err_est / err_meas worst "
              f"{res[f'err_est_over_err_meas_worst_{p}']:.3f}, chatter ratio median {res[f'chatter_ratio_median_{p}']:.4f} worst "
              f"{res[f'chatter_ratio_worst_{p}']:.4f}")
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""LQG on the sensor layer's default noise: trim -> linearise -> design (gain and Kalman filter) -> fly, one aircraft per
(airframe, airspeed).

Prints one table over airframe x V: the slowest pole of each block's filter Phi (I - L) (as a discrete radius and as a
continuous rate), the estimate's error against the measurement's on the noisiest words, and the step-to-step control chatter
with the filter (feedback = estimate) and without it (feedback = measurement), over `--seconds` of flight from trim.  The
eigenvalues are NumPy's, on the host, for the table only: the design certifies the filter per aircraft without them (status 0).

    python examples/lqg_noise.py [--seconds 10] [--dt 0.01] [--gyro 0.01]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hcrl_amd  # noqa: E402,F401
from hcrl_amd.fleet import BatchedSixDOF  # noqa: E402
from hcrl_amd.lqg import KalmanNoise, describe_status  # noqa: E402

TYPES = ("rc_plane", "cessna")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--dt", type=float, default=0.01)
    ap.add_argument("--gyro", type=float, default=0.01, help="gyro noise (rad/s); the other sensors keep their defaults")
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    speeds = np.array([12.0, 15.0, 18.0, 20.0, 25.0, 30.0])
    ty = np.repeat(np.arange(len(TYPES), dtype=np.uint8), len(speeds))
    V = np.tile(speeds, len(TYPES))
    steps = int(round(args.seconds / args.dt))
    noise = KalmanNoise(noise_config={"imu_gyro_stddev": args.gyro})
    out = {}
    for feedback in ("estimate", "measurement"):
        fleet = BatchedSixDOF(len(V), "f64", types=TYPES, type_index=ty)
        fleet.trim(V, 0.0, 0.0, strict=False)
        fleet.design_lqr(strict=False)
        kal = fleet.design_kalman(args.dt, noise, strict=False)
        fleet.lqg.seed = args.seed
        fleet.step_lqg(steps, feedback)
        s = fleet.lqg
        out[feedback] = dict(err_est=s.err_est.T.cpu().numpy() / steps, err_meas=s.err_meas.T.cpu().numpy() / steps,
                             chatter=s.chatter.T.cpu().numpy() / steps, sat=fleet.lqr_saturated_steps.cpu().numpy())
    radius = np.abs(np.linalg.eigvals(kal.filter_matrix().permute(3, 0, 1, 2).cpu().numpy())).max(axis=-1)      # [n][2]
    status = kal.status.cpu().numpy()
    e, m = out["estimate"], out["measurement"]
    print(f"{args.seconds:g} s from trim, dt {args.dt:g} s, sensor noise: velocity 0.1 m/s, gyro {args.gyro:g} rad/s, attitude 0.01 rad")
    print("airframe     V   filter radius lon / lat  (slowest pole 1/s)   rms error of q: estimate / measurement   of u: est / meas   "
          "rms chatter elevator, aileron: estimate / measurement")
    for k in range(len(V)):
        if status[k]:
            print(f"{TYPES[ty[k]]:9s} {V[k]:5.1f}  no filter: {describe_status(status[k])}")
            continue
        rate = np.log(radius[k]) / args.dt
        print(f"{TYPES[ty[k]]:9s} {V[k]:5.1f}   {radius[k, 0]:.3f} / {radius[k, 1]:.3f}  ({rate[0]:6.2f} / {rate[1]:6.2f})        "
              f"{np.sqrt(e['err_est'][k, 2]):.4f} / {np.sqrt(e['err_meas'][k, 2]):.4f}         "
              f"{np.sqrt(e['err_est'][k, 0]):.3f} / {np.sqrt(e['err_meas'][k, 0]):.3f}     "
              f"{np.sqrt(e['chatter'][k, 0]):.5f} / {np.sqrt(m['chatter'][k, 0]):.5f},  "
              f"{np.sqrt(e['chatter'][k, 1]):.5f} / {np.sqrt(m['chatter'][k, 1]):.5f}")


if __name__ == "__main__":
    main()

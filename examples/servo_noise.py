#!/usr/bin/env python3
"""The LQ servo on the sensor layer's default noise: trim -> linearise -> design (servo gain and the servo's Kalman filter) ->
command -> fly, one aircraft per (airframe, airspeed).

Every aircraft is told to speed up by 4 m/s, climb 30 m and turn 60 deg one second after the start (the probe commands of
DESIGN.md section 7j) and flies `--seconds` on the estimate (feedback = estimate) and on the raw measurements (feedback =
measurement), with the same seed.  Prints one table over airframe x V: the rms of the true airspeed, altitude and heading errors over
the last 10 s, the worst err_est / err_meas of the ten estimated words (below 1: the estimate beats the sensor), and the
step-to-step chatter of elevator, throttle and aileron with the filter relative to without it.

    python examples/servo_noise.py [--seconds 40] [--dt 0.01] [--altimeter 0.5]
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
from hcrl_amd.servo_lqg import ServoKalmanNoise, describe_status  # noqa: E402

TYPES = ("rc_plane", "cessna")
WORDS = ("u", "w", "q", "theta", "z", "v", "p", "r", "phi", "psi")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=40.0)
    ap.add_argument("--dt", type=float, default=0.01)
    ap.add_argument("--altimeter", type=float, default=0.5, help="altimeter noise (m); the other sensors keep their defaults")
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    speeds = np.array([15.0, 18.0, 20.0, 25.0, 30.0])
    ty = np.repeat(np.arange(len(TYPES), dtype=np.uint8), len(speeds))
    V = np.tile(speeds, len(TYPES))
    chunk = 10
    launches, first, tail = int(round(args.seconds / args.dt)) // chunk, int(round(1.0 / args.dt)) // chunk, int(round(10.0 / args.dt)) // chunk
    noise = ServoKalmanNoise(noise_config={"altitude_stddev": args.altimeter})
    out = {}
    for feedback in ("estimate", "measurement"):
        fleet = BatchedSixDOF(len(V), "f64", types=TYPES, type_index=ty)
        fleet.trim(V, 0.0, 0.0, strict=False)
        fleet.design_servo(strict=False)
        kal = fleet.design_servo_kalman(args.dt, noise, strict=False)
        fleet.servo_lqg.seed = args.seed
        ref = fleet.servo.ref.clone()
        sq = torch.zeros_like(fleet.servo.err)
        for k in range(launches):
            if k == first:
                fleet.command_servo(heading=ref[L.FD_SVR_HEADING] + np.radians(60.0), speed=ref[L.FD_SVR_SPEED] + 4.0,
                                    altitude=ref[L.FD_SVR_ALTITUDE] + 30.0)
            fleet.step_servo_lqg(chunk, feedback)
            if k >= launches - tail:
                sq += fleet.servo.err ** 2                       # the true errors, sampled every `chunk` steps
        s = fleet.servo_lqg
        out[feedback] = dict(rms=torch.sqrt(sq / tail).T.cpu().numpy(), ratio=(s.err_est / s.err_meas).T.cpu().numpy(),
                             chatter=s.chatter.T.cpu().numpy())
    status = kal.status.cpu().numpy()
    e, m = out["estimate"], out["measurement"]
    print(f"{args.seconds:g} s, dt {args.dt:g} s, +4 m/s, +30 m, +60 deg at 1 s; sensor noise: velocity 0.1 m/s, gyro 0.01 rad/s, attitude 0.01 rad, "
          f"altimeter {args.altimeter:g} m")
    print("airframe     V   rms |e_V| m/s, |e_h| m, |e_psi| rad over the last 10 s: estimate / measurement          worst err_est / err_meas (word)   "
          "chatter with / without the filter: elevator, throttle, aileron")
    for k in range(len(V)):
        if status[k]:
            print(f"{TYPES[ty[k]]:9s} {V[k]:5.1f}  no filter: {describe_status(status[k])}")
            continue
        w = int(np.argmax(e["ratio"][k]))
        c = e["chatter"][k] / m["chatter"][k]
        print(f"{TYPES[ty[k]]:9s} {V[k]:5.1f}   " + "   ".join(f"{e['rms'][k, j]:.4f} / {m['rms'][k, j]:.4f}" for j in range(3)) +
              f"        {e['ratio'][k, w]:.3f} ({WORDS[w]})          {c[L.FD_U_ELEVATOR]:.3f}, {c[L.FD_U_THROTTLE]:.3f}, {c[L.FD_U_AILERON]:.3f}")


if __name__ == "__main__":
    main()

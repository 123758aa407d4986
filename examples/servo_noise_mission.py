#!/usr/bin/env python3
"""The 300 m square flown by the LQ servo on the sensor layer's default noise: trim -> design (servo gain, servo filter, position
filter) -> fly the mission with the guidance on the truth, on the estimate and on the raw measurement.

The four conditions of the project's square (rc_plane at 15 and 20 m/s, cessna at 20 m/s, dt 0.01; cessna at 25 m/s, dt 0.02),
each its own fleet of one (the waypoint table carries the aircraft's own speed).  Prints per condition and feedback: completion
time, lateral chatter (aileron + rudder, relative to the truth flight), err_pos[0] / err_pos[1] (the filtered position's squared
error over the raw measurement's) and the largest TRUE cross-track distance.  Then a per-aircraft weight sweep on the estimate in
one launch per 100 steps: `--sweep` rc_planes at 20 m/s whose heading and heading-integral maxima are scaled 0.5 .. 2, ranked by
completion time.

    python examples/servo_noise_mission.py [--sweep 16] [--max-seconds 180]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hcrl_amd  # noqa: E402,F401
from hcrl_amd import layout as L  # noqa: E402
from hcrl_amd.config import square_mission  # noqa: E402
from hcrl_amd.fleet import BatchedSixDOF  # noqa: E402
from hcrl_amd.servo import ServoWeights  # noqa: E402

SQUARE = (("rc_plane", 15.0, 0.01), ("rc_plane", 20.0, 0.01), ("cessna", 20.0, 0.01), ("cessna", 25.0, 0.02))
SIZE, ALTITUDE, CHUNK = 300.0, 100.0, 100


def fly(fleet, feedback, max_steps):
    for _ in range(max_steps // CHUNK):
        fleet.fly_servo_lqg_mission(CHUNK, feedback)
        if bool(fleet.servo_mission_complete().all()):          # a read-back per launch: an example, not a benchmark
            break


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweep", type=int, default=16)
    ap.add_argument("--max-seconds", type=float, default=180.0)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    print("airframe     V    dt   feedback      complete   time s   lateral chatter / truth's   err_pos ratio   true cross-track m")
    for name, V, dt in SQUARE:
        base = None
        for feedback in ("truth", "estimate", "measurement"):
            fleet = BatchedSixDOF(1, "f64", types=(name,))
            fleet.trim(V, altitude=ALTITUDE, heading=0.3)
            fleet.design_servo()
            fleet.design_servo_kalman(dt)
            fleet.servo_lqg.seed = args.seed
            mission = fleet.start_servo_lqg_mission(square_mission(SIZE, ALTITUDE, V), acceptance_radius=40.0)
            fly(fleet, feedback, int(round(args.max_seconds / dt)))
            lat = float(fleet.servo_lqg.chatter[[L.FD_U_AILERON, L.FD_U_RUDDER]].sum())
            base = lat if base is None else base
            print(f"{name:9s} {V:5.1f}  {dt:.2f}  {feedback:12s}  {str(bool(mission.complete()[0])):8s}  {float(mission.mission_time(dt)[0]):7.2f}   "
                  f"{lat / base:24.2f}   {float(fleet.servo_position_state.error_ratio()[0]):13.3f}   {float(mission.stats[L.FD_MST_CROSS_TRACK][0]):18.2f}")

    n, dt, V = args.sweep, 0.01, 20.0
    scale = np.geomspace(0.5, 2.0, n)
    fleet = BatchedSixDOF(n, "f64", types=("rc_plane",))
    fleet.trim(V, altitude=ALTITUDE, heading=0.3)
    design = fleet.design_servo(ServoWeights(psi=0.1 * scale, i_heading=0.2 * scale), strict=False)
    fleet.design_servo_kalman(dt)
    fleet.servo_lqg.seed = args.seed
    mission = fleet.start_servo_lqg_mission(square_mission(SIZE, ALTITUDE, V), acceptance_radius=40.0)
    fly(fleet, "estimate", int(round(args.max_seconds / dt)))
    t = mission.mission_time(dt).cpu().numpy()
    done, ok = mission.complete().cpu().numpy(), design.ok.cpu().numpy()
    ct = mission.stats[L.FD_MST_CROSS_TRACK].cpu().numpy()
    lat = fleet.servo_lqg.chatter[[L.FD_U_AILERON, L.FD_U_RUDDER]].sum(dim=0).cpu().numpy()
    print(f"\nweight sweep on the estimate, rc_plane at {V:g} m/s, {n} aircraft in one fleet, ranked by completion time:")
    print("rank   psi max rad   i_heading max rad s   complete   time s   true cross-track m   lateral chatter")
    order = np.lexsort((t, ~(done & ok)))
    for rank, k in enumerate(order, 1):
        print(f"{rank:4d}   {0.1 * scale[k]:11.3f}   {0.2 * scale[k]:19.3f}   {str(bool(done[k] and ok[k])):8s}   {t[k]:6.2f}   {ct[k]:18.2f}   {lat[k]:15.4f}")
    assert torch.isfinite(fleet.x).all()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The waypoint square of configs/missions/square_pattern.yaml flown by the LQ servo in a moving air mass (fdyn_servo_mission_wind_*):
a ladder of steady crosswinds, then gusts, both airframes, every aircraft started in trim relative to its own air.

Prints per airframe and condition whether the square was completed, the completion time, the largest distance off the leg, the
altitude excursion, the lowest airspeed and the steps with a clipped control: the kernel's own running statistics.  Then a sweep
in ONE launch: every combination of three heading, altitude and bank penalties per airframe in the strongest crosswind of the
ladder plus gusts, ranked by completion, completion time and distance off the leg -- which weight set still flies the square.

    python examples/servo_wind_mission.py [--precision f64] [--speed 15] [--guidance PP] [--winds 0 2 4 6 8] [--turbulence 0.08]
"""
import argparse
import itertools
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hcrl_amd  # noqa: E402,F401
from hcrl_amd import config as cfgmod, layout as L  # noqa: E402
from hcrl_amd import servo as SV  # noqa: E402
from hcrl_amd.disturbances import Disturbances  # noqa: E402
from hcrl_amd.fleet import BatchedSixDOF  # noqa: E402

TYPES = ("rc_plane", "cessna")
HEAD = "   complete   time (s)   off the leg (m)   |altitude error| (m)   min airspeed (m/s)   saturated steps"


def fly(fleet, wind, wps, guidance, fc, max_steps, dt):
    """Put the trimmed fleet in trim relative to its air, then the whole mission in one launch -> (ServoMission, saturated steps)."""
    fleet.x.copy_(wind.ground_state(fleet.x))
    fleet._saturated_steps().zero_()
    mission = fleet.start_servo_mission(wps, guidance_type=guidance, flight_config=fc)
    fleet.fly_servo_mission(max_steps, dt, wind=wind)
    return mission, fleet.lqr_saturated_steps.cpu().numpy()


def row(mission, sat, i, dt):
    s = mission.stats.cpu().numpy()
    return (f"   {str(bool(mission.complete()[i])):>8s}   {float(mission.mission_time(dt)[i]):8.1f}   {s[L.FD_MST_CROSS_TRACK, i]:15.1f}   "
            f"{s[L.FD_MST_ALTITUDE_ERROR, i]:20.2f}   {s[L.FD_MST_MIN_AIRSPEED, i]:18.1f}   {sat[i]:15d}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="f64", choices=("f64", "mixed", "f32"))
    ap.add_argument("--speed", type=float, default=None, help="trim and mission airspeed, m/s (default: the YAML's)")
    ap.add_argument("--guidance", default=None, help="LOS, PP or anything else for the plain line of sight (default: the YAML's)")
    ap.add_argument("--winds", type=float, nargs="+", default=(0.0, 2.0, 4.0, 6.0, 8.0), help="the ladder: m/s from the west (abeam of the first leg)")
    ap.add_argument("--turbulence", type=float, default=0.08, help="gust sigma as a fraction of the airspeed")
    ap.add_argument("--gust-length", type=float, default=150.0, help="gust length scale, m")
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    fc = cfgmod.load_controller_config("cascaded_pid.yaml")
    mc = cfgmod.load_mission_config("square_pattern.yaml")
    guidance = args.guidance or mc.guidance
    speed = mc.speed if args.speed is None else args.speed
    wps = cfgmod.square_mission(mc.pattern_size, mc.altitude, speed)
    dt, max_steps = mc.dt, int(round(mc.max_duration / mc.dt))
    nt, ladder = len(TYPES), list(args.winds)

    # the ladder: one aircraft per airframe and rung, the air moving toward the east (the first leg runs north) with a 1 m/s downdraft
    n = nt * len(ladder)
    fleet = BatchedSixDOF(n, args.precision, types=TYPES, type_index=np.repeat(np.arange(nt, dtype=np.uint8), len(ladder)))
    fleet.trim(speed, altitude=mc.altitude, heading=0.0)
    fleet.design_servo()
    wind = SV.ServoWind.steady(n, fleet.device, np.tile(ladder, nt), np.pi / 2.0, vertical=np.where(np.tile(ladder, nt) > 0.0, 1.0, 0.0))
    mission, sat = fly(fleet, wind, wps, guidance, fc, max_steps, dt)
    print(f"{mc.name}: {mc.pattern_size:.0f} m square at {mc.altitude:.0f} m, {speed:.0f} m/s, guidance {guidance}, {args.precision}, dt {dt}")
    print("steady wind toward the east and a 1 m/s downdraft\n   airframe   wind (m/s)" + HEAD)
    for i in range(n):
        print(f"  {TYPES[i // len(ladder)]:>9s}   {ladder[i % len(ladder)]:10.1f}" + row(mission, sat, i, dt))

    # gusts: the same rungs with turbulence on top, normals drawn in the kernel
    fleet.trim(speed, altitude=mc.altitude, heading=0.0)
    fleet.design_servo()
    rng = np.random.default_rng(args.seed)
    gusty = SV.ServoWind.from_disturbances(Disturbances(turbulence_intensity=args.turbulence, gust_length=args.gust_length), n, speed, dt,
                                           fleet.device, rng, seed=args.seed)
    gusty.rows[:L.FD_SW_WIND_D + 1] = wind.rows[:L.FD_SW_WIND_D + 1]
    mission, sat = fly(fleet, gusty, wps, guidance, fc, max_steps, dt)
    print(f"\nthe same with gusts: sigma {args.turbulence * speed:.1f} m/s, length {args.gust_length:.0f} m\n   airframe   wind (m/s)" + HEAD)
    for i in range(n):
        print(f"  {TYPES[i // len(ladder)]:>9s}   {ladder[i % len(ladder)]:10.1f}" + row(mission, sat, i, dt))

    # the sweep: Bryson maxima of the heading, altitude and bank words in the strongest wind of the ladder plus gusts, one design launch, one flight
    grid = list(itertools.product((0.05, 0.1, 0.2), (1.0, 2.0, 4.0), (0.1, 0.2, 0.4)))                  # psi (rad), z (m), phi (rad)
    n = len(grid) * nt
    sweep = BatchedSixDOF(n, args.precision, types=TYPES, type_index=np.repeat(np.arange(nt, dtype=np.uint8), len(grid)))
    sweep.trim(speed, altitude=mc.altitude, heading=0.0)
    g = np.array(grid * nt)
    design = sweep.design_servo(weights=SV.ServoWeights(psi=g[:, 0], z=g[:, 1], phi=g[:, 2]), strict=False)
    air = SV.ServoWind.from_disturbances(Disturbances(wind_speed=max(ladder), wind_direction=np.pi / 2.0, wind_vertical=1.0,
                                                      turbulence_intensity=args.turbulence, gust_length=args.gust_length), n, speed, dt,
                                         sweep.device, rng, seed=args.seed + 1)
    m, sat = fly(sweep, air, wps, guidance, fc, max_steps, dt)
    ok = (design.ok & m.complete()).cpu().numpy()
    t, off = m.mission_time(dt).cpu().numpy(), m.stats[L.FD_MST_CROSS_TRACK].cpu().numpy()
    print(f"\nweight sweep in {max(ladder):.0f} m/s and gusts: {n} designs, {int(design.ok.sum())} certified, {int(ok.sum())} completed the mission")
    for k, name in enumerate(TYPES):
        lanes = [i for i in range(k * len(grid), (k + 1) * len(grid)) if ok[i]]
        lanes.sort(key=lambda i: (round(t[i], 2), off[i]))
        print(f"  {name}: best five of {len(lanes)} by completion time, then distance off the leg\n     max psi (rad)   max z (m)   max phi (rad)" + HEAD)
        for i in lanes[:5]:
            print(f"     {g[i, 0]:13.2f}   {g[i, 1]:9.1f}   {g[i, 2]:13.2f}" + row(m, sat, i, dt))
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()

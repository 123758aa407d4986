"""The gain schedule of include/fdyn_servo_sched.h restated in NumPy (tests/servo_sched_numpy.py), flown over the CPU oracle's RK4.

  identity   a one-node table, and a table of equal nodes, ARE the unscheduled loop of servo_numpy.fly: bit for bit
  benefit    the four speed-change flights of tests/golden/servo_sched_reference.npz (15 <-> 30 m/s on both airframes, nodes at
             15 / 20 / 25 / 30 m/s, 40 s, peaks sampled every 10 steps) are reproduced, and the schedule entered with the measured
             airspeed at least halves the peak altitude error of the single design at the start speed in all four
  frozen     at every midpoint of the ladder on both airframes the interpolated gain stabilises the model linearised there
"""
import os

import numpy as np
import pytest

import lqr_numpy as ln
import servo_numpy as sn
import servo_mission_numpy as smn
import servo_sched_numpy as ssn
from conftest import GOLDEN

FIXTURE = os.path.join(GOLDEN, "servo_sched_reference.npz")


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same(a, b):
    return all(np.array_equal(_bits(p), _bits(q)) for p, q in zip(a, b))


def test_lookup_ends_nodes_and_interior():
    t = np.arange(3 * ssn.NSS, dtype=np.float64).reshape(3, ssn.NSS) ** 1.5
    t[:, ssn.SS_V] = (10.0, 20.0, 40.0)
    for sigma, pos, want in ((5.0, 0.0, t[0]), (10.0, 0.0, t[0]), (np.nan, 0.0, t[0]), (40.0, 2.0, t[2]), (1e9, 2.0, t[2]), (np.inf, 2.0, t[2]),
                             (20.0, 1.0, t[1] + 0.0 * (t[2] - t[1])), (15.0, 0.5, t[0] + 0.5 * (t[1] - t[0])), (25.0, 1.25, t[1] + 0.25 * (t[2] - t[1]))):
        words, p = ssn.lookup(t, sigma)
        assert p == pos and np.array_equal(_bits(words), _bits(want)), sigma
    assert ssn.lookup(t[:1], 3.0)[1] == 0.0 and ssn.lookup(t[:1], 30.0)[1] == 0.0
    assert np.array_equal(ssn.lookup(t[:1], np.nan)[0], t[0])


@pytest.mark.parametrize("on", [ssn.ON_AIRSPEED, ssn.ON_COMMAND])
def test_one_node_and_equal_nodes_are_the_unscheduled_loop(on):
    """120 steps with the probe's commands from step 40 on, two aircraft (a level rc_plane, a climbing cessna)."""
    f = sn.compare_flights()
    for i in (0, 1):
        step = smn.airframe_step(f["type"][i])
        V = float(f["spec"][i][0])
        one = np.array([ssn.node(V, f["x0"][i], f["u0"][i], f["K"][i])])
        equal = np.repeat(one, 3, axis=0)                                 # the same words under three equal airspeeds
        spread = equal.copy()
        spread[:, ssn.SS_V] = (V - 2.0, V + 1.0, V + 3.0)                 # and under airspeeds the flight moves through
        want = sn.fly(step, f["K"][i], f["x0"][i], f["u0"][i], f["x0"][i], f["ref0"][i], np.zeros(3), ln.DT, 40)
        want = sn.fly(step, f["K"][i], f["x0"][i], f["u0"][i], want[0], sn.commanded(want[1]), want[2], ln.DT, 80)
        for table in (one, equal, spread):
            got = ssn.fly(step, table, f["x0"][i], f["ref0"][i], np.zeros(3), ln.DT, 40, on)
            got = ssn.fly(step, table, got[0], sn.commanded(got[1]), got[2], ln.DT, 80, on)
            assert _same(got[:4], want[:4]) and got[4] == want[4], (i, len(table))
        assert want[4] > 0                                                # the clip and the frozen integrators were flown


def test_one_node_mission_is_the_unscheduled_mission():
    f = sn.compare_flights()
    wps, C = ssn.mission_square(smn.SHARED_SPEED), smn.consts("PP", smn.RADIUS, "freeze")
    i = 0
    step = smn.airframe_step(f["type"][i])
    one = np.array([ssn.node(float(f["spec"][i][0]), f["x0"][i], f["u0"][i], f["K"][i])])
    want = smn.fly(step, f["K"][i], f["x0"][i], f["u0"][i], f["x0"][i], f["ref0"][i], np.zeros(3), wps, C, 0, ln.DT, 120)
    for on in (ssn.ON_AIRSPEED, ssn.ON_COMMAND):
        got = ssn.fly_mission(step, one, f["x0"][i], f["ref0"][i], np.zeros(3), wps, C, 0, ln.DT, 120, on)
        assert _same([got[k] for k in ("x", "ref", "integ", "u", "stats")], [want[k] for k in ("x", "ref", "integ", "u", "stats")])
        assert (got["idx"], got["reached"], got["flown"], got["sat"]) == (want["idx"], want["reached"], want["flown"], want["sat"])
    assert want["reached"] == 1 and want["flown"] == 120


def test_the_four_flights_and_what_the_schedule_buys():
    got = ssn.benefit_flights()
    ref = np.load(FIXTURE)
    assert [tuple(r) for r in ref["flights"].tolist()] == [(n, str(a), str(b)) for n, a, b in ssn.BENEFIT]
    for how in ("single", "command", "airspeed"):
        print(f"peak |e_h| (m), {how}: {got[how]}")
        assert np.abs(got[how] - ref[how]).max() <= 1e-9, how              # the same fp64 arithmetic on another host's libm
    ratio = got["airspeed"] / got["single"]
    print(f"measured-airspeed schedule / single design: {ratio}")
    assert (ratio <= 0.5).all()
    assert (got["command"] < got["single"]).all()
    assert np.isfinite(got["end"]).all()
    # all runs end on the command.  A 15 m/s change is flown with the airspeed error on its clip for seconds, so the 4 m/s probe's
    # 1e-3 gates at 40 s do not carry over; asked here: every error is inside a tenth of its clip (servo_numpy.DEFAULT_LIMITS), that
    # is, the loop has long left the clipped region and is in its linear approach
    e = np.abs(got["end"])
    print(f"end errors: V {e[..., 0].max():.3e} m/s, h {e[..., 1].max():.3e} m, psi {e[..., 2].max():.3e} rad")
    assert all(e[..., k].max() <= 0.1 * sn.DEFAULT_LIMITS[k] for k in range(3))


@pytest.mark.parametrize("name", ssn.AIRFRAMES)
def test_frozen_point_modes_between_the_nodes(name):
    rows = ssn.frozen_point_modes(name)
    print(name, [(r["V"], round(r["abscissa"], 4)) for r in rows])
    assert [r["V"] for r in rows] == [17.5, 22.5, 27.5]
    assert all(r["abscissa"] < 0.0 for r in rows)

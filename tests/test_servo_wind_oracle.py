"""The servo in wind and gusts over the UNCHANGED CPU oracle (tests/servo_wind_numpy.py: the Galilean map once per control step).

(a) a steady horizontal wind on the plain servo step is the still-air flight shifted by W t in north / east;
(b) on every flight used here and by the device tests, each velocity, rate, pitch and derivative clamp of the integrator stays
    idle in both frames (the map is only valid away from them), no aircraft excluded;
(c) behaviour: the probe conditions hold their references in a 6 m/s wind from abeam and a 1 m/s downdraft switched on at 1 s,
    within the servo's own oracle gates, and miss them with the integrators frozen;
(d) the short mission: the largest crosswind of the ladder at which all ten aircraft complete, and the well-posedness margin;
(e) the truncation yardstick D of the device comparisons.

Measured here (fp64, this file's flights):
    (c) worst end errors over the four conditions: |e_V| 1.1e-6 m/s, |e_h| 2.9e-7 m, |e_psi| 6.5e-10 rad; integrators frozen:
        |e_h| 0.99 .. 1.29 m, |e_V| 0.07 .. 0.23 m/s
    (d) all ten complete at 8 m/s, the top of the ladder (803 .. 877 steps, heading-error clip 0.2 rad: servo_wind_numpy.MISSION_LIMITS):
        the device tests fly 8 m/s
    (e) D = 3.9e-5 m (position), 2.3e-6 m/s, 2.8e-7 rad, 1.0e-6 rad/s; integrators 2.3e-6 m, 7.9e-6 m s, 4.4e-7 rad s
"""
import numpy as np
import pytest

import lqr_numpy as ln
import servo_mission_numpy as mn
import servo_numpy as sn
import servo_wind_numpy as wn

ULP_V = 2.0 ** -48                       # one ulp of a velocity word in [16, 32) m/s: every |v| + |W| here is below 32


def test_a_steady_horizontal_wind_is_the_still_air_flight_shifted():
    """One control step.  Start: the still-air state x_s, mapped to the ground (v_g = v_s + b, b = R^T W: 0.5 ulp).  The windy step
    maps to the air (v_g - b: 0.5 ulp of v_g and 0.5 ulp of the result, so v_a is within 1.5 ulp of v_s), flies the still-air RK4
    (a perturbation of the velocity passes one step of dt <= 0.02 with gain 1 + dt |df/dx| <= 2 into every word: 3 ulp), maps back
    (0.5 ulp), and the expected value x_s' + b' carries 0.5 ulp of its own: 4 ulp of a velocity word on every word but north and
    east.  North and east: the same perturbation times dt, and the rounding of the sum p + W dt: 4 ulp of a velocity word times dt, plus 1 ulp of
    the position.
    The whole flight of n steps then stays within n times the step's bound: the closed loop does not expand a perturbation."""
    f = sn.compare_flights()
    W = wn.steady_rows(6.0, np.radians(70.0))
    Wa = wn.air_mass(W)
    for i in (0, 3, 7):
        step = mn.airframe_step(f["type"][i])
        rec = []
        x_s, ref_s, integ_s, _, _ = sn.fly(step, f["K"][i], f["x0"][i], f["u0"][i], f["x0"][i], f["ref0"][i], np.zeros(3), ln.DT, 100, record=rec)
        states = [np.array(f["x0"][i])] + [r[0] for r in rec]
        ref, integ = np.array(f["ref0"][i]), np.zeros(3)
        for k in range(100):                                  # restart from the still-air flight's words every step
            x1, ref1, integ1, _, _, _ = wn.fly(step, f["K"][i], f["x0"][i], f["u0"][i], wn.to_ground(states[k], Wa), ref, integ, W, ln.DT, 1)
            _, ref, integ, _, _ = sn.fly(step, f["K"][i], f["x0"][i], f["u0"][i], states[k], ref, integ, ln.DT, 1)
            want = wn.to_ground(states[k + 1], Wa, ln.DT)
            assert np.abs(x1[2:] - want[2:]).max() <= 4 * ULP_V, (i, k, np.abs(x1[2:] - want[2:]).max() / ULP_V)
            assert np.abs(x1[:2] - want[:2]).max() <= 4 * ULP_V * ln.DT + np.spacing(np.abs(want[:2]).max()), (i, k)
            assert np.abs(integ1 - integ).max() <= 4 * ULP_V and np.array_equal(ref1, ref)
        # the whole flight, never restarted
        xw, refw, integw, rows, _, sat = wn.fly(step, f["K"][i], f["x0"][i], f["u0"][i], wn.to_ground(f["x0"][i], Wa), f["ref0"][i], np.zeros(3), W, ln.DT, 100)
        want = wn.to_ground(x_s, Wa)
        want[:2] = x_s[:2] + Wa[:2] * (100 * ln.DT)
        assert np.abs(xw[2:] - want[2:]).max() <= 100 * 4 * ULP_V and np.abs(integw - integ_s).max() <= 100 * 4 * ULP_V
        assert np.abs(xw[:2] - want[:2]).max() <= 100 * (4 * ULP_V * ln.DT + np.spacing(np.abs(want[:2]).max()))
        assert np.array_equal(rows, W) and np.array_equal(refw, ref_s)


def _flights():
    """(name, parameter block, record) of every flight the tests of this file and the device tests fly."""
    import trim_numpy as tn
    out = []
    for k, r in enumerate(wn.probe_flights()):
        out.append((f"probe {k}", r["P"], r["record"]))
    f = sn.compare_flights()
    blocks = [tn.oracle_airframe(tn.TYPES[int(t)])[4] for t in f["type"]]
    for gusts in (False, True):
        c = wn.compare_flights(gusts=gusts)
        out += [(f"compare {i} gusts={gusts}", blocks[i], c["records"][i]) for i in range(len(blocks))]
    m = wn.mission_flights(wn.chosen_crosswind())
    out += [(f"mission {i}", blocks[i], m["records"][i]) for i in range(len(blocks))]
    return out


def test_b_every_clamp_stays_idle_in_both_frames():
    for name, P, record in _flights():
        m = wn.worst_margins(P, record)
        assert all(v > 0.0 for v in m.values()), (name, m)


def test_c_references_are_held_in_wind_and_downdraft():
    for r in wn.probe_flights():
        e = np.abs(r["err"])
        assert e[0] <= sn.GATE_V and e[1] <= sn.GATE_H and e[2] <= sn.GATE_PSI, (r["dt"], r["err"])
        # the wind was felt: abeam, the full crosswind as sideslip at the step it is switched on
        n1 = int(round(sn.T_COMMAND / r["dt"]))
        assert abs(abs(r["record"][n1][1][4] - r["record"][n1 - 1][1][4]) - wn.CROSSWIND) < 0.5
    # the test can fail: without integral action the downdraft costs altitude and the wind costs speed
    for r in wn.probe_flights(frozen=True):
        e = np.abs(r["err"])
        assert e[0] > sn.GATE_V or e[1] > sn.GATE_H or e[2] > sn.GATE_PSI, (r["dt"], r["err"])
        assert e[1] > 100 * sn.GATE_H


def test_d_short_mission_completes_in_the_chosen_crosswind():
    w = wn.chosen_crosswind()
    assert w == 8.0, w                                        # recorded: the top of the ladder; the device tests fly it
    m = wn.mission_flights(w)
    assert all(r["idx"] == 3 and r["reached"] == 3 and r["flown"] < mn.SHORT_STEPS for r in m["rows"])
    # well-posedness: no step at which the waypoint test hangs on the last bits
    gap = min(abs(rec[4] - mn.RADIUS) for recs in m["records"] for rec in recs)
    assert gap >= 1e-6, gap
    # the crosswind is felt: the fleet is pushed off its legs further than in still air
    f = sn.compare_flights()
    calm = dict(rows=[mn.fly(mn.airframe_step(f["type"][i]), f["K"][i], f["x0"][i], f["u0"][i], f["x0"][i], f["ref0"][i], np.zeros(3), m["wps"], m["C"],
                             0, ln.DT, mn.SHORT_STEPS, limits=wn.MISSION_LIMITS) for i in range(len(f["type"]))])
    assert np.mean([r["stats"][mn.MST_CROSS_TRACK] for r in m["rows"]]) > np.mean([r["stats"][mn.MST_CROSS_TRACK] for r in calm["rows"]])
    # zero rows reproduce the still-air mission's events and counters
    z = wn.mission_flights(0.0, steps=mn.SHORT_STEPS)
    for a, b in zip(z["rows"], calm["rows"]):
        assert (a["idx"], a["reached"], a["flown"], a["sat"], a["events"]) == (b["idx"], b["reached"], b["flown"], b["sat"], b["events"])


def test_e_truncation_yardstick():
    Dx, Di = wn.truncation_yardstick()
    groups = wn.yardstick_groups()
    assert np.all(Dx > 0.0) and np.all(Di > 0.0)
    # fourth order: the yardstick is far below the motion it measures, and far above rounding
    for k, v in groups.items():
        assert 1e-10 < v < 1e-3, (k, v)
    # the mission's: the same events with dt and with two half steps, so the end states are comparable
    a, b = wn.mission_flights(0.0, steps=mn.SHORT_STEPS), wn.mission_flights(0.0, steps=mn.SHORT_STEPS, substeps=2)
    assert all(p["events"] == q["events"] for p, q in zip(a["rows"], b["rows"]))
    gm = wn.mission_yardstick_groups()
    for k, v in gm.items():
        assert 1e-10 < v < 1e-2, (k, v)

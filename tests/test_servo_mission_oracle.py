"""The servo's waypoint missions on the CPU: the restatement (tests/servo_mission_numpy.py) of include/fdyn_mission.h.

The restated guidance is pinned to the CPU oracle, not to itself: followed by orc_hsa_agent it must equal orc_waypoint_agent on
the same PID state bit for bit, and the restated mission update must equal orc_mission_update.  The loop is then flown over the
oracle's RK4.

Gates (none derived from what the restatement returns):
  guidance      bit-equal surfaces and PID states on 2400 seeded pairs per guidance type; every branch taken at least 20 times
  short mission three waypoints reached and the mission complete within 1500 steps; state finite; |roll| < 2.09 rad, |pitch| < 1.40 rad
                (the env's termination limits); | distance to the active waypoint - 40 m | >= 1e-6 m at every step; with restart
                at least four events in 2000 steps
  square        five waypoints within 180 s; altitude within 10 m of 100 m (the altitude error clip); airspeed above 8 m/s
Measured here: short mission with each aircraft's own trim speed 735 to 1110 steps, with the shared 20 m/s 840 to 967; the
smallest | distance - 40 m | 1.2e-3 m; restart 4 events each; square 44.4 to 72.1 s, altitude -1.3 to +3.7 m.
"""
import numpy as np
import pytest

import servo_mission_numpy as mn
from hcrl_amd import layout as L
from hcrl_amd.config import pid_table
from oracle import oracle as orc

PAIRS = 2400


def _pairs(seed, gtype):
    """Seeded (x, wp, pid_state) triples: waypoints from 0.1 m to 600 m away in every direction, one in five with a NaN speed."""
    rs = np.random.RandomState(seed)
    for _ in range(PAIRS):
        x = np.zeros(L.FD_NX)
        x[0:3] = rs.uniform(-300.0, 300.0, 2).tolist() + [-rs.uniform(50.0, 150.0)]
        x[3:6] = [rs.uniform(6.0, 30.0), rs.uniform(-2.0, 2.0), rs.uniform(-2.0, 2.0)]
        x[6:9] = [rs.uniform(-0.6, 0.6), rs.uniform(-0.3, 0.3), rs.uniform(-np.pi, np.pi)]
        x[9:12] = rs.uniform(-0.3, 0.3, 3)
        dist, bearing = 10.0 ** rs.uniform(-1.0, np.log10(600.0)), rs.uniform(-np.pi, np.pi)
        wp = np.array([x[0] + dist * np.cos(bearing), x[1] + dist * np.sin(bearing), -x[2] + rs.uniform(-20.0, 20.0),
                       np.nan if rs.rand() < 0.2 else rs.uniform(12.0, 28.0)])
        st = (rs.uniform(-0.2, 0.2, L.FD_NPID * L.FD_NPS)).astype(np.float32)
        yield x, wp, st


@pytest.mark.parametrize("gtype,name", [(mn.LOS, "LOS"), (mn.PP, "PP"), (mn.DEFAULT, "default")])
def test_restated_guidance_is_the_oracles(gtype, name):
    C = mn.consts({mn.LOS: "LOS", mn.PP: "PP", mn.DEFAULT: "none"}[gtype])
    assert int(C[L.FD_C_GUIDANCE_TYPE]) == gtype
    cfg = np.ascontiguousarray(pid_table().reshape(-1))
    count = {}
    for x, wp, st in _pairs(100 + gtype, gtype):
        d = orc.derived(x)
        st_a, st_b = st.copy(), st.copy()
        want, got = np.zeros(L.FD_NU), np.zeros(L.FD_NU)
        orc.lib.orc_waypoint_agent(orc.fp(cfg), orc.fp(st_a), orc.dp(C), orc.dp(wp), orc.dp(x), orc.dp(d), 0.01, orc.dp(want))
        taken = set()
        h, v, a = mn.guidance(C, wp, x, d, taken)
        cmd = np.array([h, v, a], np.float64)
        orc.lib.orc_hsa_agent(orc.fp(cfg), orc.fp(st_b), orc.dp(C), orc.dp(cmd), orc.dp(x), orc.dp(d), 0.01, orc.dp(got))
        assert np.array_equal(want.view(np.uint64), got.view(np.uint64)), (name, x, wp, want, got)
        assert np.array_equal(st_a.view(np.uint32), st_b.view(np.uint32)), (name, x, wp)
        for t in taken:
            count[t] = count.get(t, 0) + 1
    print(f"{name}: branches taken over {PAIRS} pairs: {sorted(count.items())}")
    need = {"nan_speed", "within_1m", "speed_reduction"} | {mn.LOS: {"los_anticipation"}, mn.PP: {"pp_proximity", "pp_within_1m"}, mn.DEFAULT: set()}[gtype]
    for branch in need:
        assert count.get(branch, 0) >= 20, (name, branch, count)


def test_restated_mission_update_is_the_oracles():
    rs = np.random.RandomState(7)
    C = mn.consts()
    wps = mn.short_mission(100.0, 20.0)
    hits = 0
    for k in range(3000):
        idx = int(rs.randint(0, len(wps) + 1))
        x = np.zeros(L.FD_NX)
        if idx < len(wps):
            r = mn.RADIUS * (1.0 + rs.uniform(-1.0, 1.0) * 10.0 ** rs.uniform(-9.0, 0.0))         # on both sides of the radius, down to 1e-9 of it
            v = rs.normal(size=3)
            x[0:3] = np.array([wps[idx][0], wps[idx][1], -wps[idx][2]]) + r * v / np.linalg.norm(v)
        i32 = np.array([idx], np.int32)
        want = orc.lib.orc_mission_update(orc.dp(C), orc.dp(np.ascontiguousarray(wps.reshape(-1))), len(wps), orc.ip(i32), orc.dp(x))
        got_idx, got = mn.mission_update(C, wps, idx, x)
        assert (got_idx, got) == (int(i32[0]), want), (k, idx, x)
        hits += got
    assert 500 < hits < 2500


@pytest.mark.parametrize("per_aircraft", [True, False], ids=["own-speed", "shared-speed"])
def test_short_mission_completes_and_its_events_are_well_posed(per_aircraft):
    r = mn.short_flights(per_aircraft=per_aircraft)
    assert len(r["rows"]) == 10
    flown, margins = [], []
    for row, rec in zip(r["rows"], r["records"]):
        assert row["reached"] == 3 and row["idx"] == 3 and row["flown"] < mn.SHORT_STEPS and len(row["events"]) == 3, row
        xs = np.array([q[0] for q in rec] + [row["x"]])
        assert np.isfinite(xs).all() and np.isfinite(row["integ"]).all() and np.isfinite(row["ref"]).all()
        assert np.abs(xs[:, mn.X_ROLL]).max() < 2.09 and np.abs(xs[:, mn.X_PITCH]).max() < 1.40
        assert row["stats"][mn.MST_ROLL] == np.abs(xs[:row["flown"], mn.X_ROLL]).max()     # the states the guidance saw
        margins.append(min(abs(q[1] - mn.RADIUS) for q in rec))
        flown.append(row["flown"])
    print(f"short mission, {'own' if per_aircraft else 'shared'} speed: {min(flown)} to {max(flown)} steps; smallest |distance - radius| {min(margins):.3e} m")
    assert min(margins) >= 1e-6, margins


def test_short_mission_with_restart_keeps_flying():
    r = mn.short_flights(on_complete="restart")
    events = [len(row["events"]) for row in r["rows"]]
    margin = min(min(abs(q[1] - mn.RADIUS) for q in rec) for rec in r["records"])
    print(f"restart, {mn.RESTART_STEPS} steps: events {events}; smallest |distance - radius| {margin:.3e} m")
    assert min(events) >= 4 and margin >= 1e-6
    assert all(row["flown"] == mn.RESTART_STEPS and row["idx"] < 3 for row in r["rows"])


def test_the_projects_square():
    for (name, V, dt), r in zip(mn.SQUARE, mn.square_flights()):
        xs = np.array([q[0] for q in r["records"]])[:r["flown"]]                    # the states the guidance saw
        alt = -xs[:, mn.X_D] - mn.SQUARE_ALTITUDE
        speed = np.sqrt((xs[:, 3:6] ** 2).sum(axis=1))
        print(f"{name} {V} m/s dt {dt}: {r['reached']} waypoints in {r['flown'] * dt:.1f} s; altitude {alt.min():+.2f} to {alt.max():+.2f} m; "
              f"airspeed {speed.min():.2f} to {speed.max():.2f} m/s; |roll| {r['stats'][mn.MST_ROLL]:.2f} rad; cross-track {r['stats'][mn.MST_CROSS_TRACK]:.1f} m; "
              f"saturated {r['sat']} of {r['flown']} steps")
        assert r["reached"] == 5 and r["idx"] == 5 and r["flown"] * dt <= mn.SQUARE_MAX_DURATION
        assert np.abs(alt).max() <= 10.0 and speed.min() > 8.0
        assert r["stats"][mn.MST_ALTITUDE_ERROR] == np.abs(alt).max() and r["stats"][mn.MST_MIN_AIRSPEED] == pytest.approx(speed.min(), abs=1e-12)

"""fdyn_servo_sched_step_* / fdyn_servo_sched_mission_* and hcrl_amd.servo_sched on the device.

Reference on the box: the NumPy restatement (tests/servo_sched_numpy.py: steps 0a-0c in front of servo_numpy's and
servo_mission_numpy's loops) over the CPU oracle's RK4 step, computed once per session, and the unscheduled entry points themselves.

Gates (none derived from what the kernels return unless said so):
  identity      a one-node table against fdyn_servo_step_* / fdyn_servo_mission_*: torch.equal, f64 / mixed / f32
  interpolation n_steps = 0 against the restatement: controls 1e-15 (test_gpu_servo.py's test_controls_only), position exactly
  closed loop   500 steps, and 300 mission steps, against the NumPy loop over the oracle: 1e-9 on the state, the integrators and the
                controls, 1e-12 on the references (test_five_hundred_steps...'s gates); split launches to the bit
  benefit       the four flights of tests/golden/servo_sched_reference.npz: peaks within 1e-6 m, scheduled <= half the single design's
  mixed, f32    see test_reduced_precision_fleets_fly_beside_f64
"""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, rel_err, STATE_ANGLE_COLS
import lqr_numpy as ln
import servo_numpy as sn
import servo_mission_numpy as smn
import servo_sched_numpy as ssn
import trim_numpy as tn
from hcrl_amd import _lib, layout as L
from hcrl_amd import servo as SV
from hcrl_amd import servo_sched as SS
from hcrl_amd.fleet import BatchedSixDOF

pytestmark = pytest.mark.gpu

SENTINEL = -12345.678
ISENT = -1234567
PAD = 96
DEV = "cuda"
ONS = ("airspeed", "command")


def _dev(a, dtype=None):
    t = torch.as_tensor(np.array(a, order="C"), device=DEV)
    return t if dtype is None else t.to(dtype)


def _padded(rows, n, dtype=torch.float64, fill=SENTINEL):
    return torch.full((rows * n + PAD,), fill, dtype=dtype, device=DEV)


def _schedule(tables):
    """Host tables [n][M][FD_NSS] -> ServoSchedule on the device."""
    t = np.ascontiguousarray(np.transpose(np.asarray(tables, np.float64), (1, 2, 0)))
    table = _dev(t)
    return SS.ServoSchedule(table, table[:, L.FD_SS_V].contiguous(), torch.zeros(t.shape[0], t.shape[2], dtype=torch.int32, device=DEV))


def _fleet(f, precision="f64", x=None, ref=None, lanes=None):
    """A fleet of the reference's aircraft (`lanes`: which of them, default all) at `x` (default: their trims) with a design holding
    the REFERENCE's gains and trim points and a servo state at `ref` (default: the trims' own references)."""
    lanes = np.arange(len(f["type"])) if lanes is None else np.asarray(lanes)
    n = len(lanes)
    fleet = BatchedSixDOF(n, precision, types=tn.TYPES, type_index=f["type"][lanes])
    fleet.reset((f["x0"] if x is None else x)[lanes])
    z = lambda dt: torch.zeros(n, dtype=dt, device=DEV)   # noqa: E731
    design = SV.ServoDesign(_dev(f["K"][lanes].T), z(torch.float64), z(torch.int32), z(torch.int32), _dev(f["x0"][lanes].T), _dev(f["u0"][lanes].T)) \
        if "K" in f else None
    fleet._servo = design if design is not None else SV.ServoDesign(*(4 * [None]))
    fleet.servo = SV.ServoState.at_trim(_dev(f["x0"][lanes].T))
    fleet.servo.ref.copy_(_dev((f["ref0"] if ref is None else ref)[lanes].T))
    return fleet, design


def _carried(fleet):
    return (fleet.x, fleet.u, fleet.servo.ref, fleet.servo.integ, fleet.servo.err, fleet.lqr_saturated_steps)


@pytest.fixture(scope="module")
def flights():
    return sn.compare_flights()


@pytest.fixture(scope="module")
def crossing():
    return ssn.crossing_flights()


# ---- one node is the unscheduled loop -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", _lib.PRECISIONS)
def test_one_node_is_the_unscheduled_step_and_mission(precision, flights):
    """The ten aircraft of compare_flights, 100 + 400 steps with its commands, then 300 mission steps: every carried word equal."""
    f = flights
    base, design = _fleet(f, precision)
    one = SS.ServoSchedule.from_design(design)
    assert one.n_nodes == 1
    base.step_servo(100, ln.DT)
    base.servo.ref.copy_(_dev(f["ref_cmd"].T))
    base.step_servo(400, ln.DT)
    wps = ssn.mission_square(smn.SHARED_SPEED)
    mbase, _ = _fleet(f, precision)
    mb = mbase.start_servo_mission(wps, acceptance_radius=smn.RADIUS)
    mbase.fly_servo_mission(300, ln.DT)
    for on in ONS:
        sched, _ = _fleet(f, precision)
        sched.step_servo(100, ln.DT, schedule=one, on=on)
        sched.servo.ref.copy_(_dev(f["ref_cmd"].T))
        sched.step_servo(400, ln.DT, schedule=one, on=on)
        for a, b in zip(_carried(base), _carried(sched)):
            assert torch.equal(a, b), (precision, on)
        msched, _ = _fleet(f, precision)
        ms = msched.start_servo_mission(wps, acceptance_radius=smn.RADIUS)
        msched.fly_servo_mission(300, ln.DT, schedule=one, on=on)
        for a, b in zip(_carried(mbase) + (mb.wp_idx, mb.reached_total, mb.steps_flown, mb.stats),
                        _carried(msched) + (ms.wp_idx, ms.reached_total, ms.steps_flown, ms.stats)):
            assert torch.equal(a, b), (precision, on, "mission")
    assert bool(base.lqr_saturated_steps.any()) and bool((mb.reached_total == 1).all()) and sched.time == pytest.approx(500 * ln.DT)
    # a table of equal nodes under airspeeds the flight moves through is the same loop too
    V = one.airspeeds[0]
    three = SS.ServoSchedule(one.table.repeat(3, 1, 1).contiguous(), torch.stack([V - 1.0, V + 0.5, V + 1.5]), torch.zeros(3, one.n, dtype=torch.int32, device=DEV))
    three.table[:, L.FD_SS_V] = three.airspeeds
    eq, _ = _fleet(f, precision)
    eq.step_servo(100, ln.DT, schedule=three)
    eq.servo.ref.copy_(_dev(f["ref_cmd"].T))
    eq.step_servo(400, ln.DT, schedule=three)
    for a, b in zip(_carried(base), _carried(eq)):
        assert torch.equal(a, b), (precision, "equal nodes")


EDGE_ROWS = dict(x=L.FD_NX, ref=L.FD_NSVR, integ=L.FD_NSVI, surf=L.FD_NU, sat=1, err=L.FD_NSVI, sigma=2, wp_idx=1, reached=1, flown=1,
                 stats=L.FD_NMST)
EDGE_INT = ("sat", "wp_idx", "reached", "flown")


def _edge_run(f, n, precision, mission, on):
    """n aircraft (the ten, repeated) through the bare entry points, every per-aircraft buffer with a sentinel pad behind it: the
    100 + 400 steps with compare_flights' commands, or 300 mission steps; on None = the unscheduled entry point.  Returns clones of
    the buffers' used parts after asserting that no pad was touched."""
    lanes = np.arange(n) % len(f["type"])
    fleet, design = _fleet(f, precision, lanes=lanes)
    bufs = {k: _padded(r, n, torch.int32 if k in EDGE_INT else (_lib.state_dtype(precision) if k in ("x", "surf") else torch.float64),
                       ISENT if k in EDGE_INT else SENTINEL) for k, r in EDGE_ROWS.items()}
    view = {k: (b[:EDGE_ROWS[k] * n].view(EDGE_ROWS[k], n) if EDGE_ROWS[k] > 1 else b[:n]) for k, b in bufs.items()}
    view["x"].copy_(fleet.x); view["ref"].copy_(fleet.servo.ref); view["integ"].zero_(); view["sat"].zero_()
    state = SV.ServoState(view["ref"], view["integ"], fleet.servo.limits, view["err"])
    one = SS.ServoSchedule.from_design(design)
    written = {"x", "ref", "integ", "surf", "sat", "err"} | ({"sigma"} if on else set())
    if mission:
        m = SV.ServoMission.start(ssn.mission_square(smn.SHARED_SPEED), n, DEV, acceptance_radius=smn.RADIUS)
        for k, t in (("wp_idx", m.wp_idx), ("reached", m.reached_total), ("flown", m.steps_flown), ("stats", m.stats)):
            view[k].copy_(t)
        m = SV.ServoMission(m.wps, m.consts, view["wp_idx"], view["reached"], view["flown"], view["stats"])
        written |= {"wp_idx", "reached", "flown", "stats"}
        if on:
            SS.sched_mission_into(precision, view["x"], one, state, m, fleet.params, fleet.type_index, ln.DT, 300, on, view["surf"], view["sat"],
                                  view["err"], view["sigma"])
        else:
            SV.mission_into(precision, view["x"], design, state, m, fleet.params, fleet.type_index, ln.DT, 300, view["surf"], view["sat"], view["err"])
    else:
        for steps in (100, 400):
            if on:
                SS.sched_step_into(precision, view["x"], one, state, fleet.params, fleet.type_index, ln.DT, steps, on, view["surf"], view["sat"],
                                   view["err"], view["sigma"])
            else:
                SV.step_into(precision, view["x"], design, state, fleet.params, fleet.type_index, ln.DT, steps, view["surf"], view["sat"], view["err"])
            if steps == 100:
                view["ref"].copy_(_dev(f["ref_cmd"][lanes].T))            # the commands, as the reference wrote them after step 100
    torch.cuda.synchronize()
    for k, b in bufs.items():
        sent = ISENT if k in EDGE_INT else SENTINEL
        assert bool((b[EDGE_ROWS[k] * n:] == sent).all()), f"wrote behind {k}"
        if k not in written:
            assert bool((b == sent).all()), f"wrote {k}"
    return {k: view[k].clone() for k in written}


@pytest.mark.parametrize("n", [65, 130])
@pytest.mark.parametrize("mission", [False, True], ids=["step", "mission"])
@pytest.mark.parametrize("precision", _lib.PRECISIONS)
def test_one_node_at_the_block_edge_with_sentinel_padding(n, mission, precision, flights):
    """Lane position and the edge of the 64-lane workgroup, for the step (100 + 400 steps with compare_flights' commands) and for
    the servo mission (300 steps): a second workgroup with one lane (n = 65) and a third with two (n = 130).  Under a one-node
    schedule, on either sigma, every lane's every word equals the unscheduled launch's, each lane equals the lane ten before it,
    and no pad behind x, ref, integ, surf_out, sat_steps, err_out, sigma_out, wp_idx, reached_total, steps_flown or stats is touched."""
    base = _edge_run(flights, n, precision, mission, None)
    for on in ONS:
        got = _edge_run(flights, n, precision, mission, on)
        for k in base:
            assert torch.equal(base[k], got[k]), (k, on)
        for j in range(10, n, 10):
            w = min(10, n - j)
            for k in got:
                assert torch.equal(got[k][..., j:j + w], got[k][..., :w]), (k, j, on)
        assert bool((got["sigma"][1] == 0.0).all()) and bool(torch.isfinite(got["sigma"][0]).all())
    assert bool(base["sat"].any())
    if mission:
        assert bool((base["flown"] == 300).all()) and bool((base["reached"] == 1).all())


# ---- interpolation alone ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on", ONS)
@pytest.mark.parametrize("M", [2, 3, 8])
def test_interpolation_alone(M, on, flights):
    """n_steps = 0, f64, 16 lanes with their own node airspeeds: sigma below the table, on its first node, between nodes (every
    interval), on an inner node where there is one, on the last node, above it, and NaN.  Controls against the restatement within
    1e-15 (NaN where it has NaN), sigma and position exactly equal, nothing else written."""
    f = flights
    n = 16
    lanes = np.arange(n) % len(f["type"])
    x = np.array([ln.perturbed(v) for v in f["x0"][lanes]])
    x[:, L.FD_X_D] += 3.0
    ref = f["ref_cmd"][lanes].copy()
    integ = np.tile([0.3, -0.5, 0.05], (n, 1)) * (1.0 + 0.1 * np.arange(n))[:, None]
    # what the table is entered with, per lane, BEFORE the cases are placed
    sigma = np.array([ssn.sigma_of(x[i], ref[i], ssn.ON_COMMAND if on == "command" else ssn.ON_AIRSPEED) for i in range(n)])
    # the words: the lane's own design at node 0, moved a few per cent per node so that every node differs in every word
    tables = np.empty((n, M, ssn.NSS))
    for i, a in enumerate(lanes):
        for k in range(M):
            tables[i, k] = ssn.node(0.0, f["x0"][a], f["u0"][a], f["K"][a]) * (1.0 + 0.03 * k) + 1e-3 * k
    # node airspeeds per lane, placed around the lane's sigma: case c of lane i
    cases = ["below", "first", "last", "above", "nan"] + ["between"] * (M - 1) + (["inner"] if M > 2 else [])
    case = [cases[i % len(cases)] for i in range(n)]
    between = 0
    for i in range(n):
        s, c = sigma[i], case[i]
        step = 1.0 + 0.01 * i
        if c == "below":
            V0 = s + 0.5
        elif c in ("first", "nan"):
            V0 = s
        elif c == "last":
            V0 = s - step * (M - 1)
        elif c == "above":
            V0 = s - step * (M - 1) - 0.25
        elif c == "inner":
            V0 = s - step * (1 + i % (M - 2))
        else:
            V0 = s - step * (between % (M - 1)) - 0.3 * step
            between += 1
        tables[i, :, ssn.SS_V] = V0 + step * np.arange(M)
        if c in ("first", "last", "inner"):                               # exactly on a node: that node's airspeed IS sigma
            k = 0 if c == "first" else (M - 1 if c == "last" else 1 + i % (M - 2))
            tables[i, k, ssn.SS_V] = s
        if c == "nan":
            if on == "command":
                ref[i, 0] = np.nan
            else:
                x[i, L.FD_X_V] = np.nan
    assert all((np.diff(tables[i, :, ssn.SS_V]) > 0).all() for i in range(n))
    want = [ssn.controls(tables[i], x[i], ref[i], integ[i], ssn.ON_COMMAND if on == "command" else ssn.ON_AIRSPEED) for i in range(n)]
    pos = np.array([w[2] for w in want])
    for c, ok in (("below", lambda p: p == 0.0), ("first", lambda p: p == 0.0), ("last", lambda p: p == M - 1), ("above", lambda p: p == M - 1),
                  ("nan", lambda p: p == 0.0), ("between", lambda p: 0.0 < p < M - 1 and p != int(p)), ("inner", lambda p: p == int(p) and 0 < p < M - 1)):
        assert all(ok(pos[i]) for i in range(n) if case[i] == c), (c, pos)
    assert {int(p) for p, c in zip(pos, case) if c == "between"} == set(range(M - 1))        # every interval is entered

    fleet, _ = _fleet(dict(f), x=None, lanes=lanes)
    fleet.reset(x)
    fleet.servo.ref.copy_(_dev(ref.T)); fleet.servo.integ.copy_(_dev(integ.T))
    before = [t.clone() for t in (fleet.x, fleet.servo.ref, fleet.servo.integ)]
    surf, sat, err, sg = _padded(L.FD_NU, n), _padded(1, n, torch.int32, 0), _padded(L.FD_NSVI, n), _padded(2, n)
    SS.sched_step_into("f64", fleet.x, _schedule(tables), fleet.servo, fleet.params, fleet.type_index, ln.DT, 0, on, surf[:L.FD_NU * n].view(L.FD_NU, n),
                       sat[:n], err[:L.FD_NSVI * n].view(L.FD_NSVI, n), sg[:2 * n].view(2, n))
    torch.cuda.synchronize()
    assert bool((surf[L.FD_NU * n:] == SENTINEL).all()) and bool((sg[2 * n:] == SENTINEL).all()) and not bool(sat.any()) and bool((err == SENTINEL).all())
    for a, b in zip(before, (fleet.x, fleet.servo.ref, fleet.servo.integ)):
        assert bool(((a == b) | ((a != a) & (b != b))).all())
    got = surf[:L.FD_NU * n].view(L.FD_NU, n).T.cpu().numpy()
    uref = np.array([ln.clip_controls(w[0])[0] for w in want])
    sgot = sg[:2 * n].view(2, n).cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(uref)) and np.isnan(uref).any() and not np.isnan(uref).all(axis=1).any()
    d = np.abs(got - uref)[~np.isnan(uref)].max()
    print(f"M = {M}, on {on}: worst |device - NumPy| on the controls {d:.3e}; positions {pos.tolist()}")
    assert d <= 1e-15
    assert np.array_equal(sgot[1], pos), (sgot[1], pos)
    is_nan = np.array([c == "nan" for c in case])
    assert np.array_equal(np.ascontiguousarray(sgot[0]).view(np.uint64)[~is_nan], np.array([w[1] for w in want]).view(np.uint64)[~is_nan])
    assert np.array_equal(np.isnan(sgot[0]), is_nan) and np.array_equal(np.isnan([w[1] for w in want]), is_nan)


# ---- the closed loop against NumPy over the oracle ----------------------------------------------------------------------------------
def _crossing_fleet(c, ref=None):
    fleet, _ = _fleet(dict(type=c["type"], x0=c["x0"], ref0=c["ref0"]), ref=ref)
    return fleet, _schedule(c["table"])


def test_five_hundred_scheduled_steps_against_the_numpy_closed_loop(crossing):
    c = crossing
    assert (c["pos_100"] < 1.0).all() and (c["pos_100"] > 0.0).all() and (c["pos"] == 2.0).all()     # the airspeed crossed both upper nodes
    fleet, sched = _crossing_fleet(c)
    sg = torch.zeros((2, fleet.n), dtype=torch.float64, device=DEV)
    fleet.step_servo(100, ln.DT, schedule=sched)
    fleet.servo.ref.copy_(_dev(c["ref_cmd"].T))
    SS.sched_step_into("f64", fleet.x, sched, fleet.servo, fleet.params, fleet.type_index, ln.DT, 400, "airspeed", fleet.u, fleet.lqr_saturated_steps,
                       fleet.servo.err, sg)
    torch.cuda.synchronize()
    err = rel_err(fleet.state_numpy(), c["x"], STATE_ANGLE_COLS)
    ierr = np.abs(fleet.servo.integ.T.cpu().numpy() - c["integ"]).max()
    rerr = np.abs(fleet.servo.ref.T.cpu().numpy() - c["ref"]).max()
    uerr = np.abs(fleet.u.T.cpu().numpy() - c["u"]).max()
    sat = fleet.lqr_saturated_steps.cpu().numpy()
    print(f"100 + 400 scheduled steps, 10 aircraft: worst |device - NumPy over the oracle| = {err.max():.3e}; integrators {ierr:.3e}; "
          f"references {rerr:.3e}; controls {uerr:.3e}; saturated steps {sat.tolist()}; sigma {np.abs(sg[0].cpu().numpy() - c['sigma']).max():.3e}")
    assert err.max() <= 1e-9 and ierr <= 1e-9 and rerr <= 1e-12 and uerr <= 1e-9
    assert np.array_equal(sat, c["sat"]) and np.array_equal(sg[1].cpu().numpy(), c["pos"]) and np.abs(sg[0].cpu().numpy() - c["sigma"]).max() <= 1e-9
    # ten 50-step launches equal the two launches above to the bit
    again, _ = _crossing_fleet(c)
    for k in range(10):
        if k == 2:
            again.servo.ref.copy_(_dev(c["ref_cmd"].T))
        again.step_servo(50, ln.DT, schedule=sched)
    for a, b in zip(_carried(again), _carried(fleet)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("on", ONS)
def test_three_hundred_scheduled_mission_steps_against_numpy(on, crossing):
    m = ssn.mission_flights(300, ssn.ON_COMMAND if on == "command" else ssn.ON_AIRSPEED)
    c, rows = crossing, m["rows"]
    assert len({round(r["pos"], 6) for r in rows}) > 1 and all(r["flown"] == 300 and r["reached"] == 1 for r in rows)
    fleet, sched = _crossing_fleet(c)
    mission = fleet.start_servo_mission(m["wps"], acceptance_radius=smn.RADIUS)
    fleet.fly_servo_mission(300, ln.DT, schedule=sched, on=on)
    torch.cuda.synchronize()
    want = lambda k: np.array([r[k] for r in rows])   # noqa: E731
    err = rel_err(fleet.state_numpy(), want("x"), STATE_ANGLE_COLS)
    ierr = np.abs(fleet.servo.integ.T.cpu().numpy() - want("integ")).max()
    rerr = np.abs(fleet.servo.ref.T.cpu().numpy() - want("ref")).max()
    uerr = np.abs(fleet.u.T.cpu().numpy() - want("u")).max()
    print(f"300 scheduled mission steps on {on}: state {err.max():.3e}, integrators {ierr:.3e}, references {rerr:.3e}, controls {uerr:.3e}")
    assert err.max() <= 1e-9 and ierr <= 1e-9 and rerr <= 1e-12 and uerr <= 1e-9
    assert np.array_equal(fleet.lqr_saturated_steps.cpu().numpy(), want("sat")) and np.array_equal(mission.wp_idx.cpu().numpy(), want("idx"))
    assert np.array_equal(mission.steps_flown.cpu().numpy(), want("flown")) and np.array_equal(mission.reached_total.cpu().numpy(), want("reached"))
    assert np.abs(mission.stats.T.cpu().numpy() - want("stats")).max() <= 1e-9
    again, _ = _crossing_fleet(c)
    ma = again.start_servo_mission(m["wps"], acceptance_radius=smn.RADIUS)
    for _ in range(6):
        again.fly_servo_mission(50, ln.DT, schedule=sched, on=on)
    for a, b in zip(_carried(again) + (ma.wp_idx, ma.reached_total, ma.steps_flown, ma.stats),
                    _carried(fleet) + (mission.wp_idx, mission.reached_total, mission.steps_flown, mission.stats)):
        assert torch.equal(a, b)


# ---- the benefit, on the device -----------------------------------------------------------------------------------------------------
def _benefit_fleet(precision, how):
    """The four flights of servo_sched_numpy.BENEFIT as one fleet on the ORACLE's ladder tables (identical inputs to the fixture's),
    flown 100 + 3900 steps as 400 launches of 10 -> (peak |e_h| [4] sampled after every launch from the state, end errors [3][4])."""
    lads = {name: ssn.ladder(name) for name in ssn.AIRFRAMES}
    start = [lads[n]["designs"][ssn.LADDER.index(a)] for n, a, _ in ssn.BENEFIT]
    f = dict(type=np.array([tn.TYPES.index(n) for n, _, _ in ssn.BENEFIT]), x0=np.array([d["x0"] for d in start]),
             ref0=np.array([sn.reference_at(d["x0"]) for d in start]))
    fleet, _ = _fleet(f, precision)
    if how == "single":
        sched = _schedule([lads[n]["table"][ssn.LADDER.index(a):ssn.LADDER.index(a) + 1] for n, a, _ in ssn.BENEFIT])
    else:
        sched = _schedule([lads[n]["table"] for n, _, _ in ssn.BENEFIT])
    on = "command" if how == "command" else "airspeed"
    peak = torch.zeros(4, dtype=torch.float64, device=DEV)
    for k in range(400):
        if k == 10:
            fleet.command_servo(speed=np.array([b for _, _, b in ssn.BENEFIT]))
        fleet.step_servo(10, ssn.DT, schedule=sched, on=on)
        peak = torch.maximum(peak, (-fleet.x[L.FD_X_D].to(torch.float64) - fleet.servo.ref[L.FD_SVR_ALTITUDE]).abs())
    x, ref = fleet.state_numpy(), fleet.servo.ref.T.cpu().numpy()
    return peak.cpu().numpy(), np.array([sn.errors(x[i], ref[i]) for i in range(4)]).T


@pytest.fixture(scope="module")
def benefit_f64():
    return {how: _benefit_fleet("f64", how) for how in ("single", "airspeed")}


def test_the_schedule_halves_the_peak_altitude_error_on_the_device(benefit_f64):
    ref = np.load(os.path.join(GOLDEN, "servo_sched_reference.npz"))
    for how in ("single", "airspeed"):
        peak = benefit_f64[how][0]
        print(f"peak |e_h| (m), {how}: device {peak}, fixture {ref[how]}, difference {np.abs(peak - ref[how]).max():.3e}")
        assert np.abs(peak - ref[how]).max() <= 1e-6, how
    assert (benefit_f64["airspeed"][0] <= 0.5 * benefit_f64["single"][0]).all()
    assert np.isfinite(benefit_f64["airspeed"][1]).all()


# worst |end error - the f64 fleet's| over the four flights on the measured-airspeed schedule, (airspeed m/s, altitude m, heading
# rad); first run on MI355X
MEASURED_MIXED = (5.974e-8, 1.066e-7, 0.0)
MEASURED_F32 = (4.456e-5, 1.922e-5, 1.192e-8)


def _round_up_one_digit(v):
    if v == 0.0:                                                         # nothing measured: nothing allowed
        return 0.0
    e = np.floor(np.log10(v))
    return float(np.ceil(v / 10.0 ** e - 1e-9) * 10.0 ** e)


def test_reduced_precision_fleets_fly_beside_f64(benefit_f64):
    """The mixed and f32 fleets fly the four flights on the measured-airspeed schedule beside the f64 fleet, whose peaks
    test_the_schedule_halves... gates against the fixture.  Their end errors (at 40 s) are compared with the f64 fleet's, gated as
    test_gpu_servo.py's test of the same name gates them: per word at ten times the value measured on the first run on MI355X,
    rounded up to one digit.  Measured (airspeed m/s, altitude m, heading rad): mixed 5.974e-08, 1.066e-07, 0; f32 4.456e-05,
    1.922e-05, 1.192e-08 (the f64 fleet's own end errors there: 2.4e-02, 1.1e-02, 0: a 15 m/s change is still settling at 40 s).
    Gates: mixed 6e-7, 2e-6, 0; f32 5e-4, 2e-4, 2e-7.  The heading gate of the mixed fleet is zero because these level flights
    never excite the lateral block: its words are exact zeros in f64 and mixed alike."""
    end = benefit_f64["airspeed"][1]
    worst = {}
    for p in ("mixed", "f32"):
        peak, e = _benefit_fleet(p, "airspeed")
        worst[p] = np.abs(e - end).max(axis=1)
        assert np.isfinite(e).all() and (peak <= 0.5 * benefit_f64["single"][0]).all(), p
    print(f"worst end-error difference to the f64 fleet (V, h, psi): mixed {worst['mixed']}, f32 {worst['f32']}; f64's own end errors {np.abs(end).max(axis=1)}")
    for p, measured in (("mixed", MEASURED_MIXED), ("f32", MEASURED_F32)):
        for k in range(3):
            assert worst[p][k] <= _round_up_one_digit(10.0 * measured[k]), (p, k, worst[p][k], measured[k])


# ---- graphs, refusals, the fleet methods ------------------------------------------------------------------------------------------
def test_graph_replay_equals_eager(crossing):
    c = crossing
    fe, sched = _crossing_fleet(c, ref=c["ref_cmd"])
    fg, _ = _crossing_fleet(c, ref=c["ref_cmd"])
    for _ in range(10):
        fe.step_servo(20, ln.DT, schedule=sched)
    saved = [t.clone() for t in (fg.x, fg.servo.ref, fg.servo.integ)]
    fg._saturated_steps()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                                 # warm-up outside the capture
        fg.step_servo(20, ln.DT, schedule=sched)
    torch.cuda.current_stream().wait_stream(s)
    for t, v in zip((fg.x, fg.servo.ref, fg.servo.integ), saved):
        t.copy_(v)
    fg.lqr_saturated_steps.zero_()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        fg.step_servo(20, ln.DT, schedule=sched)
    for t, v in zip((fg.x, fg.servo.ref, fg.servo.integ), saved):              # the capture launched nothing; start over to be sure
        t.copy_(v)
    fg.lqr_saturated_steps.zero_()
    for _ in range(10):
        gr.replay()
    torch.cuda.synchronize()
    for a, b in zip(_carried(fe), _carried(fg)):
        assert torch.equal(a, b)
    assert bool(fe.lqr_saturated_steps.any())


def test_refused_calls_launch_nothing(crossing):
    c = crossing
    fleet, sched = _crossing_fleet(c)
    n = fleet.n
    before = [t.clone() for t in (fleet.x, fleet.servo.ref, fleet.servo.integ)]
    surf, sg = torch.full((L.FD_NU, n), SENTINEL, dtype=torch.float64, device=DEV), torch.full((2, n), SENTINEL, dtype=torch.float64, device=DEV)
    lib = _lib.load()
    wps, consts, idx = _dev(ssn.mission_square(20.0)), _dev(smn.consts()), torch.zeros(n, dtype=torch.int32, device=DEV)

    def call(table=sched.table, nodes=3, on=0, mission=False):
        head = (_lib.ptr(fleet.x), _lib.ptr(table), nodes, on, _lib.ptr(fleet.servo.ref), _lib.ptr(fleet.servo.integ), _lib.ptr(fleet.servo.limits))
        mid = (_lib.ptr(fleet.type_index), _lib.ptr(fleet.params), fleet.n_types, n, ln.DT, 5, _lib.ptr(surf), None, None)
        if mission:
            return lib.fdyn_servo_sched_mission_f64(*head, _lib.ptr(idx), _lib.ptr(consts), _lib.ptr(wps), 5, *mid, None, None, None, _lib.ptr(sg),
                                                    _lib.current_stream())
        return lib.fdyn_servo_sched_step_f64(*head, *mid, _lib.ptr(sg), _lib.current_stream())
    for mission in (False, True):
        for nodes in (0, -3, L.FD_MAX_SCHED_NODES + 1):
            assert call(nodes=nodes, mission=mission) == _lib.FDYN_ERR_BAD_SIZE
        for on in (-1, 2, 99):
            assert call(on=on, mission=mission) == _lib.FDYN_ERR_BAD_SIZE
        assert call(table=None, mission=mission) == _lib.FDYN_ERR_NULL
    torch.cuda.synchronize()
    assert bool((surf == SENTINEL).all()) and bool((sg == SENTINEL).all()) and not bool(idx.any())
    for a, b in zip(before, (fleet.x, fleet.servo.ref, fleet.servo.integ)):
        assert torch.equal(a, b)
    assert call() == _lib.FDYN_OK and call(mission=True) == _lib.FDYN_OK           # and the same calls, well formed, fly
    torch.cuda.synchronize()
    assert not bool((surf == SENTINEL).any()) and not bool((sg == SENTINEL).any())


def test_fleet_methods_design_fly_and_report():
    """trim -> design_servo_schedule -> step_servo(schedule=) on the device: the device ladder equals the oracle's at the
    linearisation's own gate, the schedule refuses what it must, and the frozen-point report is stable between the nodes."""
    types = [tn.TYPES.index(n) for n in ssn.AIRFRAMES]
    fleet = BatchedSixDOF(2, "f64", types=tn.TYPES, type_index=types)
    fleet.trim(15.0, altitude=sn.ALTITUDE, heading=sn.HEADING)
    fleet.design_servo()
    sched = fleet.design_servo_schedule(ssn.LADDER, altitude=sn.ALTITUDE, heading=sn.HEADING)
    assert (sched.n, sched.n_nodes) == (2, 4) and bool(sched.ok.all()) and tuple(sched.table.shape) == (4, L.FD_NSS, 2)
    want = np.array([ssn.ladder(n)["table"] for n in ssn.AIRFRAMES])                 # [2][4][39]
    got = sched.table.permute(2, 0, 1).cpu().numpy()
    dev_ = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    print(f"device ladder against the oracle ladder: worst word deviation {dev_.max():.3e}")
    assert dev_.max() <= 1e-6                                                     # two central differences of two implementations
    # the first node is the fleet's own design: same trim, same linearisation, same solver
    assert torch.equal(sched.table[0, L.FD_SS_K:], fleet._servo.K) and torch.equal(sched.table[0, L.FD_SS_U0:L.FD_SS_K], fleet._servo.u0)
    for bad in ((15.0, 15.0), (20.0, 15.0), np.arange(9.0) + 12.0):
        with pytest.raises(ValueError):
            fleet.design_servo_schedule(bad)
    w = sn.default_weights()
    w[3] = np.nan
    with pytest.raises(ValueError, match=r"2 of 2 aircraft have a node without.*node 0: invalid model, trim or weights"):
        fleet.design_servo_schedule((15.0, 20.0), weights=w)
    refused = fleet.design_servo_schedule((15.0, 20.0), weights=w, strict=False)
    assert not bool(refused.ok.any()) and bool((refused.status == L.FD_SV_BAD_INPUT).all()) and not bool(refused.table[:, L.FD_SS_K:].any())
    wind = SV.ServoWind.steady(2, fleet.device, 5.0, 0.3)
    with pytest.raises(NotImplementedError):
        fleet.step_servo(1, 0.01, wind=wind, schedule=sched)
    fleet.start_servo_mission(ssn.mission_square(20.0))
    with pytest.raises(NotImplementedError):
        fleet.fly_servo_mission(1, 0.01, wind=wind, schedule=sched)
    with pytest.raises(ValueError, match="on must be one of"):
        fleet.step_servo(1, 0.01, schedule=sched, on="estimate")
    x_before = fleet.x.clone()
    modes, V = sched.frozen_point_modes()
    assert torch.equal(fleet.x, x_before) and tuple(V.shape) == (3, 2) and V[:, 0].tolist() == [17.5, 22.5, 27.5] and modes.n == 6
    absc = modes.abscissa().max(dim=0).values.reshape(3, 2).cpu().numpy()
    ref = np.array([[r["abscissa"] for r in ssn.frozen_point_modes(n)] for n in ssn.AIRFRAMES]).T
    print(f"frozen-point abscissae between the nodes: device {absc.tolist()}, NumPy {ref.tolist()}")
    assert bool((modes.status == 0).all()) and (absc < 0.0).all()
    # lane p n + i IS point p of aircraft i, with the K interpolated there: the device ladder's words are within 1e-6 (relative) of
    # the oracle's (asserted above), the abscissae are O(1) simple eigenvalues of matrices with O(10) entries, so 1e-5 leaves a
    # factor of ten for their conditioning; a swapped lane or point differs in the second digit
    assert np.abs(absc - ref).max() <= 1e-5, np.abs(absc - ref).max()
    assert tuple(sched.frozen_point_modes(2)[1].shape) == (6, 2)
    fleet.command_servo(speed=30.0)
    fleet.step_servo(300, 0.01, schedule=sched)
    assert bool(torch.isfinite(fleet.x).all()) and fleet.time == pytest.approx(3.0)

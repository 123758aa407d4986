"""fdyn_servo_kf_design / fdyn_servo_lqg_step_* and hcrl_amd.servo_lqg on the device.

Reference on the box: the NumPy restatement of both (tests/servo_lqg_numpy.py) -- the design on the 288 linearisations of
tests/golden/trim_reference.npz, the control step over the CPU oracle's RK4 -- computed once per session.

Gates (none derived from what the kernels return):
  F            1e-9: fp64 on both sides in the same order (fdyn_kf_design's gate); iteration counts and status equal
  truth        feedback = truth against fdyn_servo_step_*: bit for bit in x, integ, ref, surf_out, sat_steps, all three precisions
  closed loop  100 + 400 steps on replayed normals against the NumPy loop over the oracle: 1e-9 (fdyn_lqg_step's gate); saturated-step
               counts equal
  draws        (meas_out - d) / sigma against philox_numpy: 1e-5 (tests/test_gpu_device_draws.py's bound)
  behaviour    the four gates of tests/test_servo_lqg_oracle.py, in f64, mixed and f32, with in-kernel draws
"""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, rel_err, STATE_ANGLE_COLS
import lqr_numpy as ln
import servo_lqg_numpy as sl
import servo_numpy as sn
import trim_numpy as tn
from hcrl_amd import _lib, layout as L
from hcrl_amd import servo as SV
from hcrl_amd import servo_lqg as SL
from hcrl_amd.fleet import BatchedSixDOF

pytestmark = pytest.mark.gpu

SENTINEL = -12345.678
ISENT = -1234567
PAD = 96
DEV = "cuda"
PRECISIONS = ("f64", "mixed", "f32")


def _dev(a, dtype=None):
    t = torch.as_tensor(np.array(a, order="C"), device=DEV)
    return t if dtype is None else t.to(dtype)


def _padded(rows, n, dtype=torch.float64, fill=SENTINEL):
    return torch.full((rows * n + PAD,), fill, dtype=dtype, device=DEV)


def _view(buf, rows, n):
    return buf[:rows * n].view(rows, n)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---- the design --------------------------------------------------------------------------------------------------------------------
def _design(A, B, dt, noise):
    """A [n][12][12], B [n][12][4], noise [20] or [n][20] (host) -> dict of host arrays (F [n][120], residual, iters, status); every
    output buffer has a sentinel pad behind it, asserted untouched."""
    n = len(A)
    A_d, B_d = _dev(np.transpose(A, (1, 2, 0))), _dev(np.transpose(B, (1, 2, 0)))
    nz = np.asarray(noise, np.float64)
    nz_d = _dev(nz if nz.ndim == 1 else nz.T)
    F, res = _padded(L.FD_NSKF, n), _padded(1, n)
    it, st = _padded(1, n, torch.int32, ISENT), _padded(1, n, torch.int32, ISENT)
    rc = _lib.load().fdyn_servo_kf_design(_lib.ptr(A_d), _lib.ptr(B_d), float(dt), _lib.ptr(nz_d), int(nz.ndim == 2), n, _lib.ptr(F),
                                          _lib.ptr(res), _lib.ptr(it), _lib.ptr(st), _lib.current_stream())
    _lib.check(rc, "fdyn_servo_kf_design")
    torch.cuda.synchronize()
    for buf, rows, sent in ((F, L.FD_NSKF, SENTINEL), (res, 1, SENTINEL), (it, 1, ISENT), (st, 1, ISENT)):
        assert bool((buf[rows * n:] == sent).all()), "wrote behind an output buffer"
    return dict(F=_view(F, L.FD_NSKF, n).T.cpu().numpy(), residual=res[:n].cpu().numpy(), iters=it[:n].cpu().numpy(), status=st[:n].cpu().numpy())


def _same(a, b):
    res_a, res_b = a["residual"], b["residual"]
    nan = np.isnan(res_a)
    return np.array_equal(_bits(a["F"]), _bits(b["F"])) and np.array_equal(nan, np.isnan(res_b)) and \
        np.array_equal(_bits(res_a[~nan]), _bits(res_b[~nan])) and np.array_equal(a["iters"], b["iters"]) and np.array_equal(a["status"], b["status"])


def _take(r, idx):
    return {k: v[idx] for k, v in r.items()}


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "trim_reference.npz"))


@pytest.fixture(scope="module")
def grid(golden):
    """The 288 linearisations in ONE launch with shared noise, at dt 0.01."""
    return _design(golden["A"], golden["B"], 0.01, sl.default_noise())


@pytest.mark.parametrize("dt", [0.01, 0.02])
def test_grid_matches_the_restatement(golden, grid, dt):
    got = grid if dt == 0.01 else _design(golden["A"], golden["B"], dt, sl.default_noise())
    ref = sl.golden_designs(golden, dt)
    assert len(got["status"]) == 288 and not got["status"].any(), np.flatnonzero(got["status"])
    assert np.array_equal(got["status"], ref["status"]) and np.array_equal(got["iters"], ref["iters"])
    err = np.abs(got["F"] - ref["F"]).max()
    print(f"dt {dt}: worst |F - restatement| {err:.3e}; bit-identical in {int((_bits(got['F']) == _bits(ref['F'])).sum())} of {got['F'].size} "
          f"words; residual <= {got['residual'].max():.3e}; doublings {got['iters'].min()}..{got['iters'].max()}")
    assert err <= 1e-9
    assert np.abs(got["residual"] - ref["residual"]).max() <= 1e-9


@pytest.mark.parametrize("n", [1, 63, 65, 257])
def test_design_shapes_and_lane_position(n, grid, golden):
    idx = (np.arange(n) * 7 + 3) % 288
    got = _design(golden["A"][idx], golden["B"][idx], 0.01, sl.default_noise())
    assert _same(got, _take(grid, idx)), "a lane's result depends on where it sits in the launch"


def test_shared_noise_equals_the_same_noise_per_lane(grid, golden):
    assert _same(_design(golden["A"], golden["B"], 0.01, np.tile(sl.default_noise(), (288, 1))), grid)


def test_bad_lanes_and_their_neighbours(grid, golden):
    keep = np.arange(0, 288, 6)
    A, B, NZ, kind = [], [], [], []
    for j, i in enumerate(keep):
        A.append(golden["A"][i]); B.append(golden["B"][i]); NZ.append(sl.default_noise()); kind.append(0)
        if j % 3 == 2:
            a, b, nz = golden["A"][i].copy(), golden["B"][i].copy(), sl.default_noise()
            k = 1 + (j // 3) % 4
            if k == 1:
                a[L.FD_X_W, L.FD_X_D] = np.nan                           # a NaN word in the longitudinal block
            elif k == 2:
                nz[(j // 3) % 20] = (0.0, -2.0, np.nan, np.inf)[(j // 12) % 4]
            elif k == 3:
                lat = list(sl.EST_STATES[5:])
                a[np.ix_(lat, lat)] *= 1.6 / (sl.row_norm(a[np.ix_(lat, lat)]) * 0.01)   # |a|_inf dt = 1.6
            else:
                b[L.FD_X_Q, L.FD_U_ELEVATOR] = np.inf                    # a word of B that is not finite
            A.append(a); B.append(b); NZ.append(nz); kind.append(k)
    A, B, NZ, kind = np.array(A), np.array(B), np.array(NZ), np.array(kind)
    assert all((kind == k).sum() >= 3 for k in (1, 2, 3, 4))
    mixed = _design(A, B, 0.01, NZ)
    assert _same(_take(mixed, kind == 0), _take(grid, keep)), "a good lane changed because of its neighbour"
    bad = _take(mixed, kind != 0)
    assert (bad["status"] == L.FD_KF_BAD_INPUT).all() and np.isnan(bad["residual"]).all() and not bad["iters"].any()
    assert np.array_equal(_bits(bad["F"]), _bits(np.tile(sl.pass_through(), (len(bad["F"]), 1)))), "a bad lane is not the pass-through"
    ref = sl.design_many(A[kind != 0], B[kind != 0], 0.01, NZ[kind != 0])
    assert np.array_equal(bad["status"], ref["status"])


def test_design_graph_replay_equals_eager(golden):
    A_d, B_d = _dev(np.transpose(golden["A"], (1, 2, 0))), _dev(np.transpose(golden["B"], (1, 2, 0)))
    nz = SL.noise_tensor(None, 288, DEV)
    eager = SL.servo_kalman_into(A_d, B_d, 0.02, nz)
    out = SL.servo_kalman_into(A_d, B_d, 0.02, nz)
    for t in (out.F, out.residual, out.iters, out.status):
        t.fill_(7)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        SL.servo_kalman_into(A_d, B_d, 0.02, nz, out)
    torch.cuda.current_stream().wait_stream(stream)
    out.F.fill_(7)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        SL.servo_kalman_into(A_d, B_d, 0.02, nz, out)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.F, eager.F) and torch.equal(out.residual, eager.residual) and torch.equal(out.iters, eager.iters)
    assert torch.equal(out.status, eager.status) and out.count_not_ok() == 0


# ---- the step ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def flights():
    return sn.compare_flights()


@pytest.fixture(scope="module")
def lqg_flights():
    return sl.compare_flights()


def _fleet(f, F, precision="f64", idx=None, seed=0):
    """A fleet of the reference's aircraft (rows `idx` of it) at their trims with designs holding the REFERENCE's gains, trim points
    and filters, a servo state at the trims' own references and an estimator state at zero."""
    idx = np.arange(len(f["type"])) if idx is None else np.asarray(idx)
    n = len(idx)
    fleet = BatchedSixDOF(n, precision, types=tn.TYPES, type_index=f["type"][idx])
    fleet.reset(f["x0"][idx])
    zi = lambda: torch.zeros(n, dtype=torch.int32, device=DEV)   # noqa: E731
    design = SV.ServoDesign(_dev(f["K"][idx].T), torch.zeros(n, dtype=torch.float64, device=DEV), zi(), zi(), _dev(f["x0"][idx].T), _dev(f["u0"][idx].T))
    fleet._servo = design
    fleet.servo = SV.ServoState.at_trim(design.x0)
    fleet.servo.ref.copy_(_dev(f["ref0"][idx].T))
    fleet._servo_kalman = SL.ServoKalmanDesign(_dev(np.asarray(F)[idx].T), torch.zeros(n, dtype=torch.float64, device=DEV), zi(), zi(), dt=ln.DT,
                                               sigma=_dev(np.array(sl.DEFAULT_SIGMA)))
    fleet.servo_lqg = SL.ServoLqgState.zeros(n, DEV, seed=seed)
    fleet._saturated_steps()
    return fleet


def _command(fleet, f, idx=None):
    idx = np.arange(len(f["type"])) if idx is None else np.asarray(idx)
    fleet.servo.ref.copy_(_dev(f["ref_cmd"][idx].T))


def _state(fleet):
    s, q = fleet.servo, fleet.servo_lqg
    return [t.clone() for t in (fleet.x, fleet.u, s.ref, s.integ, s.err, fleet.lqr_saturated_steps, q.xhat, q.du_prev, q.step, q.err_est,
                                q.err_meas, q.chatter, q.meas)]


def _equal(a, b, skip=()):
    return all(torch.equal(x, y) for k, (x, y) in enumerate(zip(a, b)) if k not in skip)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_truth_feedback_is_the_servo_step_bit_for_bit(precision, flights, lqg_flights):
    f, idx = flights, np.arange(257) % 10
    a = _fleet(f, lqg_flights["F"], precision, idx, seed=3)
    b = _fleet(f, lqg_flights["F"], precision, idx)
    for leg in range(2):
        if leg:
            _command(a, f, idx)
            _command(b, f, idx)
        a.step_servo_lqg(100, "truth")
        b.step_servo(100, ln.DT)
    torch.cuda.synchronize()
    assert torch.equal(a.x, b.x) and torch.equal(a.servo.integ, b.servo.integ) and torch.equal(a.servo.ref, b.servo.ref)
    assert torch.equal(a.u, b.u) and torch.equal(a.lqr_saturated_steps, b.lqr_saturated_steps) and torch.equal(a.servo.err, b.servo.err)
    assert bool(a.lqr_saturated_steps.any()) and bool(a.servo_lqg.xhat.any()) and a.servo_lqg.step.tolist() == [200]   # the estimator still ran


def test_five_hundred_steps_against_the_numpy_closed_loop(flights, lqg_flights):
    f, r = flights, lqg_flights
    assert not r["kf_status"].any()
    z = _dev(np.ascontiguousarray(np.transpose(r["z"], (0, 2, 1))))                       # [500][10 words][10 aircraft]
    fleet = _fleet(f, r["F"])
    fleet.step_servo_lqg(100, "estimate", z[:100].contiguous())
    _command(fleet, f)
    fleet.step_servo_lqg(400, "estimate", z[100:].contiguous())
    torch.cuda.synchronize()
    q = fleet.servo_lqg
    err = rel_err(fleet.state_numpy(), r["x"], STATE_ANGLE_COLS).max()
    worst = dict(x=err, xhat=np.abs(q.xhat.T.cpu().numpy() - r["xhat"]).max(), du_prev=np.abs(q.du_prev.T.cpu().numpy() - r["du_prev"]).max(),
                 integ=np.abs(fleet.servo.integ.T.cpu().numpy() - r["integ"]).max(), u=np.abs(fleet.u.T.cpu().numpy() - r["u"]).max())
    for k in ("err_est", "err_meas", "chatter"):
        worst[k] = (np.abs(getattr(q, k).T.cpu().numpy() - r[k]) / np.maximum(1.0, np.abs(r[k]))).max()
    sat = fleet.lqr_saturated_steps.cpu().numpy()
    print("100 + 400 steps on replayed normals, 10 aircraft, worst |device - NumPy over the oracle|: " +
          ", ".join(f"{k} {v:.3e}" for k, v in worst.items()) + f"; saturated steps {sat.tolist()}")
    assert all(v <= 1e-9 for v in worst.values()), worst
    assert np.array_equal(sat, r["sat"]) and q.step.tolist() == [500] and q.steps_accumulated == 500


def test_in_kernel_draws_are_the_philox_model(flights, lqg_flights):
    f, idx = flights, np.arange(257) % 10
    sigma = np.array(sl.DEFAULT_SIGMA)
    for step_word in (0, 41, None):
        fleet = _fleet(f, lqg_flights["F"], "f64", idx, seed=sl.SEED)
        q = fleet.servo_lqg
        d = np.array([sl.deviation(x, x0) for x, x0 in zip(fleet.state_numpy(), f["x0"][idx])])
        if step_word is None:                                             # a NULL step pointer is step word 0
            real, q.step = q.step, None
            fleet.step_servo_lqg(1)
            q.step = real
        else:
            q.step.fill_(step_word)
            fleet.step_servo_lqg(1)
        torch.cuda.synchronize()
        got = (q.meas.T.cpu().numpy() - d) / sigma
        want = sl.lqg_normals(sl.SEED, np.arange(257), (step_word or 0) + 1)
        print(f"step word {step_word}: worst |device normal - philox_numpy| {np.abs(got - want).max():.3e}")
        assert np.abs(got - want).max() <= 1e-5


def test_launch_splits_graphs_and_lane_positions(flights, lqg_flights):
    f, r = flights, lqg_flights
    idx = np.arange(257) % 10
    z = _dev(np.ascontiguousarray(np.transpose(r["z"][:100], (0, 2, 1))[:, :, idx]))      # [100][10][257]
    one = _fleet(f, r["F"], "f64", idx)
    _command(one, f, idx)
    one.step_servo_lqg(100, "estimate", z)
    two = _fleet(f, r["F"], "f64", idx)
    _command(two, f, idx)
    two.step_servo_lqg(50, "estimate", z[:50].contiguous())
    two.step_servo_lqg(50, "estimate", z[50:].contiguous())
    torch.cuda.synchronize()
    assert _equal(_state(one), _state(two)), "two launches of 50 steps differ from one of 100"
    # a lane's flight does not depend on the fleet's size or on where the lane sits; sentinel pads behind the state, the estimator's
    # words and every accumulator stay (257 lanes too: the last workgroup has 63 idle lanes)
    for n in (1, 63, 65, 257):
        sub = _fleet(f, r["F"], "f64", idx[:n])
        _command(sub, f, idx[:n])
        q = sub.servo_lqg
        xpad = _padded(L.FD_NX, n)
        _view(xpad, L.FD_NX, n).copy_(sub.x)
        rows = dict(xhat=L.FD_NSKX, du_prev=L.FD_NU, err_est=L.FD_NSKX, err_meas=L.FD_NSKX, chatter=L.FD_NU, meas=L.FD_NSKX)
        pads = {}
        for name, k in rows.items():
            pads[name] = _padded(k, n, fill=0.0)
            pads[name][k * n:] = SENTINEL
            setattr(q, name, _view(pads[name], k, n))
        SL.lqg_step_into("f64", _view(xpad, L.FD_NX, n), sub._servo, sub._servo_kalman, sub.servo, q, sub.params, sub.type_index, ln.DT,
                         100, "estimate", z[:, :, :n].contiguous())
        torch.cuda.synchronize()
        for buf, k in [(xpad, L.FD_NX)] + [(pads[name], k) for name, k in rows.items()]:
            assert bool((buf[k * n:] == SENTINEL).all()), "wrote behind a buffer"
        assert torch.equal(_view(xpad, L.FD_NX, n), one.x[:, :n]) and torch.equal(sub.servo.integ, one.servo.integ[:, :n])
        for name in rows:
            assert torch.equal(getattr(q, name), getattr(one.servo_lqg, name)[:, :n]), name


def test_the_dynamic_lds_placement_of_the_f64_filter_is_the_same_step(flights, lqg_flights):
    """fdyn_servo_lqg_step_f64_lds against fdyn_servo_lqg_step_f64: every word equal to the bit, in-kernel draws, more than one workgroup."""
    f, idx = flights, np.arange(257) % 10
    a, b = _fleet(f, lqg_flights["F"], "f64", idx, seed=5), _fleet(f, lqg_flights["F"], "f64", idx, seed=5)
    for fleet, lds in ((a, False), (b, True)):
        _command(fleet, f, idx)
        for _ in range(2):
            SL.lqg_step_into("f64", fleet.x, fleet._servo, fleet._servo_kalman, fleet.servo, fleet.servo_lqg, fleet.params, fleet.type_index, ln.DT,
                             50, "estimate", None, fleet.u, fleet.lqr_saturated_steps, fleet.servo.err, filter_in_lds=lds)
    torch.cuda.synchronize()
    assert _equal(_state(a), _state(b)) and bool(a.servo_lqg.err_est.all())
    with pytest.raises(ValueError, match="filter_in_lds"):
        SL.lqg_step_into("mixed", a.x, a._servo, a._servo_kalman, a.servo, a.servo_lqg, a.params, a.type_index, ln.DT, 1, filter_in_lds=True)


def test_a_turn_through_pi_from_the_trim_heading():
    """The flight of tests/test_servo_lqg_oracle.py whose heading DEVIATION passes +pi (two commands of +100 deg, 40 s), on the device
    with the restatement's normals replayed: the innovation's and the estimate's wraps act here and nowhere else in this file.
    Against the restatement over the oracle within 1e-9 (the closed-loop gate above); xhat_psi in range; err_est < err_meas on psi.
    The restatement without the innovation's wrap ends elsewhere by more than the gate: this comparison would see the wrap missing."""
    r, bad = sl.wrap_flights(), sl.wrap_flights(wrap_innovation=False)
    n = len(sl.WRAP_AIRCRAFT)
    f = dict(type=r["type"], x0=r["x0"], u0=r["u0"], K=r["K"], ref0=r["ref0"])
    fleet = _fleet(f, r["F"])
    z = _dev(np.ascontiguousarray(np.transpose(r["z"], (0, 2, 1))))                       # [4000][10][2]
    at, widest = 0, torch.zeros((), dtype=torch.float64, device=DEV)
    for leg, steps in enumerate(sl.WRAP_LEGS):
        if leg:
            fleet.command_servo(heading=fleet.servo.ref[L.FD_SVR_HEADING] + sl.WRAP_TURN)
        for k in range(0, steps, 100):
            fleet.step_servo_lqg(100, "estimate", z[at + k:at + k + 100].contiguous())
            widest = torch.maximum(widest, fleet.servo_lqg.xhat[sl.PSI].abs().max())
        at += steps
    torch.cuda.synchronize()
    q = fleet.servo_lqg
    worst = dict(x=rel_err(fleet.state_numpy(), r["x"], STATE_ANGLE_COLS).max(), xhat=np.abs(q.xhat.T.cpu().numpy() - r["xhat"]).max(),
                 integ=np.abs(fleet.servo.integ.T.cpu().numpy() - r["integ"]).max(), ref=np.abs(fleet.servo.ref.T.cpu().numpy() - r["ref"]).max())
    for k in ("err_est", "err_meas", "chatter"):
        worst[k] = (np.abs(getattr(q, k).T.cpu().numpy() - r[k]) / np.maximum(1.0, np.abs(r[k]))).max()
    ratio = (q.err_est[sl.PSI] / q.err_meas[sl.PSI]).cpu().numpy()
    unwrapped = np.abs(bad["err_est"] - r["err_est"])[:, sl.PSI].min()
    print("4000 steps through psi - psi0 = pi, worst |device - NumPy over the oracle|: " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()) +
          f"; err_est / err_meas on psi {ratio}; widest |xhat_psi| {float(widest):.4f}; the restatement without the wrap differs by {unwrapped:.3e}")
    assert all(v <= 1e-9 for v in worst.values()), worst
    assert np.array_equal(fleet.lqr_saturated_steps.cpu().numpy(), r["sat"])
    assert float(widest) <= np.pi and (ratio < sl.GATE_RATIO).all()
    assert float(fleet.x[L.FD_X_YAW].min()) < 0.0 and (r["xhat"][:, sl.PSI] < -2.7).all()      # 200 deg from the trim heading = -160 deg
    assert unwrapped > 1.0


def test_ten_graphed_replays_equal_ten_eager_launches(flights, lqg_flights):
    f, idx = flights, np.arange(65) % 10
    eager = _fleet(f, lqg_flights["F"], "mixed", idx, seed=11)
    _command(eager, f, idx)
    for _ in range(10):
        eager.step_servo_lqg(10)
    graphed = _fleet(f, lqg_flights["F"], "mixed", idx, seed=11)
    _command(graphed, f, idx)
    start = _state(graphed)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        graphed.step_servo_lqg(10)                                        # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(stream)
    now = (graphed.x, graphed.u, graphed.servo.ref, graphed.servo.integ, graphed.servo.err, graphed.lqr_saturated_steps, graphed.servo_lqg.xhat,
           graphed.servo_lqg.du_prev, graphed.servo_lqg.step, graphed.servo_lqg.err_est, graphed.servo_lqg.err_meas, graphed.servo_lqg.chatter,
           graphed.servo_lqg.meas)
    for t, s in zip(now, start):
        t.copy_(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        graphed.step_servo_lqg(10)
    for t, s in zip(now, start):                                          # a capture launches nothing, but the step word must start at zero
        t.copy_(s)
    for _ in range(10):
        g.replay()
    torch.cuda.synchronize()
    assert _equal(_state(eager), _state(graphed)), "graphed replays differ from eager launches"
    assert graphed.servo_lqg.step.tolist() == [100]


def test_controls_only_and_optional_outputs(flights, lqg_flights):
    f, r = flights, lqg_flights
    n = len(f["type"])
    z = _dev(np.ascontiguousarray(np.transpose(r["z"][:100], (0, 2, 1))))
    fleet = _fleet(f, r["F"])
    _command(fleet, f)
    fleet.step_servo_lqg(100, "estimate", z)
    # n_steps = 0 writes surf_out alone and equals the law on the stored estimate
    before = _state(fleet)
    surf = _padded(L.FD_NU, n)
    for fb in ("estimate", "truth"):
        SL.lqg_step_into("f64", fleet.x, fleet._servo, fleet._servo_kalman, fleet.servo, fleet.servo_lqg, fleet.params, fleet.type_index, ln.DT, 0,
                         fb, None, _view(surf, L.FD_NU, n), fleet.lqr_saturated_steps, fleet.servo.err)
        torch.cuda.synchronize()
        assert _equal(before, _state(fleet)) and bool((surf[L.FD_NU * n:] == SENTINEL).all())
        x, xh = fleet.state_numpy(), fleet.servo_lqg.xhat.T.cpu().numpy()
        ref, integ = fleet.servo.ref.T.cpu().numpy(), fleet.servo.integ.T.cpu().numpy()
        want = np.array([ln.clip_controls(sl.controls_from(f["K"][i], f["x0"][i], f["u0"][i], x[i], xh[i], ref[i], integ[i],
                                                           sl.ESTIMATE if fb == "estimate" else sl.TRUTH))[0] for i in range(n)])
        got = _view(surf, L.FD_NU, n).T.cpu().numpy()
        print(f"controls only, {fb}: worst |device - NumPy| {np.abs(got - want).max():.3e}")
        assert np.abs(got - want).max() <= 1e-12
    # NULL for each optional output leaves the rest bit-identical
    full = _fleet(f, r["F"])
    full.step_servo_lqg(100, "estimate", z)
    bare = _fleet(f, r["F"])
    SL.lqg_step_into("f64", bare.x, bare._servo, bare._servo_kalman, bare.servo, bare.servo_lqg, bare.params, bare.type_index, ln.DT, 100,
                     "estimate", z, accumulate=False)
    torch.cuda.synchronize()
    assert torch.equal(bare.x, full.x) and torch.equal(bare.servo.integ, full.servo.integ) and torch.equal(bare.servo.ref, full.servo.ref)
    assert torch.equal(bare.servo_lqg.xhat, full.servo_lqg.xhat) and torch.equal(bare.servo_lqg.du_prev, full.servo_lqg.du_prev)
    assert not bool(bare.servo_lqg.err_est.any()) and not bool(bare.servo_lqg.meas.any()) and bool(full.servo_lqg.err_est.all())
    lib, q = _lib.load(), SL.ServoLqgState.zeros(n, DEV)
    for hole in range(4):                                                 # each of err_est, err_meas, chatter, meas_out alone
        one = _fleet(f, r["F"])
        q.reset()
        acc = [q.err_est, q.err_meas, q.chatter, q.meas]
        acc[hole] = None
        rc = lib.fdyn_servo_lqg_step_f64(_lib.ptr(one.x), _lib.ptr(one._servo.x0), _lib.ptr(one._servo.u0), _lib.ptr(one._servo.K), _lib.ptr(one.servo.ref),
                                         _lib.ptr(one.servo.integ), _lib.ptr(one.servo.limits), _lib.ptr(one.type_index), _lib.ptr(one.params),
                                         int(one.params.shape[0]), n, ln.DT, 100, None, None, None, _lib.ptr(one._servo_kalman.F),
                                         _lib.ptr(one._servo_kalman.sigma), _lib.ptr(q.xhat), _lib.ptr(q.du_prev), 0, None, _lib.ptr(z), 0,
                                         *(_lib.ptr(t) for t in acc), _lib.current_stream())
        _lib.check(rc, "fdyn_servo_lqg_step_f64")
        torch.cuda.synchronize()
        assert torch.equal(one.x, full.x) and torch.equal(q.xhat, full.servo_lqg.xhat), hole
        for k, (mine, theirs) in enumerate(zip((q.err_est, q.err_meas, q.chatter, q.meas),
                                               (full.servo_lqg.err_est, full.servo_lqg.err_meas, full.servo_lqg.chatter, full.servo_lqg.meas))):
            assert torch.equal(mine, theirs) if k != hole else not bool(mine.any()), (hole, k)


def test_pass_through_lanes_fly_on_the_measurement(flights, lqg_flights):
    f, r = flights, lqg_flights
    z = _dev(np.ascontiguousarray(np.transpose(r["z"][:100], (0, 2, 1))))
    meas = _fleet(f, r["F"])
    _command(meas, f)
    meas.step_servo_lqg(100, "measurement", z)
    thru = _fleet(f, np.tile(sl.pass_through(), (10, 1)))
    _command(thru, f)
    thru.step_servo_lqg(100, "estimate", z)
    torch.cuda.synchronize()
    err = rel_err(thru.state_numpy(), meas.state_numpy(), STATE_ANGLE_COLS).max()
    print(f"pass-through under the estimate against the designed filter under the measurement, 100 steps: worst {err:.3e}")
    assert err <= 1e-12 and (thru.servo.integ - meas.servo.integ).abs().max().item() <= 1e-12
    assert (thru.servo_lqg.xhat - thru.servo_lqg.meas).abs().max().item() <= 1e-12


def test_heading_through_pi_is_wrapped():
    """A fleet trimmed at heading 3.0 rad is told to turn by +60 deg: psi ITSELF passes +pi and comes back in at -pi, while its
    deviation from the trim heading only goes to 1.05 rad.  This exercises the wraps of the deviation d and of the law's input x0 + f;
    the wraps of the innovation and of the estimate act only in test_a_turn_through_pi_from_the_trim_heading.  The estimate's heading
    word is better than the measurement's over the flight.  At 20 s the heading error is inside 0.1 rad: a
    third of the servo's 0.3 rad error clip, which a turn flown the long way round (300 deg) is nowhere near by then."""
    fleet = BatchedSixDOF(4, "f64", types=tn.TYPES, type_index=[0, 1, 0, 1])
    fleet.trim([20.0, 25.0, 15.0, 18.0], altitude=sn.ALTITUDE, heading=3.0)
    fleet.design_servo()
    fleet.design_servo_kalman(0.01)
    fleet.servo_lqg.seed = 17
    fleet.command_servo(heading=3.0 + np.radians(60.0))
    crossed = torch.zeros(4, dtype=torch.bool, device=DEV)
    widest = torch.zeros((), dtype=torch.float64, device=DEV)
    for _ in range(200):
        fleet.step_servo_lqg(10)
        crossed |= fleet.x[L.FD_X_YAW] < 0.0
        widest = torch.maximum(widest, fleet.servo_lqg.xhat[sl.PSI].abs().max())
    torch.cuda.synchronize()
    q = fleet.servo_lqg
    ratio = (q.err_est[sl.PSI] / q.err_meas[sl.PSI]).cpu().numpy()
    print(f"heading through pi: err_est / err_meas on psi {ratio}, widest |xhat_psi| {float(widest):.4f}, |e_psi| at 20 s "
          f"{fleet.servo.err[2].abs().cpu().numpy()}")
    assert bool(crossed.all()) and float(widest) <= np.pi and (ratio < 1.0).all()
    assert float(fleet.servo.err[2].abs().max()) <= 0.1


@pytest.mark.parametrize("precision", PRECISIONS)
def test_probe_flights_on_sensor_noise_meet_the_gates(precision):
    for dt in (0.01, 0.02):
        rows = [(name, V, climb) for name, V, d, climb in sn.PROBE if d == dt]
        n1, n2, tail = int(round(sn.T_COMMAND / dt)), int(round((sn.T_END - sn.T_COMMAND) / dt)), int(round(10.0 / dt))
        out = {}
        for fb in ("estimate", "measurement"):
            fleet = BatchedSixDOF(len(rows), precision, types=tn.TYPES, type_index=[tn.TYPES.index(r[0]) for r in rows])
            fleet.trim([r[1] for r in rows], np.radians([r[2] for r in rows]), 0.0, sn.ALTITUDE, sn.HEADING)
            fleet.design_servo()
            fleet.design_servo_kalman(dt)
            fleet.servo_lqg.seed = sl.SEED
            ref = fleet.servo.ref.clone()
            att = torch.zeros((2, len(rows)), dtype=torch.float64, device=DEV)
            sq = torch.zeros((3, len(rows)), dtype=torch.float64, device=DEV)
            for k in range((n1 + n2) // 10):
                if k == n1 // 10:
                    fleet.command_servo(heading=ref[L.FD_SVR_HEADING] + sn.COMMAND["heading"], speed=ref[L.FD_SVR_SPEED] + sn.COMMAND["speed"],
                                        altitude=ref[L.FD_SVR_ALTITUDE] + sn.COMMAND["altitude"])
                # the attitude gates hold "throughout": single-step launches for the 3 s after the commands, where roll and pitch peak;
                # elsewhere, and for the rms of the last 10 s, every tenth step is seen
                for _ in range(10 if n1 // 10 <= k < (n1 + int(round(3.0 / dt))) // 10 else 1):
                    fleet.step_servo_lqg(1 if n1 // 10 <= k < (n1 + int(round(3.0 / dt))) // 10 else 10, fb)
                    att = torch.maximum(att, fleet.x[[L.FD_X_ROLL, L.FD_X_PITCH]].abs().to(torch.float64))
                if k >= (n1 + n2 - tail) // 10:
                    sq += fleet.servo.err ** 2                            # the true errors, sampled every ten steps of the last 10 s
            torch.cuda.synchronize()
            q = fleet.servo_lqg
            out[fb] = dict(ratio=(q.err_est / q.err_meas).T.cpu().numpy(), chatter=q.chatter.T.cpu().numpy(),
                           rms=torch.sqrt(sq / (tail // 10)).T.cpu().numpy(), att=att.T.cpu().numpy())
        e, m = out["estimate"], out["measurement"]
        print(f"{precision} dt {dt} {rows}: err_est / err_meas worst {e['ratio'].max(axis=1)}, chatter ratio worst {(e['chatter'] / m['chatter']).max(axis=1)}, "
              f"rms (V, h, psi) {e['rms'].tolist()}, max |roll|, |pitch| {e['att'].tolist()}")
        assert (e["ratio"] < sl.GATE_RATIO).all(), e["ratio"]
        assert (e["chatter"] / m["chatter"] <= sl.GATE_CHATTER).all()
        assert (e["rms"][:, 0] <= sl.GATE_V).all() and (e["rms"][:, 1] <= sl.GATE_H).all() and (e["rms"][:, 2] <= sl.GATE_PSI).all()
        assert (e["att"][:, 0] <= sn.GATE_ROLL).all() and (e["att"][:, 1] <= sn.GATE_PITCH).all()


def test_fleet_methods_are_the_module_functions(golden):
    fleet = BatchedSixDOF(65, "mixed", types=tn.TYPES, type_index=np.arange(65) % 2)
    with pytest.raises(ValueError, match="no servo design"):
        fleet.step_servo_lqg(1)
    tr = fleet.trim(20.0, altitude=sn.ALTITUDE, heading=sn.HEADING)
    d = fleet.design_servo()
    with pytest.raises(ValueError, match="no servo filter"):
        fleet.step_servo_lqg(1)
    kf = fleet.design_servo_kalman(0.01)
    assert kf.count_not_ok() == 0 and kf.dt == 0.01 and torch.equal(kf.sigma, _dev(np.array(sl.DEFAULT_SIGMA)))
    assert float(torch.linalg.eigvals(kf.filter_matrix().permute(0, 3, 1, 2).cpu()).abs().max()) < 1.0
    x, state, q = fleet.x.clone(), SV.ServoState.at_trim(tr.x0), SL.ServoLqgState.zeros(65, DEV)
    fleet.command_servo(speed=23.0)
    state.command(speed=23.0)
    fleet.step_servo_lqg(50)
    u, sat = torch.zeros_like(fleet.u), torch.zeros_like(fleet.lqr_saturated_steps)
    SL.lqg_step_into("mixed", x, d, kf, state, q, fleet.params, fleet.type_index, 0.01, 50, surf_out=u, sat_steps=sat, err_out=state.err)
    torch.cuda.synchronize()
    assert torch.equal(x, fleet.x) and torch.equal(u, fleet.u) and torch.equal(state.integ, fleet.servo.integ) and torch.equal(state.err, fleet.servo.err)
    assert torch.equal(q.xhat, fleet.servo_lqg.xhat) and torch.equal(q.err_est, fleet.servo_lqg.err_est) and q.step.tolist() == [50]
    assert fleet.time == pytest.approx(0.5)
    per_lane = SL.ServoKalmanNoise(rates=tuple(np.full(65, r) for r in sl.DEFAULT_RATES))
    assert torch.equal(fleet.design_servo_kalman(0.01, per_lane).F, kf.F)

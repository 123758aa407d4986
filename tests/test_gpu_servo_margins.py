"""fdyn_servo_loop_margins and hcrl_amd.servo_margins on the device.

Reference on the box: the NumPy restatement (tests/servo_margin_numpy.py) on the designs the servo and servo-Kalman restatements make
of the 288 linearisations of tests/golden/trim_reference.npz, computed once per session.

Gates (none derived from what the kernel returns):
  grid          every word of curve, alpha_s, alpha_t, idx_s, idx_t and status BIT-IDENTICAL to the restatement at dt 0.01 and 0.02
                under estimate and truth feedback (fp64 on both sides, one rounding per operation in the same order).  The one
                exception provided for: up to 4 ulp in words downstream of a square root should the device's fp64 sqrt round
                differently, indices then differing only where the two competing curve values are within those 4 ulp; the test prints
                whether it was used
  shapes        n = 1, 63, 65, 257 with sentinel pads behind every output; curve = NULL leaves the rest bit-equal; lane position
                is irrelevant;  n_omega = 1, 7, 64, 256;  n_omega 0, 257, -1, n = 0, -1 and every missing required pointer are
                refused with nothing written
  bad lanes     every kind of servo_margin_numpy.bad_cases that shares the launch's dt interleaved among good lanes: the good lanes
                bit-identical to a launch without them, the bad lanes exactly the restatement's status, NaNs and -1 indices; the
                whole launch at dt = 0 is BAD_INPUT
  graph         replay bit-equal to eager
  fleet         BatchedSixDOF.trim -> design_servo -> design_servo_kalman -> servo_loop_margins on the device against the same chain
                in NumPy over the CPU oracle (the ten aircraft of lqr_numpy.oracle_flights): alpha within 1e-9 relative; and
                bit-identical to the restatement on the fleet's own K, F and x0 read back
  flight        the golden aircraft with the smallest lateral alpha_s at dt 0.02 under truth feedback (status 0) flies
                fdyn_servo_step_f64 for 500 steps of 0.02 s from 0.1 x lqr_numpy.PERTURBATION with no control clipped and ends with
                at most 0.06 of its starting deviation: servo_numpy.fly over the CPU oracle ends at 0.030 of it, a factor 2 kept

Every test runs under a time limit of its own (a watchdog that ends the process, so nothing more is started on the device).
"""
import faulthandler
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import lqr_numpy as ln
import servo_lqg_numpy as sl
import servo_margin_numpy as sm
import servo_numpy as sn
import trim_numpy as tn
from hcrl_amd import _lib, layout as L
from hcrl_amd import servo as SV
from hcrl_amd import servo_margins as SM
from hcrl_amd.fleet import BatchedSixDOF
from hcrl_amd.params import param_table

pytestmark = pytest.mark.gpu

SENTINEL = -12345.678
ISENT = -1234567
PAD = 96
DEV = "cuda"
FEEDBACKS = (sm.ESTIMATE, sm.TRUTH)
KEYS = ("alpha_s", "idx_s", "alpha_t", "idx_t", "curve", "status")
TIME_LIMIT_S = 120
FLIGHT_STEPS, FLIGHT_SHRINK = 500, 0.06


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(TIME_LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _dev(a, dtype=None):
    t = torch.as_tensor(np.array(a, order="C"), device=DEV)
    return t if dtype is None else t.to(dtype)


def _padded(rows, n, dtype=torch.float64, fill=SENTINEL):
    return torch.full((rows * n + PAD,), fill, dtype=dtype, device=DEV)


def _margins(K, F, x0, dt, feedback, zre, zim, curve=True, n_omega=None, n=None, expect_rc=0, hole=None):
    """K [n][26], F [n][120], x0 [n][12] (host) -> dict of host arrays shaped as servo_margin_numpy.loop_margins shapes them; every
    output buffer has a sentinel pad behind it, asserted untouched.  hole: the name of a pointer to pass as NULL."""
    rows, W = len(K), len(zre) if n_omega is None else n_omega
    n_arg = rows if n is None else n
    a_s, a_t = _padded(2, rows), _padded(2, rows)
    i_s, i_t, st = _padded(2, rows, torch.int32, ISENT), _padded(2, rows, torch.int32, ISENT), _padded(1, rows, torch.int32, ISENT)
    cv = _padded(2 * max(W, 1), rows)
    p = dict(K=_dev(np.asarray(K).T), F=_dev(np.asarray(F).T), x0=_dev(np.asarray(x0).T), zre=_dev(zre), zim=_dev(zim), alpha_s=a_s, idx_s=i_s,
             alpha_t=a_t, idx_t=i_t, curve=cv if curve else None, status=st)
    if hole is not None:
        p[hole] = None
    rc = _lib.load().fdyn_servo_loop_margins(_lib.ptr(p["K"]), _lib.ptr(p["F"]), _lib.ptr(p["x0"]), float(dt), int(feedback), _lib.ptr(p["zre"]),
                                             _lib.ptr(p["zim"]), W, n_arg, _lib.ptr(p["alpha_s"]), _lib.ptr(p["idx_s"]), _lib.ptr(p["alpha_t"]),
                                             _lib.ptr(p["idx_t"]), _lib.ptr(p["curve"]), _lib.ptr(p["status"]), _lib.current_stream())
    torch.cuda.synchronize()
    assert rc == expect_rc, rc
    if rc:
        for buf, sent in ((a_s, SENTINEL), (a_t, SENTINEL), (cv, SENTINEL), (i_s, ISENT), (i_t, ISENT), (st, ISENT)):
            assert bool((buf == sent).all()), "a refused launch wrote something"
        return None
    n = rows
    for buf, r, sent in ((a_s, 2, SENTINEL), (a_t, 2, SENTINEL), (i_s, 2, ISENT), (i_t, 2, ISENT), (st, 1, ISENT), (cv, 2 * W if curve else 0, SENTINEL)):
        assert bool((buf[r * n:] == sent).all()), "wrote behind an output buffer"
    two = lambda t: t[:2 * n].reshape(2, n).T.cpu().numpy()
    return dict(alpha_s=two(a_s), idx_s=two(i_s), alpha_t=two(a_t), idx_t=two(i_t), status=st[:n].cpu().numpy(),
                curve=cv[:2 * W * n].reshape(2, W, n).permute(2, 0, 1).cpu().numpy() if curve else None)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same(a, b, keys=KEYS):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in keys)


def _take(r, idx):
    return {k: (None if r[k] is None else r[k][idx]) for k in KEYS}


def _ulps(a, b):
    """Distance in units of the last place between finite positive fp64 words of equal shape (NaN against NaN: 0)."""
    both_nan = (a != a) & (b != b)
    d = np.abs(_bits(a).astype(np.int64) - _bits(b).astype(np.int64))
    return np.where(both_nan, 0, d)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "trim_reference.npz"))


@pytest.fixture(scope="module")
def designs(golden):
    return sm.golden_designs(golden)


@pytest.fixture(scope="module")
def grids():
    return {dt: sm.unit_circle(sm.default_omega(dt), dt) for dt in sm.DTS}


@pytest.fixture(scope="module")
def want(designs, grids):
    return {(dt, fb): sm.loop_margins(designs["K"], designs["F"][dt], designs["x0"], dt, fb, *grids[dt]) for dt in sm.DTS for fb in FEEDBACKS}


@pytest.fixture(scope="module")
def grid_est(designs, grids):
    """The 288 aircraft at dt 0.01 under estimate feedback in ONE launch: what the shape tests compare with."""
    return _margins(designs["K"], designs["F"][0.01], designs["x0"], 0.01, sm.ESTIMATE, *grids[0.01])


# ---- the kernel against the restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", sm.DTS)
@pytest.mark.parametrize("fb", FEEDBACKS)
def test_grid_is_bit_identical_to_the_restatement(designs, grids, want, dt, fb):
    got, ref = _margins(designs["K"], designs["F"][dt], designs["x0"], dt, fb, *grids[dt]), want[dt, fb]
    assert got["status"].shape == (288,) and not got["status"].any(), np.flatnonzero(got["status"])
    assert np.array_equal(got["status"], ref["status"])
    worst = 0
    for k in ("curve", "alpha_s", "alpha_t"):
        ulp = _ulps(got[k], ref[k])
        worst = max(worst, int(ulp.max()))
        print(f"dt {dt} feedback {fb}: {k}: {int((ulp != 0).sum())} of {ulp.size} words differ from the restatement's, worst {int(ulp.max())} ulp")
    a = got["alpha_s"]
    print(f"dt {dt} feedback {fb}: alpha_s lon {a[:, 0].min():.4f}..{a[:, 0].max():.4f}, lat {a[:, 1].min():.4f}..{a[:, 1].max():.4f}; "
          f"the 4-ulp square-root exception was {'USED' if worst else 'not used'}")
    if worst == 0:
        assert _same(got, ref)
        return
    # every output word is downstream of a square root (V0, and the closed-form singular values): at most 4 ulp
    assert worst <= 4
    rows = np.arange(288)
    for blk in range(2):
        for idx_key, cv in (("idx_s", ref["curve"][:, blk]), ("idx_t", ref["curve_t"][:, blk])):
            gi, ri = got[idx_key][:, blk], ref[idx_key][:, blk]
            differ = gi != ri
            assert (_ulps(cv[rows, gi], cv[rows, ri])[differ] <= 4).all(), (idx_key, blk, np.flatnonzero(differ))


@pytest.mark.parametrize("n", [1, 63, 65, 257])
def test_shapes_lane_position_and_no_curve(n, grid_est, designs, grids):
    idx = (np.arange(n) * 7 + 3) % 288
    K, F, x0 = designs["K"][idx], designs["F"][0.01][idx], designs["x0"][idx]
    got = _margins(K, F, x0, 0.01, sm.ESTIMATE, *grids[0.01])
    assert _same(got, _take(grid_est, idx)), "a lane's result depends on where it sits in the launch"
    bare = _margins(K, F, x0, 0.01, sm.ESTIMATE, *grids[0.01], curve=False)
    assert bare["curve"] is None and _same(bare, got, [k for k in KEYS if k != "curve"])


@pytest.mark.parametrize("n_omega", [1, 7, 64, 256])
def test_grid_sizes(n_omega, designs, grid_est, grids):
    """Per point: a grid point's curve word does not depend on how many points the grid has, and everything is the restatement's."""
    idx = np.arange(0, 288, 9)
    omega = np.geomspace(1e-2, np.pi / 0.01, n_omega) if n_omega > 1 else np.array([np.pi / 0.01])
    omega[-1] = np.pi / 0.01
    zre, zim = sm.unit_circle(omega, 0.01)
    K, F, x0 = designs["K"][idx], designs["F"][0.01][idx], designs["x0"][idx]
    for fb in (sm.ESTIMATE, sm.MEASUREMENT):
        got = _margins(K, F, x0, 0.01, fb, zre, zim)
        assert got["curve"].shape == (len(idx), 2, n_omega) and not got["status"].any()
        ref = sm.loop_margins(K, F, x0, 0.01, fb, zre, zim)
        exact = _same(got, ref)
        assert exact or max(int(_ulps(got[k], ref[k]).max()) for k in ("curve", "alpha_s", "alpha_t")) <= 4
    # the Nyquist point is the last point of every one of these grids: the same word as in the 64-point launch
    est = _margins(K, F, x0, 0.01, sm.ESTIMATE, zre, zim)
    assert np.array_equal(_bits(est["curve"][:, :, -1]), _bits(grid_est["curve"][idx][:, :, -1]))


@pytest.mark.parametrize("n_omega", [0, 257, -1])
def test_grid_sizes_outside_1_to_256_are_refused(n_omega, designs):
    z = np.full(300, 0.5)
    assert _margins(designs["K"][:5], designs["F"][0.01][:5], designs["x0"][:5], 0.01, sm.ESTIMATE, z, z, n_omega=n_omega,
                    expect_rc=_lib.FDYN_ERR_BAD_SIZE) is None


def test_empty_fleets_missing_pointers_and_unknown_feedback_are_refused(designs, grids):
    K, F, x0 = designs["K"][:5], designs["F"][0.02][:5], designs["x0"][:5]
    for n in (0, -1):
        assert _margins(K, F, x0, 0.02, sm.ESTIMATE, *grids[0.02], n=n, expect_rc=_lib.FDYN_ERR_BAD_SIZE) is None
    for hole in ("K", "F", "x0", "zre", "zim", "alpha_s", "idx_s", "alpha_t", "idx_t", "status"):
        assert _margins(K, F, x0, 0.02, sm.ESTIMATE, *grids[0.02], hole=hole, expect_rc=_lib.FDYN_ERR_NULL) is None, hole
    assert _margins(K, F, x0, 0.02, 3, *grids[0.02], expect_rc=_lib.FDYN_ERR_BAD_SIZE) is None


def test_measurement_feedback_is_truth_feedback(designs, grids):
    K, F, x0 = designs["K"][:65], designs["F"][0.02][:65], designs["x0"][:65]
    assert _same(_margins(K, F, x0, 0.02, sm.MEASUREMENT, *grids[0.02]), _margins(K, F, x0, 0.02, sm.TRUTH, *grids[0.02]))


@pytest.mark.parametrize("fb", FEEDBACKS)
def test_bad_lanes_and_their_neighbours(fb, designs):
    zre, zim = sm.unit_circle(sm.default_omega(0.01, 7), 0.01)
    keep = np.arange(0, 288, 4)                                          # 72 good aircraft, both airframes
    cases = lambda i: [c for c in sm.bad_cases(designs["K"][i], designs["F"][0.01][i], designs["x0"][i]) if c[4] == 0.01]
    n_kinds = len(cases(0))
    assert n_kinds == 12                                                  # every kind but dt = 0, which is the launch's own
    K, F, X, kind = [], [], [], []
    for j, i in enumerate(keep):
        K.append(designs["K"][i]); F.append(designs["F"][0.01][i]); X.append(designs["x0"][i]); kind.append(-1)
        if j % 3 == 2:
            c = (j // 3) % n_kinds
            _, k, f, x, _, _, _ = cases(i)[c]
            K.append(k); F.append(f); X.append(x); kind.append(c)
    K, F, X, kind = np.array(K), np.array(F), np.array(X), np.array(kind)
    assert all((kind == c).sum() >= 2 for c in range(n_kinds))
    mixed = _margins(K, F, X, 0.01, fb, zre, zim)
    alone = _margins(designs["K"][keep], designs["F"][0.01][keep], designs["x0"][keep], 0.01, fb, zre, zim)
    assert not alone["status"].any()
    assert _same(_take(mixed, kind < 0), alone), "a good lane changed because of its neighbour"
    ref = sm.loop_margins(K, F, X, 0.01, fb, zre, zim)
    assert np.array_equal(mixed["status"], ref["status"]) and np.array_equal(mixed["idx_s"], ref["idx_s"]) and np.array_equal(mixed["idx_t"], ref["idx_t"])
    assert _same(mixed, ref) or max(int(_ulps(mixed[k], ref[k]).max()) for k in ("curve", "alpha_s", "alpha_t")) <= 4
    col = 5 if fb == sm.ESTIMATE else 6
    for c, case in enumerate(cases(0)):
        st = mixed["status"][kind == c]
        dead = (st & (sm.SINGULAR | sm.BAD_INPUT)) != 0
        assert (st == case[col]).all(), (case[0], st)
        rows = _take(mixed, kind == c)
        assert np.isnan(rows["alpha_s"][dead]).all() and np.isnan(rows["alpha_t"][dead]).all() and np.isnan(rows["curve"][dead]).all()
        assert (rows["idx_s"][dead] == -1).all() and (rows["idx_t"][dead] == -1).all()
        assert np.isfinite(rows["alpha_s"][~dead]).all() and np.isfinite(rows["curve"][~dead]).all()
        if case[col] == 0:                                                # NaN words that are not read: the good lane's own result
            assert "not read" in case[0] or "read under estimate feedback only" in case[0], case[0]
            src = np.flatnonzero(kind == c) - 1                           # the good lane in front of it is the same aircraft
            assert _same(rows, _take(mixed, src))
        if case[0] == "the pass-through filter":
            assert (st == sm.NOT_STABLE).all() and (rows["alpha_s"] == 1.0).all() and np.isposinf(rows["alpha_t"]).all()
            assert (rows["idx_s"] == 0).all() and (rows["idx_t"] == 0).all()
    # a grid that holds z = 1: every lane SINGULAR; dt = 0: every lane BAD_INPUT; both exactly the restatement's
    one = _margins(designs["K"][keep], designs["F"][0.01][keep], designs["x0"][keep], 0.01, fb, *sm.grid_with_one())
    assert (one["status"] == sm.SINGULAR).all() and np.isnan(one["curve"]).all() and (one["idx_s"] == -1).all()
    zero = _margins(designs["K"][keep], designs["F"][0.01][keep], designs["x0"][keep], 0.0, fb, zre, zim)
    assert (zero["status"] == sm.BAD_INPUT).all() and np.isnan(zero["alpha_s"]).all() and np.isnan(zero["curve"]).all() and (zero["idx_t"] == -1).all()


def test_graph_replay_equals_eager(designs, grids):
    K, F, x0 = _dev(designs["K"].T), _dev(designs["F"][0.02].T), _dev(designs["x0"].T)
    zre, zim = (_dev(v) for v in grids[0.02])
    eager = SM.servo_margins_into(K, F, x0, 0.02, zre, zim, "estimate", curve=True)
    out = SM.servo_margins_into(K, F, x0, 0.02, zre, zim, "truth", curve=True)     # other values, then overwritten by the replay
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                                 # warm-up outside the capture
        SM.servo_margins_into(K, F, x0, 0.02, zre, zim, "truth", out)
    torch.cuda.current_stream().wait_stream(s)
    assert not torch.equal(out.alpha_s, eager.alpha_s)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        SM.servo_margins_into(K, F, x0, 0.02, zre, zim, "estimate", out)
    gr.replay()
    torch.cuda.synchronize()
    for a, b in ((eager.alpha_s, out.alpha_s), (eager.idx_s, out.idx_s), (eager.alpha_t, out.alpha_t), (eager.idx_t, out.idx_t),
                 (eager.status, out.status)):
        assert torch.equal(a, b)
    assert np.array_equal(_bits(eager.curve.cpu().numpy()), _bits(out.curve.cpu().numpy()))


# ---- the fleet -----------------------------------------------------------------------------------------------------------------
def test_fleet_chain_against_numpy_over_the_oracle():
    """trim -> design_servo -> design_servo_kalman -> servo_loop_margins on the device against the same chain in NumPy over the CPU
    oracle (the ten aircraft of lqr_numpy.oracle_flights): alpha within 1e-9 relative."""
    base = sn.compare_flights()
    n = len(base["type"])
    fleet = BatchedSixDOF(n, "f64", types=tn.TYPES, type_index=base["type"])
    with pytest.raises(ValueError, match="no certified stabilising servo gain"):
        fleet.servo_loop_margins()
    fleet.trim(base["spec"][:, 0], base["spec"][:, 1], base["spec"][:, 2], ln.ALTITUDE, ln.HEADING)
    servo = fleet.design_servo()
    with pytest.raises(ValueError, match="no certified stable servo filter"):
        fleet.servo_loop_margins()
    for dt in sm.DTS:
        kal = fleet.design_servo_kalman(dt)
        F_ref = sl.design_many(base["A"], base["B"], dt, sl.default_noise())["F"]
        omega = sm.default_omega(dt)
        for name, fb in (("estimate", sm.ESTIMATE), ("truth", sm.TRUTH)):
            m = fleet.servo_loop_margins(name, curve=True)
            ref = sm.loop_margins(base["K"], F_ref, base["x0"], dt, fb, *sm.unit_circle(omega, dt))
            own = sm.loop_margins(servo.K.T.cpu().numpy(), kal.F.T.cpu().numpy(), servo.x0.T.cpu().numpy(), dt, fb, *sm.unit_circle(omega, dt))
            assert bool(m.ok.all()) and not ref["status"].any() and m.dt == dt and m.feedback == fb
            got_s, got_t = m.alpha_s.T.cpu().numpy(), m.alpha_t.T.cpu().numpy()
            exact = np.array_equal(_bits(got_s), _bits(own["alpha_s"])) and np.array_equal(_bits(got_t), _bits(own["alpha_t"]))
            assert exact or max(int(_ulps(got_s, own["alpha_s"]).max()), int(_ulps(got_t, own["alpha_t"]).max())) <= 4
            assert np.array_equal(m.idx_s.T.cpu().numpy(), own["idx_s"]) and np.array_equal(m.status.cpu().numpy(), own["status"])
            err_s = np.abs(got_s / ref["alpha_s"] - 1.0).max()
            err_t = np.abs(got_t / ref["alpha_t"] - 1.0).max()
            print(f"dt {dt} {name}: alpha_s {float(m.alpha_s.min()):.4f}..{float(m.alpha_s.max()):.4f}; fleet chain against NumPy over the "
                  f"oracle: alpha_s {err_s:.3e}, alpha_t {err_t:.3e}; bit-identical to the restatement on the fleet's own words: {exact}")
            assert err_s <= 1e-9 and err_t <= 1e-9
            assert np.array_equal(m.omega_s.cpu().numpy(), omega[m.idx_s.cpu().numpy()]) and np.array_equal(m.omega.cpu().numpy(), SM.default_grid(dt))
            low, high = m.gain_margin()
            assert bool((low < 1.0).all()) and bool((high > 1.0).all()) and bool((m.phase_margin_deg() > 0.0).all())
            assert tuple(m.curve.shape) == (2, 64, n)
    few = fleet.servo_loop_margins("estimate", omega=[1.0, 10.0, 100.0])
    assert few.curve is None and int(few.idx_s.max()) <= 2 and bool(few.ok.all())


def test_the_least_robust_certified_servo_loop_flies_stably(golden, designs, want):
    """The golden aircraft with the smallest lateral alpha_s at dt 0.02 under truth feedback, K as designed, status 0: flown by
    fdyn_servo_step_f64 for 500 steps of 0.02 s from a tenth of lqr_numpy.PERTURBATION no control clips and the deviation shrinks to
    at most FLIGHT_SHRINK of its start -- twice what the same flight leaves in NumPy over the CPU oracle."""
    dt = 0.02
    ref = want[dt, sm.TRUTH]
    i = int(np.argmin(ref["alpha_s"][:, 1]))
    assert ref["status"][i] == 0
    name = tn.TYPES[int(golden["type"][i])]
    x0, u0, K = golden["x0"][i], golden["u0"][i], designs["K"][i]
    x = np.array(x0, np.float64)
    for k, v in ln.PERTURBATION.items():
        x[k] += 0.1 * v
    start = ln.deviation(x, x0)
    # the same flight in NumPy over the CPU oracle: where the step count and the shrink factor come from
    P = tn.oracle_airframe(name, golden["scales"][i])[4]
    xe, _, _, _, sat_ref = sn.fly(sn.oracle_step(P), K, x0, u0, x, sn.reference_at(x0), np.zeros(3), dt, FLIGHT_STEPS)
    end_ref = ln.deviation(xe, x0)
    assert sat_ref == 0 and end_ref <= 0.5 * FLIGHT_SHRINK * start, (sat_ref, end_ref, start)

    fleet = BatchedSixDOF(1, "f64", types=(name,))
    fleet.params = _dev(tn.scaled_block(param_table((name,))[0], golden["scales"][i], L)[None])       # the golden grid scales the mass
    fleet.reset(x[None])
    zi, zd = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.float64, device=DEV)
    fleet._servo = SV.ServoDesign(_dev(K[None].T), zd, zi, zi.clone(), _dev(x0[None].T), _dev(u0[None].T))
    fleet.servo = SV.ServoState.at_trim(fleet._servo.x0)
    got = _margins(designs["K"][i:i + 1], designs["F"][dt][i:i + 1], designs["x0"][i:i + 1], dt, sm.TRUTH, *sm.unit_circle(sm.default_omega(dt), dt))
    assert got["status"][0] == 0 and int(_ulps(got["alpha_s"][0, 1:], ref["alpha_s"][i, 1:]).max()) <= 4
    fleet.step_servo(FLIGHT_STEPS, dt)
    torch.cuda.synchronize()
    end = ln.deviation(fleet.state_numpy()[0], x0)
    sat = int(fleet.lqr_saturated_steps[0])
    print(f"aircraft {i} ({name}): lateral alpha_s {ref['alpha_s'][i, 1]:.4f} at dt {dt}; deviation {start:.4f} -> {end:.6f} after {FLIGHT_STEPS} "
          f"steps (NumPy over the oracle: {end_ref:.6f}), saturated steps {sat}")
    assert sat == 0
    assert np.isfinite(end) and end <= FLIGHT_SHRINK * start

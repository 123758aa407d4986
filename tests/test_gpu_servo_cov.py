"""fdyn_servo_covariance, fdyn_stein_solve and hcrl_amd.servo_covariance on the device.

Reference on the box: the NumPy restatement (tests/servo_cov_numpy.py) on the 288 linearisations of tests/golden/trim_reference.npz
under the restatements' default servo and servo-Kalman designs, computed once per session and left unchanged.

Gates (none derived from what the kernel returns):
  grid          the 288 golden lanes in one launch, 3 feedbacks x dt 0.01 and 0.02, without process noise (and with the design's rates
                at dt 0.02): status, iters, residual and every word of report and cov BIT-IDENTICAL to the restatement (fp64 on both
                sides, one rounding per operation in the same order; + - * / only.  The 1e-12 fallback for a differing contraction
                is not used)
  shapes        n = 1, 63, 65, 257 with sentinel pads behind every output; shared sigma / w_rate equal per-lane sigma / w_rate to
                the bit; cov = NULL, iters = NULL or w_rate = NULL (against zero rates) leave the rest bit-equal
  bad lanes     a NaN word, a zero gain, a pass-through filter and sigma < 0 interleaved among good lanes: all NaN with the right
                status bit, the good lanes bit-identical to the restatement
  graph         replay bit-equal to eager for both entries; refused calls write nothing
  stein         fdyn_stein_solve at (N, M) = (1,1), (2,7), (5,5), (7,5), (7,7), the NaN, overflow, cap and Q = 0 lanes beside them:
                bit-identical to the restatement
  fleet         BatchedSixDOF.servo_covariance equals servo_covariance_into on the fleet's own words
  flight        256 lanes of rc_plane at 20 m/s, dt 0.01, mixed precision, in-kernel Philox draws (a row per lane), estimate feedback,
                1000 steps discarded and 3000 accumulated: the lane-mean err_est and chatter per step within 0.9 .. 1.1 of the
                device's own report (the gate of tests/test_servo_cov_oracle.py (c)), and no saturated step
"""
import faulthandler
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import servo_cov_numpy as sc
import servo_lqg_numpy as sl
import servo_margin_numpy as sm
from hcrl_amd import _lib, layout as L
from hcrl_amd import servo_covariance as SC
from hcrl_amd.fleet import BatchedSixDOF

pytestmark = pytest.mark.gpu

SENTINEL = -12345.678
ISENT = -1234567
PAD = 96
DEV = "cuda"
KEYS = ("report", "cov", "residual", "iters", "status")
TIME_LIMIT_S = 120
SIGMA, RATES = np.array(sl.DEFAULT_SIGMA), np.array(sl.DEFAULT_RATES)


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(TIME_LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _soa(a):
    """host [n][...] -> device [...][n]"""
    return torch.as_tensor(np.ascontiguousarray(np.moveaxis(np.asarray(a, np.float64), 0, -1)), device=DEV)


def _padded(rows, n, dtype=torch.float64, fill=SENTINEL):
    return torch.full((rows * n + PAD,), fill, dtype=dtype, device=DEV)


def _noise_arg(a, n):
    """None, [10] (shared) or [n][10] (per lane) -> (device tensor or None, per_lane)"""
    if a is None:
        return None, 0
    a = np.asarray(a, np.float64)
    return (_soa(a), 1) if a.ndim == 2 else (torch.as_tensor(a, device=DEV), 0)


def _cov(K, F, x0, dt, sigma, w_rate, fb, cov=True, iters=True, expect_rc=0, drop=None, n=None):
    """One launch of fdyn_servo_covariance -> dict shaped as servo_cov_numpy.servo_covariance_many shapes it; every output buffer has
    a sentinel pad behind it, asserted untouched.  drop: the name of a pointer to pass as NULL."""
    n = len(K) if n is None else n
    m = max(n, 1)
    sg, sg_pl = _noise_arg(sigma, m)
    wr, wr_pl = _noise_arg(w_rate, m)
    rep, cv, res = _padded(L.FD_NSCV, m), _padded(L.FD_NSCC, m), _padded(1, m)
    it, st = _padded(1, m, torch.int32, ISENT), _padded(1, m, torch.int32, ISENT)
    Kd, Fd, xd = _soa(K), _soa(F), _soa(x0)                      # named: they must outlive the launch
    p = dict(K=_lib.ptr(Kd), F=_lib.ptr(Fd), x0=_lib.ptr(xd), sigma=_lib.ptr(sg), w_rate=_lib.ptr(wr), report=_lib.ptr(rep),
             cov=_lib.ptr(cv) if cov else None, residual=_lib.ptr(res), iters=_lib.ptr(it) if iters else None, status=_lib.ptr(st))
    if drop:
        p[drop] = None
    rc = _lib.load().fdyn_servo_covariance(p["K"], p["F"], p["x0"], float(dt), p["sigma"], sg_pl, p["w_rate"], wr_pl, int(fb), n, p["report"],
                                           p["cov"], p["residual"], p["iters"], p["status"], _lib.current_stream())
    torch.cuda.synchronize()
    assert rc == expect_rc, rc
    if rc:
        for buf, sent in ((rep, SENTINEL), (cv, SENTINEL), (res, SENTINEL), (it, ISENT), (st, ISENT)):
            assert bool((buf == sent).all()), "a refused launch wrote something"
        return None
    for buf, r, sent in ((rep, L.FD_NSCV, SENTINEL), (cv, L.FD_NSCC if cov else 0, SENTINEL), (res, 1, SENTINEL), (it, 1 if iters else 0, ISENT),
                         (st, 1, ISENT)):
        assert bool((buf[r * n:] == sent).all()), "wrote behind an output buffer (or into one it was not given)"
    return dict(report=rep[:L.FD_NSCV * n].reshape(L.FD_NSCV, n).T.cpu().numpy(),
                cov=cv[:L.FD_NSCC * n].reshape(L.FD_NSCC, n).T.cpu().numpy() if cov else None, residual=res[:n].cpu().numpy(),
                iters=it[:n].cpu().numpy() if iters else None, status=st[:n].cpu().numpy())


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _differing(a, b, keys=KEYS):
    return [k for k in keys if not np.array_equal(_bits(a[k]), _bits(b[k]))]


def _take(r, idx, keys=KEYS):
    return {k: r[k][idx] for k in keys}


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "trim_reference.npz"))


@pytest.fixture(scope="module")
def designs(golden):
    return sm.golden_designs(golden)


# ---- the grid ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", sc.DTS)
@pytest.mark.parametrize("fb", sc.FEEDBACKS, ids=("estimate", "measurement", "truth"))
def test_grid_is_bit_identical_to_the_restatement(golden, designs, fb, dt):
    want = sc.golden_reports(golden)[dt, fb]
    got = _cov(designs["K"], designs["F"][dt], designs["x0"], dt, SIGMA, None, fb)
    assert not got["status"].any() and 9 <= got["iters"].min() and got["iters"].max() <= 20
    print(f"feedback {fb} dt {dt}: doublings {got['iters'].min()} .. {got['iters'].max()}, worst residual {got['residual'].max():.2e}")
    assert not _differing(got, want), _differing(got, want)


@pytest.mark.parametrize("fb", sc.FEEDBACKS, ids=("estimate", "measurement", "truth"))
def test_grid_with_process_noise_is_bit_identical_to_the_restatement(golden, designs, fb):
    dt = 0.02
    want = sc.golden_reports(golden, with_w=True)[dt, fb]
    got = _cov(designs["K"], designs["F"][dt], designs["x0"], dt, SIGMA, RATES, fb)
    assert not got["status"].any()
    assert not _differing(got, want), _differing(got, want)


# ---- shapes, optional pointers, shared and per-lane noise ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 63, 65, 257))
def test_shapes_pads_and_optional_pointers(golden, designs, n):
    dt, fb = 0.01, sc.ESTIMATE
    idx = (np.arange(n) * 7 + 3) % 288
    K, F, x0 = designs["K"][idx], designs["F"][dt][idx], designs["x0"][idx]
    want = _take(sc.golden_reports(golden)[dt, fb], idx)
    full = _cov(K, F, x0, dt, SIGMA, None, fb)
    assert not _differing(full, want), _differing(full, want)
    rest = [k for k in KEYS if k != "cov"]
    assert not _differing(_cov(K, F, x0, dt, SIGMA, None, fb, cov=False), want, rest)
    assert not _differing(_cov(K, F, x0, dt, SIGMA, None, fb, iters=False), want, [k for k in KEYS if k != "iters"])
    assert not _differing(_cov(K, F, x0, dt, SIGMA, np.zeros(10), fb), want)                       # w_rate = NULL is w_rate = 0
    # shared against per-lane noise
    assert not _differing(_cov(K, F, x0, dt, np.tile(SIGMA, (n, 1)), None, fb), want)
    with_w = _take(sc.golden_reports(golden, with_w=True)[0.02, sc.MEASUREMENT], idx)
    F2 = designs["F"][0.02][idx]
    assert not _differing(_cov(K, F2, x0, 0.02, SIGMA, RATES, sc.MEASUREMENT), with_w)
    assert not _differing(_cov(K, F2, x0, 0.02, np.tile(SIGMA, (n, 1)), np.tile(RATES, (n, 1)), sc.MEASUREMENT), with_w)


def test_per_lane_noise_varies_by_lane(designs):
    """A noise sweep in one launch: every lane its own sigma and rates, against the restatement lane by lane."""
    n, dt = 70, 0.02
    rs = np.random.RandomState(3)
    idx = rs.randint(0, 288, n)
    sg, wr = SIGMA * rs.uniform(0.5, 2.0, (n, 10)), RATES * rs.uniform(0.0, 2.0, (n, 10))
    K, F, x0 = designs["K"][idx], designs["F"][dt][idx], designs["x0"][idx]
    for fb in sc.FEEDBACKS:
        want = sc.servo_covariance_many(K, F, x0, dt, sg, wr, fb)
        got = _cov(K, F, x0, dt, sg, wr, fb)
        assert not want["status"].any() and not _differing(got, want), (fb, _differing(got, want))


# ---- bad lanes ---------------------------------------------------------------------------------------------------------------------
def test_bad_lanes_do_not_disturb_their_neighbours(golden, designs):
    n, dt = 130, 0.01
    K, F, x0 = designs["K"][:n].copy(), designs["F"][dt][:n].copy(), designs["x0"][:n].copy()
    sg = np.tile(SIGMA, (n, 1))
    K[3, 9] = np.nan                                             # a NaN word
    F[64, 101] = np.inf
    K[17] = 0.0                                                  # the zero gain of a failed servo design
    F[70] = sl.pass_through()                                    # the pass-through filter of a failed filter design
    sg[100, 4] = -0.5                                            # sigma < 0
    x0[129, [sc.sn.X_U, sc.sn.X_W]] = 0.0
    bad = {3: sc.BAD_INPUT, 64: sc.BAD_INPUT, 17: sc.UNSTABLE, 70: sc.UNSTABLE, 100: sc.BAD_INPUT, 129: sc.BAD_INPUT}
    for fb in sc.FEEDBACKS:
        got = _cov(K, F, x0, dt, sg, None, fb)
        want = sc.servo_covariance_many(K, F, x0, dt, sg, None, fb)
        assert {int(i): int(s) for i, s in enumerate(got["status"]) if s} == bad
        for i in bad:
            assert np.isnan(got["report"][i]).all() and np.isnan(got["cov"][i]).all() and np.isnan(got["residual"][i]) and got["iters"][i] == 0
        assert not _differing(got, want), _differing(got, want)
        good = np.array([i for i in range(n) if i not in bad])
        assert not _differing(_take(got, good), _take(sc.golden_reports(golden)[dt, fb], good))


# ---- graph and refusals -----------------------------------------------------------------------------------------------------------
def test_graph_replay_is_bit_equal_to_eager(designs):
    dt, n = 0.02, 288
    K, F, x0, sg, wr = _soa(designs["K"]), _soa(designs["F"][dt]), _soa(designs["x0"]), torch.as_tensor(SIGMA, device=DEV), torch.as_tensor(RATES, device=DEV)
    eager = SC.servo_covariance_into(K, F, x0, dt, sg, wr, "estimate")
    out = SC.empty(n, K.device)
    for t in (out.report, out.cov, out.residual):
        t.fill_(SENTINEL)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        SC.servo_covariance_into(K, F, x0, dt, sg, wr, "estimate", out)
    gr.replay()
    torch.cuda.synchronize()
    assert bool(eager.ok.all())
    for a, b in ((eager.report, out.report), (eager.cov, out.cov), (eager.residual, out.residual)):
        assert np.array_equal(_bits(a.cpu().numpy()), _bits(b.cpu().numpy()))
    assert torch.equal(eager.iterations, out.iterations) and torch.equal(eager.status, out.status)

    A, B, Q = (torch.as_tensor(np.ascontiguousarray(np.repeat(v[..., None], 65, axis=-1)), device=DEV) for v in sc.stein_cases()[7, 5])
    eager = SC.stein_solve(A, B, Q)
    sol = SC.SteinSolution(torch.full_like(eager.X, SENTINEL), torch.full_like(eager.residual, SENTINEL), torch.zeros_like(eager.iterations),
                           torch.zeros_like(eager.status))
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        SC.stein_solve(A, B, Q, sol)
    gr.replay()
    torch.cuda.synchronize()
    assert bool(eager.ok.all()) and np.array_equal(_bits(eager.X.cpu().numpy()), _bits(sol.X.cpu().numpy()))
    assert torch.equal(eager.residual, sol.residual) and torch.equal(eager.iterations, sol.iterations) and torch.equal(eager.status, sol.status)


def test_refused_calls_write_nothing(designs):
    K, F, x0 = designs["K"][:4], designs["F"][0.01][:4], designs["x0"][:4]
    for n in (0, -1):
        assert _cov(K, F, x0, 0.01, SIGMA, None, 0, expect_rc=_lib.FDYN_ERR_BAD_SIZE, n=n) is None
    assert _cov(K, F, x0, 0.01, SIGMA, None, 3, expect_rc=_lib.FDYN_ERR_BAD_SIZE) is None
    for drop in ("K", "F", "x0", "sigma", "report", "residual", "status"):
        assert _cov(K, F, x0, 0.01, SIGMA, None, 0, expect_rc=_lib.FDYN_ERR_NULL, drop=drop) is None
    for dt in (0.0, 2.0):
        assert _cov(K, F, x0, dt, SIGMA, None, 0, expect_rc=_lib.FDYN_ERR_BAD_DT) is None


# ---- the general solver --------------------------------------------------------------------------------------------------------------
def test_stein_solve_is_bit_identical_to_the_restatement():
    cases = sc.stein_cases()
    for (N, M), (A, B, Q) in cases.items():
        lanes = [(A, B, Q), (0.5 * A, B, -Q), (A, 0.25 * B, Q + 1.0), (A, B, np.zeros((N, M))), (A, B, np.where(np.arange(N * M).reshape(N, M) == 0, np.nan, Q)),
                 (4.0 * A, 4.0 * B, Q)]
        if (N, M) == (2, 7):
            lanes = lanes * 11                                   # more than one workgroup
        want = [sc.stein_solve(*lane) for lane in lanes]
        n = len(lanes)
        As, Bs, Qs = (torch.as_tensor(np.ascontiguousarray(np.stack([lane[k] for lane in lanes], axis=-1)), device=DEV) for k in range(3))
        X, res = _padded(N * M, n), _padded(1, n)
        it, st = _padded(1, n, torch.int32, ISENT), _padded(1, n, torch.int32, ISENT)
        rc = _lib.load().fdyn_stein_solve(_lib.ptr(As), _lib.ptr(Bs), _lib.ptr(Qs), N, M, n, _lib.ptr(X), _lib.ptr(res), _lib.ptr(it), _lib.ptr(st),
                                          _lib.current_stream())
        torch.cuda.synchronize()
        assert rc == 0
        for buf, r, sent in ((X, N * M, SENTINEL), (res, 1, SENTINEL), (it, 1, ISENT), (st, 1, ISENT)):
            assert bool((buf[r * n:] == sent).all())
        gotX = X[:N * M * n].reshape(N, M, n).permute(2, 0, 1).cpu().numpy()
        assert np.array_equal(_bits(gotX), _bits(np.array([w["X"] for w in want]))), (N, M)
        assert np.array_equal(_bits(res[:n].cpu().numpy()), _bits(np.array([w["residual"] for w in want], np.float64))), (N, M)
        assert np.array_equal(it[:n].cpu().numpy(), np.array([w["iters"] for w in want], np.int32))
        status = np.array([w["status"] for w in want], np.int32)
        assert np.array_equal(st[:n].cpu().numpy(), status)
        assert list(status[:6]) == [0, 0, 0, 0, sc.BAD_INPUT, sc.NOT_CONVERGED], (N, M, status[:6])
    # the cap, through the host function with residual and iters left out of nothing
    A, B, Q = (torch.as_tensor(np.ascontiguousarray(np.repeat(v[..., None], 3, axis=-1)), device=DEV) for v in sc.cap_case())
    sol = SC.stein_solve(A, B, Q)
    torch.cuda.synchronize()
    want = sc.stein_solve(*sc.cap_case())
    assert want["status"] == sc.NOT_CONVERGED and want["iters"] == sc.MAX_DOUBLINGS
    assert bool((sol.status == sc.NOT_CONVERGED).all()) and bool((sol.iterations == sc.MAX_DOUBLINGS).all()) and bool(torch.isnan(sol.X).all())
    assert np.array_equal(_bits(sol.residual.cpu().numpy()), _bits(np.full(3, want["residual"])))


# ---- the fleet, and one flight -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def flown_fleet():
    """256 rc_planes at 20 m/s, mixed precision, dt 0.01: trimmed, designed, 1000 steps discarded and 3000 accumulated on in-kernel
    draws (Philox row = lane).  Once per session."""
    n, dt = 256, 0.01
    fleet = BatchedSixDOF(n, "mixed", types=("rc_plane",))
    fleet.trim(20.0)
    fleet.design_servo()
    fleet.design_servo_kalman(dt)
    fleet.step_servo_lqg(1000, "estimate")
    for t in (fleet.servo_lqg.err_est, fleet.servo_lqg.err_meas, fleet.servo_lqg.chatter):
        t.zero_()
    fleet.step_servo_lqg(3000, "estimate")
    torch.cuda.synchronize()
    return fleet


def test_fleet_method_equals_the_into_function(flown_fleet):
    fleet = flown_fleet
    for fb in ("estimate", "measurement", "truth"):
        a = fleet.servo_covariance(fb)
        b = SC.servo_covariance_into(fleet._servo.K, fleet._servo_kalman.F, fleet._servo.x0, fleet._servo_kalman.dt, fleet._servo_kalman.sigma, None, fb)
        torch.cuda.synchronize()
        assert bool(a.ok.all()) and a.feedback == b.feedback and a.dt == 0.01
        for x, y in ((a.report, b.report), (a.cov, b.cov), (a.residual, b.residual)):
            assert np.array_equal(_bits(x.cpu().numpy()), _bits(y.cpu().numpy()))
        assert torch.equal(a.iterations, b.iterations)
    # against the restatement on the fleet's own words
    host = lambda t: np.ascontiguousarray(t.cpu().numpy().T)    # noqa: E731
    want = sc.servo_covariance_many(host(fleet._servo.K), host(fleet._servo_kalman.F), host(fleet._servo.x0), 0.01, fleet._servo_kalman.sigma.cpu().numpy(),
                                    RATES, sc.ESTIMATE)
    got = fleet.servo_covariance("estimate", process_rates=RATES)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(got.report.T.cpu().numpy()), _bits(want["report"])) and np.array_equal(_bits(got.cov.T.cpu().numpy()), _bits(want["cov"]))
    room = fleet.servo_covariance("estimate").headroom(fleet._servo.u0)     # 8.6 sigma on the throttle on the CPU (test_servo_cov_oracle.py)
    assert room.shape == (4, fleet.n) and bool((room > 3.0).all())


def test_the_flight_meets_the_devices_own_prediction(flown_fleet):
    fleet = flown_fleet
    pred = fleet.servo_covariance("estimate")
    torch.cuda.synchronize()
    assert bool(pred.ok.all()) and int(fleet.lqr_saturated_steps.sum()) == 0 and fleet.servo_lqg.steps_accumulated == 4000
    want_est, want_chatter = pred.expected_accumulators(3000)
    r_est = (fleet.servo_lqg.err_est.mean(dim=1) / want_est.mean(dim=1)).cpu().numpy()
    r_chatter = (fleet.servo_lqg.chatter.mean(dim=1) / want_chatter.mean(dim=1)).cpu().numpy()
    room = float(pred.headroom(fleet._servo.u0)[L.FD_U_THROTTLE].min())
    print(f"flown / predicted over 256 lanes x 3000 steps: err_est {r_est.min():.3f} .. {r_est.max():.3f}, chatter {r_chatter.min():.3f} .. "
          f"{r_chatter.max():.3f}; throttle headroom {room:.1f} sigma; predicted altitude RMS {float(pred.rms_tracking()[1].max()):.3f} m")
    assert (r_est >= 0.9).all() and (r_est <= 1.1).all(), r_est
    assert (r_chatter >= 0.9).all() and (r_chatter <= 1.1).all(), r_chatter

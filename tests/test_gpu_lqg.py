"""fdyn_kf_design / fdyn_lqg_step_* and hcrl_amd.lqg on the device.

Reference on the box: the NumPy restatement of both (tests/kf_numpy.py) -- the design on the 288 linearisations of
tests/golden/trim_reference.npz, the closed loop over the CPU oracle's RK4 step with the host Philox model's normals -- computed
once per session.

Gates (none derived from what the kernels return):
  design        all 80 words of F, iters and status BIT-IDENTICAL to the restatement (fp64 on both sides, one rounding per
                operation in the same order); residual <= 1e-10
  truth         feedback = truth against fdyn_lqr_step_*: x, surf_out, sat_steps bit for bit, all three precisions
  closed loop   f64, replayed normals, 500 steps, ten aircraft against the restatement over the oracle: 1e-9 on x, xhat, du_prev
                and the accumulators (the gate test_gpu_lqr.py holds the state-feedback loop to); saturated steps equal
  draws         (meas_out - d) / sigma against the host model's normals: 1.0e-5, the bound tests/test_gpu_device_draws.py holds
                the same fast-intrinsic Box-Muller to
  statistics    the three conditions of tests/test_kf_oracle.py, per aircraft, in all three precisions, in-kernel draws
  failed lanes  pass-through filter against feedback = measurement on the same normals, 100 steps: 1e-12.  xhat = pred + (y - pred)
                is y to one rounding (2^-53 * 0.3), times |K| <= 30 is 1e-15 of control per step, summed over 100 steps by a
                loop that contracts: 1e-13, gate ten times that
Measured on MI355X: F 23 040 of 23 040 words equal, residual 4.2e-16, 9 iterations; 500 steps x 8.9e-15, xhat 3.4e-15, du_prev
3.2e-16, accumulators 8.3e-16; draws 2.0e-6; statistics 0.250 / 0.0130 / 0.012..0.235 in f64, mixed and f32; failed lanes 2.8e-17.
"""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, rel_err, STATE_ANGLE_COLS
import kf_numpy as kn
import lqr_numpy as ln
import trim_numpy as tn
from hcrl_amd import _lib, layout as L
from hcrl_amd import lqg as G
from hcrl_amd import lqr as Q
from hcrl_amd.fleet import BatchedSixDOF

pytestmark = pytest.mark.gpu

SENTINEL = -12345.678
ISENT = -1234567
PAD = 96
DEV = "cuda"
DT = kn.DT


def _dev(a, dtype=None):
    t = torch.as_tensor(np.array(a, order="C"), device=DEV)
    return t if dtype is None else t.to(dtype)


def _padded(rows, n, dtype=torch.float64, fill=SENTINEL):
    return torch.full((rows * n + PAD,), fill, dtype=dtype, device=DEV)


def _design(A, B, dt, noise):
    """A [n][12][12], B [n][12][4], noise [16] or [n][16] (host) -> dict of host arrays (F [n][80], residual, iters, status); every
    output buffer has a sentinel pad behind it, asserted untouched."""
    n = len(A)
    A_d, B_d = _dev(np.transpose(A, (1, 2, 0))), _dev(np.transpose(B, (1, 2, 0)))
    nz = np.asarray(noise, np.float64)
    nz_d = _dev(nz if nz.ndim == 1 else nz.T)
    F, res = _padded(L.FD_NKF, n), _padded(1, n)
    it, st = _padded(1, n, torch.int32, ISENT), _padded(1, n, torch.int32, ISENT)
    rc = _lib.load().fdyn_kf_design(_lib.ptr(A_d), _lib.ptr(B_d), float(dt), _lib.ptr(nz_d), int(nz.ndim == 2), n, _lib.ptr(F),
                                    _lib.ptr(res), _lib.ptr(it), _lib.ptr(st), _lib.current_stream())
    _lib.check(rc, "fdyn_kf_design")
    torch.cuda.synchronize()
    for buf, rows, sent in ((F, L.FD_NKF, SENTINEL), (res, 1, SENTINEL), (it, 1, ISENT), (st, 1, ISENT)):
        assert bool((buf[rows * n:] == sent).all()), "wrote behind an output buffer"
    return dict(F=F[:L.FD_NKF * n].reshape(L.FD_NKF, n).T.cpu().numpy(), residual=res[:n].cpu().numpy(), iters=it[:n].cpu().numpy(),
                status=st[:n].cpu().numpy())


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same_design(a, b):
    return np.array_equal(_bits(a["F"]), _bits(b["F"])) and np.array_equal(a["iters"], b["iters"]) and \
        np.array_equal(a["status"], b["status"])


def _take(r, idx):
    return {k: v[idx] for k, v in r.items()}


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "trim_reference.npz"))


@pytest.fixture(scope="module")
def want(golden):
    return kn.design_many(golden["A"], golden["B"], DT, kn.default_noise())


@pytest.fixture(scope="module")
def grid(golden):
    """The 288 linearisations in ONE launch with shared noise."""
    return _design(golden["A"], golden["B"], DT, kn.default_noise())


# ---- design ----------------------------------------------------------------------------------------------------------------------
def test_grid_is_bit_identical_to_the_restatement(grid, want):
    assert len(grid["status"]) == 288 and not grid["status"].any(), np.flatnonzero(grid["status"])
    print(f"residual: worst {grid['residual'].max():.3e}; iterations {grid['iters'].min()}..{grid['iters'].max()}; "
          f"F words equal to the restatement's: {int((_bits(grid['F']) == _bits(want['F'])).sum())} of {grid['F'].size}")
    assert grid["residual"].max() <= 1e-10
    assert _same_design(grid, want)
    assert np.array_equal(_bits(grid["residual"]), _bits(want["residual"]))


def test_a_second_step_size_is_bit_identical_too(golden):
    idx = np.arange(0, 288, 9)
    got = _design(golden["A"][idx], golden["B"][idx], 0.02, kn.default_noise())
    assert _same_design(got, kn.design_many(golden["A"][idx], golden["B"][idx], 0.02, kn.default_noise())) and not got["status"].any()


@pytest.mark.parametrize("n", [1, 63, 65, 257])
def test_shapes_and_lane_position(n, grid, golden):
    idx = (np.arange(n) * 7 + 3) % 288
    got = _design(golden["A"][idx], golden["B"][idx], DT, kn.default_noise())
    assert _same_design(got, _take(grid, idx)), "a lane's result depends on where it sits in the launch"


def test_shared_noise_equals_the_same_noise_per_lane(grid, golden):
    per_lane = _design(golden["A"], golden["B"], DT, np.tile(kn.default_noise(), (288, 1)))
    assert _same_design(per_lane, grid)


def test_bad_lanes_and_their_neighbours(grid, golden):
    keep = np.arange(0, 288, 6)                                          # 48 good aircraft, both airframes
    nz0 = kn.default_noise()
    A, B, N, kind = [], [], [], []
    for j, i in enumerate(keep):
        A.append(golden["A"][i]); B.append(golden["B"][i]); N.append(nz0); kind.append(0)
        if j % 3 == 2:
            a, b, nz = golden["A"][i].copy(), golden["B"][i].copy(), nz0.copy()
            k = 1 + (j // 3) % 4
            if k == 1:                                                   # a NaN word in a block of A
                a[L.FD_X_V, L.FD_X_R] = np.nan
            elif k == 2:                                                 # a bad sigma or rate
                nz[(3 * j) % 16] = (0.0, -2.0, np.nan, np.inf)[(j // 12) % 4]
            elif k == 3:                                                 # |a|_inf dt = 1.6 > 1.5
                a[L.FD_X_U, L.FD_X_W] = 160.0
            else:                                                        # an infinite word of B
                b[L.FD_X_Q, L.FD_U_ELEVATOR] = -np.inf
            A.append(a); B.append(b); N.append(nz); kind.append(k)
    A, B, N, kind = np.array(A), np.array(B), np.array(N), np.array(kind)
    assert all((kind == k).sum() >= 3 for k in (1, 2, 3, 4))
    mixed = _design(A, B, DT, N)
    assert _same_design(_take(mixed, kind == 0), _take(grid, keep)), "a good lane changed because of its neighbour"
    bad = _take(mixed, kind != 0)
    assert (bad["status"] == L.FD_KF_BAD_INPUT).all() and np.isnan(bad["residual"]).all() and not bad["iters"].any()
    assert all(np.array_equal(_bits(row), _bits(kn.pass_through())) for row in bad["F"]), "a bad lane is not the pass-through"
    assert _same_design(bad, kn.design_many(A[kind != 0], B[kind != 0], DT, N[kind != 0]))


# ---- the closed loop -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def flights():
    return kn.oracle_flights()


def _setup(f, precision="f64", idx=None, x=None, seed=0, F=None):
    """A fleet of the reference's aircraft (rows idx of the ten) at `x` (default: the trim), designs holding the REFERENCE's
    gains, trim points and filters, and a fresh loop state: the step kernels are compared on identical inputs."""
    base, rows = f["base"], f["rows"]
    idx = np.arange(len(rows)) if idx is None else np.asarray(idx)
    n = len(idx)
    fleet = BatchedSixDOF(n, precision, types=tn.TYPES, type_index=base["type"][idx])
    fleet.reset(base["x0"][idx] if x is None else x)
    zi = lambda: torch.zeros(n, dtype=torch.int32, device=DEV)
    zd = lambda: torch.zeros(n, dtype=torch.float64, device=DEV)
    lqr = Q.LqrDesign(_dev(base["K"][idx].T), zd(), zi(), zi(), _dev(base["x0"][idx].T), _dev(base["u0"][idx].T))
    Fh = np.array([rows[i]["F"] for i in idx]) if F is None else F
    kal = G.KalmanDesign(_dev(Fh.T), zd(), zi(), zi(), DT, _dev(np.array(kn.DEFAULT_SIGMA)))
    return fleet, lqr, kal, G.LqgState.zeros(n, DEV, seed)


def _step(fleet, lqr, kal, state, n_steps, feedback="estimate", z=None, surf=None, sat=None):
    G.step_into(fleet.precision, fleet.x, lqr, kal, state, fleet.params, fleet.type_index, DT, n_steps, feedback, z,
                fleet.u if surf is None else surf, sat)


@pytest.mark.parametrize("precision", ["f64", "mixed", "f32"])
def test_truth_feedback_is_the_lqr_step_to_the_bit(flights, precision):
    base = flights["base"]
    n = 257
    idx = np.arange(n) % 10
    fa, lqr, kal, state = _setup(flights, precision, idx, base["x_start"][idx])
    fb, _, _, _ = _setup(flights, precision, idx, base["x_start"][idx])
    sat_a, sat_b = (_padded(1, n, torch.int32, 0) for _ in range(2))
    dt_ = fa.x.dtype
    surf_a, surf_b = _padded(L.FD_NU, n, dt_), _padded(L.FD_NU, n, dt_)
    _step(fa, lqr, kal, state, 100, "truth", None, surf_a, sat_a)
    Q.step_into(precision, fb.x, lqr, fb.params, fb.type_index, DT, 100, surf_b, sat_b)
    torch.cuda.synchronize()
    assert torch.equal(fa.x, fb.x) and torch.equal(surf_a, surf_b) and torch.equal(sat_a, sat_b)
    assert bool(sat_a[:n].any()) and bool((surf_a[L.FD_NU * n:] == SENTINEL).all()) and int(state.step) == 100
    assert bool(state.xhat.any()) and bool(state.err_meas.any())          # the estimator ran beside it


def _close(got, ref, what, tol=1e-9):
    err = np.abs(np.asarray(got) - ref) / np.maximum(1.0, np.abs(ref))
    print(f"  {what}: worst |device - NumPy| / max(1, |NumPy|) = {err.max():.3e}")
    assert err.max() <= tol, (what, err.max())


def test_five_hundred_steps_against_the_numpy_loop(flights):
    rows = flights["rows"]
    n = len(rows)
    fleet, lqr, kal, state = _setup(flights)
    z = _dev(np.array([r["z"][:kn.STEPS_COMPARE] for r in rows]).transpose(1, 2, 0))          # [500][8][n]
    sat = torch.zeros(n, dtype=torch.int32, device=DEV)
    _step(fleet, lqr, kal, state, kn.STEPS_COMPARE, "estimate", z, None, sat)
    torch.cuda.synchronize()
    ref = {k: np.array([r["est_500"][k] for r in rows]) for k in ("x", "xhat", "du_prev", "u", "err_est", "err_meas", "chatter", "y")}
    err = rel_err(fleet.state_numpy(), ref["x"], STATE_ANGLE_COLS)
    print(f"500 LQG steps, 10 aircraft: worst |device - NumPy over the oracle| = {err.max():.3e}")
    assert err.max() <= 1e-9
    for name, got in (("xhat", state.xhat), ("du_prev", state.du_prev), ("u", fleet.u), ("err_est", state.err_est),
                      ("err_meas", state.err_meas), ("chatter", state.chatter), ("y", state.meas)):
        _close(got.T.cpu().numpy(), ref[name], name)
    assert np.array_equal(sat.cpu().numpy(), np.array([r["est_500"]["sat"] for r in rows]))


def test_controls_only_and_two_launches_equal_one(flights):
    base = flights["base"]
    n = len(flights["rows"])
    one, lqr, kal, s1 = _setup(flights, seed=5)
    two, _, _, s2 = _setup(flights, seed=5)
    _step(one, lqr, kal, s1, 100)
    _step(two, lqr, kal, s2, 50)
    _step(two, lqr, kal, s2, 50)
    torch.cuda.synchronize()
    for a, b in ((one.x, two.x), (one.u, two.u), (s1.xhat, s2.xhat), (s1.du_prev, s2.du_prev), (s1.err_est, s2.err_est),
                 (s1.err_meas, s2.err_meas), (s1.chatter, s2.chatter), (s1.meas, s2.meas), (s1.step, s2.step)):
        assert torch.equal(a, b)
    assert int(s1.step) == 100 and bool(s1.xhat.any())
    # n_steps = 0: the controls from the stored estimate, nothing else touched
    before = [t.clone() for t in (one.x, s1.xhat, s1.du_prev, s1.err_est, s1.err_meas, s1.chatter, s1.meas, s1.step)]
    surf = _padded(L.FD_NU, n)
    _step(one, lqr, kal, s1, 0, "estimate", None, surf)
    torch.cuda.synchronize()
    for a, b in zip(before, (one.x, s1.xhat, s1.du_prev, s1.err_est, s1.err_meas, s1.chatter, s1.meas, s1.step)):
        assert torch.equal(a, b)
    xh = s1.xhat.T.cpu().numpy()
    ref = np.array([ln.clip_controls(kn.controls_from(base["K"][i], base["u0"][i], xh[i]))[0] for i in range(n)])
    assert np.array_equal(surf[:L.FD_NU * n].reshape(L.FD_NU, n).T.cpu().numpy(), ref) and bool((surf[L.FD_NU * n:] == SENTINEL).all())
    _step(one, lqr, kal, s1, 0, "truth", None, surf)
    ref = np.array([ln.clip_controls(ln.controls(base["K"][i], base["x0"][i], base["u0"][i], one.state_numpy()[i]))[0] for i in range(n)])
    assert np.abs(surf[:L.FD_NU * n].reshape(L.FD_NU, n).T.cpu().numpy() - ref).max() <= 1e-15


@pytest.mark.parametrize("seed", [12345, (7 << 32) + 99])
def test_in_kernel_draws_match_the_host_model(flights, seed):
    """One step on a constant state (every lane at aircraft 0's trim, so d = 0 and y = sigma z): the normals come back."""
    n = 1000
    sigma = np.array(kn.DEFAULT_SIGMA)
    got = {}
    for step0 in (0, 1, 41):
        fleet, lqr, kal, state = _setup(flights, "f64", np.zeros(n, np.int64), seed=seed)
        state.step.fill_(step0)
        _step(fleet, lqr, kal, state, 1)
        torch.cuda.synchronize()
        got[step0] = state.meas.T.cpu().numpy() / sigma
        want_z = kn.lqg_normals(seed, np.arange(n), step0 + 1)
        err = np.abs(got[step0] - want_z).max()
        print(f"seed {seed:#x}, step word {step0}: worst |device normal - model| = {err:.3e}, extremes {want_z.min():.2f} .. {want_z.max():.2f}")
        assert err <= 1.0e-5
        assert int(state.step) == step0 + 1
    assert not np.array_equal(got[0], got[1]) and not np.array_equal(got[1], got[41])


@pytest.mark.parametrize("precision", ["f64", "mixed", "f32"])
def test_statistics_hold_on_the_device(flights, precision):
    """The three conditions of tests/test_kf_oracle.py per aircraft with in-kernel draws: 1000 steps from trim under the estimate
    and under the measurement; the true rates are read after each of the last 500 steps."""
    words = [ln.DELTA_STATES[k] for k in kn.RATE_WORDS]
    out = {}
    for fb in ("estimate", "measurement"):
        fleet, lqr, kal, state = _setup(flights, precision, seed=kn.SEED)
        _step(fleet, lqr, kal, state, kn.STEPS // 2, fb)
        ms = torch.zeros((3, fleet.n), dtype=torch.float64, device=DEV)
        x0 = lqr.x0[words]
        for _ in range(kn.STEPS // 2):
            _step(fleet, lqr, kal, state, 1, fb)
            ms += (fleet.x[words].to(torch.float64) - x0) ** 2
        out[fb] = dict(err_est=state.err_est.cpu().numpy(), err_meas=state.err_meas.cpu().numpy(), chatter=state.chatter.cpu().numpy(),
                       rate=(ms / (kn.STEPS // 2)).cpu().numpy())
        assert int(state.step) == kn.STEPS
    e, m = out["estimate"], out["measurement"]
    err, chat, rate = e["err_est"] / e["err_meas"], e["chatter"] / m["chatter"], e["rate"] / m["rate"]
    print(f"{precision}: err_est / err_meas up to {err.max():.3f}, chatter ratio up to {chat.max():.4f}, true-rate ratio {rate.min():.3f}..{rate.max():.3f}")
    assert (e["err_est"] < 0.5 * e["err_meas"]).all(), err
    assert (e["chatter"] < 0.5 * m["chatter"]).all(), chat
    assert (e["rate"] < m["rate"]).all(), rate


def test_failed_design_lanes_fly_on_the_measurement(flights):
    rows = flights["rows"]
    n = len(rows)
    z = _dev(np.array([r["z"][:100] for r in rows]).transpose(1, 2, 0))
    F = np.array([r["F"] for r in rows])
    F[::2] = kn.pass_through()                                            # every other lane's design "failed"
    a, lqr, kal, sa = _setup(flights, F=F)
    b, _, kal_b, sb = _setup(flights)
    _step(a, lqr, kal, sa, 100, "estimate", z)
    _step(b, lqr, kal_b, sb, 100, "measurement", z)
    torch.cuda.synchronize()
    err = rel_err(a.state_numpy(), b.state_numpy(), STATE_ANGLE_COLS)
    print(f"pass-through lanes against feedback = measurement: {err[::2].max():.3e}; filtered lanes differ by {err[1::2].max():.3e}")
    assert err[::2].max() <= 1e-12
    assert err[1::2].max() > 1e-6                                         # the other lanes do filter
    assert float((sa.xhat[:, ::2] - sa.meas[:, ::2]).abs().max()) <= 1e-15


def test_fleet_methods(flights):
    """BatchedSixDOF.trim -> design_lqr -> design_kalman -> step_lqg against the same designs through lqg.step_into; the guards."""
    base = flights["base"]
    n = len(base["type"])
    fleet = BatchedSixDOF(n, "f64", types=tn.TYPES, type_index=base["type"])
    with pytest.raises(ValueError, match="has no trim"):
        fleet.design_kalman(DT)
    fleet.trim(base["spec"][:, 0], base["spec"][:, 1], base["spec"][:, 2], ln.ALTITUDE, ln.HEADING)
    with pytest.raises(ValueError, match="no certified stabilising gain"):
        fleet.step_lqg(1)
    lqr = fleet.design_lqr()
    with pytest.raises(ValueError, match="no certified stable filter"):
        fleet.step_lqg(1)
    kal = fleet.design_kalman(DT)
    assert bool(kal.ok.all()) and kal.count_not_ok() == 0 and kal.dt == DT and tuple(kal.sigma.cpu().numpy()) == kn.DEFAULT_SIGMA
    # A and B come from central differences of two implementations of the dynamics: the linearisation's own gate of 1e-6
    err = np.abs(kal.F.T.cpu().numpy() - np.array([r["F"] for r in flights["rows"]]))
    print(f"fleet filter against the oracle's: worst |F - F_ref| = {err.max():.3e}")
    assert err.max() <= 1e-6
    radius = max(np.abs(np.linalg.eigvals(m)).max() for m in kal.filter_matrix().permute(0, 3, 1, 2).reshape(-1, 4, 4).cpu().numpy())
    print(f"spectral radius of Phi (I - L): {radius:.3f}")
    assert radius < 1.0
    with pytest.raises(ValueError, match=rf"{n} of {n} aircraft.*invalid model, noise or dt"):
        fleet.design_kalman(DT, noise=G.KalmanNoise(sigma=(0.0,) * 8))
    bad = fleet.design_kalman(DT, noise=G.KalmanNoise(sigma=(0.0,) * 8), strict=False)
    assert bool((bad.status == L.FD_KF_BAD_INPUT).all()) and np.array_equal(bad.F[:, 0].cpu().numpy(), kn.pass_through())
    fleet.design_kalman(DT)
    fleet.lqg.seed = 3
    twin = BatchedSixDOF(n, "f64", types=tn.TYPES, type_index=base["type"])
    twin.reset(fleet.state_numpy())
    state = G.LqgState.zeros(n, DEV, 3)
    fleet.step_lqg(20)
    G.step_into("f64", twin.x, lqr, fleet._kalman, state, twin.params, twin.type_index, DT, 20, "estimate", None, twin.u)
    assert torch.equal(fleet.x, twin.x) and torch.equal(fleet.lqg.xhat, state.xhat) and fleet.time == pytest.approx(20 * DT)
    fleet.lqg.reset()
    assert not bool(fleet.lqg.xhat.any()) and int(fleet.lqg.step) == 0 and not bool(fleet.lqg.chatter.any())


def test_graph_replay_equals_eager(golden, flights):
    A, B = _dev(np.transpose(golden["A"], (1, 2, 0))), _dev(np.transpose(golden["B"], (1, 2, 0)))
    nz = _dev(kn.default_noise())
    eager = G.kalman_into(A, B, DT, nz)
    fe, lqr, kal, se = _setup(flights, seed=11)
    fg, _, _, sg = _setup(flights, seed=11)
    _step(fe, lqr, kal, se, 50)
    out = G.KalmanDesign(torch.zeros_like(eager.F), torch.zeros_like(eager.residual), torch.zeros_like(eager.iters), torch.zeros_like(eager.status))
    scratch, _, _, ss = _setup(flights, seed=11)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                                 # warm-up outside the capture, on copies
        G.kalman_into(A, B, DT, nz, out)
        _step(scratch, lqr, kal, ss, 50)
    torch.cuda.current_stream().wait_stream(s)
    for t in (out.F, out.residual, out.iters, out.status):
        t.zero_()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        G.kalman_into(A, B, DT, nz, out)
        _step(fg, lqr, kal, sg, 50)
    gr.replay()
    torch.cuda.synchronize()
    for a, b in ((eager.F, out.F), (eager.residual, out.residual), (eager.iters, out.iters), (eager.status, out.status),
                 (fe.x, fg.x), (fe.u, fg.u), (se.xhat, sg.xhat), (se.du_prev, sg.du_prev), (se.err_est, sg.err_est), (se.chatter, sg.chatter),
                 (se.meas, sg.meas), (se.step, sg.step)):
        assert torch.equal(a, b)

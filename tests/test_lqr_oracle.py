"""Gain-scheduled LQR, CPU side: the NumPy restatement of fdyn_lqr_design / fdyn_lqr_step (tests/lqr_numpy.py) against
scipy's Riccati solver on the 288 linearisations of tests/golden/trim_reference.npz, flown over the CPU oracle, and the host
logic of hcrl_amd.lqr that needs no device.

Gates (none derived from what the code under test returns):
  K           1e-9 max|K| against scipy.linalg.solve_continuous_are: two fp64 solvers of one equation agree in X to a few 1e-14
              (measured 2.1e-14); the margin covers the conditioning of R^-1 b^T
  residual    <= 1e-10 (measured 3.3e-14), iterations <= 12 (measured 8..10), status 0 on every aircraft
  poles       every block's closed loop <= -0.3 1/s (measured -0.61); the coupled 8-state A - B K Hurwitz on all 288
  recovery    deviation from trim <= 1e-4 after 20 s from the perturbation (measured 1.7e-6); controls held at u0 >= 0.1 away
              (measured >= 0.59)
"""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import lqr_numpy as ln
import trim_numpy as tn
from hcrl_amd import layout as L
from hcrl_amd import lqr as Q
from hcrl_amd import trim as T


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "trim_reference.npz"))


@pytest.fixture(scope="module")
def designed(golden):
    return ln.design_many(golden["A"], golden["B"], ln.default_weights())


def test_constants_mirror_the_header():
    assert (ln.NOT_CONVERGED, ln.NO_CERTIFICATE, ln.BAD_INPUT) == (L.FD_LQR_NOT_CONVERGED, L.FD_LQR_NO_CERTIFICATE, L.FD_LQR_BAD_INPUT) == (1, 2, 4)
    assert (ln.NLQW, ln.NLQK) == (L.FD_NLQW, L.FD_NLQK) == (12, 16)
    assert (L.FD_LQW_Q_LON, L.FD_LQW_Q_LAT, L.FD_LQW_R_LON, L.FD_LQW_R_LAT, L.FD_LQK_LON, L.FD_LQK_LAT) == (0, 4, 8, 10, 0, 8)
    assert ln.LON_STATES == T.LONGITUDINAL_STATES and ln.LON_CONTROLS == T.LONGITUDINAL_CONTROLS
    assert ln.LAT_STATES == T.LATERAL_STATES and ln.LAT_CONTROLS == T.LATERAL_CONTROLS


def test_restatement_matches_scipy_on_the_golden_grid(golden, designed):
    sl = pytest.importorskip("scipy.linalg")
    w = ln.default_weights()
    assert len(designed["status"]) == 288 and not designed["status"].any()
    print(f"residual: worst {designed['residual'].max():.3e}; iterations {designed['iters'].min()}..{designed['iters'].max()}")
    assert designed["residual"].max() <= 1e-10 and designed["iters"].max() <= 12
    worst = 0.0
    for i in range(288):
        for k, (a, b) in enumerate(ln.blocks(golden["A"][i], golden["B"][i])):
            q, r = w[4 * k:4 * k + 4], w[8 + 2 * k:10 + 2 * k]
            X = sl.solve_continuous_are(a, b, np.diag(q), np.diag(r))
            want = (b.T @ X) / r[:, None]
            got = designed["K"][i][8 * k:8 * k + 8].reshape(2, 4)
            err = np.abs(got - want).max() / np.abs(want).max()
            worst = max(worst, err)
            assert err <= 1e-9, (i, k, err)
    print(f"K against scipy: worst relative deviation {worst:.3e}")


def test_every_closed_loop_is_stable(golden, designed):
    worst_block, worst_open, worst_full = -np.inf, -np.inf, -np.inf
    idx = list(ln.DELTA_STATES)
    for i in range(288):
        for k, (a, b) in enumerate(ln.blocks(golden["A"][i], golden["B"][i])):
            Kb = designed["K"][i][8 * k:8 * k + 8].reshape(2, 4)
            worst_block = max(worst_block, np.linalg.eigvals(a - b @ Kb).real.max())
            worst_open = max(worst_open, np.linalg.eigvals(a).real.max())
        full = (golden["A"][i] - golden["B"][i] @ ln.gain_matrix(designed["K"][i]))[np.ix_(idx, idx)]
        worst_full = max(worst_full, np.linalg.eigvals(full).real.max())
    print(f"worst pole real part: blocks {worst_block:.3f}, coupled 8-state {worst_full:.3f}, open loop {worst_open:.3f}")
    assert worst_block <= -0.3
    assert worst_full < 0.0
    assert worst_open > 0.0                                  # there is something to stabilise (the slow phugoid)


def test_nonlinear_recovery_over_the_oracle():
    f = ln.oracle_flights()["listed"]
    assert len(f["dev"]) == 5 and not f["status"].any()
    for k, (name, V, g, w) in enumerate(ln.CONDITIONS):
        print(f"{name} V={V} climb={g} turn={w}: deviation at 5/10/20 s {f['dev'][k][0]:.2e} {f['dev'][k][1]:.2e} {f['dev'][k][2]:.2e}, "
              f"saturated steps {f['sat'][k]}, controls held at u0: {f['open_dev'][k]:.2f}")
    assert f["dev"][:, 2].max() <= 1e-4
    assert f["open_dev"].min() >= 0.1
    assert f["sat"].max() > 0                                # the clip is exercised


# ---- degenerate inputs -----------------------------------------------------------------------------------------------------------
STABLE = -np.eye(4) + 0.1 * np.triu(np.ones((4, 4)), 1)


def test_unstabilisable_block_is_not_converged():
    r = ln.design_block(0.5 * np.eye(4), np.zeros((4, 2)), np.ones(4), np.ones(2))
    assert r["status"] & ln.NOT_CONVERGED and r["iters"] <= ln.MAX_ITERS


def test_stable_block_without_authority_gives_zero_gain():
    r = ln.design_block(STABLE, np.zeros((4, 2)), np.ones(4), np.ones(2))
    assert r["status"] == 0 and not r["K"].any() and r["residual"] <= 1e-10


def test_bad_inputs(golden):
    A, B, w = golden["A"][0], golden["B"][0], ln.default_weights()
    assert ln.design(A, B, w)["status"] == 0
    An = A.copy(); An[L.FD_X_W, L.FD_X_Q] = np.nan
    Bn = B.copy(); Bn[L.FD_X_P, L.FD_U_AILERON] = np.inf
    for a, b, ww in ((An, B, w), (A, Bn, w)) + tuple((A, B, np.where(np.arange(12) == k, v, w)) for k in (0, 5, 9, 11)
                                                      for v in (0.0, -1.0, np.nan, np.inf)):
        r = ln.design(a, b, ww)
        assert r["status"] == ln.BAD_INPUT and np.isnan(r["residual"]) and not r["K"].any() and r["iters"] == 0


def test_one_dead_control_still_solves(golden):
    w = ln.default_weights()
    for i in (0, 150, 287):
        for col in (L.FD_U_THROTTLE, L.FD_U_ELEVATOR):
            B = golden["B"][i].copy()
            B[:, col] = 0.0
            r = ln.design(golden["A"][i], B, w)
            print(f"aircraft {i}, control {col} dead: status {r['status']}, iterations {r['iters']}, residual {r['residual']:.2e}")
            assert r["status"] == 0 and r["residual"] <= 1e-10             # status 0: converged inside the cap
            dead = {L.FD_U_ELEVATOR: slice(0, 4), L.FD_U_THROTTLE: slice(4, 8)}[col]
            assert not r["K"][dead].any() and r["K"][8:].any()


def test_inverse_matches_numpy_and_flags_singular():
    rs = np.random.RandomState(3)
    a = rs.normal(size=(4, 4))
    x, ok = ln.inv4(a)
    assert ok and np.abs(x - np.linalg.inv(a)).max() < 1e-12
    a[:, 2] = 0.0
    assert not ln.inv4(a)[1]
    a[:, 2] = np.nan
    assert not ln.inv4(a)[1]
    assert ln.ldl_positive(np.eye(4) + 0.1) and not ln.ldl_positive(np.diag([1.0, 1.0, -1e-3, 1.0])) and not ln.ldl_positive(np.full((4, 4), np.nan))


def test_closed_loop_pieces():
    x0 = np.arange(12.0) * 0.1
    x = x0.copy()
    x[L.FD_X_ROLL] += 2 * np.pi + 0.01                       # a whole turn away is 0.01 away
    d = ln.delta(x, x0)
    assert abs(d[7] - 0.01) < 1e-12 and np.abs(np.delete(d, 7)).max() == 0.0
    K = np.zeros(16); K[8 + 3] = 2.0                         # aileron <- phi
    u = ln.controls(K, x0, np.array([0.1, 0.2, 0.3, 0.4]), x)
    assert np.allclose(u, [0.1, 0.2 - 0.02, 0.3, 0.4], atol=1e-12)
    c, clipped = ln.clip_controls(np.array([1.5, -0.2, -3.0, -0.1]))
    assert c.tolist() == [1.0, -0.2, -1.0, 0.0] and clipped and not ln.clip_controls(c)[1]


# ---- hcrl_amd.lqr without a device -----------------------------------------------------------------------------------------------
def test_weights_vector_and_rows():
    w = Q.LqrWeights()
    assert np.array_equal(w.vector(), ln.default_weights()) and not w.per_lane
    assert w.vector()[L.FD_LQW_Q_LON + 3] == pytest.approx(100.0) and w.vector()[L.FD_LQW_R_LAT] == pytest.approx(1 / 0.09)
    sweep = Q.LqrWeights(theta=[0.1, 0.2, 0.05], rudder=0.5)
    assert sweep.per_lane
    rows = sweep.rows(3)
    assert rows.shape == (L.FD_NLQW, 3) and rows.dtype == np.float64
    assert np.allclose(rows[3], [100.0, 25.0, 400.0]) and np.allclose(rows[11], [4.0] * 3) and np.array_equal(rows[0], [0.25] * 3)
    with pytest.raises(ValueError):
        sweep.rows(4)
    cpu = torch.device("cpu")
    assert tuple(Q.weights_tensor(None, 3, cpu).shape) == (12,) and tuple(Q.weights_tensor(sweep, 3, cpu).shape) == (12, 3)
    assert Q.weights_tensor(np.ones(12), 3, cpu).dtype == torch.float64
    with pytest.raises(ValueError):
        Q.weights_tensor(np.ones(11), 3, cpu)


def _design(status, n=None):
    n = len(status)
    K = torch.arange(16.0 * n, dtype=torch.float64).reshape(16, n)
    return Q.LqrDesign(K, torch.zeros(n, dtype=torch.float64), torch.full((n,), 9, dtype=torch.int32),
                       torch.tensor(status, dtype=torch.int32))


def test_gain_matrix_placement_and_closed_loop():
    d = _design([0, 0, 0])
    K = d.gain_matrix()
    assert tuple(K.shape) == (4, 12, 3)
    for lane in range(3):
        assert np.array_equal(K[:, :, lane].numpy(), ln.gain_matrix(d.K[:, lane].numpy()))
    assert torch.equal(K[L.FD_U_THROTTLE, L.FD_X_Q], d.K[4 + 2]) and torch.equal(K[L.FD_U_RUDDER, L.FD_X_ROLL], d.K[8 + 4 + 3])
    assert not K[:, [L.FD_X_N, L.FD_X_E, L.FD_X_D, L.FD_X_YAW]].any() and not K[L.FD_U_ELEVATOR, L.FD_X_V].any()
    rs = np.random.RandomState(0)
    A, B = torch.as_tensor(rs.normal(size=(12, 12, 3))), torch.as_tensor(rs.normal(size=(12, 4, 3)))
    cl = d.closed_loop(A, B)
    for lane in range(3):
        assert np.allclose(cl[:, :, lane].numpy(), A[:, :, lane].numpy() - B[:, :, lane].numpy() @ K[:, :, lane].numpy(), atol=1e-12)


def test_status_decoding_and_the_strict_error():
    d = _design([0, 3, 0, 4, 2])
    assert d.n == 5 and d.ok.tolist() == [True, False, True, False, False] and d.count_not_ok() == 3
    assert Q.describe_status(0) == "ok" and Q.describe_status(3) == "not converged, no stability certificate"
    assert Q.describe_status(4) == "invalid model or weights"
    Q.require_ok(_design([0, 0]))
    with pytest.raises(ValueError, match=r"3 of 5 aircraft.*first: aircraft 1: not converged, no stability certificate"):
        Q.require_ok(d, "BatchedSixDOF.design_lqr")


def test_design_lqr_needs_a_trim():
    from hcrl_amd.fleet import BatchedSixDOF
    fleet = BatchedSixDOF.__new__(BatchedSixDOF)             # no device: only the guard is exercised
    with pytest.raises(ValueError, match="has no trim"):
        fleet.design_lqr()


def test_lqr_into_refuses_wrong_shapes():
    A, B = torch.zeros((12, 12, 2), dtype=torch.float64), torch.zeros((12, 4, 2), dtype=torch.float64)
    with pytest.raises(ValueError):
        Q.lqr_into(A, B[:, :3], torch.ones(12, dtype=torch.float64))
    with pytest.raises(ValueError):
        Q.lqr_into(A, B, torch.ones((12, 3), dtype=torch.float64))
    with pytest.raises(ValueError):
        Q.lqr_into(A.float(), B, torch.ones(12, dtype=torch.float64))

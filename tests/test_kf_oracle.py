"""The steady-state Kalman filter and the LQG loop, CPU side: the NumPy restatement of fdyn_kf_design / fdyn_lqg_step
(tests/kf_numpy.py) against scipy on the 288 linearisations of tests/golden/trim_reference.npz (both blocks, dt = 0.01 and 0.02),
flown over the CPU oracle with the Philox normals, and the host logic of hcrl_amd.lqg that needs no device.

Gates (none derived from what the code under test returns):
  Phi      1e-12 absolute against scipy.linalg.expm (measured 1.9e-15)
  Gamma    1e-12 absolute against expm of the augmented matrix [[a, b], [0, 0]] dt (measured 1.4e-14)
  P        1e-9 max|P| against scipy.linalg.solve_discrete_are, the LQR test's own gate (measured 3.1e-14)
  L        1e-9 max|L| against P (P + V)^-1 from scipy's P (measured 1.7e-13)
  status 0 on all 576 designs, relative residual <= 1e-10 (measured 5.8e-16), iterations <= 12 (measured 9 on every aircraft),
  |a|_inf dt below the 1.5 cap (measured 0.67 at dt = 0.01, 1.35 at dt = 0.02)
  poles    spectral radius of Phi (I - L) < 1 on all 576 x 2 blocks (measured 0.951 at dt = 0.01, 0.931 at dt = 0.02: filter poles near -5 1/s)
  closed loop, ten aircraft (lqr_numpy.CONDITIONS on both airframes) from trim, 1000 steps of 0.01 s, Philox normals of
  kf_numpy.SEED: err_est < 0.5 err_meas per word (measured ratios 0.016..0.250), chatter under the estimate < 0.5 of that
  under the measurement per control (measured 0.0014..0.0130), mean square of the true p, q, r over the last 500 steps lower
  under the estimate (measured ratios 0.012..0.235)
"""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import kf_numpy as kn
import lqr_numpy as ln
import philox_numpy as pn
from hcrl_amd import layout as L
from hcrl_amd import lqg as G

DTS = (0.01, 0.02)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "trim_reference.npz"))


@pytest.fixture(scope="module")
def designed(golden):
    return {dt: kn.design_many(golden["A"], golden["B"], dt, kn.default_noise()) for dt in DTS}


def test_constants_mirror_the_header():
    assert (kn.NOT_CONVERGED, kn.NO_CERTIFICATE, kn.BAD_INPUT) == (L.FD_KF_NOT_CONVERGED, L.FD_KF_NO_CERTIFICATE, L.FD_KF_BAD_INPUT) == (1, 2, 4)
    assert (kn.NKF, kn.NKFN, kn.W_LQG) == (L.FD_NKF, L.FD_NKFN, L.FD_PHX_LQG) == (80, 16, 0x70)
    assert (kn.PHI_LON, kn.PHI_LAT, kn.GAMMA_LON, kn.GAMMA_LAT, kn.L_LON, kn.L_LAT) == \
        (L.FD_KF_PHI_LON, L.FD_KF_PHI_LAT, L.FD_KF_GAMMA_LON, L.FD_KF_GAMMA_LAT, L.FD_KF_L_LON, L.FD_KF_L_LAT)
    assert (kn.ESTIMATE, kn.MEASUREMENT, kn.TRUTH) == (L.FD_LQG_ESTIMATE, L.FD_LQG_MEASUREMENT, L.FD_LQG_TRUTH)
    assert (L.FD_KFN_SIGMA, L.FD_KFN_RATE) == (0, 8)
    assert np.array_equal(G.KalmanNoise().vector(), kn.default_noise()) and tuple(G.sensor_sigma()) == kn.DEFAULT_SIGMA
    assert G.DEFAULT_RATES == kn.DEFAULT_RATES


@pytest.mark.parametrize("dt", DTS)
def test_restatement_matches_scipy_on_the_golden_grid(golden, designed, dt):
    sl = pytest.importorskip("scipy.linalg")
    d, nz = designed[dt], kn.default_noise()
    assert len(d["status"]) == 288 and not d["status"].any(), np.flatnonzero(d["status"])
    norm = max(kn.row_norm(a) for i in range(288) for a, _ in ln.blocks(golden["A"][i], golden["B"][i])) * dt
    print(f"dt {dt}: residual worst {d['residual'].max():.3e}; iterations {d['iters'].min()}..{d['iters'].max()}; |a|_inf dt {norm:.3f}")
    assert d["residual"].max() <= 1e-10 and d["iters"].max() <= 12 and norm <= kn.NORM_MAX
    worst = dict(Phi=0.0, Gamma=0.0, P=0.0, L=0.0, radius=0.0)
    for i in range(288):
        for k, ((a, b), (Phi, Gamma, Lg)) in enumerate(zip(ln.blocks(golden["A"][i], golden["B"][i]), kn.matrices(d["F"][i]))):
            aug = np.zeros((6, 6))
            aug[:4, :4], aug[:4, 4:] = a * dt, b * dt
            E = sl.expm(aug)
            worst["Phi"] = max(worst["Phi"], np.abs(Phi - sl.expm(a * dt)).max())
            worst["Gamma"] = max(worst["Gamma"], np.abs(Gamma - E[:4, 4:]).max())
            V, W = np.diag(nz[4 * k:4 * k + 4] ** 2), np.diag(nz[8 + 4 * k:12 + 4 * k] ** 2 * dt)
            P_ref = sl.solve_discrete_are(Phi.T, np.eye(4), W, V)
            L_ref = P_ref @ np.linalg.inv(P_ref + V)
            P = kn.design_block(a, b, dt, nz[4 * k:4 * k + 4], nz[8 + 4 * k:12 + 4 * k])["P"]
            worst["P"] = max(worst["P"], np.abs(P - P_ref).max() / np.abs(P_ref).max())
            worst["L"] = max(worst["L"], np.abs(Lg - L_ref).max() / np.abs(L_ref).max())
            worst["radius"] = max(worst["radius"], np.abs(np.linalg.eigvals(Phi @ (np.eye(4) - Lg))).max())
    print(f"dt {dt}: against scipy: " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    assert worst["Phi"] <= 1e-12 and worst["Gamma"] <= 1e-12
    assert worst["P"] <= 1e-9 and worst["L"] <= 1e-9
    assert worst["radius"] < 1.0


def test_bad_inputs_give_status_4_and_the_pass_through(golden):
    A, B, nz = golden["A"][0], golden["B"][0], kn.default_noise()
    assert kn.design(A, B, 0.01, nz)["status"] == 0
    An = A.copy(); An[L.FD_X_W, L.FD_X_Q] = np.nan
    Bn = B.copy(); Bn[L.FD_X_P, L.FD_U_AILERON] = np.inf
    big = A.copy(); big[L.FD_X_U, L.FD_X_W] = 160.0            # |a|_inf dt = 1.6 at dt = 0.01
    cases = [(An, B, 0.01, nz), (A, Bn, 0.01, nz), (big, B, 0.01, nz), (A, B, 0.0, nz), (A, B, np.nan, nz), (A, B, 2.0, nz)]
    cases += [(A, B, 0.01, np.where(np.arange(16) == k, v, nz)) for k in (0, 7, 8, 15) for v in (0.0, -1.0, np.nan, np.inf)]
    for a, b, dt, n_ in cases:
        r = kn.design(a, b, dt, n_)
        assert r["status"] == kn.BAD_INPUT and np.isnan(r["residual"]) and r["iters"] == 0
        assert np.array_equal(r["F"], kn.pass_through())
    Phi, Gamma, Lg = kn.matrices(kn.pass_through())[1]
    assert np.array_equal(Phi, np.eye(4)) and not Gamma.any() and np.array_equal(Lg, np.eye(4))
    # the pass-through filter's estimate is the measurement
    y = np.arange(1.0, 9.0)
    assert np.allclose(kn.kalman_update(kn.pass_through(), np.full(8, 0.3), np.full(4, 0.2), y), y, rtol=0, atol=1e-15)


def test_series_cut_and_the_norm_cap():
    """The first dropped term of S is (a dt)^18 / 19!: at the cap |a|_inf dt = 1.5 it is 1.5^18 / 19! = 1.2e-14, which is where the
    cap comes from; Phi's first dropped term is one power higher, 1.5^19 / 19! = 1.8e-14."""
    from math import factorial
    assert 1.0e-14 < 1.5 ** 18 / factorial(19) < 1.3e-14


def _pack(ctr):
    c = np.asarray(ctr, np.int64).reshape(-1, 4)
    assert c.min() >= 0 and c.max() < 1 << 16
    return ((c[:, 0] << 48) | (c[:, 1] << 32) | (c[:, 2] << 16) | c[:, 3]).astype(np.uint64)


def test_lqg_counters_are_disjoint_from_every_other_consumer():
    """The enumeration of tests/test_device_draw_model.py (1024 rows, episodes 0..3, steps 0..8) with the LQG consumer added:
    its counters repeat nowhere, inside the consumer or in any other layout."""
    rows, eps, steps = np.arange(1024), np.arange(4), np.arange(9)
    R, E = np.meshgrid(rows, eps, indexing="ij")
    R3, E3, S3 = np.meshgrid(rows, eps, steps, indexing="ij")
    others = {
        "reset": pn.reset_counters(R, E), "dr_reset": pn.dr_reset_counters(R, E),
        "random_walk": pn.step_counters(R3, E3, S3, pn.W_RANDOM_WALK), "gust": pn.step_counters(R3, E3, S3, pn.W_GUST),
        "action": np.stack([pn.row_counters(rows, s, pn.W_ACTION, 1) for s in steps]),
        "sensor": np.stack([pn.row_counters(rows, s, pn.W_SENSOR, 5) for s in steps]),
    }
    lqg = _pack(np.stack([kn.lqg_counters(rows, s) for s in steps]))
    assert lqg.size == 1024 * 9 * 2 and np.unique(lqg).size == lqg.size
    for name, ctr in others.items():
        assert np.intersect1d(lqg, _pack(ctr)).size == 0, f"lqg and {name} share a counter"
    c = kn.lqg_counters(np.array([5, (3 << 32) + 5]), 7)
    assert c[0].tolist() == [[5, 0, 7, 0x70], [5, 0, 7, 0x71]] and c[1, 1].tolist() == [5, 3, 7, 0x71]
    z = kn.lqg_normal_sequence(9, np.arange(4096), 0, 4)
    assert z.shape == (4, 4096, 8) and abs(z.mean()) < 5 / np.sqrt(z.size) and abs(z.var() - 1.0) < 5 * np.sqrt(2.0 / z.size)
    assert not np.array_equal(z[0], z[1])


def test_closed_loop_over_the_oracle():
    """The three conditions of the issue on all ten aircraft (the five listed conditions are rows 0..4)."""
    f = kn.oracle_flights()
    rows = f["rows"]
    assert len(rows) == 10 and not any(r["kf_status"] for r in rows) and not f["base"]["status"].any()
    worst_err, worst_chat, worst_rate = 0.0, 0.0, 0.0
    for i, r in enumerate(rows):
        err = r["est"]["err_est"] / r["est"]["err_meas"]
        chat = r["est"]["chatter"] / r["meas"]["chatter"]
        rate = r["est"]["rate_ms"] / r["meas"]["rate_ms"]
        print(f"aircraft {i}: err_est / err_meas {err.min():.3f}..{err.max():.3f}, chatter ratio {chat.min():.4f}..{chat.max():.4f}, "
              f"true q, p, r mean-square ratio {rate.min():.3f}..{rate.max():.3f}, saturated steps {r['est']['sat']} / {r['meas']['sat']}")
        assert (r["est"]["err_est"] < 0.5 * r["est"]["err_meas"]).all(), (i, err)
        assert (r["est"]["chatter"] < 0.5 * r["meas"]["chatter"]).all(), (i, chat)
        assert (r["est"]["rate_ms"] < r["meas"]["rate_ms"]).all(), (i, rate)
        worst_err, worst_chat, worst_rate = max(worst_err, err.max()), max(worst_chat, chat.max()), max(worst_rate, rate.max())
    print(f"worst: error ratio {worst_err:.3f}, chatter ratio {worst_chat:.4f}, rate ratio {worst_rate:.3f}")


# ---- hcrl_amd.lqg without a device ------------------------------------------------------------------------------------------------
def test_noise_vector_rows_and_the_sensor_config():
    nz = G.KalmanNoise()
    assert not nz.per_lane and nz.vector().shape == (16,)
    loud = G.KalmanNoise(noise_config={"imu_gyro_stddev": 0.05, "gps_velocity_stddev": 0.3, "attitude_stddev": 0.02})
    assert loud.vector()[:8].tolist() == [0.3, 0.3, 0.05, 0.02, 0.3, 0.05, 0.05, 0.02]
    sweep = G.KalmanNoise(rates=(0.1, 0.1, np.array([0.05, 0.1, 0.2]), 0.005, 0.1, 0.05, 0.05, 0.005))
    assert sweep.per_lane
    rows = sweep.rows(3)
    assert rows.shape == (16, 3) and rows[10].tolist() == [0.05, 0.1, 0.2] and rows[0].tolist() == [0.1] * 3
    with pytest.raises(ValueError):
        sweep.rows(4)
    with pytest.raises(ValueError):
        G.KalmanNoise(sigma=(0.1,) * 7).vector()
    cpu = torch.device("cpu")
    assert tuple(G.noise_tensor(None, 3, cpu).shape) == (16,) and tuple(G.noise_tensor(sweep, 3, cpu).shape) == (16, 3)
    with pytest.raises(ValueError):
        G.noise_tensor(np.ones(15), 3, cpu)


def _design(status):
    n = len(status)
    F = torch.as_tensor(np.random.RandomState(1).normal(size=(80, n)))
    return G.KalmanDesign(F, torch.zeros(n, dtype=torch.float64), torch.full((n,), 6, dtype=torch.int32),
                          torch.tensor(status, dtype=torch.int32), 0.01)


def test_design_matrices_and_the_strict_error():
    d = _design([0, 3, 0, 4])
    assert d.n == 4 and d.ok.tolist() == [True, False, True, False] and d.count_not_ok() == 2
    for lane in range(4):
        for k, (Phi, Gamma, Lg) in enumerate(kn.matrices(d.F[:, lane].numpy())):
            assert np.array_equal(d.phi()[k, :, :, lane].numpy(), Phi) and np.array_equal(d.gamma()[k, :, :, lane].numpy(), Gamma)
            assert np.array_equal(d.gain()[k, :, :, lane].numpy(), Lg)
            assert np.allclose(d.filter_matrix()[k, :, :, lane].numpy(), Phi @ (np.eye(4) - Lg), atol=1e-12)
    assert G.describe_status(0) == "ok" and G.describe_status(5) == "not converged, invalid model, noise or dt"
    G.require_ok(_design([0, 0]))
    with pytest.raises(ValueError, match=r"2 of 4 aircraft.*first: aircraft 1: not converged, no stability certificate"):
        G.require_ok(d, "BatchedSixDOF.design_kalman")


def test_fleet_guards_need_no_device():
    from hcrl_amd.fleet import BatchedCascade, BatchedSixDOF
    from hcrl_amd.hybrid import HybridFleet
    assert HybridFleet.design_kalman is BatchedSixDOF.design_kalman and HybridFleet.step_lqg is BatchedSixDOF.step_lqg
    assert BatchedCascade.design_kalman is BatchedSixDOF.design_kalman and BatchedCascade.step_lqg is BatchedSixDOF.step_lqg
    fleet = BatchedSixDOF.__new__(BatchedSixDOF)
    fleet.n = 3
    with pytest.raises(ValueError, match="has no trim"):
        fleet.design_kalman(0.01)
    with pytest.raises(ValueError, match=r"3 of 3 aircraft have no certified stabilising gain"):
        fleet.step_lqg(1)
    fleet._lqr = object()
    with pytest.raises(ValueError, match=r"3 of 3 aircraft have no certified stable filter"):
        fleet.step_lqg(1)


def test_kalman_into_refuses_wrong_shapes():
    A, B = torch.zeros((12, 12, 2), dtype=torch.float64), torch.zeros((12, 4, 2), dtype=torch.float64)
    with pytest.raises(ValueError):
        G.kalman_into(A, B[:, :3], 0.01, torch.ones(16, dtype=torch.float64))
    with pytest.raises(ValueError):
        G.kalman_into(A, B, 0.01, torch.ones((16, 3), dtype=torch.float64))
    with pytest.raises(ValueError):
        G.kalman_into(A.float(), B, 0.01, torch.ones(16, dtype=torch.float64))

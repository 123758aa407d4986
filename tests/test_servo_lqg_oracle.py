"""The servo's estimator on the CPU: the NumPy restatement (tests/servo_lqg_numpy.py) of fdyn_servo_kf_design against SciPy's
matrix exponential and discrete Riccati solver, and of the control step flown over the CPU oracle's RK4 on the sensor layer's noise.

Gates (none derived from what the restatement returns):
  design   Phi against scipy.linalg.expm and Gamma against the augmented exponential: 1e-12 absolute; P and L against
           scipy.linalg.solve_discrete_are: 1e-9 relative to max|.|; status 0 everywhere and the spectral radius of Phi (I - L) < 1
           (numpy.linalg.eigvals); psi's column of Phi_lat the unit vector exactly; all 288 golden linearisations, dt 0.01 and 0.02
  flight   the four probe conditions, trim -> +4 m/s, +30 m, +60 deg at 1 s -> 40 s, Philox normals of seed 20241020, under the
           estimate and under the measurement on the same normals:
           err_est / err_meas < 1 on each of the ten words (the estimate beats the sensor);
           chatter(estimate) / chatter(measurement) <= 0.5 on each control (fdyn_lqg_step's gate);
           rms of the true errors over the last 10 s under the estimate: |e_V| <= 0.1 m/s, |e_h| <= 0.5 m, |e_psi| <= 0.01 rad (the
           GPS-velocity, altimeter and attitude sigma); |roll| <= 1.3 rad and |pitch| <= 0.9 rad throughout (the servo's gates)
"""
import os

import numpy as np
import pytest
import scipy.linalg

import servo_lqg_numpy as sl
import servo_numpy as sn
from conftest import GOLDEN


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "trim_reference.npz"))


@pytest.mark.parametrize("dt", [0.01, 0.02])
def test_design_agrees_with_scipy_on_all_golden_aircraft(golden, dt):
    ref = sl.golden_designs(golden, dt)
    assert len(ref["status"]) == 288 and not ref["status"].any(), np.flatnonzero(ref["status"])
    nz = sl.default_noise()
    worst = dict(phi=0.0, gamma=0.0, P=0.0, L=0.0, rho=0.0, norm=0.0)
    for i in range(288):
        for k, ((a, b), (Phi, Gamma, Lg)) in enumerate(zip(sl.blocks(golden["A"][i], golden["B"][i]), sl.matrices(ref["F"][i]))):
            worst["norm"] = max(worst["norm"], sl.row_norm(a) * dt)
            E = scipy.linalg.expm(np.block([[a, b], [np.zeros((2, 7))]]) * dt)
            worst["phi"] = max(worst["phi"], float(np.abs(Phi - E[:5, :5]).max()))
            worst["gamma"] = max(worst["gamma"], float(np.abs(Gamma - E[:5, 5:]).max()))
            sigma, rates = nz[5 * k:5 * k + 5], nz[10 + 5 * k:15 + 5 * k]
            V, W = np.diag(sigma ** 2), np.diag(rates ** 2 * dt)
            Ps = scipy.linalg.solve_discrete_are(E[:5, :5].T, np.eye(5), W, V)
            Ls = Ps @ np.linalg.inv(Ps + V)
            P = sl.design_block(a, b, dt, sigma, rates)["P"]
            worst["P"] = max(worst["P"], float(np.abs(P - Ps).max() / np.abs(Ps).max()))
            worst["L"] = max(worst["L"], float(np.abs(Lg - Ls).max() / np.abs(Ls).max()))
            worst["rho"] = max(worst["rho"], float(np.abs(np.linalg.eigvals(Phi @ (np.eye(5) - Lg))).max()))
            if k == 1:                                      # psi's column of A is zero: the heading wrap commutes with the prediction
                assert np.array_equal(Phi[:, 4], np.array([0.0, 0.0, 0.0, 0.0, 1.0])), i
    print(f"dt {dt}: 576 blocks, worst |Phi - expm| {worst['phi']:.3e}, |Gamma - expm| {worst['gamma']:.3e}, P {worst['P']:.3e}, L {worst['L']:.3e} "
          f"relative, spectral radius {worst['rho']:.4f}, |a|_inf dt {worst['norm']:.4f}, doublings {ref['iters'].min()}..{ref['iters'].max()}")
    assert worst["norm"] <= sl.NORM_MAX                     # the cap refuses none of the golden aircraft
    assert worst["phi"] <= 1e-12 and worst["gamma"] <= 1e-12
    assert worst["P"] <= 1e-9 and worst["L"] <= 1e-9
    assert worst["rho"] < 1.0


def test_bad_input_is_refused_with_the_pass_through(golden):
    A, B = golden["A"][5], golden["B"][5]
    good = sl.design(A, B, 0.01, sl.default_noise())
    assert good["status"] == 0
    nan_a, zero = A.copy(), sl.default_noise()
    nan_a[3, 2] = np.nan                                    # d udot / d z: read by the longitudinal block
    zero[13] = 0.0
    for bad in (sl.design(nan_a, B, 0.01, sl.default_noise()), sl.design(A, B, 0.01, zero), sl.design(A, B, 0.0, sl.default_noise()),
                sl.design(A * 100.0, B, 0.02, sl.default_noise())):
        assert bad["status"] == sl.BAD_INPUT == 4 and np.isnan(bad["residual"]) and bad["iters"] == 0
        for Phi, Gamma, Lg in sl.matrices(bad["F"]):
            assert np.array_equal(Phi, np.eye(5)) and not Gamma.any() and np.array_equal(Lg, np.eye(5))
    unread = A.copy()
    unread[0, 0] = np.nan                                   # the north row is in neither block
    assert np.array_equal(sl.design(unread, B, 0.01, sl.default_noise())["F"], good["F"])


def test_philox_words_meet_no_other_consumer():
    import kf_numpy as kn
    import servo_wind_numpy as wn
    mine = {sl.W_SERVO_LQG + b for b in range(3)}
    assert mine == {0x7A, 0x7B, 0x7C}
    others = set(range(0, 4)) | {7, 16, 17, 18, 19, 20, 0x51} | {0x60 + k for k in range(5)} | {kn.W_LQG, kn.W_LQG + 1, wn.W_SERVO_GUST}
    assert not mine & others
    c = sl.lqg_counters(np.array([3, 2 ** 33 + 1]), 41)
    assert c.shape == (2, 3, 4) and c[0, :, 3].tolist() == [0x7A, 0x7B, 0x7C] and c[1, 0, :3].tolist() == [1, 2, 41]
    z = sl.lqg_normals(sl.SEED, np.arange(4000), 1)
    assert z.shape == (4000, 10) and abs(z.mean()) < 0.02 and abs(z.std() - 1.0) < 0.02


def _report(rows):
    for (name, V, dt, climb), r in zip(sn.PROBE, rows):
        e, m = r["est"], r["meas"]
        print(f"{name} V {V} dt {dt} climb {climb}: err_est / err_meas {np.round(e['err_est'] / e['err_meas'], 3)}, chatter ratio "
              f"{np.round(e['chatter'] / m['chatter'], 4)}, rms (V, h, psi) estimate {e['rms']}, measurement {m['rms']}, max |roll| {e['roll']:.3f}, "
              f"max |pitch| {e['pitch']:.3f}")


def test_probe_flights_on_sensor_noise_meet_the_gates():
    rows = sl.probe_flights()
    _report(rows)
    for r in rows:
        e, m = r["est"], r["meas"]
        assert r["kf_status"] == 0
        assert (e["err_est"] / e["err_meas"] < sl.GATE_RATIO).all(), e["err_est"] / e["err_meas"]
        assert (e["chatter"] / m["chatter"] <= sl.GATE_CHATTER).all(), e["chatter"] / m["chatter"]
        assert e["rms"][0] <= sl.GATE_V and e["rms"][1] <= sl.GATE_H and e["rms"][2] <= sl.GATE_PSI, e["rms"]
        assert e["roll"] <= sn.GATE_ROLL and e["pitch"] <= sn.GATE_PITCH, (e["roll"], e["pitch"])


def test_a_filter_that_trusts_the_trim_model_is_worse_than_its_sensors():
    """The test that can fail: fdyn_kf_design's rates, extended to z and psi, bias the estimate far from the trim."""
    rows = sl.probe_flights(sl.TRIM_RATES)
    _report(rows)
    for r in rows:
        assert r["kf_status"] == 0
        ratio = r["est"]["err_est"] / r["est"]["err_meas"]
        assert ratio.max() > sl.GATE_RATIO, ratio


def test_a_turn_through_pi_from_the_trim_heading_needs_the_wrapped_innovation():
    """Two commands of +100 deg (at 1 s and at 9 s, flown to the probe's 40 s) carry psi - psi0 through +pi: the measured deviation
    jumps to -pi there, and the innovation's wrap is what keeps the estimate on it.  Gates: the estimate stays in [-pi, pi); it is
    never further from the true deviation than 0.3 rad, the servo's heading-error clip (an estimate off by more saturates the law;
    without the wrap it is off by about 2 pi for a while); err_est < err_meas on psi over the flight, the issue's gate on its own
    horizon; the turn arrives within ten attitude sigmas.  The same flight on the same normals with the innovation left unwrapped
    breaks the second and the third: the test that can fail.
    Measured: the estimate lags the true heading by 0.025 .. 0.035 rad while the aircraft turns at up to 1.9 rad/s, before, at and
    after the crossing alike -- the trim's wings-level model, not the wrap -- so that over the first 20 s alone, half of them spent
    turning, err_est / err_meas on psi is 0.91 (rc_plane) and 1.01 (cessna)."""
    good, bad = sl.wrap_flights(), sl.wrap_flights(wrap_innovation=False)
    for i in range(len(sl.WRAP_AIRCRAFT)):
        d = good["d_psi"][i]
        jump = np.flatnonzero(np.abs(np.diff(d)) > np.pi)
        assert len(jump) >= 1 and d[jump[0]] > 3.0 and d[jump[0] + 1] < -3.0, "the deviation from the trim heading never passed +pi"
        assert d[-1] < -2.7                                               # 200 deg from the trim heading = -160 deg
        off, off_bad = (np.abs(sl.wrap_angle(r["xhat_psi"][i] - r["d_psi"][i])).max() for r in (good, bad))
        ratio, ratio_bad = (r["err_est"][i][sl.PSI] / r["err_meas"][i][sl.PSI] for r in (good, bad))
        arrived = abs(sl.wrap_angle(good["x"][i][sn.X_YAW] - good["ref"][i][2]))
        print(f"{sl.WRAP_AIRCRAFT[i]}: d_psi passes +pi at step {jump[0] + 1}; with the wrapped innovation err_est / err_meas on psi {ratio:.3f}, "
              f"worst |xhat_psi - d_psi| {off:.4f} rad, widest |xhat_psi| {np.abs(good['xhat_psi'][i]).max():.4f}, heading error at 40 s {arrived:.2e} "
              f"rad; without it {ratio_bad:.3e} and {off_bad:.4f} rad")
        assert good["kf_status"][i] == 0 and np.abs(good["xhat_psi"][i]).max() <= np.pi
        assert off <= sn.DEFAULT_LIMITS[2]
        assert ratio < sl.GATE_RATIO
        assert arrived <= sl.GATE_PSI * 10
        assert off_bad > sn.DEFAULT_LIMITS[2] and ratio_bad > sl.GATE_RATIO, "the flight does not need the wrap: it tests nothing"

"""The restatement of the servo's predicted covariances (servo_cov_numpy, which the host build of csrc/fdyn_stein_n.hpp equals bit for
bit: test_servo_cov_host.py) against three references it shares no code with.

(a) Every solve against SciPy: the two Lyapunov equations against scipy.linalg.solve_discrete_lyapunov and the Stein equation
    against a Kronecker solve (I - B (x) A) vec X = vec Q, on all 288 golden linearisations x 2 blocks x 2 steps x 3 feedbacks.  Gate
    1e-10 relative to max|X|; at most 20 doublings.

(b) The independent reference for the 34 report words: the joint one-step linear map of (d, i, xhat, du_prev) and its noise input,
    built by pushing vectors through the restatement's own servo_lqg_numpy.kalman_update and servo_numpy.controls (the flight's
    code, not the report's), the RK4 replaced by d+ = Phi d + Gamma du + w; the joint Lyapunov equation solved by SciPy; every word
    derived from it, the chatter through the lag-one covariance.  Gate 1e-9 relative on every word, all three feedbacks, W = 0 and
    W = the design's rates.  This decides the W terms and the truth form, which no flight checks.
      The pushes.  kalman_update is linear as it stands (unit pushes).  controls is linear while unclipped and unwrapped EXCEPT
      for the airspeed error, sqrt(u^2 + v^2 + w^2) - V_c.  At a trim with v0 = 0 (all 288) that is exactly linear along the trim
      velocity (cu, cw) and even across it and in v, so the law's matrix is taken by central differences of +- 1/8 (inside the
      0.3 rad heading clip) in a basis whose (u, w) pair is rotated to (along, across): odd terms survive, even terms cancel to
      the bit, and nothing is left of the square root but its derivative.  The two functions are pushed SEPARATELY and their
      matrices composed: pushed through both at once, the filter would hand the law (u, w) directions that are neither along
      nor across, and the cubic term of the square root leaves 1e-9 .. 6e-8 on the speed words (measured).
      Every word the restatement returns non-zero is held to plain 1e-9 relative.  The words that are structurally zero (truth
      feedback with W = 0: everything but VAR_EST, where the restatement gives exactly 0) come out of SciPy as 1e-20 noise and
      have no relative error; for them alone the reference is held to its own rounding, |ref| <= 64 eps max|Sigma_joint|.

(c) Flights of the restatement's own loop over the CPU restatement's RK4 (default sigma, default rates, Philox normals of seed
    20241020, 16 noise rows, 10 s discarded, 30 s accumulated), the three conditions without a saturated step: flown / predicted
    within 0.9 .. 1.1 for err_est and chatter and within 0.8 .. 1.25 for the true-error mean squares and VAR_X.  The figures
    measured are printed and recorded in DESIGN.md 7q.

(d) The tests that can fail: the measurement-feedback prediction set against the estimate flight misses the chatter gate by more
    than a factor of 10; rc_plane 15 m/s at dt 0.02 under measurement feedback has a predicted throttle headroom below 1 and flies
    an altitude mean square more than 5 times the prediction -- `headroom` flags what it should.
"""
import os

import numpy as np
import pytest
import scipy.linalg as sla

import servo_cov_numpy as sc
import servo_lqg_numpy as sl
import servo_margin_numpy as sm
import servo_modes_numpy as smn
import servo_numpy as sn
from conftest import GOLDEN

EPS = 2.0 ** -52
GATE_SOLVE, GATE_WORD, MAX_DOUBLINGS_SEEN = 1e-10, 1e-9, 20
PUSH = 0.125
ROWS, T_DISCARD, T_ACCUMULATE = 16, 10.0, 30.0
GATE_ACC, GATE_TRUE = (0.9, 1.1), (0.8, 1.25)
CONTROL_LOW, CONTROL_HIGH = np.array([-1.0, -1.0, -1.0, 0.0]), np.ones(4)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "trim_reference.npz"))


# ---- (a) -------------------------------------------------------------------------------------------------------------------------
def test_every_solve_against_scipy(golden):
    d = sm.golden_designs(golden)
    sigma, rates = np.array(sl.DEFAULT_SIGMA), np.array(sl.DEFAULT_RATES)
    worst, most, solves = 0.0, 0, 0
    for dt in sc.DTS:
        for fb in sc.FEEDBACKS:
            rep = sc.golden_reports(golden, with_w=True)[dt, fb]
            assert not rep["status"].any()
            most = max(most, int(rep["iters"].max()))
            for i in range(len(d["K"])):
                loops, filt = smn.sampled_blocks(d["K"][i], d["F"][dt][i], d["x0"][i], dt), smn.filter_blocks(d["F"][dt][i])
                cov = rep["cov"][i]
                for blk, NA in enumerate((sc.NLON, sc.NLAT)):
                    Acl, Ae = loops[blk], filt[blk]
                    _, Gamma, L = sl.matrices(d["F"][dt][i])[blk]
                    Se = cov[sc.CC_E[blk]:sc.CC_E[blk] + 25].reshape(5, 5)
                    Sxe = cov[sc.CC_XE[blk]:sc.CC_XE[blk] + NA * 5].reshape(NA, 5)
                    Sx = cov[sc.CC_X[blk]:sc.CC_X[blk] + NA * NA].reshape(NA, NA)
                    v, w = sigma[5 * blk:5 * blk + 5] ** 2, rates[5 * blk:5 * blk + 5] ** 2 * dt
                    ImL = np.eye(5) - L
                    Kx = d["K"][i][(0, 14)[blk]:(0, 14)[blk] + 2 * NA].reshape(2, NA)[:, :5]
                    Bf = np.vstack([-Gamma @ Kx, Acl[5:, :5]])
                    Wt = np.zeros((NA, NA))
                    Wt[:5, :5] = np.diag(w)
                    ref_e = sla.solve_discrete_lyapunov(Ae, ImL @ np.diag(w) @ ImL.T + L @ np.diag(v) @ L.T)
                    pairs = [(Se, ref_e)]
                    if fb == sc.ESTIMATE:
                        Qxe = -Bf @ ref_e @ Ae.T
                        Qxe[:5] += np.diag(w) @ ImL.T
                        ref_xe = np.linalg.solve(np.eye(NA * 5) - np.kron(Acl, Ae), Qxe.reshape(-1)).reshape(NA, 5)   # row-major vec
                        G = Acl @ ref_xe @ Bf.T
                        Qx = Bf @ ref_e @ Bf.T - G - G.T + Wt
                        pairs.append((Sxe, ref_xe))
                    else:
                        assert not Sxe.any()
                        Qx = (Bf @ np.diag(v) @ Bf.T if fb == sc.MEASUREMENT else 0.0) + Wt
                    pairs.append((Sx, sla.solve_discrete_lyapunov(Acl, Qx)))
                    for got, ref in pairs:
                        worst = max(worst, float(np.abs(got - ref).max() / np.abs(ref).max()))
                        solves += 1
    print(f"(a) {solves} solves: worst relative difference to SciPy {worst:.2e}, most doublings {most}")
    assert worst <= GATE_SOLVE and most <= MAX_DOUBLINGS_SEEN


# ---- (b) -------------------------------------------------------------------------------------------------------------------------
NS, NV = 27, 20                                                  # (d 10, i 3, xhat 10, du_prev 4); (v 10, w 10)


def _pushed(fn, n_in, basis=None, push=1.0):
    """The matrix of a function that is linear (odd, at least) in its n_in inputs: column j = (fn(+push b_j) - fn(-push b_j)) / 2 push
    over the columns b_j of an orthogonal basis, turned back to the unit vectors."""
    basis = np.eye(n_in) if basis is None else basis
    cols = [(fn(push * basis[:, j]) - fn(-push * basis[:, j])) / (2.0 * push) for j in range(n_in)]
    return np.array(cols).T @ basis.T


def joint_map(K, F, x0, u0, dt, feedback):
    """-> (A [27][27], G [27][20], C [17][27], D [17][20]): s+ = A s + G (v, w) and the outputs (xhat+ - d [10], the true errors
    [3], du [4]) = C s + D (v, w), composed from the matrices of the flight's own functions."""
    cu, cw, ok = smn._directions(x0)
    assert ok and x0[sn.X_V] == 0.0
    ref0 = sn.reference_at(x0)
    # the filter: xhat+ = Ux xhat + Ud du_prev + Uy y.  Linear as it stands: unit pushes.
    U = _pushed(lambda z: sl.kalman_update(F, z[:10], z[10:14], z[14:24]), 24)
    Ux, Ud, Uy = U[:, :10], U[:, 10:14], U[:, 14:]

    # the law on x0 + f and the integrators: (du, e) = (Uf f + Ui i, Ef f), the (u, w) pair of f pushed along and across the trim
    # velocity; the true errors of x0 + d are the same rows Ef
    def law(z):
        u, e = sn.controls(K, x0, u0, sl.law_input(x0, x0, z[:10]), ref0, z[10:13])
        return np.concatenate([u - u0, e])
    basis = np.eye(13)
    basis[0:2, 0:2] = [[cu, -cw], [cw, cu]]
    Lw = _pushed(law, 13, basis, PUSH)
    Uf, Ui, Ef = Lw[:4, :10], Lw[:4, 10:], Lw[4:, :10]
    assert not Lw[4:, 10:].any()

    def truth(z):
        x = np.array(x0, np.float64)
        for j, s in enumerate(sl.EST_STATES):
            x[s] = x0[s] + z[j]
        u, _ = sn.controls(K, x0, u0, x, ref0, np.zeros(3))
        return np.concatenate([u - u0, sn.errors(x, ref0)])
    Tr = _pushed(truth, 10, basis[:10, :10], PUSH)
    assert np.array_equal(Tr[:4], Uf) and np.array_equal(Tr[4:], Ef)  # the stored state and x0 + d are the same law input
    Phi, Gam = np.zeros((10, 10)), np.zeros((10, 4))
    for k, ((P, Gm, _), ctl) in enumerate(zip(sl.matrices(F), (sn.LON_CONTROLS, sn.LAT_CONTROLS))):
        Phi[5 * k:5 * k + 5, 5 * k:5 * k + 5] = P
        Gam[5 * k:5 * k + 5, list(ctl)] = Gm
    # z = (d, i, xhat, du_prev | v, w): rows of every quantity as a map of z
    Z = np.eye(NS + NV)
    d_, i_, xh_, du_, v_, w_ = Z[0:10], Z[10:13], Z[13:23], Z[23:27], Z[27:37], Z[37:47]
    y = d_ + v_
    xh1 = Ux @ xh_ + Ud @ du_ + Uy @ y
    f = xh1 if feedback == sc.ESTIMATE else (y if feedback == sc.MEASUREMENT else d_)
    du1 = Uf @ f + Ui @ i_
    i1 = i_ + dt * (Ef @ f)
    d1 = Phi @ d_ + Gam @ du1 + w_
    Ms, Mo = np.vstack([d1, i1, xh1, du1]), np.vstack([xh1 - d_, Ef @ d_, du1])
    return Ms[:, :NS], Ms[:, NS:], Mo[:, :NS], Mo[:, NS:]


def joint_words(K, F, x0, u0, dt, sigma, rates, feedback):
    """-> (the 34 report words from the joint Lyapunov solution, max|Sigma_joint|)"""
    A, G, C, D = joint_map(K, F, x0, u0, dt, feedback)
    N = np.diag(np.concatenate([np.asarray(sigma) ** 2, np.asarray(rates) ** 2 * dt]))
    S = sla.solve_discrete_lyapunov(A, G @ N @ G.T)
    O = C @ S @ C.T + D @ N @ D.T
    lag = (C @ S)[13:17, 23:27]                                  # E[u_k u_{k-1}^T]: du_prev of s_k is u_{k-1}
    rep = np.zeros(sc.NSCV)
    rep[sc.VAR_X:sc.VAR_X + 10], rep[sc.VAR_EST:sc.VAR_EST + 10] = np.diag(S)[:10], np.diag(O)[:10]
    rep[sc.VAR_ERR:sc.VAR_ERR + 3], rep[sc.VAR_INTEG:sc.VAR_INTEG + 3] = np.diag(O)[10:13], np.diag(S)[10:13]
    rep[sc.VAR_U:sc.VAR_U + 4] = np.diag(O)[13:17]
    rep[sc.VAR_DU:sc.VAR_DU + 4] = (np.diag(O)[13:17] + np.diag(S)[23:27]) - 2.0 * np.diag(lag)
    return rep, float(np.abs(S).max())


JOINT_LANES = tuple(range(0, 288, 12)) + (97, 200, 287)


def test_every_report_word_against_the_joint_model(golden):
    d = sm.golden_designs(golden)
    u0 = np.asarray(golden["u0"], np.float64)
    worst, cases = 0.0, 0
    for with_w in (False, True):
        reports = sc.golden_reports(golden, with_w)
        rates = sl.DEFAULT_RATES if with_w else np.zeros(10)
        for dt in sc.DTS:
            for fb in sc.FEEDBACKS:
                for i in JOINT_LANES:
                    got = reports[dt, fb]["report"][i]
                    ref, scale = joint_words(d["K"][i], d["F"][dt][i], d["x0"][i], u0[i], dt, sl.DEFAULT_SIGMA, rates, fb)
                    zero = got == 0.0                            # structurally zero: the restatement gives exactly 0
                    if fb == sc.TRUTH and not with_w:            # X is exactly zero: nothing moves but the estimate
                        assert zero.sum() == sc.NSCV - 10 and not zero[sc.VAR_EST:sc.VAR_EST + 10].any()
                    else:
                        assert not zero.any(), (i, dt, fb, with_w, np.nonzero(zero)[0])
                    rel = np.abs(got - ref)[~zero] / np.abs(ref)[~zero]
                    assert (rel <= GATE_WORD).all(), (i, dt, fb, with_w, np.nonzero(~zero)[0][rel > GATE_WORD], rel[rel > GATE_WORD])
                    assert (np.abs(ref)[zero] <= 64.0 * EPS * scale).all(), (i, dt, fb, with_w, ref[zero])
                    worst = max(worst, float(rel.max()))
                    cases += 1
    print(f"(b) {cases} cases x 34 words: worst relative difference to the joint model {worst:.2e}")


# ---- (c), (d) --------------------------------------------------------------------------------------------------------------------
_FLOWN = {}


def flown(name, V, dt, feedback):
    """One condition flown as the issue states -> dict(err_est [10], chatter [4], err2 [3], var_x [10]: means per step over the 16
    rows and the accumulated 30 s; sat: saturated steps of all rows, discarded part included; pred {feedback: the restatement's
    lane}; u0).  Once per session."""
    key = (name, V, dt, feedback)
    if key not in _FLOWN:
        des = sn.oracle_design(name, V)
        step = sn.oracle_step(des["P"])
        kf = sl.design(des["A"], des["B"], dt, sl.default_noise())
        assert des["status"] == 0 and kf["status"] == 0
        n1, n2 = int(round(T_DISCARD / dt)), int(round(T_ACCUMULATE / dt))
        z = sl.lqg_normal_sequence(sl.SEED, np.arange(ROWS), 0, n1 + n2)
        acc = dict(err_est=np.zeros(10), chatter=np.zeros(4), err2=np.zeros(3), var_x=np.zeros(10))
        sat = 0
        for row in range(ROWS):
            a = sl.fly(step, des["K"], kf["F"], sl.DEFAULT_SIGMA, des["x0"], des["u0"], des["x0"], sn.reference_at(des["x0"]), np.zeros(3), dt,
                       z[:n1, row], feedback)
            rec = []
            b = sl.fly(step, des["K"], kf["F"], sl.DEFAULT_SIGMA, des["x0"], des["u0"], a["x"], a["ref"], a["integ"], dt, z[n1:, row], feedback,
                       xhat=a["xhat"], du_prev=a["du_prev"], record=rec)
            sat += a["sat"] + b["sat"]
            acc["err_est"] += b["err_est"]
            acc["chatter"] += b["chatter"]
            acc["err2"] += np.sum(np.array([r[1] for r in rec]) ** 2, axis=0)
            acc["var_x"] += np.sum(np.array([sl.deviation(r[0], des["x0"]) for r in rec]) ** 2, axis=0)
        out = {k: v / (ROWS * n2) for k, v in acc.items()}
        out["sat"], out["u0"] = sat, des["u0"]
        out["pred"] = {fb: sc.servo_covariance(des["K"], kf["F"], des["x0"], dt, sl.DEFAULT_SIGMA, None, fb) for fb in (sc.ESTIMATE, sc.MEASUREMENT)}
        assert all(p["status"] == 0 for p in out["pred"].values())
        _FLOWN[key] = out
    return _FLOWN[key]


def _ratios(fl, pred):
    r = pred["report"]
    return dict(err_est=fl["err_est"] / r[sc.VAR_EST:sc.VAR_EST + 10], chatter=fl["chatter"] / r[sc.VAR_DU:sc.VAR_DU + 4],
                err2=fl["err2"] / r[sc.VAR_ERR:sc.VAR_ERR + 3], var_x=fl["var_x"] / r[sc.VAR_X:sc.VAR_X + 10])


def _headroom(pred, u0):
    return np.minimum(u0 - CONTROL_LOW, CONTROL_HIGH - u0) / np.sqrt(pred["report"][sc.VAR_U:sc.VAR_U + 4])


@pytest.mark.parametrize("name, V, dt, feedback", (("rc_plane", 20.0, 0.01, sc.ESTIMATE), ("cessna", 25.0, 0.02, sc.ESTIMATE),
                                                   ("cessna", 25.0, 0.02, sc.MEASUREMENT)),
                         ids=("rc_plane-20-0.01-estimate", "cessna-25-0.02-estimate", "cessna-25-0.02-measurement"))
def test_flights_meet_the_prediction(name, V, dt, feedback):
    fl = flown(name, V, dt, feedback)
    r = _ratios(fl, fl["pred"][feedback])
    print(f"(c) {name} {V} m/s dt {dt} feedback {feedback}: saturated steps {fl['sat']}, throttle headroom "
          f"{_headroom(fl['pred'][feedback], fl['u0'])[3]:.1f}; flown / predicted err_est {r['err_est'].min():.3f} .. {r['err_est'].max():.3f}, "
          f"chatter {r['chatter'].min():.3f} .. {r['chatter'].max():.3f}, true errors (V, h, psi) {np.round(r['err2'], 3)}, "
          f"VAR_X {r['var_x'].min():.3f} .. {r['var_x'].max():.3f}")
    assert fl["sat"] == 0
    for key, (lo, hi) in (("err_est", GATE_ACC), ("chatter", GATE_ACC), ("err2", GATE_TRUE), ("var_x", GATE_TRUE)):
        assert (r[key] >= lo).all() and (r[key] <= hi).all(), (key, r[key])


def test_the_wrong_feedbacks_prediction_misses_the_chatter_gate():
    """The estimate flight against the MEASUREMENT-feedback prediction: off by more than a factor of 10 on every control, so the
    chatter gate of (c) tells the two predictions apart."""
    fl = flown("rc_plane", 20.0, 0.01, sc.ESTIMATE)
    r = _ratios(fl, fl["pred"][sc.MEASUREMENT])["chatter"]
    print("(d) estimate flight / measurement prediction, chatter:", np.round(r, 4))
    assert (np.maximum(r, 1.0 / r) > 10.0).all(), r


def test_headroom_flags_the_condition_the_prediction_fails_on():
    """rc_plane 15 m/s, dt 0.02, measurement feedback: predicted throttle headroom below 1, thousands of saturated steps, and a flown
    altitude mean square more than 5 times the prediction."""
    fl = flown("rc_plane", 15.0, 0.02, sc.MEASUREMENT)
    pred = fl["pred"][sc.MEASUREMENT]
    room, r = _headroom(pred, fl["u0"]), _ratios(fl, pred)
    print(f"(d) rc_plane 15 m/s dt 0.02 measurement: throttle headroom {room[3]:.2f}, saturated steps {fl['sat']}, flown / predicted altitude "
          f"mean square {r['err2'][1]:.2f}, throttle chatter {r['chatter'][3]:.3f}")
    assert room[3] < 1.0 and fl["sat"] > 0
    assert r["err2"][1] > 5.0

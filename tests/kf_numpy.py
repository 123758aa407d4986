"""The steady-state Kalman filter and the LQG loop of include/fdyn.h (fdyn_kf_design, fdyn_lqg_step_*) restated in NumPy: the
same formulas in the same order of operations (products summed left to right, the elimination of trim_numpy, the doubling loop
and stopping rule of lqr_numpy), the LQG normals from the host Philox model (philox_numpy, consumer word 0x70), and the closed
loop over ANY `step(x[12], u_clipped[4], dt) -> x[12]`.  Shared by the CPU test and the GPU test; nothing here imports the
product package.
"""
import numpy as np

import philox_numpy as pn
from lqr_numpy import (mm, inv4, ldl_positive, blocks, delta, clip_controls, MAX_ITERS, TOL, RES_MAX, LON_CONTROLS, LAT_CONTROLS,
                       DELTA_STATES, _worse)
from trim_numpy import maxabs

NKF, NKFN, SERIES_TERMS, NORM_MAX = 80, 16, 17, 1.5
PHI_LON, PHI_LAT, GAMMA_LON, GAMMA_LAT, L_LON, L_LAT = 0, 16, 32, 40, 48, 64
NOT_CONVERGED, NO_CERTIFICATE, BAD_INPUT = 1, 2, 4
ESTIMATE, MEASUREMENT, TRUTH = 0, 1, 2
W_LQG = 0x70                                                   # FD_PHX_LQG: blocks 0x70 (longitudinal four), 0x71 (lateral four)
# sigma of (u, w, q, theta | v, p, r, phi): the sensor layer's default GPS-velocity, gyro and attitude noise; then the rates s
DEFAULT_SIGMA = (0.1, 0.1, 0.01, 0.01, 0.1, 0.01, 0.01, 0.01)
DEFAULT_RATES = (0.1, 0.1, 0.05, 0.005, 0.1, 0.05, 0.05, 0.005)
DIAG = np.arange(4)


def default_noise():
    return np.array(DEFAULT_SIGMA + DEFAULT_RATES, np.float64)


def pass_through():
    """F of a lane whose design failed: Phi = I, Gamma = 0, L = I."""
    F = np.zeros(NKF)
    for base in (PHI_LON, PHI_LAT, L_LON, L_LAT):
        F[base:base + 16] = np.eye(4).reshape(16)
    return F


def row_norm(a):
    """max over the rows of |a_r0| + |a_r1| + |a_r2| + |a_r3|, summed in that order."""
    m = 0.0
    for r in range(4):
        rs = abs(a[r, 0])
        for c in range(1, 4):
            rs = rs + abs(a[r, c])
        m = rs if rs > m else m
    return m


def discretise(a, b, dt):
    """-> (Phi, Gamma): S = sum_k (a dt)^k / (k + 1)! cut after SERIES_TERMS terms, Phi = I + a dt S, Gamma = dt S b."""
    ad = a * dt
    T, S = np.eye(4), np.eye(4)
    for k in range(1, SERIES_TERMS + 1):
        T = mm(T, ad) / float(k + 1)
        S = S + T
    Phi = mm(ad, S)
    Phi[DIAG, DIAG] = 1.0 + Phi[DIAG, DIAG]
    return Phi, dt * mm(S, b)


def doubling(Ak, Gk, Hk):
    """lqr_numpy.design_block's loop on given start values -> (H, iterations, failed, converged)."""
    I = np.eye(4)
    it, failed, converged = 0, False, False
    while not failed and not converged and it < MAX_ITERS:
        Mi, ok = inv4(I + mm(Gk, Hk))
        if not ok:
            failed = True
            break
        AM, MA = mm(Ak, Mi), mm(Mi, Ak)
        A1 = mm(AM, Ak)
        G1 = Gk + mm(mm(AM, Gk), Ak.T)
        H1 = Hk + mm(Ak.T, mm(Hk, MA))
        it += 1
        hmax, diff = maxabs(H1), maxabs(H1 - Hk)
        Ak, Gk, Hk = A1, G1, H1
        if not (np.isfinite(hmax) and np.isfinite(diff)):
            failed = True
            break
        converged = bool(diff <= TOL * max(1.0, hmax))
    return Hk, it, failed, converged


def design_block(a, b, dt, sigma, rates):
    """One 4-state block, every state measured -> dict(Phi, Gamma [4][2], L, P, residual, iters, status bits 1 | 2)."""
    with np.errstate(all="ignore"):
        a, b, sigma, rates = (np.array(v, np.float64) for v in (a, b, sigma, rates))
        v, w = sigma * sigma, (rates * rates) * dt
        Phi, Gamma = discretise(a, b, dt)
        H, it, failed, converged = doubling(Phi.T.copy(), np.diag(1.0 / v), np.diag(w))
        P = 0.5 * (H + H.T)
        PV = P.copy()
        PV[DIAG, DIAG] = P[DIAG, DIAG] + v
        PVi, gain_ok = inv4(PV)
        L = mm(P, PVi)
        T = mm(mm(Phi, P - mm(L, P)), Phi.T)
        T[DIAG, DIAG] = T[DIAG, DIAG] + w
        R = T - P
        res = maxabs(R) / maxabs(P)
        status = 0
        if failed or not converged:
            status |= NOT_CONVERGED
        if not gain_ok or not ldl_positive(P) or not res <= RES_MAX:
            status |= NO_CERTIFICATE
        return dict(Phi=Phi, Gamma=Gamma, L=L, P=P, residual=res, iters=it, status=status)


def design(A, B, dt, noise):
    """One aircraft -> dict(F [80], residual, iters, status): what fdyn_kf_design writes for a lane."""
    nz = np.asarray(noise, np.float64)
    bl = blocks(A, B)
    with np.errstate(all="ignore"):
        ok = bool(dt > 1e-6) and not dt > 1.0 and bool(np.isfinite(nz).all()) and bool((nz > 0.0).all())
        ok = ok and all(np.isfinite(a).all() and np.isfinite(b).all() for a, b in bl)
        ok = ok and all(row_norm(a) * dt <= NORM_MAX for a, _ in bl)
    if not ok:
        return dict(F=pass_through(), residual=np.nan, iters=0, status=BAD_INPUT)
    F, res, it, st = np.zeros(NKF), 0.0, 0, 0
    for k, (a, b) in enumerate(bl):
        r = design_block(a, b, dt, nz[4 * k:4 * k + 4], nz[8 + 4 * k:12 + 4 * k])
        F[PHI_LON + 16 * k:PHI_LON + 16 * k + 16] = r["Phi"].reshape(16)
        F[GAMMA_LON + 8 * k:GAMMA_LON + 8 * k + 8] = r["Gamma"].reshape(8)
        F[L_LON + 16 * k:L_LON + 16 * k + 16] = r["L"].reshape(16)
        res, it, st = _worse(res, r["residual"]), max(it, r["iters"]), st | r["status"]
    if st:
        F = pass_through()
    return dict(F=F, residual=res, iters=it, status=st)


def design_many(A, B, dt, noise):
    """A [n][12][12], B [n][12][4], noise [16] or [n][16] -> dict of arrays F [n][80], residual, iters, status."""
    n = len(A)
    nz = np.broadcast_to(np.asarray(noise, np.float64), (n, NKFN))
    rows = [design(A[i], B[i], dt, nz[i]) for i in range(n)]
    return dict(F=np.array([r["F"] for r in rows]), residual=np.array([r["residual"] for r in rows]),
                iters=np.array([r["iters"] for r in rows], np.int32), status=np.array([r["status"] for r in rows], np.int32))


def matrices(F):
    """F [80] -> ((Phi_lon, Gamma_lon, L_lon), (Phi_lat, Gamma_lat, L_lat))."""
    F = np.asarray(F)
    return tuple((F[PHI_LON + 16 * k:PHI_LON + 16 * k + 16].reshape(4, 4), F[GAMMA_LON + 8 * k:GAMMA_LON + 8 * k + 8].reshape(4, 2),
                  F[L_LON + 16 * k:L_LON + 16 * k + 16].reshape(4, 4)) for k in range(2))


# ---- the LQG normals -----------------------------------------------------------------------------------------------------------
def lqg_counters(rows, step):
    """[n, 2 blocks, 4 words]; `step` = the word the step pointer holds at launch + s + 1 for step s of the launch."""
    return pn.row_counters(rows, step, W_LQG, 2)


def lqg_normals(seed, rows, step):
    """[n, 8] standard normals of one LQG step in delta's order: block 0 the longitudinal four, block 1 the lateral four."""
    c = lqg_counters(np.atleast_1d(rows), step)
    return pn.normals4(pn.philox(seed, c[..., 0], c[..., 1], c[..., 2], c[..., 3])).reshape(len(np.atleast_1d(rows)), 8)


def lqg_normal_sequence(seed, rows, step0, n_steps):
    """[n_steps, n, 8]: what a launch of n_steps draws when the step word holds step0."""
    return np.stack([lqg_normals(seed, rows, step0 + s + 1) for s in range(n_steps)])


# ---- the closed loop -----------------------------------------------------------------------------------------------------------
def kalman_update(F, xhat, du_prev, y):
    """pred = Phi xhat + Gamma du_prev, xhat = pred + L (y - pred) per block; du_prev [4] in FD_U_* order.  Every sum left to right."""
    out = np.zeros(8)
    for k, ((Phi, Gamma, L), ctl) in enumerate(zip(matrices(F), (LON_CONTROLS, LAT_CONTROLS))):
        xh, yy = xhat[4 * k:4 * k + 4], y[4 * k:4 * k + 4]
        pred, e = np.zeros(4), np.zeros(4)
        for r in range(4):
            p = Phi[r, 0] * xh[0]
            for c in range(1, 4):
                p = p + Phi[r, c] * xh[c]
            g = Gamma[r, 0] * du_prev[ctl[0]] + Gamma[r, 1] * du_prev[ctl[1]]
            pred[r] = p + g
            e[r] = yy[r] - pred[r]
        for r in range(4):
            c = L[r, 0] * e[0]
            for j in range(1, 4):
                c = c + L[r, j] * e[j]
            out[4 * k + r] = pred[r] + c
    return out


def controls_from(K16, u0, f):
    """u = u0 - K f for eight words f in delta's order, each row summed left to right -> unclipped [4] in FD_U_* order."""
    u = np.array(u0, np.float64)
    for blk, ctl in enumerate((LON_CONTROLS, LAT_CONTROLS)):
        for j, c in enumerate(ctl):
            k = np.asarray(K16[8 * blk + 4 * j:8 * blk + 4 * j + 4])
            ff = f[4 * blk:4 * blk + 4]
            s = k[0] * ff[0]
            for m in range(1, 4):
                s = s + k[m] * ff[m]
            u[c] = u0[c] - s
    return u


def fly(step, K16, F, sigma, x0, u0, x, dt, z, feedback=ESTIMATE, xhat=None, du_prev=None, record=None):
    """len(z) steps of the LQG loop from state x; z [n_steps][8] standard normals.  -> dict(x, xhat, du_prev, u (last clipped
    controls), sat, err_est [8], err_meas [8], chatter [4], y (last measurement)).  record: optional list that receives a copy of
    x after every step."""
    x = np.array(x, np.float64)
    sigma = np.asarray(sigma, np.float64)
    xhat = np.zeros(8) if xhat is None else np.array(xhat, np.float64)
    du = np.zeros(4) if du_prev is None else np.array(du_prev, np.float64)
    err_est, err_meas, chatter, sat = np.zeros(8), np.zeros(8), np.zeros(4), 0
    u, y = None, np.zeros(8)
    for zs in np.asarray(z, np.float64):
        d = delta(x, x0)
        y = d + sigma * zs
        xhat = kalman_update(F, xhat, du, y)
        err_est = err_est + (xhat - d) ** 2
        err_meas = err_meas + (y - d) ** 2
        f = xhat if feedback == ESTIMATE else (y if feedback == MEASUREMENT else d)
        u, clipped = clip_controls(controls_from(K16, u0, f))
        sat += int(clipped)
        chatter = chatter + (u - (u0 + du)) ** 2
        du = u - u0
        x = step(x, u, dt)
        if record is not None:
            record.append(x.copy())
    return dict(x=x, xhat=xhat, du_prev=du, u=u, sat=sat, err_est=err_est, err_meas=err_meas, chatter=chatter, y=y)


# ---- what both test files fly ---------------------------------------------------------------------------------------------------
SEED, DT, STEPS, STEPS_COMPARE = 20240607, 0.01, 1000, 500
RATE_WORDS = (2, 5, 6)                                          # q, p, r inside delta's eight words
_FLIGHTS = {}


def oracle_flights():
    """The ten aircraft of lqr_numpy.oracle_flights (the five conditions on both airframes; the issue's five first) with a filter
    designed at DT with the default noise, flown FROM TRIM over the CPU oracle's RK4 step for STEPS steps with the Philox normals
    of seed SEED (row = the aircraft's index, step word 0 at launch), once under the estimate and once under the measurement.
    Once per test session, read-only.  Per aircraft: F, kf_status, z [STEPS][8]; est / meas: dicts of fly()'s outputs after
    STEPS steps plus rate_ms [3] (mean square of the true q, p, r over the last STEPS // 2 steps); est_500: fly()'s outputs
    after STEPS_COMPARE steps under the estimate."""
    if _FLIGHTS:
        return _FLIGHTS
    import lqr_numpy as ln
    import trim_numpy as tn
    from oracle import oracle as orc
    base = ln.oracle_flights()["all"]
    n = len(base["type"])
    z = lqg_normal_sequence(SEED, np.arange(n), 0, STEPS).transpose(1, 0, 2)          # [n][STEPS][8]
    rows = []
    for i in range(n):
        P = tn.oracle_airframe(tn.TYPES[int(base["type"][i])])[4]

        def step(x, u, dt, P=P):
            x = x.copy()
            orc.rk4_step(P, x, np.ascontiguousarray(u), dt)
            return x

        kf = design(base["A"][i], base["B"][i], DT, default_noise())
        row = dict(F=kf["F"], kf_status=kf["status"], z=z[i])
        for name, fb in (("est", ESTIMATE), ("meas", MEASUREMENT)):
            rec = []
            out = fly(step, base["K"][i], kf["F"], DEFAULT_SIGMA, base["x0"][i], base["u0"][i], base["x0"][i], DT, z[i], fb, record=rec)
            d = np.array([delta(xx, base["x0"][i]) for xx in rec[STEPS // 2:]])
            out["rate_ms"] = np.mean(d[:, RATE_WORDS] ** 2, axis=0)
            row[name] = out
        row["est_500"] = fly(step, base["K"][i], kf["F"], DEFAULT_SIGMA, base["x0"][i], base["u0"][i], base["x0"][i], DT,
                             z[i][:STEPS_COMPARE], ESTIMATE)
        rows.append(row)
    _FLIGHTS["base"] = base
    _FLIGHTS["rows"] = rows
    return _FLIGHTS

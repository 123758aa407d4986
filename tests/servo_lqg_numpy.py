"""The servo's estimator of include/fdyn_servo_lqg.h (fdyn_servo_kf_design, fdyn_servo_lqg_step_*) restated in NumPy fp64: the
Kalman design of csrc/fdyn_kalman_n.hpp in the same order of operations for any block size (kf_numpy's at N, on servo_numpy's
elimination, doubling loop and L D L^T test), the measurement normals from the host Philox model (philox_numpy, consumer words
0x7A..0x7C), and the control step -- measure, filter with the heading innovation wrapped, servo_numpy's law on trim + f -- over ANY
`step(x[12], u_clipped[4], dt) -> x[12]`.  Shared by the CPU tests and the GPU test; nothing here imports the product package.
"""
import numpy as np

import philox_numpy as pn
import servo_numpy as sn
from lqr_numpy import mm, wrap_angle, clip_controls
from trim_numpy import maxabs

NB, NSKX, NSKN, NSKF, SERIES_TERMS, NORM_MAX = 5, 10, 20, 120, 17, 1.5
PHI_LON, PHI_LAT, GAMMA_LON, GAMMA_LAT, L_LON, L_LAT = 0, 25, 50, 60, 70, 95
NOT_CONVERGED, NO_CERTIFICATE, BAD_INPUT = 1, 2, 4
ESTIMATE, MEASUREMENT, TRUTH = 0, 1, 2
W_SERVO_LQG = 0x7A                                             # FD_PHX_SERVO_LQG: three blocks, 0x7A..0x7C
EST_STATES = sn.LON_STATES + sn.LAT_STATES                     # (u, w, q, theta, z | v, p, r, phi, psi) inside x[12]
ANGLE_WORDS, PSI = (3, 8, 9), 9                                # theta, phi, psi inside the ten
# sigma: the sensor layer's default GPS-velocity, gyro, attitude and altitude noise; then the rates s
DEFAULT_SIGMA = (0.1, 0.1, 0.01, 0.01, 0.5, 0.1, 0.01, 0.01, 0.01, 0.01)
DEFAULT_RATES = (0.3, 0.5, 0.1, 0.03, 0.3, 0.3, 0.1, 0.1, 0.03, 0.03)
# fdyn_kf_design's rates, extended by 0.1 on z and 0.005 on psi: a filter that trusts the trim's model, for the test that can fail
TRIM_RATES = (0.1, 0.1, 0.05, 0.005, 0.1, 0.1, 0.05, 0.05, 0.005, 0.005)


def default_noise(rates=DEFAULT_RATES):
    return np.array(DEFAULT_SIGMA + tuple(rates), np.float64)


def pass_through():
    """F of a lane whose design failed: Phi = I, Gamma = 0, L = I."""
    F = np.zeros(NSKF)
    for base in (PHI_LON, PHI_LAT, L_LON, L_LAT):
        F[base:base + NB * NB] = np.eye(NB).reshape(-1)
    return F


def blocks(A, B):
    """-> ((a_lon [5][5], b_lon [5][2]), (a_lat, b_lat)): the five physical states of each augmented block of the servo."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    return ((A[np.ix_(sn.LON_STATES, sn.LON_STATES)], B[np.ix_(sn.LON_STATES, sn.LON_CONTROLS)]),
            (A[np.ix_(sn.LAT_STATES, sn.LAT_STATES)], B[np.ix_(sn.LAT_STATES, sn.LAT_CONTROLS)]))


def row_norm(a):
    """max over the rows of |a_r0| + |a_r1| + ..., summed in that order."""
    m = 0.0
    for row in np.abs(a):
        rs = row[0]
        for v in row[1:]:
            rs = rs + v
        m = rs if rs > m else m
    return m


def discretise(a, b, dt):
    """-> (Phi, Gamma): S = sum_k (a dt)^k / (k + 1)! cut after SERIES_TERMS terms, Phi = I + a dt S, Gamma = dt S b."""
    n = len(a)
    ad = a * dt
    T, S = np.eye(n), np.eye(n)
    for k in range(1, SERIES_TERMS + 1):
        T = mm(T, ad) / float(k + 1)
        S = S + T
    Phi = mm(ad, S)
    d = np.arange(n)
    Phi[d, d] = 1.0 + Phi[d, d]
    return Phi, dt * mm(S, b)


def kalman_solve(Phi, sigma, rates, dt):
    """One N-state block, every state measured -> dict(L, P, residual, iters, failed, converged, gain_ok, positive, status bits
    1 | 2): csrc/fdyn_kalman_n.hpp's kalman_solve, operation for operation."""
    with np.errstate(all="ignore"):
        Phi, sigma, rates = (np.array(v, np.float64) for v in (Phi, sigma, rates))
        d = np.arange(len(Phi))
        v, w = sigma * sigma, (rates * rates) * dt
        _, _, H, it, failed, converged = sn.doubling(Phi.T.copy(), np.diag(1.0 / v), np.diag(w))
        P = 0.5 * (H + H.T)
        PV = P.copy()
        PV[d, d] = P[d, d] + v
        PVi, gain_ok = sn.inv(PV)
        L = mm(P, PVi)
        T = mm(mm(Phi, P - mm(L, P)), Phi.T)
        T[d, d] = T[d, d] + w
        res = maxabs(T - P) / maxabs(P)
        positive = sn.ldl_positive(P)
        status = 0
        if failed or not converged:
            status |= NOT_CONVERGED
        if not gain_ok or not positive or not res <= sn.RES_MAX:
            status |= NO_CERTIFICATE
        return dict(L=L, P=P, residual=res, iters=it, failed=failed, converged=converged, gain_ok=bool(gain_ok), positive=positive,
                    status=status)


def design_block(a, b, dt, sigma, rates):
    """discretise + kalman_solve -> kalman_solve's dict plus Phi, Gamma."""
    with np.errstate(all="ignore"):
        Phi, Gamma = discretise(np.array(a, np.float64), np.array(b, np.float64), dt)
    return dict(kalman_solve(Phi, sigma, rates, dt), Phi=Phi, Gamma=Gamma)


def design(A, B, dt, noise):
    """One aircraft -> dict(F [120], residual, iters, status): what fdyn_servo_kf_design writes for a lane."""
    nz = np.asarray(noise, np.float64)
    bl = blocks(A, B)
    with np.errstate(all="ignore"):
        ok = bool(dt > 1e-6) and not dt > 1.0 and bool(np.isfinite(nz).all()) and bool((nz > 0.0).all())
        ok = ok and all(np.isfinite(a).all() and np.isfinite(b).all() for a, b in bl)
        ok = ok and all(row_norm(a) * dt <= NORM_MAX for a, _ in bl)
    if not ok:
        return dict(F=pass_through(), residual=np.nan, iters=0, status=BAD_INPUT)
    F, res, it, st = np.zeros(NSKF), 0.0, 0, 0
    for k, (a, b) in enumerate(bl):
        r = design_block(a, b, dt, nz[NB * k:NB * k + NB], nz[NSKX + NB * k:NSKX + NB * k + NB])
        F[PHI_LON + 25 * k:PHI_LON + 25 * k + 25] = r["Phi"].reshape(-1)
        F[GAMMA_LON + 10 * k:GAMMA_LON + 10 * k + 10] = r["Gamma"].reshape(-1)
        F[L_LON + 25 * k:L_LON + 25 * k + 25] = r["L"].reshape(-1)
        res, it, st = sn._worse(res, r["residual"]), max(it, r["iters"]), st | r["status"]
    if st:
        F = pass_through()
    return dict(F=F, residual=res, iters=it, status=st)


def design_many(A, B, dt, noise):
    """A [n][12][12], B [n][12][4], noise [20] or [n][20] -> dict of arrays F [n][120], residual, iters, status."""
    n = len(A)
    nz = np.broadcast_to(np.asarray(noise, np.float64), (n, NSKN))
    rows = [design(A[i], B[i], dt, nz[i]) for i in range(n)]
    return dict(F=np.array([r["F"] for r in rows]), residual=np.array([r["residual"] for r in rows]),
                iters=np.array([r["iters"] for r in rows], np.int32), status=np.array([r["status"] for r in rows], np.int32))


def matrices(F):
    """F [120] -> ((Phi_lon, Gamma_lon, L_lon), (Phi_lat, Gamma_lat, L_lat))."""
    F = np.asarray(F)
    return tuple((F[PHI_LON + 25 * k:PHI_LON + 25 * k + 25].reshape(NB, NB), F[GAMMA_LON + 10 * k:GAMMA_LON + 10 * k + 10].reshape(NB, 2),
                  F[L_LON + 25 * k:L_LON + 25 * k + 25].reshape(NB, NB)) for k in range(2))


_CACHE = {}


def golden_designs(golden, dt):
    """The restatement on the 288 linearisations of tests/golden/trim_reference.npz with the default noise at dt, once per session."""
    if ("golden", dt) not in _CACHE:
        out = design_many(golden["A"], golden["B"], dt, default_noise())
        for v in out.values():
            v.setflags(write=False)
        _CACHE["golden", dt] = out
    return _CACHE["golden", dt]


# ---- the measurement normals ---------------------------------------------------------------------------------------------------
def lqg_counters(rows, step):
    """[n, 3 blocks, 4 words]; `step` = the word the step pointer holds at launch + s + 1 for step s of the launch."""
    return pn.row_counters(rows, step, W_SERVO_LQG, 3)


def lqg_normals(seed, rows, step):
    """[n, 10] standard normals of one step in d's order: the first ten of the twelve the three blocks give."""
    rows = np.atleast_1d(rows)
    c = lqg_counters(rows, step)
    return pn.normals4(pn.philox(seed, c[..., 0], c[..., 1], c[..., 2], c[..., 3])).reshape(len(rows), 12)[:, :NSKX]


def lqg_normal_sequence(seed, rows, step0, n_steps):
    """[n_steps, n, 10]: what a launch of n_steps draws when the step word holds step0."""
    return np.stack([lqg_normals(seed, rows, step0 + s + 1) for s in range(n_steps)])


# ---- the control step ----------------------------------------------------------------------------------------------------------
def deviation(x, x0):
    """d: the ten words of x - x0, the theta, phi and psi differences wrapped."""
    d = np.array([x[s] - x0[s] for s in EST_STATES])
    for k in ANGLE_WORDS:
        d[k] = wrap_angle(d[k])
    return d


def kalman_update(F, xhat, du_prev, y, wrap_innovation=True):
    """pred = Phi xhat + Gamma du_prev, e = y - pred with the psi word wrapped, xhat = pred + L e with the psi word wrapped, per
    block; du_prev [4] in FD_U_* order.  Every sum left to right.  wrap_innovation=False: what the step would be without the wrap
    of e_psi (for the test that shows the wrap is needed)."""
    out = np.zeros(NSKX)
    for k, ((Phi, Gamma, L), ctl) in enumerate(zip(matrices(F), (sn.LON_CONTROLS, sn.LAT_CONTROLS))):
        xh, yy = xhat[NB * k:NB * k + NB], y[NB * k:NB * k + NB]
        pred, e = np.zeros(NB), np.zeros(NB)
        for r in range(NB):
            p = Phi[r, 0] * xh[0]
            for c in range(1, NB):
                p = p + Phi[r, c] * xh[c]
            g = Gamma[r, 0] * du_prev[ctl[0]] + Gamma[r, 1] * du_prev[ctl[1]]
            pred[r] = p + g
            e[r] = yy[r] - pred[r]
        if k == 1 and wrap_innovation:
            e[NB - 1] = wrap_angle(e[NB - 1])
        for r in range(NB):
            c = L[r, 0] * e[0]
            for j in range(1, NB):
                c = c + L[r, j] * e[j]
            out[NB * k + r] = pred[r] + c
    out[PSI] = wrap_angle(out[PSI])
    return out


def law_input(x, x0, f):
    """x_f: x0 + f on the ten words with the psi word wrapped, the stored state elsewhere."""
    xf = np.array(x, np.float64)
    for j, s in enumerate(EST_STATES):
        xf[s] = x0[s] + f[j]
    xf[sn.X_YAW] = wrap_angle(xf[sn.X_YAW])
    return xf


def controls_from(K26, x0, u0, x, xhat, ref, integ, feedback=ESTIMATE, limits=sn.DEFAULT_LIMITS):
    """n_steps = 0: the unclipped controls from the stored estimate (from the stored state for TRUTH)."""
    xf = x if feedback == TRUTH else law_input(x, x0, xhat)
    return sn.controls(K26, x0, u0, xf, ref, integ, limits)[0]


def fly(step, K26, F, sigma, x0, u0, x, ref, integ, dt, z, feedback=ESTIMATE, xhat=None, du_prev=None, limits=sn.DEFAULT_LIMITS,
        record=None, wrap_innovation=True, trace=None):
    """len(z) control steps of include/fdyn_servo_lqg.h from state x; z [n_steps][10] standard normals.  -> dict(x, ref, integ,
    xhat, du_prev, u (last clipped controls), sat, err_est [10], err_meas [10], chatter [4], y (last measurement), err (the last
    errors of the true state before their clip)).  record: optional list that receives (x, true errors) after every step; trace:
    optional list that receives (d_psi, y_psi, xhat_psi) of every step."""
    x, ref, integ = np.array(x, np.float64), np.array(ref, np.float64), np.array(integ, np.float64)
    sigma = np.asarray(sigma, np.float64)
    xhat = np.zeros(NSKX) if xhat is None else np.array(xhat, np.float64)
    du = np.zeros(4) if du_prev is None else np.array(du_prev, np.float64)
    err_est, err_meas, chatter, sat = np.zeros(NSKX), np.zeros(NSKX), np.zeros(4), 0
    u0 = np.asarray(u0, np.float64)
    uc, y, err = None, np.zeros(NSKX), np.zeros(3)
    for zs in np.asarray(z, np.float64):
        d = deviation(x, x0)
        y = d + sigma * zs
        xhat = kalman_update(F, xhat, du, y, wrap_innovation)
        if trace is not None:
            trace.append((d[PSI], y[PSI], xhat[PSI]))
        de = xhat - d
        de[PSI] = wrap_angle(de[PSI])
        err_est = err_est + de ** 2
        err_meas = err_meas + (y - d) ** 2
        err = sn.errors(x, ref)
        xf = x if feedback == TRUTH else law_input(x, x0, xhat if feedback == ESTIMATE else y)
        u, e = sn.controls(K26, x0, u0, xf, ref, integ, limits)
        uc, _ = clip_controls(u)
        lon = bool(uc[0] != u[0] or uc[3] != u[3])
        lat = bool(uc[1] != u[1] or uc[2] != u[2])
        sat += int(lon or lat)
        if not lon:
            integ[0] = integ[0] + e[0] * dt
            integ[1] = integ[1] + e[1] * dt
        if not lat:
            integ[2] = integ[2] + e[2] * dt
        chatter = chatter + (uc - (u0 + du)) ** 2
        du = uc - u0
        x = step(x, uc, dt)
        ref[1] = ref[1] + ref[3] * dt
        ref[2] = wrap_angle(ref[2] + ref[4] * dt)
        if record is not None:
            record.append((x.copy(), sn.errors(x, ref)))
    return dict(x=x, ref=ref, integ=integ, xhat=xhat, du_prev=du, u=uc, sat=sat, err_est=err_est, err_meas=err_meas, chatter=chatter,
                y=y, err=err)


# ---- what the test files fly ---------------------------------------------------------------------------------------------------
SEED = 20241020
GATE_RATIO, GATE_CHATTER, GATE_V, GATE_H, GATE_PSI = 1.0, 0.5, 0.1, 0.5, 0.01      # the issue's gates (sensor sigmas, fdyn_lqg's chatter gate)


def probe_flights(rates=DEFAULT_RATES):
    """The four probe conditions of servo_numpy.PROBE flown over the CPU oracle's RK4 on the default sensor noise with Philox
    normals of seed SEED (row = the condition's index, step word 0 at the start): trim, the probe's commands at 1 s, to 40 s; each
    once under the estimate and once under the measurement, on the same normals.  Once per test session per `rates`.  Per
    condition: est / meas dicts of err_est, err_meas, chatter (sums over the whole flight), rms [3] of the true errors over the
    last 10 s, roll, pitch (largest magnitudes), kf_status."""
    key = ("probe", tuple(rates))
    if key in _CACHE:
        return _CACHE[key]
    rows = []
    for i, (name, V, dt, climb) in enumerate(sn.PROBE):
        d = sn.oracle_design(name, V, climb)
        step = sn.oracle_step(d["P"])
        kf = design(d["A"], d["B"], dt, default_noise(rates))
        n1, n2 = int(round(sn.T_COMMAND / dt)), int(round((sn.T_END - sn.T_COMMAND) / dt))
        z = lqg_normal_sequence(SEED, np.array([i]), 0, n1 + n2)[:, 0, :]
        row = dict(kf_status=kf["status"], dt=dt)
        for label, fb in (("est", ESTIMATE), ("meas", MEASUREMENT)):
            rec = []
            a = fly(step, d["K"], kf["F"], DEFAULT_SIGMA, d["x0"], d["u0"], d["x0"], sn.reference_at(d["x0"]), np.zeros(3), dt, z[:n1], fb,
                    record=rec)
            b = fly(step, d["K"], kf["F"], DEFAULT_SIGMA, d["x0"], d["u0"], a["x"], sn.commanded(a["ref"]), a["integ"], dt, z[n1:], fb,
                    xhat=a["xhat"], du_prev=a["du_prev"], record=rec)
            xs, es = np.array([r[0] for r in rec]), np.array([r[1] for r in rec])
            last = es[-int(round(10.0 / dt)):]
            row[label] = dict(err_est=a["err_est"] + b["err_est"], err_meas=a["err_meas"] + b["err_meas"], chatter=a["chatter"] + b["chatter"],
                              rms=np.sqrt(np.mean(last ** 2, axis=0)), roll=float(np.abs(xs[:, 6]).max()), pitch=float(np.abs(xs[:, 7]).max()))
        rows.append(row)
    _CACHE[key] = rows
    return rows


COMPARE_STEPS = (100, 400)


def compare_flights():
    """The ten aircraft of servo_numpy.compare_flights, each with a filter designed at dt 0.01 on the default noise, flown from its
    trim over the CPU oracle under the estimate on replayed Philox normals (seed SEED, row = the aircraft's index): 100 steps,
    the probe's commands, 400 more.  Read-only: F [10][120], z [500][10 aircraft][10], and fly()'s outputs after step 500 with
    the accumulators summed over both legs."""
    if "compare" not in _CACHE:
        import lqr_numpy as ln
        import trim_numpy as tn
        base = sn.compare_flights()
        n = len(base["type"])
        z = lqg_normal_sequence(SEED, np.arange(n), 0, sum(COMPARE_STEPS))                # [500][n][10]
        rows = []
        for i in range(n):
            P = tn.oracle_airframe(tn.TYPES[int(base["type"][i])])[4]
            step = sn.oracle_step(P)
            kf = design(base["A"][i], base["B"][i], ln.DT, default_noise())
            a = fly(step, base["K"][i], kf["F"], DEFAULT_SIGMA, base["x0"][i], base["u0"][i], base["x0"][i], base["ref0"][i], np.zeros(3),
                    ln.DT, z[:COMPARE_STEPS[0], i])
            b = fly(step, base["K"][i], kf["F"], DEFAULT_SIGMA, base["x0"][i], base["u0"][i], a["x"], sn.commanded(a["ref"]), a["integ"],
                    ln.DT, z[COMPARE_STEPS[0]:, i], xhat=a["xhat"], du_prev=a["du_prev"])
            rows.append(dict(F=kf["F"], kf_status=kf["status"], x=b["x"], xhat=b["xhat"], du_prev=b["du_prev"], integ=b["integ"], ref=b["ref"],
                             u=b["u"], sat=a["sat"] + b["sat"], err_est=a["err_est"] + b["err_est"], err_meas=a["err_meas"] + b["err_meas"],
                             chatter=a["chatter"] + b["chatter"]))
        out = {k: np.array([r[k] for r in rows]) for k in rows[0]}
        out["z"] = z
        for v in out.values():
            v.setflags(write=False)
        _CACHE["compare"] = out
    return _CACHE["compare"]


# ---- a turn through more than pi from the trim heading -----------------------------------------------------------------------------
# The filter works on psi - psi0, so the wraps of the innovation and of the estimate act only once the DEVIATION passes +-pi.  A
# single command beyond 180 deg is flown the short way round and never gets there; two commands of +100 deg each do.
WRAP_AIRCRAFT = (("rc_plane", 20.0), ("cessna", 25.0))
WRAP_LEGS = (100, 800, 3100)                                   # steps from trim; then +100 deg; then +100 deg more; dt 0.01: 40 s, the probe's horizon
WRAP_TURN = np.radians(100.0)


def wrap_flights(wrap_innovation=True):
    """The aircraft of WRAP_AIRCRAFT flown over the CPU oracle under the estimate on Philox normals (seed SEED + 1, row = the
    aircraft's index, step word 0): WRAP_LEGS.  Once per session per flag.  Read-only dict: type, x0, u0, K, F, ref0, z [4000][2][10]
    and after the last step x, xhat, du_prev, integ, ref, sat, err_est, err_meas, chatter (summed over the legs); d_psi, y_psi,
    xhat_psi [2][4000] over the flight."""
    key = ("wrap", wrap_innovation)
    if key not in _CACHE:
        import trim_numpy as tn
        n, dt = len(WRAP_AIRCRAFT), 0.01
        z = lqg_normal_sequence(SEED + 1, np.arange(n), 0, sum(WRAP_LEGS))
        rows = []
        for i, (name, V) in enumerate(WRAP_AIRCRAFT):
            d = sn.oracle_design(name, V)
            step = sn.oracle_step(d["P"])
            kf = design(d["A"], d["B"], dt, default_noise())
            ref0 = sn.reference_at(d["x0"])
            x, ref, integ, xhat, du, at = d["x0"], ref0, np.zeros(3), None, None, 0
            acc, sat, trace = dict(err_est=0.0, err_meas=0.0, chatter=0.0), 0, []
            for leg, steps in enumerate(WRAP_LEGS):
                if leg:
                    ref = sn.command(ref, heading=ref[2] + WRAP_TURN)
                r = fly(step, d["K"], kf["F"], DEFAULT_SIGMA, d["x0"], d["u0"], x, ref, integ, dt, z[at:at + steps, i], ESTIMATE, xhat, du,
                        wrap_innovation=wrap_innovation, trace=trace)
                x, ref, integ, xhat, du, at, sat = r["x"], r["ref"], r["integ"], r["xhat"], r["du_prev"], at + steps, sat + r["sat"]
                for k in acc:
                    acc[k] = acc[k] + r[k]
            tr = np.array(trace).T
            rows.append(dict(type=tn.TYPES.index(name), x0=d["x0"], u0=d["u0"], K=d["K"], F=kf["F"], kf_status=kf["status"], ref0=ref0, x=x, xhat=xhat,
                             du_prev=du, integ=integ, ref=ref, sat=sat, d_psi=tr[0], y_psi=tr[1], xhat_psi=tr[2], **acc))
        out = {k: np.array([r[k] for r in rows]) for k in rows[0]}
        out["z"] = z
        for v in out.values():
            v.setflags(write=False)
        _CACHE[key] = out
    return _CACHE[key]

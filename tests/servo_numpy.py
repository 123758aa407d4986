"""The LQ servo of include/fdyn_servo.h (fdyn_servo_design, fdyn_servo_step_*) restated in NumPy fp64: the augmented models, the
Riccati solver of csrc/fdyn_riccati_n.hpp in the same order of operations (products summed left to right, the same elimination
with partial pivoting, the same Cayley start and stopping rule) for any block size, and the control step over ANY
`step(x[12], u_clipped[4], dt) -> x[12]`.  Shared by the CPU tests and the GPU test; nothing here imports the product package.
"""
import numpy as np

import lqr_numpy as ln
from lqr_numpy import mm, wrap_angle, clip_controls
from trim_numpy import gauss_solve, maxabs

NSVW, NSVK, NSVR, NSVI, NLON, NLAT = 17, 26, 5, 3, 7, 6
MAX_ITERS, TOL, PIVOT_REL, RES_MAX = ln.MAX_ITERS, ln.TOL, ln.PIVOT_REL, ln.RES_MAX
NOT_CONVERGED, NO_CERTIFICATE, BAD_INPUT = 1, 2, 4
# rows / columns of the two augmented blocks inside A [12][12] and B [12][4] (FD_X_* / FD_U_* numbering); the integrators follow
LON_STATES, LON_CONTROLS = (3, 5, 10, 7, 2), (0, 3)       # u, w, q, theta, z | elevator, throttle
LAT_STATES, LAT_CONTROLS = (4, 9, 11, 6, 8), (1, 2)       # v, p, r, phi, psi | aileron, rudder
X_D, X_U, X_V, X_W, X_YAW = 2, 3, 4, 5, 8
# Bryson maxima: longitudinal (u, w, q, theta, z, i_V, i_h), lateral (v, p, r, phi, psi, i_psi), controls
DEFAULT_MAXIMA = (2.0, 2.0, 0.5, 0.1, 2.0, 4.0, 4.0, 2.0, 1.0, 0.5, 0.2, 0.1, 0.2, 0.3, 0.3, 0.3, 0.3)
DEFAULT_LIMITS = (3.0, 10.0, 0.3)


def default_weights():
    m = np.array(DEFAULT_MAXIMA)
    return 1.0 / (m * m)


def inv(a):
    """Inverse: trim_numpy's elimination on [a | I] -> (inverse, ok)."""
    return gauss_solve(a, np.eye(len(a)), PIVOT_REL)


def ldl_positive(x):
    """True when the symmetric x has an L D L^T factorisation with every d > 0 (positive definite)."""
    n = len(x)
    L, d = np.zeros((n, n)), np.zeros(n)
    ok = True
    for j in range(n):
        s = x[j, j]
        for k in range(j):
            s = s - L[j, k] * L[j, k] * d[k]
        d[j] = s
        ok = ok and bool(s > 0.0)
        for i in range(j + 1, n):
            t = x[i, j]
            for k in range(j):
                t = t - L[i, k] * L[j, k] * d[k]
            L[i, j] = t / s
    return ok


def doubling(Ak, Gk, Hk, failed=False):
    """riccati_doubling -> (A, G, H, iterations, failed, converged)."""
    I = np.eye(len(Ak))
    it, converged = 0, False
    while not failed and not converged and it < MAX_ITERS:
        Mi, ok = inv(I + mm(Gk, Hk))
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
    return Ak, Gk, Hk, it, failed, converged


def care_solve(a, b, q, r):
    """One N-state, 2-control block -> dict(K [2][N], X [N][N], residual, iters, failed, converged, positive, status bits 1 | 2).
    q [N], r [2] diagonal.  csrc/fdyn_riccati_n.hpp's care_solve, operation for operation."""
    with np.errstate(all="ignore"):
        a, b, q, r = (np.array(v, np.float64) for v in (a, b, q, r))
        I = np.eye(len(a))
        bs = b * (1.0 / r)[None, :]                      # b R^-1
        G = mm(bs, b.T)
        gamma = 1.0
        for row in np.abs(a):
            rs = row[0]
            for v in row[1:]:
                rs = rs + v
            gamma = rs if rs > gamma else gamma
        ag = a - gamma * I
        agi, ok1 = inv(ag)
        S1 = mm(agi, G)                                  # a_g^-1 G
        W = ag.T + q[:, None] * S1
        Wi, ok2 = inv(W)
        g2 = 2.0 * gamma
        Ak = I + g2 * Wi.T
        Gk = g2 * mm(S1, Wi)
        Hk = g2 * mm(Wi, q[:, None] * agi)
        Ak, Gk, Hk, it, failed, converged = doubling(Ak, Gk, Hk, not (ok1 and ok2))
        X = 0.5 * (Hk + Hk.T)
        K = mm(bs.T, X)
        R = ((mm(a.T, X) + mm(X, a)) - mm(mm(X, G), X)) + np.diag(q)
        xmax = maxabs(X)
        res = maxabs(R) / (xmax if xmax > 1.0 else (1.0 if xmax == xmax else np.nan))
        positive = ldl_positive(X)
        status = 0
        if failed or not converged:
            status |= NOT_CONVERGED
        if not positive or not res <= RES_MAX:
            status |= NO_CERTIFICATE
        return dict(K=K, X=X, residual=res, iters=it, failed=failed, converged=converged, positive=positive, status=status)


def augmented_blocks(A, B, x0):
    """-> ((a_lon [7][7], b_lon [7][2]), (a_lat [6][6], b_lat [6][2])) of A [12][12], B [12][4] at the trim x0 [12]."""
    A, B, x0 = np.asarray(A, np.float64), np.asarray(B, np.float64), np.asarray(x0, np.float64)
    with np.errstate(all="ignore"):
        u0, w0 = x0[X_U], x0[X_W]
        V0 = np.sqrt(u0 * u0 + w0 * w0)
        a_lon, b_lon = np.zeros((NLON, NLON)), np.zeros((NLON, 2))
        a_lon[:5, :5] = A[np.ix_(LON_STATES, LON_STATES)]
        b_lon[:5] = B[np.ix_(LON_STATES, LON_CONTROLS)]
        a_lon[5, 0], a_lon[5, 1], a_lon[6, 4] = u0 / V0, w0 / V0, -1.0
        a_lat, b_lat = np.zeros((NLAT, NLAT)), np.zeros((NLAT, 2))
        a_lat[:5, :5] = A[np.ix_(LAT_STATES, LAT_STATES)]
        b_lat[:5] = B[np.ix_(LAT_STATES, LAT_CONTROLS)]
        a_lat[5, 4] = 1.0
    return (a_lon, b_lon), (a_lat, b_lat)


def block_weights(w):
    """weights [17] -> ((q_lon [7], r_lon [2]), (q_lat [6], r_lat [2]))"""
    w = np.asarray(w, np.float64)
    return (w[0:7], w[13:15]), (w[7:13], w[15:17])


def _worse(a, b):
    return b if (b > a or b != b) else a


def design(A, B, x0, weights, keep_x=False):
    """One aircraft -> dict(K [26], residual, iters, status): what fdyn_servo_design writes for a lane (keep_x: also X_lon, X_lat)."""
    w = np.asarray(weights, np.float64)
    A, B, x0 = np.asarray(A, np.float64), np.asarray(B, np.float64), np.asarray(x0, np.float64)
    with np.errstate(all="ignore"):
        read = [A[np.ix_(s, s)] for s in (LON_STATES, LAT_STATES)] + [B[np.ix_(LON_STATES, LON_CONTROLS)], B[np.ix_(LAT_STATES, LAT_CONTROLS)]]
        finite = all(np.isfinite(m).all() for m in read) and np.isfinite(x0[X_U]) and np.isfinite(x0[X_W])
        V0 = np.sqrt(x0[X_U] * x0[X_U] + x0[X_W] * x0[X_W])
        if not (finite and np.isfinite(w).all() and (w > 0.0).all() and V0 > 0.0):
            return dict(K=np.zeros(NSVK), residual=np.nan, iters=0, status=BAD_INPUT)
    K, res, it, st, xs = np.zeros(NSVK), 0.0, 0, 0, []
    at = 0
    for (a, b), (q, r) in zip(augmented_blocks(A, B, x0), block_weights(w)):
        c = care_solve(a, b, q, r)
        K[at:at + 2 * len(a)] = c["K"].reshape(-1)
        at += 2 * len(a)
        res, it, st = _worse(res, c["residual"]), max(it, c["iters"]), st | c["status"]
        xs.append(c["X"])
    if st:
        K[:] = 0.0
    out = dict(K=K, residual=res, iters=it, status=st)
    if keep_x:
        out["X"] = xs
    return out


def design_many(A, B, x0, weights):
    """A [n][12][12], B [n][12][4], x0 [n][12], weights [17] or [n][17] -> dict of arrays K [n][26], residual, iters, status."""
    n = len(A)
    w = np.broadcast_to(np.asarray(weights, np.float64), (n, NSVW))
    rows = [design(A[i], B[i], x0[i], w[i]) for i in range(n)]
    return dict(K=np.array([r["K"] for r in rows]), residual=np.array([r["residual"] for r in rows]),
                iters=np.array([r["iters"] for r in rows], np.int32), status=np.array([r["status"] for r in rows], np.int32))


def closed_loops(A, B, x0, K26):
    """-> (a_lon - b_lon K_lon [7][7], a_lat - b_lat K_lat [6][6])"""
    (a_lon, b_lon), (a_lat, b_lat) = augmented_blocks(A, B, x0)
    return a_lon - b_lon @ np.asarray(K26[:14]).reshape(2, 7), a_lat - b_lat @ np.asarray(K26[14:]).reshape(2, 6)


# ---- the closed loop -----------------------------------------------------------------------------------------------------------
def reference_at(x0):
    """ref [5] of a fleet just trimmed at x0: its own airspeed, altitude and heading, moving at its climb rate and turn rate."""
    n_, e_, d_, u, v, w, phi, th, psi, p, q, r = np.asarray(x0, np.float64)
    sph, cph, sth, cth = np.sin(phi), np.cos(phi), np.sin(th), np.cos(th)
    return np.array([np.sqrt(u * u + v * v + w * w), -d_, psi, u * sth - v * sph * cth - w * cph * cth, (q * sph + r * cph) / cth])


def clipv(x, lo, hi):
    return lo if x < lo else (hi if x > hi else x)


def errors(x, ref):
    """The three errors before their clip: airspeed, altitude, heading."""
    V = np.sqrt((x[X_U] * x[X_U] + x[X_V] * x[X_V]) + x[X_W] * x[X_W])
    return np.array([V - ref[0], -x[X_D] - ref[1], wrap_angle(x[X_YAW] - ref[2])])


def controls(K26, x0, u0, x, ref, integ, limits=DEFAULT_LIMITS):
    """Steps 1-3 -> (u unclipped [4] in FD_U_* order, clipped errors e [3])."""
    err = errors(x, ref)
    e = np.array([clipv(err[k], -limits[k], limits[k]) for k in range(3)])
    tu, tw = x0[X_U], x0[X_W]
    V0 = np.sqrt(tu * tu + tw * tw)
    cu, cw = (tu / V0, tw / V0) if V0 > 0.0 else (0.0, 0.0)
    dV = ref[0] - V0
    d = ln.delta(x, x0)                                  # (u, w, q, theta | v, p, r, phi), both angle differences wrapped
    dl = np.array([d[0] - dV * cu, d[1] - dV * cw, d[2], d[3], -e[1], integ[0], integ[1]])
    da = np.array([d[4], d[5], d[6], d[7], e[2], integ[2]])
    u = np.array(u0, np.float64)
    for ctl, k, dd in ((LON_CONTROLS, np.asarray(K26[:14]).reshape(2, 7), dl), (LAT_CONTROLS, np.asarray(K26[14:]).reshape(2, 6), da)):
        for j, c in enumerate(ctl):
            s = k[j, 0] * dd[0]
            for m in range(1, len(dd)):
                s = s + k[j, m] * dd[m]
            u[c] = u0[c] - s
    return u, e


def fly(step, K26, x0, u0, x, ref, integ, dt, n_steps, limits=DEFAULT_LIMITS, record=None):
    """n_steps control steps of include/fdyn_servo.h -> (x, ref, integ, last clipped controls, steps with a clipped control).
    record: optional list that receives (x, errors before the step's clip) copies after every step."""
    x, ref, integ = np.array(x, np.float64), np.array(ref, np.float64), np.array(integ, np.float64)
    uc, sat = None, 0
    for _ in range(n_steps):
        u, e = controls(K26, x0, u0, x, ref, integ, limits)
        uc, _ = clip_controls(u)
        lon = bool(uc[0] != u[0] or uc[3] != u[3])
        lat = bool(uc[1] != u[1] or uc[2] != u[2])
        sat += int(lon or lat)
        if not lon:
            integ[0] = integ[0] + e[0] * dt
            integ[1] = integ[1] + e[1] * dt
        if not lat:
            integ[2] = integ[2] + e[2] * dt
        x = step(x, uc, dt)
        ref[1] = ref[1] + ref[3] * dt
        ref[2] = wrap_angle(ref[2] + ref[4] * dt)
        if record is not None:
            record.append((x.copy(), errors(x, ref)))
    return x, ref, integ, uc, sat


def command(ref, heading=None, speed=None, altitude=None):
    """ServoState.command on one aircraft: a heading or altitude command stops that reference's own motion."""
    ref = np.array(ref, np.float64)
    if speed is not None:
        ref[0] = speed
    if altitude is not None:
        ref[1], ref[3] = altitude, 0.0
    if heading is not None:
        ref[2], ref[4] = wrap_angle(heading), 0.0
    return ref


# ---- what the test files fly ---------------------------------------------------------------------------------------------------
# the issue's four probe conditions: (airframe, V, dt, climb (deg)); commands of +4 m/s, +30 m and +60 deg at t = 1 s, flown to 40 s
PROBE = (("rc_plane", 20.0, 0.01, 0.0), ("cessna", 25.0, 0.02, 0.0), ("rc_plane", 15.0, 0.02, 0.0), ("cessna", 18.0, 0.01, 2.0))
COMMAND = dict(speed=4.0, altitude=30.0, heading=np.radians(60.0))
T_COMMAND, T_END = 1.0, 40.0
GATE_V, GATE_H, GATE_PSI, GATE_ROLL, GATE_PITCH = 1e-3, 1e-3, 1e-4, 1.3, 0.9
ALTITUDE, HEADING = ln.ALTITUDE, ln.HEADING


def commanded(ref):
    """The probe's commands applied to a reference: +4 m/s, +30 m, +60 deg."""
    return command(ref, heading=ref[2] + COMMAND["heading"], speed=ref[0] + COMMAND["speed"], altitude=ref[1] + COMMAND["altitude"])


def oracle_step(P):
    from oracle import oracle as orc

    def step(x, u, dt):
        x = x.copy()
        orc.rk4_step(P, x, np.ascontiguousarray(u), dt)
        return x
    return step


def oracle_design(name, V, climb_deg=0.0, turn=0.0, scales=None):
    """Trim, linearise and design one aircraft over the CPU oracle -> dict(type, spec, x0, u0, A, B, K, status, P)."""
    import trim_numpy as tn
    f, grav, max_alpha, max_pitch, P = tn.oracle_airframe(name, scales)
    spec = np.array([V, np.radians(climb_deg), turn, ALTITUDE, HEADING])
    tr = tn.trim(f, spec, grav, max_alpha, max_pitch)
    assert tr["status"] == 0, (name, V, tr["status"])
    A, B = tn.linearize(f, tr["x0"], tr["u0"])
    d = design(A, B, tr["x0"], default_weights())
    return dict(type=tn.TYPES.index(name), spec=spec, x0=tr["x0"], u0=tr["u0"], A=A, B=B, K=d["K"], status=d["status"], P=P)


_CACHE = {}


def golden_designs(golden):
    """The restatement on the 288 linearisations of tests/golden/trim_reference.npz with the default weights, once per test
    session: dict of K [288][26], residual, iters, status and X (a list of (X_lon, X_lat))."""
    if "golden" not in _CACHE:
        rows = [design(golden["A"][i], golden["B"][i], golden["x0"][i], default_weights(), keep_x=True) for i in range(len(golden["A"]))]
        _CACHE["golden"] = dict(K=np.array([r["K"] for r in rows]), residual=np.array([r["residual"] for r in rows]),
                                iters=np.array([r["iters"] for r in rows], np.int32), status=np.array([r["status"] for r in rows], np.int32),
                                X=[r["X"] for r in rows])
    return _CACHE["golden"]


def probe_flights():
    """The four probe conditions flown over the CPU oracle's RK4, once per test session: per condition the design row, dt, the
    end errors (before the clip), the largest |roll| and |pitch|, the saturated steps and the step count."""
    if "probe" not in _CACHE:
        rows = []
        for name, V, dt, climb in PROBE:
            d = oracle_design(name, V, climb)
            step = oracle_step(d["P"])
            n1, n2 = int(round(T_COMMAND / dt)), int(round((T_END - T_COMMAND) / dt))
            rec = []
            x, ref, integ, _, sat1 = fly(step, d["K"], d["x0"], d["u0"], d["x0"], reference_at(d["x0"]), np.zeros(3), dt, n1, record=rec)
            x, ref, integ, _, sat2 = fly(step, d["K"], d["x0"], d["u0"], x, commanded(ref), integ, dt, n2, record=rec)
            xs = np.array([r[0] for r in rec])
            rows.append(dict(d, dt=dt, err=errors(x, ref), roll=float(np.abs(xs[:, 6]).max()), pitch=float(np.abs(xs[:, 7]).max()),
                             sat=sat1 + sat2, steps=n1 + n2, x_end=x, integ_end=integ, ref_end=ref))
        _CACHE["probe"] = rows
    return _CACHE["probe"]


def compare_flights():
    """The ten aircraft of lqr_numpy.oracle_flights (its five conditions on both airframes), each designed as a servo and flown
    from its trim over the CPU oracle at dt 0.01: 100 steps, then the probe's commands, then 400 more.  Read-only arrays:
    type, spec, x0, u0, K, ref0, ref_cmd (the references written after step 100), x_500, u_500, integ_500, ref_500, sat_500."""
    if "compare" not in _CACHE:
        import trim_numpy as tn
        listed = [(tn.TYPES.index(name), V, g, w) for name, V, g, w in ln.CONDITIONS]
        rows = []
        for t, V, g, w in listed + [(1 - t, V, g, w) for t, V, g, w in listed]:
            d = oracle_design(tn.TYPES[t], V, g, w)
            step = oracle_step(d["P"])
            ref0 = reference_at(d["x0"])
            x, ref, integ, _, sat1 = fly(step, d["K"], d["x0"], d["u0"], d["x0"], ref0, np.zeros(3), ln.DT, 100)
            cmd = commanded(ref)
            x, ref, integ, u, sat2 = fly(step, d["K"], d["x0"], d["u0"], x, cmd, integ, ln.DT, 400)
            d.pop("P")
            rows.append(dict(d, ref0=ref0, ref_cmd=cmd, x_500=x, u_500=u, integ_500=integ, ref_500=ref, sat_500=sat1 + sat2))
        out = {k: np.array([r[k] for r in rows]) for k in rows[0]}
        for v in out.values():
            v.setflags(write=False)
        _CACHE["compare"] = out
    return _CACHE["compare"]

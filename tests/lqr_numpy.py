"""The gain-scheduled LQR of include/fdyn.h (fdyn_lqr_design, fdyn_lqr_step_*) restated in NumPy: the same formulas in the same
order of operations (products summed left to right, the same elimination with partial pivoting, the same stopping rule), and
the closed-loop step over ANY `step(x[12], u_clipped[4], dt) -> x[12]`.  Shared by the CPU test and the GPU test; nothing here
imports the product package.
"""
import numpy as np

from trim_numpy import gauss_solve, maxabs

NLQW, NLQK, MAX_ITERS, TOL, PIVOT_REL, RES_MAX = 12, 16, 30, 1e-13, 1e-14, 1e-8
NOT_CONVERGED, NO_CERTIFICATE, BAD_INPUT = 1, 2, 4
# rows / columns of the two sub-systems inside A [12][12] and B [12][4] (FD_X_* / FD_U_* numbering)
LON_STATES, LON_CONTROLS = (3, 5, 10, 7), (0, 3)          # u, w, q, theta | elevator, throttle
LAT_STATES, LAT_CONTROLS = (4, 9, 11, 6), (1, 2)          # v, p, r, phi   | aileron, rudder
DELTA_STATES = LON_STATES + LAT_STATES                    # the eight regulated words, in K's column order
ANGLE_WORDS = (3, 7)                                      # positions of theta and phi in DELTA_STATES
DEFAULT_MAXIMA = (2.0, 2.0, 0.5, 0.1, 2.0, 1.0, 0.5, 0.2, 0.3, 0.3, 0.3, 0.3)


def default_weights():
    """Bryson's rule on the default maxima: 1 / max^2, q_lon(4) q_lat(4) r_lon(2) r_lat(2)."""
    m = np.array(DEFAULT_MAXIMA)
    return 1.0 / (m * m)


def mm(a, b):
    """a @ b with every element summed k = 0, 1, 2, ... in that order, one rounding per operation."""
    c = a[:, 0:1] * b[0:1, :]
    for k in range(1, a.shape[1]):
        c = c + a[:, k:k + 1] * b[k:k + 1, :]
    return c


def inv4(a):
    """Inverse: trim_numpy's elimination on [a | I] -> (inverse, ok)."""
    return gauss_solve(a, np.eye(4), PIVOT_REL)


def ldl_positive(x):
    """True when the symmetric 4 x 4 x has an L D L^T factorisation with every d > 0 (positive definite)."""
    L, d = np.zeros((4, 4)), np.zeros(4)
    ok = True
    for j in range(4):
        s = x[j, j]
        for k in range(j):
            s = s - L[j, k] * L[j, k] * d[k]
        d[j] = s
        ok = ok and bool(s > 0.0)
        for i in range(j + 1, 4):
            t = x[i, j]
            for k in range(j):
                t = t - L[i, k] * L[j, k] * d[k]
            L[i, j] = t / s
    return ok


def design_block(a, b, q, r):
    """One 4-state, 2-control block -> dict(K [2][4], X [4][4], residual, iters, status bits 1 | 2).  q [4], r [2] diagonal."""
    with np.errstate(all="ignore"):
        a, b, q, r = (np.array(v, np.float64) for v in (a, b, q, r))
        I = np.eye(4)
        bs = b * (1.0 / r)[None, :]                      # b R^-1
        G = mm(bs, b.T)
        gamma = max(1.0, float(np.max(np.sum(np.abs(a), axis=1))))
        ag = a - gamma * I
        agi, ok1 = inv4(ag)
        S1 = mm(agi, G)                                  # a_g^-1 G
        W = ag.T + q[:, None] * S1
        Wi, ok2 = inv4(W)
        g2 = 2.0 * gamma
        Ak = I + g2 * Wi.T
        Gk = g2 * mm(S1, Wi)
        Hk = g2 * mm(Wi, q[:, None] * agi)
        it, failed, converged = 0, not (ok1 and ok2), False
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
        X = 0.5 * (Hk + Hk.T)
        K = mm(bs.T, X)
        R = ((mm(a.T, X) + mm(X, a)) - mm(mm(X, G), X)) + np.diag(q)
        xmax = maxabs(X)
        res = maxabs(R) / (xmax if xmax > 1.0 else (1.0 if xmax == xmax else np.nan))
        status = 0
        if failed or not converged:
            status |= NOT_CONVERGED
        if not ldl_positive(X) or not res <= RES_MAX:
            status |= NO_CERTIFICATE
        return dict(K=K, X=X, residual=res, iters=it, status=status)


def blocks(A, B):
    """-> ((a_lon, b_lon), (a_lat, b_lat)) of A [12][12], B [12][4]."""
    A, B = np.asarray(A), np.asarray(B)
    return ((A[np.ix_(LON_STATES, LON_STATES)], B[np.ix_(LON_STATES, LON_CONTROLS)]),
            (A[np.ix_(LAT_STATES, LAT_STATES)], B[np.ix_(LAT_STATES, LAT_CONTROLS)]))


def _worse(a, b):
    """max with NaN winning."""
    return b if (b > a or b != b) else a


def design(A, B, weights):
    """One aircraft -> dict(K [16], residual, iters, status): what fdyn_lqr_design writes for a lane."""
    w = np.asarray(weights, np.float64)
    bl = blocks(A, B)
    with np.errstate(all="ignore"):
        finite = all(np.isfinite(a).all() and np.isfinite(b).all() for a, b in bl)
        if not (finite and np.isfinite(w).all() and (w > 0.0).all()):
            return dict(K=np.zeros(NLQK), residual=np.nan, iters=0, status=BAD_INPUT)
    K, res, it, st = np.zeros(NLQK), 0.0, 0, 0
    for k, (a, b) in enumerate(bl):
        r = design_block(a, b, w[4 * k:4 * k + 4], w[8 + 2 * k:10 + 2 * k])
        K[8 * k:8 * k + 8] = r["K"].reshape(8)
        res, it, st = _worse(res, r["residual"]), max(it, r["iters"]), st | r["status"]
    if st:
        K[:] = 0.0
    return dict(K=K, residual=res, iters=it, status=st)


def design_many(A, B, weights):
    """A [n][12][12], B [n][12][4], weights [12] or [n][12] -> dict of arrays K [n][16], residual, iters, status."""
    n = len(A)
    w = np.broadcast_to(np.asarray(weights, np.float64), (n, NLQW))
    rows = [design(A[i], B[i], w[i]) for i in range(n)]
    return dict(K=np.array([r["K"] for r in rows]), residual=np.array([r["residual"] for r in rows]),
                iters=np.array([r["iters"] for r in rows], np.int32), status=np.array([r["status"] for r in rows], np.int32))


def gain_matrix(K16):
    """K [16] -> the [4][12] feedback matrix on the full state, zeros outside the two blocks."""
    K = np.zeros((4, 12))
    K[np.ix_(LON_CONTROLS, LON_STATES)] = np.asarray(K16[:8]).reshape(2, 4)
    K[np.ix_(LAT_CONTROLS, LAT_STATES)] = np.asarray(K16[8:]).reshape(2, 4)
    return K


# ---- the closed loop -----------------------------------------------------------------------------------------------------------
def wrap_angle(a):
    """(a + pi) % (2 pi) - pi with floor-mod: [-pi, pi)."""
    return (a + np.pi) % (2.0 * np.pi) - np.pi


def delta(x, x0):
    """The eight regulated words of x - x0 (u, w, q, theta | v, p, r, phi), both angle differences wrapped."""
    d = np.array([x[s] - x0[s] for s in DELTA_STATES])
    for k in ANGLE_WORDS:
        d[k] = wrap_angle(d[k])
    return d


def controls(K16, x0, u0, x):
    """u = u0 - K delta, each row summed left to right -> (u unclipped [4] in FD_U_* order)."""
    d = delta(x, x0)
    u = np.array(u0, np.float64)
    for blk, ctl in enumerate((LON_CONTROLS, LAT_CONTROLS)):
        for j, c in enumerate(ctl):
            k = np.asarray(K16[8 * blk + 4 * j:8 * blk + 4 * j + 4])
            dd = d[4 * blk:4 * blk + 4]
            s = k[0] * dd[0]
            for m in range(1, 4):
                s = s + k[m] * dd[m]
            u[c] = u0[c] - s
    return u


def clip_controls(u):
    """set_controls' clip: surfaces to [-1, 1], throttle (word 3) to [0, 1] -> (clipped, any clipped)."""
    c = np.array([min(max(u[0], -1.0), 1.0), min(max(u[1], -1.0), 1.0), min(max(u[2], -1.0), 1.0), min(max(u[3], 0.0), 1.0)])
    return c, bool(np.any(c != u))


def fly(step, K16, x0, u0, x, dt, n_steps, record=None):
    """n_steps x {u = clip(u0 - K delta); x = step(x, u, dt)} -> (x, last clipped controls, steps with a clipped control).
    record: optional list that receives a copy of x after every step."""
    x = np.array(x, np.float64)
    u, sat = clip_controls(controls(K16, x0, u0, x))[0], 0
    for _ in range(n_steps):
        u, clipped = clip_controls(controls(K16, x0, u0, x))
        sat += int(clipped)
        x = step(x, u, dt)
        if record is not None:
            record.append(x.copy())
    return x, u, sat


def rk4_of(f):
    """A plain RK4 step over `f(x, u) -> xdot` (no state clamps), for closed loops over a model that has none."""
    def step(x, u, dt):
        k1 = f(x, u); k2 = f(x + 0.5 * dt * k1, u); k3 = f(x + 0.5 * dt * k2, u); k4 = f(x + dt * k3, u)
        return x + dt / 6.0 * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
    return step


# ---- what both test files fly ---------------------------------------------------------------------------------------------------
PERTURBATION = {3: 2.0, 4: 1.0, 5: -1.0, 6: 0.15, 7: 0.08, 9: 0.3, 10: -0.2, 11: 0.1}      # d(u, v, w, phi, theta, p, q, r)
# (airframe, V, climb (deg), turn rate)
CONDITIONS = (("rc_plane", 20.0, 0.0, 0.0), ("cessna", 25.0, 3.0, 0.0), ("rc_plane", 20.0, 0.0, 0.2), ("cessna", 18.0, 0.0, -0.3),
              ("rc_plane", 15.0, 0.0, 0.0))


def perturbed(x0):
    x = np.array(x0, np.float64)
    for k, v in PERTURBATION.items():
        x[k] += v
    return x


def deviation(x, x0):
    """max |delta|: the worst of the eight regulated words."""
    return float(np.max(np.abs(delta(x, x0))))


_FLIGHTS = {}
DT, STEPS_20S, STEPS_COMPARE = 0.01, 2000, 500
ALTITUDE, HEADING = 100.0, 0.3


def oracle_flights():
    """The five conditions on BOTH airframes (ten aircraft; the issue's own five pairings first) trimmed, linearised, designed
    with the default weights and flown from the perturbation over the CPU oracle's RK4 step, once per test session.  Read-only.
    Every aircraft: type, spec, x0, u0, A, B, K, status, x_start, x_500 (state after STEPS_COMPARE steps), u_500, sat_500.
    The first five also: dev (deviation at 5, 10, 20 s), sat (saturated steps of 2000), x_2000, open_dev (controls held at u0)."""
    if _FLIGHTS:
        return _FLIGHTS
    import trim_numpy as tn
    from oracle import oracle as orc
    listed = [(tn.TYPES.index(name), V, g, w) for name, V, g, w in CONDITIONS]
    others = [(1 - t, V, g, w) for t, V, g, w in listed]
    rows = []
    for k, (t, V, g, w) in enumerate(listed + others):
        f, grav, max_alpha, max_pitch, P = tn.oracle_airframe(tn.TYPES[t])
        spec = np.array([V, np.radians(g), w, ALTITUDE, HEADING])
        tr = tn.trim(f, spec, grav, max_alpha, max_pitch)
        assert tr["status"] == 0, (k, tr["status"])
        A, B = tn.linearize(f, tr["x0"], tr["u0"])
        d = design(A, B, default_weights())

        def step(x, u, dt, P=P):
            x = x.copy()
            orc.rk4_step(P, x, np.ascontiguousarray(u), dt)
            return x

        x_start = perturbed(tr["x0"])
        row = dict(type=t, spec=spec, x0=tr["x0"], u0=tr["u0"], A=A, B=B, K=d["K"], status=d["status"], x_start=x_start)
        full = k < len(listed)
        rec = []
        x, u, sat = fly(step, d["K"], tr["x0"], tr["u0"], x_start, DT, STEPS_COMPARE, rec)
        row["x_500"], row["u_500"], row["sat_500"] = x, u, sat
        if full:
            x, u, sat2 = fly(step, d["K"], tr["x0"], tr["u0"], x, DT, STEPS_20S - STEPS_COMPARE, rec)
            row["dev"] = tuple(deviation(rec[s - 1], tr["x0"]) for s in (500, 1000, 2000))
            row["sat"], row["x_2000"] = sat + sat2, x
            xo = x_start.copy()
            uo = clip_controls(tr["u0"])[0]
            for _ in range(STEPS_20S):
                xo = step(xo, uo, DT)
            row["open_dev"] = deviation(xo, tr["x0"])
        rows.append(row)
    keys = set(rows[0]) & set(rows[-1])
    _FLIGHTS["all"] = {k: np.array([r[k] for r in rows]) for k in keys}
    _FLIGHTS["listed"] = {k: np.array([r[k] for r in rows[:len(listed)]]) for k in rows[0]}
    for part in _FLIGHTS.values():
        for v in part.values():
            v.setflags(write=False)
    return _FLIGHTS

"""The predicted steady-state covariances of the LQ servo loop of include/fdyn_servo_covariance.h (fdyn_servo_covariance,
fdyn_stein_solve; csrc/fdyn_stein_n.hpp) restated on NumPy fp64: the same operations in the same order -- the Smith doubling for
X = A X B^T + Q, its residual, the three equations per block (estimation error, cross covariance, loop state), and the 34 report
words -- so that the host program and the kernel can be held to it bit for bit.  The loop matrices are
servo_modes_numpy.sampled_blocks' and filter_blocks', the ones the modes and margins reports speak of.  Shared by the CPU tests and
the GPU test; nothing here imports the product package.
"""
import numpy as np

import servo_lqg_numpy as sl
import servo_margin_numpy as sm
import servo_modes_numpy as smn
import servo_numpy as sn
from lqr_numpy import mm
from trim_numpy import maxabs

NB, NLON, NLAT = 5, 7, 6
NSCV, NSCC = 34, 200                                             # FD_NSCV, FD_NSCC
VAR_X, VAR_EST, VAR_ERR, VAR_INTEG, VAR_U, VAR_DU = 0, 10, 20, 23, 26, 30            # FD_SCV_VAR_*
CC_E, CC_XE, CC_X = (0, 25), (50, 85), (115, 164)                # FD_SCC_{E,XE,X}_{LON,LAT}
NOT_CONVERGED, UNSTABLE, BAD_INPUT = 1, 2, 4                     # FD_SCV_*
ESTIMATE, MEASUREMENT, TRUTH = sl.ESTIMATE, sl.MEASUREMENT, sl.TRUTH
FEEDBACKS = (ESTIMATE, MEASUREMENT, TRUTH)
MAX_DOUBLINGS, STEIN_TOL, RES_MAX = 40, 1e-17, 1e-9              # STEIN_MAX_DOUBLINGS, STEIN_TOL, STEIN_RES_MAX
MIN_N, MAX_N = 1, 7
DTS = smn.DTS
CONTROLS = ((0, 3), (1, 2))                                      # FD_U_* of (elevator, throttle | aileron, rudder)


# ---- the solver ------------------------------------------------------------------------------------------------------------------
def stein_doubling(A, B, Q, symmetric=False):
    """X = A X B^T + Q, A [N][N], B [M][M], Q [N][M] -> dict(X, residual, iters, converged, failed).  X_0 = Q, then
    D = (A_k X_k) B_k^T, X_{k+1} = X_k + D, A_{k+1} = A_k A_k, B_{k+1} = B_k B_k until max|D| <= STEIN_TOL max|X_{k+1}| or
    MAX_DOUBLINGS steps; failed when max|X| or max|D| stops being finite.  symmetric: B is A (squared once) and the result is
    (X + X^T) / 2.  residual = max|(A X) B^T + Q - X| / max|X| with the A, B, Q given, 0 when X is exactly 0, NaN when failed."""
    with np.errstate(all="ignore"):
        A, Q = np.array(A, np.float64), np.array(Q, np.float64)
        B = A if symmetric else np.array(B, np.float64)
        X, Ak, Bk = Q.copy(), A, B
        it, converged, failed = 0, False, False
        while not failed and not converged and it < MAX_DOUBLINGS:
            D = mm(mm(Ak, X), Bk.T)
            X = X + D
            Ak = mm(Ak, Ak)
            Bk = Ak if symmetric else mm(Bk, Bk)
            it += 1
            xmax, dmax = maxabs(X), maxabs(D)
            if not (np.isfinite(xmax) and np.isfinite(dmax)):
                failed = True
                break
            converged = bool(dmax <= STEIN_TOL * xmax)
        if symmetric:
            X = 0.5 * (X + X.T)
        R = (mm(mm(A, X), B.T) + Q) - X
        xmax = maxabs(X)
        res = np.nan if failed else (0.0 if xmax == 0.0 else maxabs(R) / xmax)
    return dict(X=X, residual=res, iters=it, converged=converged, failed=failed)


def stein_status(s):
    return 0 if (not s["failed"] and s["converged"] and s["residual"] <= RES_MAX) else NOT_CONVERGED


def stein_solve(A, B, Q):
    """What fdyn_stein_solve writes for one lane: dict(X [N][M], residual, iters, status); BAD_INPUT (nothing solved, X and residual
    NaN, iters 0) for a word that is not finite; a lane with a non-zero status has NaN in every word of X."""
    A, B, Q = (np.asarray(v, np.float64) for v in (A, B, Q))
    if not (np.isfinite(A).all() and np.isfinite(B).all() and np.isfinite(Q).all()):
        return dict(X=np.full(Q.shape, np.nan), residual=np.nan, iters=0, status=BAD_INPUT)
    s = stein_doubling(A, B, Q)
    st = stein_status(s)
    return dict(X=np.full(Q.shape, np.nan) if st else s["X"], residual=s["residual"], iters=s["iters"], status=st)


# ---- one block -------------------------------------------------------------------------------------------------------------------
def quad(a, S, b):
    """a^T S b: t_i = sum_j S_ij b_j, then sum_i a_i t_i, both left to right."""
    out = None
    for i in range(len(a)):
        t = S[i, 0] * b[0]
        for j in range(1, len(b)):
            t = t + S[i, j] * b[j]
        out = a[i] * t if out is None else out + a[i] * t
    return out


def dquad(a, d):
    """sum_k (a_k d_k) a_k, left to right."""
    out = (a[0] * d[0]) * a[0]
    for k in range(1, len(a)):
        out = out + (a[k] * d[k]) * a[k]
    return out


def vecmat(a, M, minus_identity=False):
    """(a^T M)_c = sum_r a_r (M_rc - [r == c]), left to right."""
    out = np.zeros(M.shape[1])
    for c in range(M.shape[1]):
        s = None
        for r in range(len(a)):
            m = M[r, c] - (1.0 if r == c else 0.0) if minus_identity else M[r, c]
            s = a[r] * m if s is None else s + a[r] * m
        out[c] = s
    return out


def block_covariance(blk, Acl, Ae, Kb, Gamma, L, Ci, v, w, feedback):
    """One block.  Acl [NA][NA], Ae [5][5], Kb [2][NA], Gamma [5][2], L [5][5], Ci [n_i][5] (without dt), v = sigma^2 [5],
    w = s^2 dt [5] -> dict(Se, Sxe, Sx, var_x, var_est, var_err, var_integ, var_u [2], var_du [2], residual, iters, status)."""
    with np.errstate(all="ignore"):
        NA = len(Acl)
        Kx = Kb[:, :NB]
        ImL = np.eye(NB) - L
        Bf = np.zeros((NA, NB))
        Bf[:NB] = -(Gamma[:, 0:1] * Kx[0:1, :] + Gamma[:, 1:2] * Kx[1:2, :])
        Bf[NB:] = Acl[NB:, :NB]
        # the estimation error: the estimator always runs
        Qe = mm(ImL * w[None, :], ImL.T) + mm(L * v[None, :], L.T)
        se = stein_doubling(Ae, None, Qe, symmetric=True)
        Se = se["X"]
        solves = [se]
        # what the law is fed beside the truth: n = f - d with covariance Nn; Sxe = E[xi e^T] is non-zero under the estimate only
        Sxe = np.zeros((NA, NB))
        if feedback == ESTIMATE:
            Qxe = -mm(mm(Bf, Se), Ae.T)
            Qxe[:NB] = w[:, None] * ImL.T + Qxe[:NB]
            sxe = stein_doubling(Acl, Ae, Qxe)
            Sxe = sxe["X"]
            solves.append(sxe)
            Nn = Se
        elif feedback == MEASUREMENT:
            Nn = np.diag(v)
        else:
            Nn = np.zeros((NB, NB))
        G = mm(mm(Acl, Sxe), Bf.T)
        H = mm(mm(Bf, Nn), Bf.T)
        Qx = (H - G) - G.T
        d = np.arange(NB)
        Qx[d, d] = Qx[d, d] + w
        sx = stein_doubling(Acl, None, Qx, symmetric=True)
        Sx = sx["X"]
        solves.append(sx)

        var_u, var_du = np.zeros(2), np.zeros(2)
        vw = v + w
        for a in range(2):
            kb, kx = Kb[a], Kx[a]
            var_u[a] = (quad(kb, Sx, kb) - 2.0 * quad(kb, Sxe, kx)) + quad(kx, Nn, kx)
            mx = -vecmat(kb, Acl, minus_identity=True)
            kbf = vecmat(kb, Bf)
            q = quad(mx, Sx, mx)
            if feedback == ESTIMATE:
                me = kbf + vecmat(kx, Ae, minus_identity=True)
                kl = vecmat(kx, L)
                var_du[a] = ((q + 2.0 * quad(mx, Sxe, me)) + quad(me, Se, me)) + dquad(kl, vw)
            elif feedback == MEASUREMENT:
                var_du[a] = ((q + dquad(kx - kbf, v)) + dquad(kx, v)) + dquad(kx, w)
            else:
                var_du[a] = q + dquad(kx, w)
        Sd = Sx[:NB, :NB]
        status = 0
        for s in solves:
            status |= stein_status(s)
        return dict(Se=Se, Sxe=Sxe, Sx=Sx, var_x=np.diag(Sx)[:NB].copy(), var_est=np.diag(Se).copy(),
                    var_err=np.array([quad(c, Sd, c) for c in Ci]), var_integ=np.diag(Sx)[NB:].copy(), var_u=var_u, var_du=var_du,
                    residual=[s["residual"] for s in solves], iters=max(s["iters"] for s in solves), status=status)


def _worse(a, b):
    """nan_max: the larger, NaN wins and stays."""
    return b if (b > a or b != b) else a


def servo_covariance(K26, F120, x0, dt, sigma, w_rate, feedback):
    """One aircraft: what fdyn_servo_covariance writes for a lane -> dict(report [34], cov [200], residual, iters, status).
    w_rate None = no process noise."""
    K26, F120, x0, sigma = (np.asarray(v, np.float64) for v in (K26, F120, x0, sigma))
    rate = np.zeros(sl.NSKX) if w_rate is None else np.asarray(w_rate, np.float64)
    nan = dict(report=np.full(NSCV, np.nan), cov=np.full(NSCC, np.nan), residual=np.nan, iters=0)
    with np.errstate(all="ignore"):
        cu, cw, ok = smn._directions(x0)
        ok = ok and bool(dt > 1e-6) and not dt > 1.0
        ok = ok and bool(np.isfinite(K26).all() and np.isfinite(F120).all())
        ok = ok and bool(np.isfinite(sigma).all() and (sigma >= 0.0).all() and np.isfinite(rate).all() and (rate >= 0.0).all())
        if not ok:
            return dict(nan, status=BAD_INPUT)
        loops, filt = smn.sampled_blocks(K26, F120, x0, dt), smn.filter_blocks(F120)
        if any(m is None for m in loops) or any(m is None for m in filt):
            return dict(nan, status=BAD_INPUT)
        for m in (*loops, *filt):
            if not bool(sm.schur_by_squaring(m[:, :, None])[0][0]):
                return dict(nan, status=UNSTABLE)
        report, cov, res, it, st = np.zeros(NSCV), np.zeros(NSCC), 0.0, 0, 0
        for blk, (NA, at) in enumerate(((NLON, 0), (NLAT, 14))):
            _, Gamma, L = sl.matrices(F120)[blk]
            sg, rt = sigma[NB * blk:NB * blk + NB], rate[NB * blk:NB * blk + NB]
            b = block_covariance(blk, loops[blk], filt[blk], K26[at:at + 2 * NA].reshape(2, NA), Gamma, L,
                                 smn.integrator_rows(blk, cu, cw), sg * sg, (rt * rt) * dt, feedback)
            report[VAR_X + NB * blk:VAR_X + NB * blk + NB] = b["var_x"]
            report[VAR_EST + NB * blk:VAR_EST + NB * blk + NB] = b["var_est"]
            ne, ni = (0, 2) if blk == 0 else (2, 1)
            report[VAR_ERR + ne:VAR_ERR + ne + ni] = b["var_err"]
            report[VAR_INTEG + ne:VAR_INTEG + ne + ni] = b["var_integ"]
            for a, c in enumerate(CONTROLS[blk]):
                report[VAR_U + c], report[VAR_DU + c] = b["var_u"][a], b["var_du"][a]
            cov[CC_E[blk]:CC_E[blk] + NB * NB] = b["Se"].reshape(-1)
            cov[CC_XE[blk]:CC_XE[blk] + NA * NB] = b["Sxe"].reshape(-1)
            cov[CC_X[blk]:CC_X[blk] + NA * NA] = b["Sx"].reshape(-1)
            for r in b["residual"]:
                res = _worse(res, r)
            it, st = max(it, b["iters"]), st | b["status"]
        if st:
            return dict(report=nan["report"], cov=nan["cov"], residual=res, iters=it, status=st)
        return dict(report=report, cov=cov, residual=res, iters=it, status=0)


def servo_covariance_many(K, F, x0, dt, sigma, w_rate, feedback):
    """K [n][26], F [n][120], x0 [n][12]; sigma [10] or [n][10]; w_rate None, [10] or [n][10] -> dict of arrays, lane-major."""
    n = len(K)
    sg = np.broadcast_to(np.asarray(sigma, np.float64), (n, sl.NSKX))
    wr = None if w_rate is None else np.broadcast_to(np.asarray(w_rate, np.float64), (n, sl.NSKX))
    rows = [servo_covariance(K[i], F[i], x0[i], dt, sg[i], None if wr is None else wr[i], feedback) for i in range(n)]
    return dict(report=np.array([r["report"] for r in rows]), cov=np.array([r["cov"] for r in rows]),
                residual=np.array([r["residual"] for r in rows]), iters=np.array([r["iters"] for r in rows], np.int32),
                status=np.array([r["status"] for r in rows], np.int32))


# ---- what the test files share -------------------------------------------------------------------------------------------------
_CACHE = {}


def golden_reports(golden, with_w=False):
    """The restatement on the 288 golden designs (servo_margin_numpy.golden_designs) at the default sigma: {(dt, feedback): dict of
    arrays}; with_w: the design's own rates acting as process noise.  Once per session, read-only."""
    key = ("reports", with_w)
    if key not in _CACHE:
        d = sm.golden_designs(golden)
        rates = sl.DEFAULT_RATES if with_w else None
        out = {(dt, fb): servo_covariance_many(d["K"], d["F"][dt], d["x0"], dt, sl.DEFAULT_SIGMA, rates, fb) for dt in DTS for fb in FEEDBACKS}
        for rep in out.values():
            for v in rep.values():
                v.setflags(write=False)
        _CACHE[key] = out
    return _CACHE[key]


def stein_cases(rng_seed=7):
    """(N, M) -> (A [N][N], B [M][M], Q [N][M]) with spectral radii below 1: what the fdyn_stein_solve tests solve."""
    rs = np.random.RandomState(rng_seed)
    out = {}
    for N, M in ((1, 1), (2, 7), (5, 5), (7, 5), (7, 7)):
        A, B = rs.standard_normal((N, N)), rs.standard_normal((M, M))
        A *= 0.9 / max(abs(np.linalg.eigvals(A)))
        B *= 0.7 / max(abs(np.linalg.eigvals(B)))
        out[N, M] = (A, B, rs.standard_normal((N, M)))
    return out


def cap_case():
    """A 2 x 2 with spectral radius 1 - 1e-13: the increments stay far above STEIN_TOL for MAX_DOUBLINGS doublings and the words stay
    finite, so the lane ends at the cap."""
    r = 1.0 - 1e-13
    return np.array([[r, 0.5], [0.0, 0.5]]), np.array([[r, 0.0], [0.25, 0.5]]), np.array([[1.0, 0.5], [0.5, 2.0]])

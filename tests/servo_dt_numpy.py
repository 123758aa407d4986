"""The sampled-data design of the LQ servo of include/fdyn_servo_dt.h (fdyn_servo_design_dt, csrc/fdyn_servo_dt.hpp) restated in NumPy
fp64, operation for operation: servo_lqg_numpy's discretisation of the five physical states, the sampled model with its Euler
integrators, servo_numpy's doubling loop started at (A_d, B_d R_d^-1 B_d^T, Q dt), the closed-form 2 x 2 inverse, the gain, the
residual of the discrete Riccati equation, the L D L^T test and servo_margin_numpy's squaring certificate on A_d - B_d K.  Shared by
the CPU tests and the GPU test; nothing here imports the product package.
"""
import numpy as np

import servo_lqg_numpy as sl
import servo_margin_numpy as sm
import servo_numpy as sn
from lqr_numpy import mm
from trim_numpy import maxabs

NB = sl.NB
NOT_CONVERGED, NO_CERTIFICATE, BAD_INPUT = sn.NOT_CONVERGED, sn.NO_CERTIFICATE, sn.BAD_INPUT
DTS = (0.01, 0.02)                                               # the gated steps


def sampled_model(Phi, Gamma, ci, dt):
    """-> (A_d [N][N], B_d [N][2]) = [[Phi, 0], [dt C_i, I]], [[Gamma], [0]]; ci [n_i][5] the integrator rows."""
    N = NB + len(ci)
    Ad, Bd = np.zeros((N, N)), np.zeros((N, 2))
    Ad[:NB, :NB], Ad[NB:, :NB], Ad[NB:, NB:] = Phi, dt * np.asarray(ci, np.float64), np.eye(N - NB)
    Bd[:NB] = Gamma
    return Ad, Bd


def dare_solve(Ad, Bd, q, r, dt):
    """One sampled N-state, 2-control block -> dict(K [2][N], X [N][N], residual, iters, failed, converged, positive, gain_ok,
    stable, status bits 1 | 2).  q [N], r [2] the continuous weights.  csrc/fdyn_servo_dt.hpp's dare_solve, operation for operation."""
    with np.errstate(all="ignore"):
        Ad, Bd, q, r = (np.array(v, np.float64) for v in (Ad, Bd, q, r))
        d = np.arange(len(Ad))
        h, rd = q * dt, r * dt
        rdi = 1.0 / rd
        bs = Bd * rdi[None, :]
        _, _, H, it, failed, converged = sn.doubling(Ad.copy(), mm(bs, Bd.T), np.diag(h))
        X = 0.5 * (H + H.T)
        XB = mm(X, Bd)
        S = mm(Bd.T, XB)
        S[0, 0], S[1, 1] = rd[0] + S[0, 0], rd[1] + S[1, 1]
        det = S[0, 0] * S[1, 1] - S[0, 1] * S[1, 0]
        gain_ok = bool(S[0, 0] > 0.0) and bool(det > 0.0)
        Si = np.array([[S[1, 1] / det, -S[0, 1] / det], [-S[1, 0] / det, S[0, 0] / det]])
        XA = mm(X, Ad)
        K = mm(Si, mm(Bd.T, XA))
        E = mm(Ad.T, XA) - mm(mm(Ad.T, XB), K)
        E[d, d] = E[d, d] + h
        xmax = maxabs(X)
        res = maxabs(X - E) / (xmax if xmax > 1.0 else (1.0 if xmax == xmax else np.nan))
        positive = sn.ldl_positive(X)
        stable = bool(sm.schur_by_squaring((Ad - mm(Bd, K))[:, :, None])[0][0])
        status = 0
        if failed or not converged:
            status |= NOT_CONVERGED
        if not positive or not res <= sn.RES_MAX or not gain_ok or not stable:
            status |= NO_CERTIFICATE
        return dict(K=K, X=X, residual=res, iters=it, failed=failed, converged=converged, positive=positive, gain_ok=gain_ok,
                    stable=stable, status=status)


def integrator_rows(x0):
    """(C_i lon [2][5], C_i lat [1][5]): the integrator rows of servo_numpy.augmented_blocks at the trim x0."""
    (a_lon, _), (a_lat, _) = sn.augmented_blocks(np.zeros((12, 12)), np.zeros((12, 4)), x0)
    return a_lon[NB:, :NB], a_lat[NB:, :NB]


def design(A, B, x0, weights, dt, keep_x=False):
    """One aircraft -> dict(K [26], residual, iters, status): what fdyn_servo_design_dt writes for a lane."""
    w = np.asarray(weights, np.float64)
    A, B, x0 = np.asarray(A, np.float64), np.asarray(B, np.float64), np.asarray(x0, np.float64)
    bl = sl.blocks(A, B)
    with np.errstate(all="ignore"):
        ok = bool(dt > 1e-6) and not dt > 1.0 and bool(np.isfinite(w).all()) and bool((w > 0.0).all())
        V0 = np.sqrt(x0[sn.X_U] * x0[sn.X_U] + x0[sn.X_W] * x0[sn.X_W])
        ok = ok and bool(np.isfinite(x0[sn.X_U])) and bool(np.isfinite(x0[sn.X_W])) and bool(V0 > 0.0)
        ok = ok and all(np.isfinite(a).all() and np.isfinite(b).all() for a, b in bl)
        ok = ok and all(sl.row_norm(a) * dt <= sl.NORM_MAX for a, _ in bl)
    if not ok:
        return dict(K=np.zeros(sn.NSVK), residual=np.nan, iters=0, status=BAD_INPUT)
    K, res, it, st, xs, at = np.zeros(sn.NSVK), 0.0, 0, 0, [], 0
    for (a, b), ci, (q, r) in zip(bl, integrator_rows(x0), sn.block_weights(w)):
        with np.errstate(all="ignore"):
            Phi, Gamma = sl.discretise(np.array(a, np.float64), np.array(b, np.float64), dt)
        c = dare_solve(*sampled_model(Phi, Gamma, ci, dt), q, r, dt)
        N = NB + len(ci)
        K[at:at + 2 * N] = c["K"].reshape(-1)
        at += 2 * N
        res, it, st = sn._worse(res, c["residual"]), max(it, c["iters"]), st | c["status"]
        xs.append(c["X"])
    if st:
        K[:] = 0.0
    out = dict(K=K, residual=res, iters=it, status=st)
    if keep_x:
        out["X"] = xs
    return out


def design_many(A, B, x0, weights, dt):
    """A [n][12][12], B [n][12][4], x0 [n][12], weights [17] or [n][17] -> dict of arrays K [n][26], residual, iters, status."""
    n = len(A)
    w = np.broadcast_to(np.asarray(weights, np.float64), (n, sn.NSVW))
    rows = [design(A[i], B[i], x0[i], w[i], dt) for i in range(n)]
    return dict(K=np.array([r["K"] for r in rows]), residual=np.array([r["residual"] for r in rows]),
                iters=np.array([r["iters"] for r in rows], np.int32), status=np.array([r["status"] for r in rows], np.int32))


_CACHE = {}


def golden_designs(golden, dt):
    """The restatement on the 288 linearisations of tests/golden/trim_reference.npz with the default weights at dt, once per session."""
    if dt not in _CACHE:
        out = design_many(golden["A"], golden["B"], golden["x0"], sn.default_weights(), dt)
        for v in out.values():
            v.setflags(write=False)
        _CACHE[dt] = out
    return _CACHE[dt]


# ---- the gates both the CPU test and the GPU test apply to margins ---------------------------------------------------------------
# Measured with this restatement on the 288 golden aircraft under truth feedback, default 64-point grid (tests/test_servo_dt_oracle.py
# prints them): the worst per-aircraft alpha_s(sampled) / alpha_s(continuous) over both blocks, per dt; the fleet-worst alpha_s at
# dt 0.02 of the continuous and of the sampled design.  The gates are geometric means, by the project's convention: of the worst
# ratio and 1 (it is above 1 on every aircraft at both dt), and of the two fleet-worst margins.
RATIO_MEASURED = {0.01: 1.00471, 0.02: 1.01988}
WORST_MEASURED = (0.0710, 0.5862)


def ratio_gate(dt):
    return float(np.sqrt(RATIO_MEASURED[dt] * 1.0))


def worst_gate():
    return float(np.sqrt(WORST_MEASURED[0] * WORST_MEASURED[1]))


def margin_gates(cont, samp):
    """alpha_s [288][2] of the continuous and of the sampled gain at one dt -> (worst per-aircraft ratio per block [2], the fleet-
    worst alpha_s of the continuous design, of the sampled design)."""
    ratio = samp / cont
    return ratio.min(axis=0), float(cont.min()), float(samp.min())

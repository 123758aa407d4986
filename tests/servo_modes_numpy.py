"""The servo's flight-mode report of include/fdyn_servo_modes.h (fdyn_servo_flight_modes, fdyn_servo_sampled_modes,
fdyn_servo_filter_modes, fdyn_square_modes; csrc/fdyn_eig_n.hpp) restated on NumPy fp64 scalars: the same operations in the same
order -- Householder reduction to Hessenberg form at size N, Francis double-shift sweeps over the active window [l, en], 2 x 2
blocks by modes_numpy.eig2, the eigenvalues written back into the matrix, the odd-even transposition network, the summary words,
and the three compositions -- so that the host program and the kernel can be held to it bit for bit.  Shared by the CPU tests and
the GPU test; nothing here imports the product package.
"""
import numpy as np

import modes_numpy as mo
import servo_lqg_numpy as sl
import servo_numpy as sn
from lqr_numpy import mm
from modes_numpy import MAX_SWEEPS, EPS, NOT_CONVERGED, BAD_INPUT, NMO, F, ZERO, eig2

NLON, NLAT, NB, NEIG, NFILTER = 7, 6, 5, 13, 10                  # FD_SV_NLON, FD_SV_NLAT, FD_SK_NB, FD_NSMO_EIG, FD_NSMO_FILTER_EIG
SMO_LON, SMO_LAT, SMO_FILTER_LON, SMO_FILTER_LAT, MIN_N, MAX_N = 0, 7, 0, 5, 2, 7
DTS = (0.01, 0.02)
ONE = F(1.0)


def hessenberg(a):
    """In place on a list of N lists of fp64 scalars: modes_numpy.hessenberg4 at size N."""
    N = len(a)
    for k in range(N - 2):
        m = k + 1
        below = abs(a[m + 1][k])
        for i in range(m + 2, N):
            below = below + abs(a[i][k])
        if below != 0.0:
            scale = abs(a[m][k]) + below
            o = [None] * N
            for i in range(m, N):
                o[i] = a[i][k] / scale
            h = o[m] * o[m]
            for i in range(m + 1, N):
                h = h + o[i] * o[i]
            rt = np.sqrt(h)
            g = -rt if o[m] >= 0.0 else rt
            h = h - o[m] * g
            o[m] = o[m] - g
            for j in range(m, N):
                f = o[m] * a[m][j]
                for i in range(m + 1, N):
                    f = f + o[i] * a[i][j]
                f = f / h
                for i in range(m, N):
                    a[i][j] = a[i][j] - f * o[i]
            for i in range(N):
                f = o[m] * a[i][m]
                for j in range(m + 1, N):
                    f = f + o[j] * a[i][j]
                f = f / h
                for j in range(m, N):
                    a[i][j] = a[i][j] - f * o[j]
            a[m][k] = scale * g
            for i in range(m + 1, N):
                a[i][k] = ZERO


def francis_window(h, l, en, its):
    """One double-shift sweep over rows and columns l .. en, en - l >= 2: modes_numpy.francis_step with 0 -> l, N - 1 -> en."""
    x, y, w = h[en][en], h[en - 1][en - 1], h[en][en - 1] * h[en - 1][en]
    if its == 10:
        s = abs(h[l + 1][l]) + abs(h[l + 2][l + 1])
        x = F(0.75) * s + h[l][l]; y = x; w = F(-0.4375) * s * s
    elif its == 20:
        s = abs(h[en][en - 1]) + abs(h[en - 1][en - 2])
        x = F(0.75) * s + h[en][en]; y = x; w = F(-0.4375) * s * s
    z = h[l][l]
    r, s = x - z, y - z
    p = (r * s - w) / h[l + 1][l] + h[l][l + 1]
    q = ((h[l + 1][l + 1] - z) - r) - s
    r = h[l + 2][l + 1]
    s = (abs(p) + abs(q)) + abs(r)
    p, q, r = p / s, q / s, r / s
    for k in range(l, en):
        last = k == en - 1
        sc = ZERO
        if k != l:
            p, q = h[k][k - 1], h[k + 1][k - 1]
            sc = abs(p) + abs(q)
            if not last:
                r = h[k + 2][k - 1]
                sc = sc + abs(r)
            if sc != 0.0:
                p, q = p / sc, q / sc
                if not last:
                    r = r / sc
        nn = p * p + q * q
        if not last:
            nn = nn + r * r
        rt = np.sqrt(nn)
        s = rt if p >= 0.0 else -rt
        if s != 0.0:
            if k != l:
                h[k][k - 1] = -s * sc
            p = p + s
            x, y = p / s, q / s
            q = q / p
            if not last:
                z = r / s
                r = r / p
            for j in range(k, en + 1):
                t = h[k][j] + q * h[k + 1][j]
                if not last:
                    t = t + r * h[k + 2][j]
                    h[k + 2][j] = h[k + 2][j] - t * z
                h[k + 1][j] = h[k + 1][j] - t * y
                h[k][j] = h[k][j] - t * x
            for i in range(l, min(k + 3, en) + 1):
                t = x * h[i][k] + y * h[i][k + 1]
                if not last:
                    t = t + z * h[i][k + 2]
                    h[i][k + 2] = h[i][k + 2] - t * r
                h[i][k + 1] = h[i][k + 1] - t * q
                h[i][k] = h[i][k] - t
        if k != l:
            h[k + 1][k - 1] = ZERO
            if not last:
                h[k + 2][k - 1] = ZERO


def eig_n(m, trace=None):
    """One finite N x N, 2 <= N <= 7 -> (re [N], im [N], sweeps, ok) in canonical order; all NaN when not ok.  trace: an optional
    list that receives the sweeps of every deflation."""
    with np.errstate(all="ignore"):
        h = mo._rows(m)
        N = len(h)
        hessenberg(h)
        norm = ZERO
        for i in range(N):
            for j in range(max(i - 1, 0), N):
                norm = norm + abs(h[i][j])
        failed = not np.isfinite(norm)
        sweeps, en, its = 0, N - 1, 0
        while not failed and en >= 0:
            l, t = 0, ZERO
            for k in range(1, en + 1):
                sub = abs(h[k][k - 1])
                s = abs(h[k - 1][k - 1]) + abs(h[k][k])
                s = norm if s == 0.0 else s
                if sub <= EPS * s:
                    l = k
                t = t + sub
            if l == en:
                h[en][en - 1 if en != 0 else N - 1] = ZERO
                if trace is not None:
                    trace.append(its)
                en, its = en - 1, 0
            elif l == en - 1:
                (re0, im0), (re1, im1) = eig2(h[l][l], h[l][en], h[en][l], h[en][en])
                h[l][l], h[en][en] = re0, re1
                h[en][l] = im1
                h[l][l - 1 if l != 0 else N - 1] = im0
                if trace is not None:
                    trace.append(its)
                en, its = en - 2, 0
            elif its == MAX_SWEEPS or not np.isfinite(t):
                failed = True
                if trace is not None:
                    trace.append(its)
            else:
                francis_window(h, l, en, its)
                its += 1
                sweeps += 1
        re = [h[k][k] for k in range(N)]
        im = [h[k][k - 1 if k != 0 else N - 1] for k in range(N)]
        for rnd in range(N):
            for i in range(rnd % 2, N - 1, 2):
                j = i + 1
                mi, mj = abs(im[i]), abs(im[j])
                if re[j] > re[i] or (re[j] == re[i] and (mj > mi or (mj == mi and im[j] > im[i]))):
                    re[i], re[j], im[i], im[j] = re[j], re[i], im[j], im[i]
        re, im = np.array(re, np.float64), np.array(im, np.float64)
        ok = (not failed) and bool(np.isfinite(re).all() and np.isfinite(im).all())
        if not ok:
            re, im = np.full(N, np.nan), np.full(N, np.nan)
        return re, im, sweeps, ok


def summary(re, im):
    """The six FD_MO_* words of N eigenvalues (modes_numpy.summary at size N)."""
    with np.errstate(all="ignore"):
        absc, rad, mn, zeta, nu, nc = F(re[0]), ZERO, ZERO, ZERO, ZERO, ZERO
        for k in range(len(re)):
            rk, ik = F(re[k]), F(im[k])
            m = np.sqrt(rk * rk + ik * ik)
            z = ZERO if m == 0.0 else -rk / m
            absc = rk if rk > absc else absc
            rad = m if (k == 0 or m > rad) else rad
            mn = m if (k == 0 or m < mn) else mn
            zeta = z if (k == 0 or z < zeta) else zeta
            nu = nu + ONE if rk > 0.0 else nu
            nc = nc + ONE if ik != 0.0 else nc
        return np.array([absc, rad, mn, zeta, nu, nc], np.float64)


def blocks_modes(blocks):
    """blocks: per lane a list of square matrices (or None = a block that cannot be composed) -> dict(re [n][sum N], im, summary
    [n][blocks][6], iters [n], status [n]): what every entry point writes, lane-major, the blocks' eigenvalues one after the other."""
    n, sizes = len(blocks), [len(b) for b in blocks[0]]
    out = dict(re=np.full((n, sum(sizes)), np.nan), im=np.full((n, sum(sizes)), np.nan), summary=np.full((n, len(sizes), NMO), np.nan),
               iters=np.zeros(n, np.int32), status=np.zeros(n, np.int32))
    for i, lane in enumerate(blocks):
        if any(b is None or not np.isfinite(b).all() for b in lane):
            out["status"][i] = BAD_INPUT
            continue
        good, it, at = True, 0, 0
        for b, M in enumerate(lane):
            re, im, sweeps, ok = eig_n(np.asarray(M, np.float64) + 0.0)              # -0 enters as +0
            good, it = good and ok, max(it, sweeps)
            out["re"][i, at:at + len(M)], out["im"][i, at:at + len(M)], out["summary"][i, b] = re, im, summary(re, im)
            at += len(M)
        out["iters"][i] = it
        if not good:
            out["status"][i] = NOT_CONVERGED
            out["re"][i], out["im"][i], out["summary"][i] = np.nan, np.nan, np.nan
    return out


def square_modes(M):
    """M [n][N][N] -> what fdyn_square_modes writes (summary [n][1][6])."""
    return blocks_modes([[np.asarray(m, np.float64)] for m in M])


# ---- the three compositions ------------------------------------------------------------------------------------------------------
def _directions(x0):
    u0, w0 = F(x0[sn.X_U]), F(x0[sn.X_W])
    V0 = np.sqrt(u0 * u0 + w0 * w0)
    ok = bool(np.isfinite(u0) and np.isfinite(w0) and V0 > 0.0)
    return u0 / V0, w0 / V0, ok


def integrator_rows(blk, cu, cw):
    """C_i [n_i][5] of block blk."""
    if blk:
        return np.array([[0.0, 0.0, 0.0, 0.0, 1.0]])
    return np.array([[cu, cw, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0, -1.0]])


def continuous_blocks(A, B, x0, K26):
    """One aircraft -> [m_lon [7][7], m_lat [6][6]] or None entries: rows 0-4 a - (b_0 k_0 + b_1 k_1) with a = 0.0 in the integrator
    columns, then the integrator rows; None where a word that is read is not finite or V0 is not > 0."""
    A, B, K26 = np.asarray(A, np.float64), np.asarray(B, np.float64), np.asarray(K26, np.float64)
    with np.errstate(all="ignore"):
        cu, cw, ok = _directions(x0)
        out = []
        for blk, (st, ct, NA, at) in enumerate(((sn.LON_STATES, sn.LON_CONTROLS, NLON, 0), (sn.LAT_STATES, sn.LAT_CONTROLS, NLAT, 14))):
            a, b = np.zeros((NB, NA)), B[np.ix_(st, ct)]
            a[:, :NB] = A[np.ix_(st, st)]
            k = K26[at:at + 2 * NA].reshape(2, NA)
            m = np.zeros((NA, NA))
            m[:NB] = a - (b[:, 0:1] * k[0:1, :] + b[:, 1:2] * k[1:2, :])
            m[NB:, :NB] = integrator_rows(blk, cu, cw)
            good = ok and np.isfinite(b).all() and np.isfinite(k).all() and np.isfinite(m).all()
            out.append(m if good else None)
        return out


def sampled_blocks(K26, F120, x0, dt):
    """One aircraft -> [[Phi - Gamma Kx, -Gamma Ki], [dt C_i, I]] of both blocks (7 x 7, 6 x 6), every element as
    servo_margin_numpy.block_setup forms its `aug`; None entries for a word read that is not finite, V0 not > 0 or a bad dt."""
    K26, F120 = np.asarray(K26, np.float64), np.asarray(F120, np.float64)
    with np.errstate(all="ignore"):
        cu, cw, ok = _directions(x0)
        ok = ok and bool(dt > 1e-6) and not dt > 1.0
        out = []
        for blk, (NA, at) in enumerate(((NLON, 0), (NLAT, 14))):
            Phi, Gamma, _ = sl.matrices(F120)[blk]
            k = K26[at:at + 2 * NA].reshape(2, NA)
            m = np.zeros((NA, NA))
            m[:NB, :NB] = Phi - (Gamma[:, 0:1] * k[0:1, :NB] + Gamma[:, 1:2] * k[1:2, :NB])
            m[:NB, NB:] = -(Gamma[:, 0:1] * k[0:1, NB:] + Gamma[:, 1:2] * k[1:2, NB:])
            m[NB:, :NB] = F(dt) * integrator_rows(blk, cu, cw)
            m[NB:, NB:] = np.eye(NA - NB)
            good = ok and np.isfinite(Phi).all() and np.isfinite(Gamma).all() and np.isfinite(k).all() and np.isfinite(m).all()
            out.append(m if good else None)
        return out


def filter_blocks(F120):
    """One aircraft -> [(I - L) Phi of the longitudinal block, of the lateral block], each product summed k = 0 .. 4 in that order."""
    with np.errstate(all="ignore"):
        out = []
        for Phi, _, L in sl.matrices(np.asarray(F120, np.float64)):
            m = mm(np.eye(NB) - L, Phi)
            out.append(m if (np.isfinite(Phi).all() and np.isfinite(L).all() and np.isfinite(m).all()) else None)
        return out


def _sized(lanes, sizes):
    """None entries need a size for blocks_modes' bookkeeping: a NaN matrix of the block's size is refused the same way."""
    return [[np.full((s, s), np.nan) if b is None else b for b, s in zip(lane, sizes)] for lane in lanes]


def servo_flight_modes(A, B, x0, K):
    """A [n][12][12], B [n][12][4], x0 [n][12], K [n][26] -> what fdyn_servo_flight_modes writes."""
    return blocks_modes(_sized([continuous_blocks(A[i], B[i], x0[i], K[i]) for i in range(len(A))], (NLON, NLAT)))


def servo_sampled_modes(K, F120, x0, dt):
    return blocks_modes(_sized([sampled_blocks(K[i], F120[i], x0[i], dt) for i in range(len(K))], (NLON, NLAT)))


def servo_filter_modes(F120):
    return blocks_modes(_sized([filter_blocks(f) for f in F120], (NB, NB)))


# ---- the gates of the oracle test (and of the GPU test's fleet check) -----------------------------------------------------------
def assignment_gap(got, ref):
    """The smallest over all matchings of max |got_p(k) - ref_k| between two multisets of N <= 12 complex numbers: a minimum-cost
    (bottleneck) assignment, not a comparison by sorted position.  Threshold search over the N^2 distances with a bipartite matching."""
    got, ref = np.asarray(got, complex), np.asarray(ref, complex)
    n = len(got)
    D = np.abs(got[:, None] - ref[None, :])

    def feasible(t):
        match = [-1] * n

        def augment(i, seen):
            for j in range(n):
                if D[i, j] <= t and not seen[j]:
                    seen[j] = True
                    if match[j] < 0 or augment(match[j], seen):
                        match[j] = i
                        return True
            return False
        return all(augment(i, [False] * n) for i in range(n))
    for t in np.unique(D):
        if feasible(t):
            return float(t)
    raise AssertionError("no matching")


def bauer_fike(M):
    """-> (LAPACK's eigenvalues, kappa_2(V) |M|_2, |M|_2) of one matrix."""
    lam, V = np.linalg.eig(np.asarray(M, np.float64))
    nrm = float(np.linalg.norm(M, 2))
    return lam, float(np.linalg.cond(V)) * nrm, nrm


# ---- what the test files share ---------------------------------------------------------------------------------------------------
def cyclic(w):
    """The weighted cyclic N x N with subdiagonal w[1:] and corner w[0]: its standard shifts are zero and change nothing."""
    k = len(w)
    c = np.zeros((k, k))
    c[0, k - 1] = w[0]
    for i in range(1, k):
        c[i, i - 1] = w[i]
    return c


def companion(roots):
    """The companion matrix (first row) of prod (x - r)."""
    N = len(roots)
    c = np.zeros((N, N))
    c[0] = -np.real(np.poly(roots))[1:]
    for i in range(1, N):
        c[i, i - 1] = 1.0
    return c


KNOWN_ROOTS = {2: (-1.0, -3.0), 3: (-0.5, -1.0 + 2.0j, -1.0 - 2.0j), 4: (-0.2 + 3.0j, -0.2 - 3.0j, -2.0 + 1.0j, -2.0 - 1.0j),
               5: (-0.5, -1.0, -2.0, -4.0, -8.0), 6: (-0.1 + 1.0j, -0.1 - 1.0j, -1.0 + 0.5j, -1.0 - 0.5j, -3.0, 0.25),
               7: (-0.3, -0.6 + 2.0j, -0.6 - 2.0j, -1.5 + 1.5j, -1.5 - 1.5j, -5.0, 0.125)}


def degenerate_cases(N):
    """(name, m [N][N]): the ends of the solver at size N -- no reflector to build, nothing to sweep, exact zeros on the subdiagonal,
    ties in the canonical order, entries at both ends of the exponent range, and words that are not finite."""
    rs = np.random.RandomState(100 + N)
    idx = np.arange(1.0, N * N + 1.0).reshape(N, N)
    tri = np.triu(idx * np.where(np.arange(N) % 2 == 0, 1.0, -0.5)[:, None])
    hess = np.triu(rs.uniform(-2.0, 2.0, (N, N)), -1)
    split = hess.copy()
    if N > 2:
        split[N // 2, N // 2 - 1] = 0.0
    jordan = np.diag(np.full(N, -1.5)) + np.diag(np.ones(N - 1), 1)
    tied = np.diag([(-1.0, 0.5, -1.0, 0.5, 2.0, 2.0, -1.0)[k] for k in range(N)])
    line = np.zeros((N, N))                                      # rotations and a real pole that share ONE real part: the tie rule
    for k in range(0, N - 1, 2):
        w = 1.0 + k
        line[k:k + 2, k:k + 2] = [[-1.0, w], [-w, -1.0]]
    if N % 2:
        line[N - 1, N - 1] = -1.0
    dense = rs.uniform(-1.0, 1.0, (N, N))
    nan, inf, ninf = dense.copy(), dense.copy(), dense.copy()
    nan[N - 1, 0], inf[0, N - 1], ninf[N // 2, N // 2] = np.nan, np.inf, -np.inf
    return [("the zero matrix", np.zeros((N, N))), ("the identity", np.eye(N)), ("a diagonal with tied entries", tied),
            ("upper triangular", tri), ("lower triangular", tri.T.copy()), ("already Hessenberg", hess),
            ("Hessenberg with a zero subdiagonal", split), ("a Jordan block", jordan), ("a companion matrix", companion(KNOWN_ROOTS[N])),
            ("rotations and a real pole on one vertical line", line), ("dense", dense), ("dense scaled by 1e100", dense * 1e100),
            ("dense scaled by 1e-100", dense * 1e-100), ("a NaN word", nan), ("a +inf word", inf), ("a -inf word", ninf)]


def shift_cases(N):
    """(name, m [N][N], sweeps of one deflation at least, converges): what reaches the exceptional shifts.  The cyclic permutation
    matrix has zero standard shifts and does not move before sweep 10; weighted cyclic matrices whose weights spread over many
    binades are still cyclic after the first exceptional shift, and with a wide enough spread after both: the sweep cap, status
    FD_MO_NOT_CONVERGED, never a wrong pole.  N = 2 has nothing to sweep (a 2 x 2 is solved in closed form): no matrix exists.
    The weighted ones were found by a search over powers of two with eig_n's trace."""
    if N == 2:
        return []
    out = [(f"cyclic {N} x {N}", cyclic([1.0] * N), 11, True)]
    out += [(name, cyclic(w), least, conv) for name, w, least, conv in WEIGHTED[N]]
    return out


p14, p8, p6, P6, P8 = 2.0 ** -14, 2.0 ** -8, 2.0 ** -6, 2.0 ** 6, 2.0 ** 8
# per N: (name, weights, sweeps of one deflation at least, converges).  Every N from 3 up has a matrix past sweep 20 and one at the cap.
WEIGHTED = {
    3: [("weighted cyclic 3 x 3 past sweep 20", [p8, 1.0, p8], 21, True), ("weighted cyclic 3 x 3 to the cap", [p14, P8, p14], 30, False)],
    4: [("weighted cyclic 4 x 4 past sweep 20", [-p8, p8, P8, 1.0], 21, True), ("weighted cyclic 4 x 4 to the cap", [-p8, P6, p8, 1.0], 30, False)],
    5: [("weighted cyclic 5 x 5 past sweep 20", [p8, -1.0, P8, -P8, 1.0], 21, True),
        ("weighted cyclic 5 x 5 to the cap", [p8, -P8, P6, p8, P6], 30, False)],
    6: [("weighted cyclic 6 x 6 past sweep 20", [-p8, P6, P8, p8, -P8, -p6], 21, True),
        ("weighted cyclic 6 x 6 to the cap", [-1.0, P8, P6, 1.0, P8, p6], 30, False)],
    7: [("weighted cyclic 7 x 7 past sweep 20", [-P6, P6, P6, p6, -1.0, -p8, -P6], 21, True),
        ("weighted cyclic 7 x 7 to the cap", [P6, -P8, p8, 1.0, p6, P8, -p6], 30, False)],
}


# One servo loop that ends at the sweep cap without being built for it: the continuous longitudinal closed loop of aircraft 4497 of
# scripts/servo_modes_throughput.py's 65 536-aircraft fleet (rc_plane, default weights), as the device composed it.  After two real
# poles deflate, the window left holds two complex pairs under a trailing 2 x 2 with real eigenvalues; the standard double shift
# wanders on it, the exceptional shifts at 10 and 20 do not land it, and 30 sweeps run out: FD_MO_NOT_CONVERGED, never a wrong pole.
STALLED_LOOP = np.array(
    [[-0.7745846445322425, 0.4148153684081843, -0.13554796387785384, -9.421737570325352, 0.23276108106449128, -0.2016191105113204, -0.051329566209265834],
     [-0.7400444796948372, -4.793498772786325, 18.521069092474384, -40.15468608262992, 1.696451303802355, 0.14723454080125847, -0.5341832307137138],
     [0.24670647544321192, 0.5596459990553886, -34.69150202605003, -247.61130217713568, 10.603109389078229, 0.9202409397000448, -3.338736111301079],
     [0.0, 0.0, 0.9496546275434179, 0.0, 0.0, 0.0, 0.0],
     [-0.05774475437375255, 0.9480700143828469, 0.0, -23.967732681488428, 0.0, 0.0, 0.0],
     [0.9999727683305161, 0.007379877871895753, 0.0, 0.0, 0.0, 0.0, 0.0],
     [0.0, 0.0, 0.0, 0.0, -1.0, 0.0, 0.0]])


def sweeps_of(m):
    """-> (largest number of sweeps of one deflation, converged)"""
    tr = []
    _, _, _, ok = eig_n(np.asarray(m, np.float64) + 0.0, tr)
    return max(tr), ok


_CACHE = {}


def golden_loops(golden):
    """The servo matrices of the 288 linearisations of tests/golden/trim_reference.npz under the restatements' default servo and
    servo-Kalman designs: dict(K, x0, F {dt}, status (servo design), continuous [288] lists of [7 x 7, 6 x 6], sampled {dt}, filter
    {dt}).  Once per session, read-only."""
    if "loops" not in _CACHE:
        import servo_margin_numpy as sm
        d = sm.golden_designs(golden)
        A, B = golden["A"], golden["B"]
        n = len(A)
        out = dict(K=d["K"], x0=d["x0"], F=d["F"], status=sn.golden_designs(golden)["status"])
        out["continuous"] = [continuous_blocks(A[i], B[i], d["x0"][i], d["K"][i]) for i in range(n)]
        out["sampled"] = {dt: [sampled_blocks(d["K"][i], d["F"][dt][i], d["x0"][i], dt) for i in range(n)] for dt in DTS}
        out["filter"] = {dt: [filter_blocks(d["F"][dt][i]) for i in range(n)] for dt in DTS}
        _CACHE["loops"] = out
    return _CACHE["loops"]


def golden_reports(golden):
    """The restatement's report on every loop of golden_loops: dict(continuous, sampled {dt}, filter {dt}) of blocks_modes' dicts.
    Once per session."""
    if "reports" not in _CACHE:
        lo = golden_loops(golden)
        _CACHE["reports"] = dict(continuous=blocks_modes(lo["continuous"]), sampled={dt: blocks_modes(lo["sampled"][dt]) for dt in DTS},
                                 filter={dt: blocks_modes(lo["filter"][dt]) for dt in DTS})
    return _CACHE["reports"]

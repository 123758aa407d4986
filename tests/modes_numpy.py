"""The flight-mode report of include/fdyn_modes.h (fdyn_flight_modes, fdyn_block_modes; csrc/fdyn_eig.hpp) restated on NumPy fp64
scalars: the same operations in the same order -- Householder reduction to Hessenberg form, Francis double-shift sweeps over the
whole 4 x 4 and then over the 3 x 3 a deflation leaves, 2 x 2 blocks in closed form, the sorting network, the summary words -- so
that the host program and the kernel can be held to it bit for bit.  Shared by the CPU tests and the GPU test; nothing here imports
the product package.
"""
import numpy as np

from lqr_numpy import LON_STATES, LON_CONTROLS, LAT_STATES, LAT_CONTROLS

MAX_SWEEPS, EPS = 30, np.float64(2.0 ** -52)
NOT_CONVERGED, BAD_INPUT = 1, 2
ABSCISSA, RADIUS, MIN_ABS, MIN_ZETA, N_UNSTABLE, N_COMPLEX, NMO = 0, 1, 2, 3, 4, 5, 6
F = np.float64
ZERO = F(0.0)


def _rows(m):
    return [[F(v) for v in row] for row in np.asarray(m, np.float64)]


def hessenberg4(a):
    """In place on a list of four lists of fp64 scalars."""
    for k in range(2):
        m = k + 1
        below = abs(a[m + 1][k])
        for i in range(m + 2, 4):
            below = below + abs(a[i][k])
        if below != 0.0:
            scale = abs(a[m][k]) + below
            o = [None] * 4
            for i in range(m, 4):
                o[i] = a[i][k] / scale
            h = o[m] * o[m]
            for i in range(m + 1, 4):
                h = h + o[i] * o[i]
            rt = np.sqrt(h)
            g = -rt if o[m] >= 0.0 else rt
            h = h - o[m] * g
            o[m] = o[m] - g
            for j in range(m, 4):
                f = o[m] * a[m][j]
                for i in range(m + 1, 4):
                    f = f + o[i] * a[i][j]
                f = f / h
                for i in range(m, 4):
                    a[i][j] = a[i][j] - f * o[i]
            for i in range(4):
                f = o[m] * a[i][m]
                for j in range(m + 1, 4):
                    f = f + o[j] * a[i][j]
                f = f / h
                for j in range(m, 4):
                    a[i][j] = a[i][j] - f * o[j]
            a[m][k] = scale * g
            for i in range(m + 1, 4):
                a[i][k] = ZERO


def find_split(h, norm):
    l = 0
    for k in range(1, len(h)):
        s = abs(h[k - 1][k - 1]) + abs(h[k][k])
        s = norm if s == 0.0 else s
        if abs(h[k][k - 1]) <= EPS * s:
            l = k
    return l


def francis_step(h, its):
    N = len(h)
    E = N - 1
    x, y, w = h[E][E], h[E - 1][E - 1], h[E][E - 1] * h[E - 1][E]
    if its == 10:
        s = abs(h[1][0]) + abs(h[2][1])
        x = F(0.75) * s + h[0][0]; y = x; w = F(-0.4375) * s * s
    elif its == 20:
        s = abs(h[E][E - 1]) + abs(h[E - 1][E - 2])
        x = F(0.75) * s + h[E][E]; y = x; w = F(-0.4375) * s * s
    z = h[0][0]
    r, s = x - z, y - z
    p = (r * s - w) / h[1][0] + h[0][1]
    q = ((h[1][1] - z) - r) - s
    r = h[2][1]
    s = (abs(p) + abs(q)) + abs(r)
    p, q, r = p / s, q / s, r / s
    for k in range(E):
        last = k == E - 1
        sc = ZERO
        if k != 0:
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
            if k != 0:
                h[k][k - 1] = -s * sc
            p = p + s
            x, y = p / s, q / s
            q = q / p
            if not last:
                z = r / s
                r = r / p
            for j in range(k, N):
                t = h[k][j] + q * h[k + 1][j]
                if not last:
                    t = t + r * h[k + 2][j]
                    h[k + 2][j] = h[k + 2][j] - t * z
                h[k + 1][j] = h[k + 1][j] - t * y
                h[k][j] = h[k][j] - t * x
            for i in range(min(k + 3, E) + 1):
                t = x * h[i][k] + y * h[i][k + 1]
                if not last:
                    t = t + z * h[i][k + 2]
                    h[i][k + 2] = h[i][k + 2] - t * r
                h[i][k + 1] = h[i][k + 1] - t * q
                h[i][k] = h[i][k] - t
        if k != 0:
            h[k + 1][k - 1] = ZERO
            if not last:
                h[k + 2][k - 1] = ZERO


def deflate(h, norm):
    """-> (split row, sweeps, failed)"""
    k = 0
    while True:
        l = find_split(h, norm)
        if l != 0:
            return l, k, False
        t = abs(h[1][0])
        for j in range(2, len(h)):
            t = t + abs(h[j][j - 1])
        if k == MAX_SWEEPS or not np.isfinite(t):
            return 0, k, True
        francis_step(h, k)
        k += 1


def eig2(a, b, c, d):
    """-> ((re0, im0), (re1, im1))"""
    p, bc = F(0.5) * (a - d), b * c
    disc = p * p + bc
    if b == 0.0 or c == 0.0:
        return (a, ZERO), (d, ZERO)
    if disc >= 0.0:
        z = np.sqrt(disc)
        zz = p + (z if p >= 0.0 else -z)
        re0 = d + zz
        return (re0, ZERO), ((d - bc / zz) if zz != 0.0 else re0, ZERO)
    re, im = F(0.5) * (a + d), np.sqrt(-disc)
    return (re, im), (re, -im)


NET = ((0, 1), (2, 3), (0, 2), (1, 3), (1, 2))


def eig4(m):
    """One 4 x 4 (finite) -> (re [4], im [4], sweeps, ok) in canonical order; re, im are what the arithmetic gave when not ok."""
    with np.errstate(all="ignore"):
        h = _rows(m)
        hessenberg4(h)
        norm = ZERO
        for i in range(4):
            for j in range(max(i - 1, 0), 4):
                norm = norm + abs(h[i][j])
        failed = not np.isfinite(norm)
        sweeps = 0
        l = 2
        if not failed:
            l, k, failed = deflate(h, norm)
            sweeps += k
        top = l == 3
        t = [[h[r][c] if top else h[r + 1][c + 1] for c in range(3)] for r in range(3)]
        r1 = h[3][3] if top else h[0][0]
        two = l == 2
        l3 = 2
        if not (two or failed):
            l3, k, failed = deflate(t, norm)
            sweeps += k
        top3 = l3 == 2
        r2 = t[2][2] if top3 else t[0][0]
        if two:
            e = list(eig2(h[0][0], h[0][1], h[1][0], h[1][1])) + list(eig2(h[2][2], h[2][3], h[3][2], h[3][3]))
        else:
            o = 0 if top3 else 1
            e = list(eig2(t[o][o], t[o][o + 1], t[o + 1][o], t[o + 1][o + 1])) + list(eig2(r2, ZERO, ZERO, r1))
        re, im = [v[0] for v in e], [v[1] for v in e]
        for i, j in NET:
            mi, mj = abs(im[i]), abs(im[j])
            if re[j] > re[i] or (re[j] == re[i] and (mj > mi or (mj == mi and im[j] > im[i]))):
                re[i], re[j], im[i], im[j] = re[j], re[i], im[j], im[i]
        re, im = np.array(re, np.float64), np.array(im, np.float64)
        return re, im, sweeps, (not failed) and bool(np.isfinite(re).all() and np.isfinite(im).all())


def summary(re, im):
    """The six FD_MO_* words of four eigenvalues."""
    with np.errstate(all="ignore"):
        absc, rad, mn, zeta, nu, nc = F(re[0]), ZERO, ZERO, ZERO, ZERO, ZERO
        for k in range(4):
            rk, ik = F(re[k]), F(im[k])
            m = np.sqrt(rk * rk + ik * ik)
            z = ZERO if m == 0.0 else -rk / m
            absc = rk if rk > absc else absc
            rad = m if (k == 0 or m > rad) else rad
            mn = m if (k == 0 or m < mn) else mn
            zeta = z if (k == 0 or z < zeta) else zeta
            nu = nu + F(1.0) if rk > 0.0 else nu
            nc = nc + F(1.0) if ik != 0.0 else nc
        return np.array([absc, rad, mn, zeta, nu, nc], np.float64)


def block_modes(M):
    """M [n][2][4][4] -> dict(re [n][2][4], im [n][2][4], summary [n][2][6], iters [n] int32, status [n] int32): what
    fdyn_block_modes writes, lane-major."""
    M = np.asarray(M, np.float64)
    n = len(M)
    out = dict(re=np.full((n, 2, 4), np.nan), im=np.full((n, 2, 4), np.nan), summary=np.full((n, 2, NMO), np.nan),
               iters=np.zeros(n, np.int32), status=np.zeros(n, np.int32))
    for i in range(n):
        if not np.isfinite(M[i]).all():
            out["status"][i] = BAD_INPUT
            continue
        good, it = True, 0
        for b in range(2):
            re, im, sweeps, ok = eig4(M[i, b] + 0.0)             # -0 enters as +0
            good, it = good and ok, max(it, sweeps)
            out["re"][i, b], out["im"][i, b], out["summary"][i, b] = re, im, summary(re, im)
        out["iters"][i] = it
        if not good:
            out["status"][i] = NOT_CONVERGED
            out["re"][i], out["im"][i], out["summary"][i] = np.nan, np.nan, np.nan
    return out


def closed_blocks(A, B, K=None):
    """A [n][12][12], B [n][12][4], K [n][16] or None -> M [n][2][4][4]: a - b Kb per block, each product pair summed left to
    right, as fdyn_flight_modes forms it; entries outside the blocks are not read.  K None: the open loop."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    n = len(A)
    M = np.empty((n, 2, 4, 4))
    with np.errstate(all="ignore"):
        for b, (st, ct) in enumerate(((LON_STATES, LON_CONTROLS), (LAT_STATES, LAT_CONTROLS))):
            a = A[:, st][:, :, st]
            if K is None:
                M[:, b] = a
            else:
                bb = B[:, st][:, :, ct]                              # [n][4][2]
                kb = np.asarray(K, np.float64)[:, 8 * b:8 * b + 8].reshape(n, 2, 4)
                s = bb[:, :, 0:1] * kb[:, 0:1, :] + bb[:, :, 1:2] * kb[:, 1:2, :]
                M[:, b] = a - s
    return M


def flight_modes(A, B, K=None):
    """What fdyn_flight_modes writes for A [n][12][12], B [n][12][4], K [n][16] or None (status 2 where a word that is read --
    the blocks of A, and of B and K when K is given -- is not finite)."""
    M = closed_blocks(A, B, K)
    if K is not None:
        A, B, K = np.asarray(A, np.float64), np.asarray(B, np.float64), np.asarray(K, np.float64)
        for b, (st, ct) in enumerate(((LON_STATES, LON_CONTROLS), (LAT_STATES, LAT_CONTROLS))):
            bad = ~(np.isfinite(B[:, st][:, :, ct]).all(axis=(1, 2)) & np.isfinite(K).all(axis=1))
            M[bad, b] = np.nan                                   # an infinite b times a zero gain is caught by M already
    return block_modes(M)


def match_gap(got, ref):
    """Largest distance after the nearest matching of two multisets of four complex numbers (all 24 pairings)."""
    from itertools import permutations
    got, ref = np.asarray(got), np.asarray(ref)
    return min(float(np.max(np.abs(got[list(p)] - ref))) for p in permutations(range(4)))


def norm_inf(m):
    return float(np.max(np.sum(np.abs(m), axis=1)))


# ---- what the test files share ---------------------------------------------------------------------------------------------------
def degenerate_cases():
    """(name, m [4][4]): the ends of the solver -- no reflector to build, nothing to sweep, exact zeros on the subdiagonal."""
    rot = np.zeros((4, 4))
    rot[:2, :2] = [[-0.7, 2.5], [-2.5, -0.7]]
    rot[2, 2], rot[3, 3] = 0.3, -4.0
    tri = np.triu(np.arange(1.0, 17.0).reshape(4, 4) * np.array([1.0, -1.0, 0.5, -0.25])[:, None])
    hess = np.array([[1.0, 2.0, -3.0, 0.5], [0.7, -1.5, 0.25, 2.0], [0.0, -0.9, 0.3, 1.0], [0.0, 0.0, 1.7, -2.2]])
    split = hess.copy()
    split[2, 1] = 0.0
    jordan = np.diag([-1.5, -1.5, 0.4, -3.0])
    jordan[0, 1] = 1.0
    first = np.array([[2.0, 1.0, 0.0, -1.0], [0.5, -1.0, 3.0, 0.2], [0.0, 0.4, -0.6, 1.1], [0.0, -0.8, 0.9, 0.1]])
    companion = np.zeros((4, 4))
    companion[0] = [-2.4, -7.44, -6.112, -9.1296]                  # two complex pairs
    companion[1, 0] = companion[2, 1] = companion[3, 2] = 1.0
    line2 = np.zeros((4, 4))                                        # two pairs with ONE real part: the tie rule keeps each pair together
    line2[:2, :2], line2[2:, 2:] = [[-1.0, 2.0], [-2.0, -1.0]], [[-1.0, 3.0], [-3.0, -1.0]]
    line1 = line2.copy()                                           # a pair and a real pole with one real part
    line1[2:, 2:] = [[-1.0, 0.0], [0.0, 0.5]]
    return [("two pairs on one vertical line", line2), ("a pair and a real pole on one vertical line", line1),
            ("the zero matrix", np.zeros((4, 4))), ("the identity", np.eye(4)), ("a diagonal", np.diag([3.0, -1.0, 0.5, -2.0])),
            ("upper triangular", tri), ("lower triangular", tri.T.copy()), ("already Hessenberg", hess),
            ("Hessenberg with a zero subdiagonal", split), ("rotation block and a diagonal", rot), ("Jordan block and a diagonal", jordan),
            ("first column already reduced", first), ("a companion matrix", companion)]


def cyclic(w, lead=None):
    """The weighted cyclic matrix with subdiagonal w[1:] and corner w[0]: 4 x 4 for four weights; for three, `lead` (+) the 3 x 3,
    which splits off at once and leaves the 3 x 3 stage the work.  The standard shifts of a cyclic matrix are zero and change
    nothing: only the exceptional shifts move it."""
    k = len(w)
    c = np.zeros((k, k))
    c[0, k - 1] = w[0]
    for i in range(1, k):
        c[i, i - 1] = w[i]
    if k == 4:
        return c
    m = np.zeros((4, 4))
    m[0, 0], m[1:, 1:] = lead, c
    return m


def shift_cases():
    """(name, m, size of the stage that stalls, sweeps of that deflation at least, converges): what reaches the exceptional shifts
    at sweeps 10 and 20 of one deflation, in both stages, and the one known way to the sweep cap.  Without balancing a cyclic matrix
    whose weights spread over 2^14 is still cyclic after both exceptional shifts: status FD_MO_NOT_CONVERGED, never a wrong pole."""
    p = 2.0 ** -8
    return [("cyclic 4 x 4", cyclic([1.0, 1.0, 1.0, 1.0]), 4, 11, True),
            ("0.5 (+) cyclic 3 x 3", cyclic([1.0, 1.0, 1.0], 0.5), 3, 11, True),
            ("weighted cyclic 4 x 4 past sweep 20", cyclic([-p, p, 2.0 ** 8, 1.0]), 4, 21, True),
            ("0.5 (+) weighted cyclic 3 x 3 past sweep 20", cyclic([p, 1.0, p], 0.5), 3, 21, True),
            ("weighted cyclic 4 x 4 to the cap", cyclic([-p, 2.0 ** 6, p, 1.0]), 4, 30, False)]


SLOW_GOLDEN = (("open", 273, 0), ("closed", 69, 1))              # the golden blocks that need more than 10 sweeps of one deflation
_BLOCKS = {}
DTS = (0.01, 0.02)


def golden_blocks(golden):
    """The 4 x 4 blocks of the 288 linearisations of tests/golden/trim_reference.npz: dict(open [288][2][4][4], closed (under the
    restatement's default LQR), K [288][16], filter {dt: [288][2][4][4]} = Phi (I - L) of kf_numpy's default filter).  Once per
    session, read-only."""
    if not _BLOCKS:
        import kf_numpy as kn
        import lqr_numpy as ln
        import margin_numpy as mn
        A, B = golden["A"], golden["B"]
        d = mn.golden_designs(golden)                            # the session's one copy of the default designs
        _BLOCKS["K"] = d["K"]
        _BLOCKS["open"], _BLOCKS["closed"] = closed_blocks(A, B), closed_blocks(A, B, d["K"])
        _BLOCKS["filter"] = {dt: np.array([[ln.mm(Phi, np.eye(4) - L) for Phi, _, L in kn.matrices(f)] for f in d["F"][dt]]) for dt in DTS}
        for v in (_BLOCKS["K"], _BLOCKS["open"], _BLOCKS["closed"], *_BLOCKS["filter"].values()):
            v.setflags(write=False)
    return _BLOCKS

"""The loop margins of include/fdyn.h (fdyn_loop_margins, csrc/fdyn_margin.hpp) restated in NumPy, operation for operation: the
same complex elimination (pivot size |re| + |im|, the first largest entry of the column pivots, row swaps as selects, every
multiplier a product with the pivot's reciprocal), the same summation order, the same closed-form singular values, np.sqrt for
the square root.  Every scalar of the header is an array here over (aircraft, grid point): the operations are elementwise, so each
element sees exactly the header's sequence of IEEE operations.  Shared by the CPU tests and the GPU test; nothing here imports the
product package.
"""
import numpy as np

from lqr_numpy import mm, PIVOT_REL

NOT_STABLE, SINGULAR, BAD_INPUT = 1, 2, 4
ESTIMATE, MEASUREMENT, TRUTH = 0, 1, 2
MAX_SQUARINGS, MAX_OMEGA = 30, 256
PHI, GAMMA, LG = (0, 16), (32, 40), (48, 64)                     # FD_KF_*_LON, FD_KF_*_LAT


def nan_max(m, v):
    """max, NaN wins and stays."""
    return np.where((v > m) | (v != v), v, m)


def cgauss_solve(ar, ai, br, bi, pivot_rel=PIVOT_REL):
    """a x = b over the complex numbers: a [N][N][...], b [N][M][...] as real and imaginary parts -> (xr, xi, ok [...])."""
    ar, ai, br, bi = (np.asarray(v, np.float64) for v in (ar, ai, br, bi))
    N, M = ar.shape[0], br.shape[1]
    batch = np.broadcast_shapes(ar.shape[2:], br.shape[2:])
    ar, ai = (np.broadcast_to(v, (N, N) + batch).copy() for v in (ar, ai))
    br, bi = (np.broadcast_to(v, (N, M) + batch).copy() for v in (br, bi))
    mx = np.zeros(batch)
    for r in range(N):
        for c in range(N):
            mx = nan_max(mx, np.abs(ar[r, c]) + np.abs(ai[r, c]))
    floor = pivot_rel * mx
    ivr, ivi = np.zeros((N,) + batch), np.zeros((N,) + batch)
    ok = np.ones(batch, bool)
    for k in range(N):
        p = np.full(batch, k)
        best = np.abs(ar[k, k]) + np.abs(ai[k, k])
        for r in range(k + 1, N):
            v = np.abs(ar[r, k]) + np.abs(ai[r, k])
            t = v > best
            best = np.where(t, v, best)
            p = np.where(t, r, p)
        for r in range(k + 1, N):
            sw = p == r
            for m in (ar, ai):
                t = m[k, k:].copy()
                m[k, k:] = np.where(sw, m[r, k:], t)
                m[r, k:] = np.where(sw, t, m[r, k:])
            for m in (br, bi):
                t = m[k].copy()
                m[k] = np.where(sw, m[r], t)
                m[r] = np.where(sw, t, m[r])
        ok = ok & (best >= floor) & (best > 0.0)
        pr, pi = ar[k, k], ai[k, k]
        den = pr * pr + pi * pi
        ivr[k] = pr / den
        ivi[k] = -pi / den
        for r in range(k + 1, N):
            mr = ar[r, k] * ivr[k] - ai[r, k] * ivi[k]
            mi = ar[r, k] * ivi[k] + ai[r, k] * ivr[k]
            for c in range(k + 1, N):
                tr, ti = mr * ar[k, c] - mi * ai[k, c], mr * ai[k, c] + mi * ar[k, c]
                ar[r, c] = ar[r, c] - tr
                ai[r, c] = ai[r, c] - ti
            for c in range(M):
                tr, ti = mr * br[k, c] - mi * bi[k, c], mr * bi[k, c] + mi * br[k, c]
                br[r, c] = br[r, c] - tr
                bi[r, c] = bi[r, c] - ti
    xr, xi = np.zeros_like(br), np.zeros_like(bi)
    for k in range(N - 1, -1, -1):
        for j in range(M):
            sr, si = br[k, j].copy(), bi[k, j].copy()
            for c in range(k + 1, N):
                tr, ti = ar[k, c] * xr[c, j] - ai[k, c] * xi[c, j], ar[k, c] * xi[c, j] + ai[k, c] * xr[c, j]
                sr = sr - tr
                si = si - ti
            xr[k, j] = sr * ivr[k] - si * ivi[k]
            xi[k, j] = sr * ivi[k] + si * ivr[k]
    return xr, xi, ok


def row_norm(m):
    """|m|_inf of m [4][4][...]: the largest row sum of magnitudes, each row summed left to right; NaN wins."""
    nrm = np.zeros(m.shape[2:])
    for r in range(4):
        rs = np.abs(m[r, 0])
        for c in range(1, 4):
            rs = rs + np.abs(m[r, c])
        nrm = nan_max(nrm, rs)
    return nrm


def schur_by_squaring(m):
    """m [4][4][n] -> (certified [n] bool, squarings [n]): m <- m m until |m|_inf < 1, at most MAX_SQUARINGS times."""
    m = np.array(m, np.float64)
    n = m.shape[2:]
    active, certified, squarings = np.ones(n, bool), np.zeros(n, bool), np.zeros(n, np.int32)
    while True:
        nrm = row_norm(m)
        active = active & np.isfinite(nrm)
        hit = active & (nrm < 1.0)
        certified |= hit
        active = active & ~hit & (squarings < MAX_SQUARINGS)
        if not active.any():
            return certified, squarings
        m = np.where(active, mm(m, m), m)
        squarings = squarings + active


def sigma_2x2(mr, mi):
    """(s_max, |det|) of the complex 2 x 2 m [2][2][...] in closed form."""
    F = mr[0, 0] * mr[0, 0] + mi[0, 0] * mi[0, 0]
    for a, b in ((0, 1), (1, 0), (1, 1)):
        F = F + mr[a, b] * mr[a, b]
        F = F + mi[a, b] * mi[a, b]
    dr = (mr[0, 0] * mr[1, 1] - mi[0, 0] * mi[1, 1]) - (mr[0, 1] * mr[1, 0] - mi[0, 1] * mi[1, 0])
    di = (mr[0, 0] * mi[1, 1] + mi[0, 0] * mr[1, 1]) - (mr[0, 1] * mi[1, 0] + mi[0, 1] * mr[1, 0])
    D2 = dr * dr + di * di
    disc = F * F - 4.0 * D2
    disc = np.where(disc > 0.0, disc, 0.0)
    return np.sqrt(0.5 * (F + np.sqrt(disc))), np.sqrt(D2)


def block_setup(Phi, Gamma, Kb, Lk):
    """Phi [4][4][n], Gamma [4][2][n], Kb [2][4][n], Lk [4][4][n] -> (Acl = Phi - Gamma Kb, Fc = (I - L) Acl, Fe = (I - L) Phi)."""
    eye = np.eye(4).reshape(4, 4, *([1] * (Phi.ndim - 2)))
    ImL = eye - Lk
    Acl = np.zeros_like(Phi)
    for r in range(4):
        for c in range(4):
            Acl[r, c] = Phi[r, c] - (Gamma[r, 0] * Kb[0, c] + Gamma[r, 1] * Kb[1, c])
    return Acl, mm(ImL, Acl), mm(ImL, Phi)


def block_points(Phi, Gamma, Kb, Lk, Fc, estimate, zr, zi):
    """Every grid point of one block: matrices [.][.][n][1], zr / zi [1][W] -> (sig_s [n][W], inv_sig_t [n][W], ok [n][W])."""
    n, W = Phi.shape[2], zr.shape[-1]
    zero, eye = np.zeros((n, W)), np.eye(4, dtype=bool).reshape(4, 4, 1, 1)
    xr = xi = None
    ok = np.ones((n, W), bool)
    for ps in range(2 if estimate else 1):
        mat = Fc if ps else Phi
        ar = np.where(eye, zr, 0.0) - mat                        # (r == c ? zr : 0.0) - word
        ai = np.where(eye, zi, 0.0) + zero
        if ps:
            br, bi = mm(Lk, xr), mm(Lk, xi)
        else:
            br, bi = Gamma + zero, np.zeros((4, 2, n, W))
        xr, xi, solved = cgauss_solve(ar, ai, br, bi)
        ok = ok & solved
    sr, si = mm(Kb, xr), mm(Kb, xi)
    if estimate:
        lr, li = sr * zr - si * zi, sr * zi + si * zr
    else:
        lr, li = sr, si
    mr, mi = lr.copy(), li.copy()
    for a in range(2):
        mr[a, a] = 1.0 + lr[a, a]
    smax, absdet = sigma_2x2(mr, mi)
    sig_s = absdet / smax
    nr, ni = np.zeros_like(lr), np.zeros_like(li)
    for a in range(2):
        nr[a, 0] = (lr[a, 0] * mr[1, 1] - li[a, 0] * mi[1, 1]) - (lr[a, 1] * mr[1, 0] - li[a, 1] * mi[1, 0])
        ni[a, 0] = (lr[a, 0] * mi[1, 1] + li[a, 0] * mr[1, 1]) - (lr[a, 1] * mi[1, 0] + li[a, 1] * mr[1, 0])
        nr[a, 1] = (lr[a, 1] * mr[0, 0] - li[a, 1] * mi[0, 0]) - (lr[a, 0] * mr[0, 1] - li[a, 0] * mi[0, 1])
        ni[a, 1] = (lr[a, 1] * mi[0, 0] + li[a, 1] * mr[0, 0]) - (lr[a, 0] * mi[0, 1] + li[a, 0] * mr[0, 1])
    nmax, _ = sigma_2x2(nr, ni)
    return sig_s, absdet / nmax, ok


def block_matrices(K, F, blk, estimate):
    """K [n][16], F [n][80] -> (Phi [4][4][n], Gamma [4][2][n], Kb [2][4][n], Lk [4][4][n]); Lk = I where it is not read."""
    n = len(K)
    Phi = F[:, PHI[blk]:PHI[blk] + 16].T.reshape(4, 4, n).copy()
    Gamma = F[:, GAMMA[blk]:GAMMA[blk] + 8].T.reshape(4, 2, n).copy()
    Kb = K[:, 8 * blk:8 * blk + 8].T.reshape(2, 4, n).copy()
    Lk = F[:, LG[blk]:LG[blk] + 16].T.reshape(4, 4, n).copy() if estimate else np.eye(4)[:, :, None] + np.zeros((4, 4, n))
    return Phi, Gamma, Kb, Lk


def loop_margins(K, F, feedback, zre, zim):
    """K [n][16], F [n][80], zre / zim [W] -> dict(alpha_s [n][2], idx_s, alpha_t, idx_t, curve [n][2][W], status [n],
    squarings [n][2] (the most of the block's certificates) and curve_t [n][2][W] (1 / sigma_max(T) at every point): the last two are
    not outputs of the entry point)."""
    K, F = np.array(K, np.float64, ndmin=2), np.array(F, np.float64, ndmin=2)
    zr, zi = np.asarray(zre, np.float64)[None, :], np.asarray(zim, np.float64)[None, :]
    n, W = len(K), zr.shape[1]
    assert 1 <= W <= MAX_OMEGA
    estimate = feedback == ESTIMATE
    fin = np.isfinite(K).all(axis=1) & np.isfinite(F[:, :80 if estimate else 48]).all(axis=1)
    status = np.where(fin, 0, BAD_INPUT).astype(np.int32)
    alpha_s, alpha_t = np.zeros((n, 2)), np.zeros((n, 2))
    idx_s, idx_t = np.zeros((n, 2), np.int32), np.zeros((n, 2), np.int32)
    curve, curve_t, squarings = np.zeros((n, 2, W)), np.zeros((n, 2, W)), np.zeros((n, 2), np.int32)
    with np.errstate(all="ignore"):
        for blk in range(2):
            Phi, Gamma, Kb, Lk = block_matrices(K, F, blk, estimate)
            Acl, Fc, Fe = block_setup(Phi, Gamma, Kb, Lk)
            stable, squarings[:, blk] = schur_by_squaring(Acl)
            if estimate:
                st2, sq2 = schur_by_squaring(Fe)
                stable, squarings[:, blk] = stable & st2, np.maximum(squarings[:, blk], sq2)
            e = lambda m: m[..., None]
            s, t, ok = block_points(e(Phi), e(Gamma), e(Kb), e(Lk), e(Fc), estimate, zr, zi)
            ok = (ok & np.isfinite(s) & (t == t)).all(axis=1)
            status |= np.where(fin & ~stable, NOT_STABLE, 0).astype(np.int32) | np.where(fin & ~ok, SINGULAR, 0).astype(np.int32)
            for val, alpha, idx in ((s, alpha_s, idx_s), (t, alpha_t, idx_t)):
                # `if (v < best) { best = v; at = k; }` from best = +inf, at = 0: the first minimum (a NaN never wins)
                v = np.where(val == val, val, np.inf)
                idx[:, blk] = np.argmin(v, axis=1)
                alpha[:, blk] = v[np.arange(n), idx[:, blk]]
            curve[:, blk], curve_t[:, blk] = s, t
    dead = (status & (SINGULAR | BAD_INPUT)) != 0
    alpha_s[dead], alpha_t[dead], curve[dead], curve_t[dead] = np.nan, np.nan, np.nan, np.nan
    idx_s[dead], idx_t[dead] = -1, -1
    return dict(alpha_s=alpha_s, idx_s=idx_s, alpha_t=alpha_t, idx_t=idx_t, curve=curve, status=status, squarings=squarings, curve_t=curve_t)


# ---- the host side of the grid (hcrl_amd.margins.default_grid / unit_circle restated) ---------------------------------------
def default_omega(dt, n=64):
    w = np.geomspace(1e-2, np.pi / dt, n)
    w[-1] = np.pi / dt
    return w


def unit_circle(omega, dt):
    """-> (zre, zim); a point at the Nyquist rate pi / dt is stored exactly as (-1, 0)."""
    w = np.asarray(omega, np.float64)
    zre, zim = np.cos(w * dt), np.sin(w * dt)
    ny = w >= np.pi / dt
    return np.where(ny, -1.0, zre), np.where(ny, 0.0, zim)


# ---- the independent reference: complex solves and an SVD ----------------------------------------------------------------------
def reference(Phi, Gamma, Kb, Lk, estimate, z):
    """One block of n aircraft (Phi [n][4][4], Gamma [n][4][2], Kb [n][2][4], Lk [n][4][4]) at the complex points z [W] ->
    (sigma_min(I + L_i) [n][W], 1 / sigma_max(T) [n][W]) by np.linalg.solve on complex matrices and np.linalg.svd."""
    I4, I2 = np.eye(4), np.eye(2)
    e = lambda m: np.asarray(m)[:, None]                        # [n][1][.][.] against z [W][1][1]
    zz = np.asarray(z, complex)[:, None, None]
    Phi, Gamma, Kb, Lk = e(Phi), e(Gamma), e(Kb), e(Lk)
    G = np.linalg.solve(zz * I4 - Phi, Gamma + 0j * zz)
    if estimate:
        Fc = (I4 - Lk) @ (Phi - Gamma @ Kb)
        Li = Kb @ (zz * np.linalg.solve(zz * I4 - Fc, Lk @ G))
    else:
        Li = Kb @ G
    s = np.linalg.svd(I2 + Li, compute_uv=False)[..., -1]
    t = 1.0 / np.linalg.svd(Li @ np.linalg.inv(I2 + Li), compute_uv=False)[..., 0]
    return s, t


def perturbed_loop(Phi, Gamma, Kb, Lk, estimate, gains):
    """The closed-loop matrix with the two plant-input channels scaled by `gains`: 4 x 4 under truth feedback, the 8 x 8 of plant
    and estimator (state x, xhat) under estimate feedback."""
    GD = Gamma @ np.diag(gains)
    if not estimate:
        return Phi - GD @ Kb
    Fc = (np.eye(4) - Lk) @ (Phi - Gamma @ Kb)
    return np.block([[Phi, -GD @ Kb], [Lk @ Phi, Fc - Lk @ GD @ Kb]])


# ---- what the test files share -------------------------------------------------------------------------------------------------
DTS = (0.01, 0.02)
_DESIGNS = {}


def golden_designs(golden):
    """The 288 linearisations of tests/golden/trim_reference.npz designed by the restatements with the default weights and noise:
    dict(K [288][16], F {dt: [288][80]}), every design certified.  Once per test session, read-only."""
    if not _DESIGNS:
        import kf_numpy as kn
        import lqr_numpy as ln
        lq = ln.design_many(golden["A"], golden["B"], ln.default_weights())
        assert not lq["status"].any()
        _DESIGNS["K"] = lq["K"]
        _DESIGNS["F"] = {}
        for dt in DTS:
            kf = kn.design_many(golden["A"], golden["B"], dt, kn.default_noise())
            assert not kf["status"].any()
            _DESIGNS["F"][dt] = kf["F"]
        for v in (_DESIGNS["K"], *_DESIGNS["F"].values()):
            v.setflags(write=False)
    return _DESIGNS


def pass_through_filter():
    """kf_numpy.pass_through(): Phi = I, Gamma = 0, L = I."""
    F = np.zeros(80)
    for base in PHI + LG:
        F[base:base + 16] = np.eye(4).reshape(16)
    return F


def bad_cases(K, F):
    """One good lane (K [16], F [80]) -> list of (name, K, F, status under estimate feedback, status under truth feedback) on a grid
    that holds z = (-1, 0).  None: whatever the restatement gives, with the SINGULAR bit set."""
    out = [("Kb -> -0.5 Kb: positive feedback, the squaring overflows", -0.5 * K, F, NOT_STABLE, NOT_STABLE)]
    for name, which, word, value in (("a NaN word of K", "K", 5, np.nan), ("an infinite word of K", "K", 12, np.inf),
                                     ("an infinite word of Phi", "F", PHI[1] + 6, -np.inf), ("a NaN word of Gamma", "F", GAMMA[0] + 3, np.nan)):
        k, f = K.copy(), F.copy()
        (k if which == "K" else f)[word] = value
        out.append((name, k, f, BAD_INPUT, BAD_INPUT))
    f = F.copy()
    f[LG[1] + 9] = np.nan
    out.append(("a NaN word of L: read under estimate feedback only", K.copy(), f, BAD_INPUT, 0))
    f = F.copy()
    f[PHI[0]:PHI[0] + 16] = np.diag([-1.0, 0.5, 0.25, 0.125]).reshape(16)
    out.append(("a pole of the plant on a grid point", K.copy(), f, None, None))
    out.append(("the pass-through filter", K.copy(), pass_through_filter(), NOT_STABLE, NOT_STABLE))
    return out

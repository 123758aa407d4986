"""The servo's loop margins of include/fdyn_servo_margins.h (fdyn_servo_loop_margins, csrc/fdyn_servo_margin.hpp) restated in NumPy
fp64, operation for operation: margin_numpy's complex elimination and closed-form singular values at N = 5, the squaring
certificate on the augmented 7 x 7 words (the lateral block carries a second, all-zero integrator exactly as the header does),
Kc(z) = Kx + E / (z - 1) and the complex F_c(z), every sum left to right, np.sqrt for the square root.  Every scalar of the header is
an array here over (aircraft, grid point).  Built on servo_numpy / servo_lqg_numpy's layouts; shared by the CPU tests and the GPU
test; nothing here imports the product package.
"""
import numpy as np

import margin_numpy as mn
import servo_lqg_numpy as sl
import servo_numpy as sn
from lqr_numpy import mm
from margin_numpy import NOT_STABLE, SINGULAR, BAD_INPUT, ESTIMATE, MEASUREMENT, TRUTH, MAX_SQUARINGS, MAX_OMEGA, default_omega, unit_circle

N, NI, NA = 5, 2, 7
N_INTEG = (2, 1)                                                 # integrators of the longitudinal | lateral block
K_AT = (0, 14)                                                   # FD_SVK_LON, FD_SVK_LAT
PHI, GAMMA, LG = (sl.PHI_LON, sl.PHI_LAT), (sl.GAMMA_LON, sl.GAMMA_LAT), (sl.L_LON, sl.L_LAT)
DTS = mn.DTS


def row_norm(m):
    """|m|_inf of m [N][N][...]: the largest row sum of magnitudes, each row summed left to right; NaN wins."""
    nrm = np.zeros(m.shape[2:])
    for r in range(m.shape[0]):
        rs = np.abs(m[r, 0])
        for c in range(1, m.shape[1]):
            rs = rs + np.abs(m[r, c])
        nrm = mn.nan_max(nrm, rs)
    return nrm


def schur_by_squaring(m):
    """m [N][N][n] -> (certified [n] bool, squarings [n]): m <- m m until |m|_inf < 1, at most MAX_SQUARINGS times."""
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


def block_matrices(K, F, x0, dt, blk, estimate):
    """K [n][26], F [n][120], x0 [n][12] -> dict of the block's matrices with the aircraft last: Phi [5][5][n], Gamma [5][2][n],
    Kx [2][5][n], Ki [2][2][n] (the lateral block's second column 0.0), dC [2][5][n] = dt C_i (its second row 0.0), Lk [5][5][n]
    (I where it is not read)."""
    n, ni = len(K), N_INTEG[blk]
    stride = N + ni
    Phi = F[:, PHI[blk]:PHI[blk] + 25].T.reshape(N, N, n).copy()
    Gamma = F[:, GAMMA[blk]:GAMMA[blk] + 10].T.reshape(N, 2, n).copy()
    Kb = K[:, K_AT[blk]:K_AT[blk] + 2 * stride].T.reshape(2, stride, n)
    Kx = Kb[:, :N].copy()
    Ki = np.zeros((2, NI, n))
    Ki[:, :ni] = Kb[:, N:]
    Lk = F[:, LG[blk]:LG[blk] + 25].T.reshape(N, N, n).copy() if estimate else np.eye(N)[:, :, None] + np.zeros((N, N, n))
    u0, w0 = x0[:, sn.X_U], x0[:, sn.X_W]
    V0 = np.sqrt(u0 * u0 + w0 * w0)
    C = np.zeros((NI, N, n))
    if blk == 0:
        C[0, 0], C[0, 1], C[1, 4] = u0 / V0, w0 / V0, -1.0
    else:
        C[0, 4] = 1.0
    return dict(Phi=Phi, Gamma=Gamma, Kx=Kx, Ki=Ki, dC=dt * C, Lk=Lk, n_i=ni)


def block_setup(b):
    """-> the block's derived words: E = Ki dC [2][5][n], A1 = (I - L) Phi, B1 = (I - L) Gamma, and the augmented 7 x 7 matrix
    [[Phi - Gamma Kx, -Gamma Ki], [dC, I]] (the unit entry of the zero integrator is 0.0)."""
    Phi, Gamma, Kx, Ki, dC, Lk = b["Phi"], b["Gamma"], b["Kx"], b["Ki"], b["dC"], b["Lk"]
    n = Phi.shape[2:]
    eye = np.eye(N).reshape(N, N, *([1] * len(n)))
    ImL = eye - Lk
    E = np.zeros((2, N) + n)
    for a in range(2):
        for c in range(N):
            E[a, c] = Ki[a, 0] * dC[0, c] + Ki[a, 1] * dC[1, c]
    aug = np.zeros((NA, NA) + n)
    for r in range(N):
        for q in range(N):
            aug[r, q] = Phi[r, q] - (Gamma[r, 0] * Kx[0, q] + Gamma[r, 1] * Kx[1, q])
        for j in range(NI):
            aug[r, N + j] = -(Gamma[r, 0] * Ki[0, j] + Gamma[r, 1] * Ki[1, j])
    for j in range(NI):
        aug[N + j, :N] = dC[j]
        aug[N + j, N + j] = 1.0 if j < b["n_i"] else 0.0
    return dict(E=E, A1=mm(ImL, Phi), B1=mm(ImL, Gamma), aug=aug)


def cmul_sum(ar, ai, br, bi):
    """sum_k (ar + j ai)[., k] (br + j bi)[k, .], k = 0, 1, ... in that order, each product (ac - bd, ad + bc) formed first."""
    sr = ar[:, 0:1] * br[0:1, :] - ai[:, 0:1] * bi[0:1, :]
    si = ar[:, 0:1] * bi[0:1, :] + ai[:, 0:1] * br[0:1, :]
    for k in range(1, ar.shape[1]):
        sr = sr + (ar[:, k:k + 1] * br[k:k + 1, :] - ai[:, k:k + 1] * bi[k:k + 1, :])
        si = si + (ar[:, k:k + 1] * bi[k:k + 1, :] + ai[:, k:k + 1] * br[k:k + 1, :])
    return sr, si


def block_points(b, d, estimate, zr, zi):
    """Every grid point of one block: matrices [.][.][n][1], zr / zi [1][W] -> (sig_s [n][W], inv_sig_t [n][W], ok [n][W])."""
    Phi, Gamma, Kx, Lk, E, A1, B1 = b["Phi"], b["Gamma"], b["Kx"], b["Lk"], d["E"], d["A1"], d["B1"]
    n, W = Phi.shape[2], zr.shape[-1]
    zero, eye = np.zeros((n, W)), np.eye(N, dtype=bool).reshape(N, N, 1, 1)
    wr, wi = zr - 1.0, zi
    den = wr * wr + wi * wi
    qr, qi = wr / den, -wi / den
    kr, ki = Kx + E * qr, E * qi + zero
    ok = np.ones((n, W), bool)
    ar = np.where(eye, zr, 0.0) - Phi
    ai = np.where(eye, zi, 0.0) + zero
    xr, xi, solved = mn.cgauss_solve(ar, ai, Gamma + zero, np.zeros((N, 2, n, W)))
    ok = ok & solved
    if estimate:
        ar, ai = np.zeros((N, N, n, W)), np.zeros((N, N, n, W))
        for r in range(N):
            for c in range(N):
                gr = B1[r, 0] * kr[0, c] + B1[r, 1] * kr[1, c]
                gi = B1[r, 0] * ki[0, c] + B1[r, 1] * ki[1, c]
                fr = A1[r, c] - gr
                ar[r, c] = (zr if r == c else 0.0) - fr
                ai[r, c] = (zi if r == c else 0.0) + gi
        xr, xi, solved = mn.cgauss_solve(ar, ai, mm(Lk, xr), mm(Lk, xi))
        ok = ok & solved
    sr, si = cmul_sum(kr, ki, xr, xi)
    if estimate:
        lr, li = sr * zr - si * zi, sr * zi + si * zr
    else:
        lr, li = sr, si
    mr, mi = lr.copy(), li.copy()
    for a in range(2):
        mr[a, a] = 1.0 + lr[a, a]
    smax, absdet = mn.sigma_2x2(mr, mi)
    sig_s = absdet / smax
    nr, ni = np.zeros_like(lr), np.zeros_like(li)
    for a in range(2):
        nr[a, 0] = (lr[a, 0] * mr[1, 1] - li[a, 0] * mi[1, 1]) - (lr[a, 1] * mr[1, 0] - li[a, 1] * mi[1, 0])
        ni[a, 0] = (lr[a, 0] * mi[1, 1] + li[a, 0] * mr[1, 1]) - (lr[a, 1] * mi[1, 0] + li[a, 1] * mr[1, 0])
        nr[a, 1] = (lr[a, 1] * mr[0, 0] - li[a, 1] * mi[0, 0]) - (lr[a, 0] * mr[0, 1] - li[a, 0] * mi[0, 1])
        ni[a, 1] = (lr[a, 1] * mi[0, 0] + li[a, 1] * mr[0, 0]) - (lr[a, 0] * mi[0, 1] + li[a, 0] * mr[0, 1])
    nmax, _ = mn.sigma_2x2(nr, ni)
    return sig_s, absdet / nmax, ok


def loop_margins(K, F, x0, dt, feedback, zre, zim):
    """K [n][26], F [n][120], x0 [n][12], dt, zre / zim [W] -> dict(alpha_s [n][2], idx_s, alpha_t, idx_t, curve [n][2][W], status [n],
    squarings [n][2] (the most of the block's certificates) and curve_t [n][2][W]: the last two are not outputs of the entry point)."""
    K, F, x0 = np.array(K, np.float64, ndmin=2), np.array(F, np.float64, ndmin=2), np.array(x0, np.float64, ndmin=2)
    zr, zi = np.asarray(zre, np.float64)[None, :], np.asarray(zim, np.float64)[None, :]
    n, W = len(K), zr.shape[1]
    assert 1 <= W <= MAX_OMEGA
    estimate = feedback == ESTIMATE
    alpha_s, alpha_t = np.zeros((n, 2)), np.zeros((n, 2))
    idx_s, idx_t = np.zeros((n, 2), np.int32), np.zeros((n, 2), np.int32)
    curve, curve_t, squarings = np.zeros((n, 2, W)), np.zeros((n, 2, W)), np.zeros((n, 2), np.int32)
    with np.errstate(all="ignore"):
        u0, w0 = x0[:, sn.X_U], x0[:, sn.X_W]
        fin = np.isfinite(K).all(axis=1) & np.isfinite(F[:, :120 if estimate else LG[0]]).all(axis=1) & np.isfinite(u0) & np.isfinite(w0)
        V0 = np.sqrt(u0 * u0 + w0 * w0)
        good = fin & (V0 > 0.0) & bool(dt > 1e-6) & (not dt > 1.0)
        status = np.where(good, 0, BAD_INPUT).astype(np.int32)
        for blk in range(2):
            b = block_matrices(K, F, x0, dt, blk, estimate)
            d = block_setup(b)
            stable, squarings[:, blk] = schur_by_squaring(d["aug"])
            if estimate:
                fe = np.zeros((NA, NA, n))
                fe[:N, :N] = d["A1"]
                st2, sq2 = schur_by_squaring(fe)
                stable, squarings[:, blk] = stable & st2, np.maximum(squarings[:, blk], sq2)
            e = lambda m: m[..., None]
            s, t, ok = block_points({k: (e(v) if isinstance(v, np.ndarray) else v) for k, v in b.items()}, {k: e(v) for k, v in d.items()},
                                    estimate, zr, zi)
            ok = (ok & np.isfinite(s) & (t == t)).all(axis=1)
            status |= np.where(good & ~stable, NOT_STABLE, 0).astype(np.int32) | np.where(good & ~ok, SINGULAR, 0).astype(np.int32)
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


# ---- the independent reference: complex solves on the AUGMENTED system and an SVD ----------------------------------------------
def reference_blocks(K26, F120, x0, dt, blk):
    """One aircraft -> (Phi [5][5], Gamma [5][2], Lk [5][5], Kb [2][5 + n_i], Ci [n_i][5]) from servo_numpy / servo_lqg_numpy's own
    layouts: the integrator rows are those of servo_numpy.augmented_blocks."""
    Phi, Gamma, Lk = sl.matrices(F120)[blk]
    (a_lon, _), (a_lat, _) = sn.augmented_blocks(np.zeros((12, 12)), np.zeros((12, 4)), x0)
    ni = N_INTEG[blk]
    Kb = np.asarray(K26[K_AT[blk]:K_AT[blk] + 2 * (N + ni)]).reshape(2, N + ni)
    return Phi, Gamma, Lk, Kb, (a_lat if blk else a_lon)[N:, :N]


def reference(K, F, x0, dt, blk, estimate, z):
    """One block of n aircraft (K [n][26], F [n][120], x0 [n][12]) at the complex points z [W] -> (sigma_min(I + L_i) [n][W],
    1 / sigma_max(T) [n][W]) by np.linalg.solve on the AUGMENTED complex system -- the integrators are states here, not a factor
    1 / (z - 1) -- and np.linalg.svd.
      truth:     states (x, i):        z x = Phi x + Gamma u_in;  z i = i + dt C_i x;  u_out = -(Kx x + Ki i)
      estimate:  states (x, xhat, i):  xhat_k = (I - L)(Phi xhat_{k-1} + Gamma du_{k-1}) + L x_k,  du = -(Kx xhat + Ki i),
                 z i = i + dt C_i xhat  (the estimator equation multiplied by z)
    L_i = -u_out / u_in at the plant input."""
    z = np.asarray(z, complex)
    n, W, ni = len(K), len(z), N_INTEG[blk]
    size = (2 * N if estimate else N) + ni
    M = np.zeros((n, W, size, size), complex)
    rhs = np.zeros((n, W, size, 2), complex)
    pick = np.zeros((n, 2, size))                                # L_i = pick @ solution
    zz = z[:, None, None]
    I5, Ii = np.eye(N), np.eye(ni)
    for a in range(n):
        Phi, Gamma, Lk, Kb, Ci = reference_blocks(K[a], F[a], x0[a], dt, blk)
        Kx, Ki = Kb[:, :N], Kb[:, N:]
        rhs[a, :, :N] = Gamma
        M[a, :, :N, :N] = zz * I5 - Phi
        if not estimate:
            M[a, :, N:, :N] = -dt * Ci
            M[a, :, N:, N:] = (zz - 1.0) * Ii
            pick[a, :, :N], pick[a, :, N:] = Kx, Ki
        else:
            ImL = I5 - Lk
            M[a, :, N:2 * N, :N] = -zz * Lk
            M[a, :, N:2 * N, N:2 * N] = zz * I5 - ImL @ Phi + ImL @ Gamma @ Kx
            M[a, :, N:2 * N, 2 * N:] = ImL @ Gamma @ Ki
            M[a, :, 2 * N:, N:2 * N] = -dt * Ci
            M[a, :, 2 * N:, 2 * N:] = (zz - 1.0) * Ii
            pick[a, :, N:2 * N], pick[a, :, 2 * N:] = Kx, Ki
    Li = pick[:, None] @ np.linalg.solve(M, rhs)
    I2 = np.eye(2)
    s = np.linalg.svd(I2 + Li, compute_uv=False)[..., -1]
    t = 1.0 / np.linalg.svd(Li @ np.linalg.inv(I2 + Li), compute_uv=False)[..., 0]
    return s, t


def perturbed_loop(K26, F120, x0, dt, blk, estimate, gains):
    """The closed-loop matrix with the two plant-input channels scaled by `gains`: states (x, i) under truth feedback; plant,
    estimate and integrators (x, xhat, i) under estimate feedback, where the estimator is fed the controller's own unperturbed du
    and the plant gets diag(g) du.  Written with xhat_{k+1} in terms of x_{k+1} = Phi x + Gamma diag(g) du."""
    Phi, Gamma, Lk, Kb, Ci = reference_blocks(K26, F120, x0, dt, blk)
    ni = len(Ci)
    Kx, Ki = Kb[:, :N], Kb[:, N:]
    GD = Gamma @ np.diag(gains)
    if not estimate:
        return np.block([[Phi - GD @ Kx, -GD @ Ki], [dt * Ci, np.eye(ni)]])
    ImL = np.eye(N) - Lk
    # du = -(Kx xhat + Ki i);  x+ = Phi x + GD du;  xhat+ = ImL (Phi xhat + Gamma du) + L x+;  i+ = i + dt Ci xhat
    return np.block([[Phi, -GD @ Kx, -GD @ Ki],
                     [Lk @ Phi, ImL @ (Phi - Gamma @ Kx) - Lk @ GD @ Kx, -ImL @ Gamma @ Ki - Lk @ GD @ Ki],
                     [np.zeros((ni, N)), dt * Ci, np.eye(ni)]])


# ---- what the test files share -------------------------------------------------------------------------------------------------
_DESIGNS = {}


def golden_designs(golden):
    """The 288 linearisations of tests/golden/trim_reference.npz designed by the restatements with the default servo weights and the
    default servo Kalman noise: dict(K [288][26], F {dt: [288][120]}, x0 [288][12]), every design certified.  Once per test session,
    read-only."""
    if not _DESIGNS:
        sv = sn.golden_designs(golden)
        assert not sv["status"].any()
        _DESIGNS["K"] = np.array(sv["K"])
        _DESIGNS["x0"] = np.array(golden["x0"], np.float64)
        _DESIGNS["F"] = {}
        for dt in DTS:
            kf = sl.golden_designs(golden, dt)
            assert not kf["status"].any()
            _DESIGNS["F"][dt] = np.array(kf["F"])
        for v in (_DESIGNS["K"], _DESIGNS["x0"], *_DESIGNS["F"].values()):
            v.setflags(write=False)
    return _DESIGNS


def grid_with_one(n=7, dt=0.01):
    """The 7-point default grid with its first point replaced by z = (1, 0): the point no servo loop can be evaluated at."""
    zre, zim = unit_circle(default_omega(dt, n), dt)
    zre, zim = zre.copy(), zim.copy()
    zre[0], zim[0] = 1.0, 0.0
    return zre, zim


def bad_cases(K, F, x0):
    """One good lane (K [26], F [120], x0 [12]) at dt 0.01 -> list of (name, K, F, x0, dt, status under estimate feedback, status
    under truth feedback), on any grid without z = 1."""
    dt = 0.01
    out = [("Kb -> -0.5 Kb: positive feedback, the squaring overflows", -0.5 * K, F, x0, dt, NOT_STABLE, NOT_STABLE)]
    for name, which, word, value in (("a NaN word of K", "K", 5, np.nan), ("an infinite word of K", "K", 19, np.inf),
                                     ("an infinite word of Phi", "F", PHI[1] + 6, -np.inf), ("a NaN word of Gamma", "F", GAMMA[0] + 3, np.nan),
                                     ("a NaN word of Phi", "F", PHI[0] + 24, np.nan), ("an infinite word of Gamma", "F", GAMMA[1] + 9, np.inf)):
        k, f = K.copy(), F.copy()
        (k if which == "K" else f)[word] = value
        out.append((name, k, f, x0, dt, BAD_INPUT, BAD_INPUT))
    for name, value in (("a NaN word of L: read under estimate feedback only", np.nan), ("an infinite word of L: read under estimate feedback only", np.inf)):
        f = F.copy()
        f[LG[1] + 9] = value
        out.append((name, K.copy(), f, x0, dt, BAD_INPUT, 0))
    x = x0.copy()
    x[sn.X_U] = x[sn.X_W] = 0.0
    out.append(("u0 = w0 = 0: no airspeed direction", K.copy(), F.copy(), x, dt, BAD_INPUT, BAD_INPUT))
    out.append(("dt = 0", K.copy(), F.copy(), x0, 0.0, BAD_INPUT, BAD_INPUT))
    x = x0.copy()
    for k in range(12):
        if k not in (sn.X_U, sn.X_W):
            x[k] = np.nan
    out.append(("NaN words of x0 outside u and w: not read", K.copy(), F.copy(), x, dt, 0, 0))
    out.append(("the pass-through filter", K.copy(), sl.pass_through(), x0, dt, NOT_STABLE, NOT_STABLE))
    return out

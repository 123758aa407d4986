"""Domain randomisation of the rate env (fdyn_rate_env_{reset,step}_dr_*, GpuRateVecEnv(disturbances=...)) on the MI355X.

Neutral ranges reproduce the plain entry points bit for bit; per-env parameter scales and wind are checked against the
unchanged CPU oracle (wind through Galilean invariance: a uniform air-mass velocity W, constant over a step, is still air in
coordinates moving with it); the gust rows are checked as the Gauss-Markov process they claim to be.
"""
import numpy as np
import pytest
import torch

from conftest import rel_err, STATE_ANGLE_COLS
from hcrl_amd import _lib, layout as L, samplers
from hcrl_amd.disturbances import Disturbances
from hcrl_amd.params import AircraftParams
from hcrl_amd.rate_env import GpuRateVecEnv

pytestmark = pytest.mark.gpu

DOC = Disturbances.design_doc()
NEUTRAL = Disturbances()


def _R(phi, th, psi):
    """body -> NED rotation matrices [N][3][3]"""
    sp, cp, st, ct, sy, cy = np.sin(phi), np.cos(phi), np.sin(th), np.cos(th), np.sin(psi), np.cos(psi)
    R = np.empty(phi.shape + (3, 3))
    R[..., 0, 0], R[..., 0, 1], R[..., 0, 2] = ct * cy, sp * st * cy - cp * sy, cp * st * cy + sp * sy
    R[..., 1, 0], R[..., 1, 1], R[..., 1, 2] = ct * sy, sp * st * sy + cp * cy, cp * st * sy - sp * cy
    R[..., 2, 0], R[..., 2, 1], R[..., 2, 2] = -st, sp * ct, cp * ct
    return R


def _body(x, W):
    """R^T W per env; x [12][N], W [3][N]"""
    R = _R(x[6], x[7], x[8])
    return np.einsum("nji,jn->in", R, W)


def _air(env):
    dr = env.dr.double().cpu().numpy()
    return dr[L.FD_DR_WIND_N:L.FD_DR_WIND_D + 1] + dr[L.FD_DR_GUST_N:L.FD_DR_GUST_D + 1]


def _actions(n, k, scale=1.0, device="cuda"):
    g = torch.Generator(device=device).manual_seed(1000 + k)
    a = (torch.rand((n, 4), device=device, generator=g) * 2 - 1) * scale
    a[:, 3] = torch.rand(n, device=device, generator=g) * 0.5 + 0.4
    return a


def _events(env):
    ints, flts = env.episode_events()
    order = torch.argsort(ints[:, 0])
    return ints[order], flts[order]


@pytest.mark.parametrize("precision,pid", [("f64", False), ("mixed", False), ("mixed", True)])
def test_neutral_ranges_equal_plain_env(precision, pid):
    """Neutral ranges: the _dr entry points step like the plain ones.  Every step starts both from the plain env's words, so
    rounding differences cannot grow; mixed keeps the state bit for bit, f64 within rounding (FMA contraction of the
    air-relative aerodynamics is the compiler's)."""
    n, steps = 65536, 1000
    a = GpuRateVecEnv(n, "medium", 10.0, 0.02, "step", seed=21, precision=precision)
    b = GpuRateVecEnv(n, "medium", 10.0, 0.02, "step", seed=21, precision=precision, disturbances=NEUTRAL)
    assert a.dr is None and b.dr is not None
    assert torch.equal(a.reset(), b.reset())
    assert torch.equal(a.x, b.x)
    ends, worst_x, worst_o, worst_r = 0, 0.0, 0.0, 0.0
    for k in range(steps):
        for t in ("x", "e", "ei", "pid_state"):
            getattr(b, t).copy_(getattr(a, t))
        act = None if pid else _actions(n, k)
        a.step_device(act)
        b.step_device(act)
        for t in ("ei", "terminated", "truncated"):
            assert torch.equal(getattr(a, t), getattr(b, t)), (t, k)
        if precision == "mixed":
            assert torch.equal(a.x, b.x) and torch.equal(a.pid_state, b.pid_state), k
        assert torch.allclose(a.e.double(), b.e.double(), rtol=1e-6, atol=1e-5), k
        worst_x = max(worst_x, ((a.x - b.x).abs() / a.x.abs().clamp_min(1.0)).max().item())
        worst_o = max(worst_o, ((a.obs - b.obs).abs() / a.obs.abs().clamp_min(1.0)).max().item())
        worst_r = max(worst_r, (a.rewards_full - b.rewards_full).abs().max().item())
        ia, fa = _events(a)
        ib, fb = _events(b)
        assert torch.equal(ia, ib) and torch.allclose(fa, fb, rtol=1e-6, atol=1e-6), k
        ends += ia.shape[0]
    assert ends > 0
    print(f"\n[dr neutral] {precision} pid={pid}: {steps} steps, {ends} episode ends; worst rel diff state {worst_x:.2e}, "
          f"obs {worst_o:.2e}, reward abs {worst_r:.2e}")
    assert worst_x < 1e-12 and worst_o < 1e-6 and worst_r < 1e-5


def _scaled_block(P, row):
    Pi = P.copy()
    Pi[L.FD_P_MASS] *= row[L.FD_DR_MASS_S]
    Pi[L.FD_P_IXX] *= row[L.FD_DR_IXX_S]
    Pi[L.FD_P_IYY] *= row[L.FD_DR_IYY_S]
    Pi[L.FD_P_IZZ] *= row[L.FD_DR_IZZ_S]
    Pi[L.FD_P_AIR_DENSITY] *= row[L.FD_DR_RHO_S]
    return Pi


@pytest.mark.parametrize("precision,tol", [("f64", 1e-12), ("mixed", 1e-4)])
def test_parameter_scales_against_oracle(oracle, precision, tol):
    n, steps = 4096, 10
    d = Disturbances(mass=(0.9, 1.1), inertia_xx=(0.8, 1.2), inertia_yy=(0.8, 1.2), inertia_zz=(0.8, 1.2),
                     air_density=(0.95, 1.05))
    env = GpuRateVecEnv(n, "medium", 10.0, 0.02, "step", seed=5, precision=precision, disturbances=d)
    env.reset()
    dr = env.dr.double().cpu().numpy()
    assert np.ptp(dr[L.FD_DR_MASS_S]) > 0.1 and np.all(dr[:L.FD_DR_GUST_D + 1] == 0) and np.all(dr[L.FD_DR_GUST_B] == 0)
    P = AircraftParams().to_block()
    blocks = [_scaled_block(P, dr[:, i]) for i in range(n)]
    dtp = samplers.env_consts("medium", 10.0, 0.02, "step")[L.FD_EC_DT_PHYSICS]
    worst = 0.0
    for k in range(steps):
        x0 = env.x.double().cpu().numpy().T.copy()
        act = _actions(n, k, 0.5)
        env.step_device(act, auto_reset=False)
        a = np.clip(act.cpu().numpy().astype(np.float64), [-1, -1, -1, 0], 1)
        u = np.ascontiguousarray(a[:, [1, 0, 2, 3]])          # oracle order: elevator, aileron, rudder, throttle
        x1 = env.x.double().cpu().numpy().T
        for i in range(n):
            xi = x0[i].copy()
            oracle.backend_step(blocks[i], xi, u[i], 0.02, dtp)
            worst = max(worst, rel_err(x1[i], xi, STATE_ANGLE_COLS).max())
    print(f"\n[dr scales] {precision}: worst per-step rel err {worst:.3e} over {n} envs x {steps} steps")
    assert worst < tol, worst


@pytest.mark.parametrize("precision,tol", [("f64", 1e-9), ("mixed", 1e-4)])
def test_wind_by_galilean_invariance_against_oracle(oracle, precision, tol):
    n, steps = 2048, 200                             # 2048 x 200 host oracle steps per precision (~20 s)
    d = Disturbances(wind_speed=(2.0, 6.0), wind_direction=(0.0, 2 * np.pi), wind_vertical=(-1.0, 1.0),
                     turbulence_intensity=(0.05, 0.2), gust_length=(50.0, 200.0))
    env = GpuRateVecEnv(n, "easy", 10.0, 0.02, "step", seed=9, precision=precision, disturbances=d)
    env.reset()
    P = AircraftParams().to_block()
    dt, dtp = 0.02, samplers.env_consts("easy", 10.0, 0.02, "step")[L.FD_EC_DT_PHYSICS]
    vmax, amax = P[L.FD_P_MAX_VELOCITY], P[L.FD_P_MAX_ACCELERATION]
    excluded = np.zeros(n, bool)
    worst = np.zeros(n)
    for k in range(steps):
        x0 = env.x.double().cpu().numpy()
        W = _air(env)
        act = _actions(n, k, 0.15)
        env.step_device(act, auto_reset=False)
        x1 = env.x.double().cpu().numpy()
        a = np.clip(act.cpu().numpy().astype(np.float64), [-1, -1, -1, 0], 1)
        u = np.ascontiguousarray(a[:, [1, 0, 2, 3]])
        xa = x0.copy()
        xa[3:6] -= _body(x0, W)                      # to air-relative coordinates
        acc = np.zeros(n, bool)
        for i in np.flatnonzero(~excluded):
            xi = np.ascontiguousarray(xa[:, i])
            # the derivative clamp on dv/dt acts on a frame-dependent quantity (dv_air/dt = dv/dt + omega x R^T W)
            acc[i] = np.abs(oracle.dynamics(P, xi, u[i])[3:6]).max() > 0.5 * amax
            oracle.backend_step(P, xi, u[i], dt, dtp)
            xa[:, i] = xi
        xb = xa.copy()                               # ... and back
        xb[0:3] += W * dt
        xb[3:6] += _body(xa, W)
        # a clamp acts on the stored (ground-relative) state in the kernel and on the air-relative one in the oracle
        clamp = (np.abs(x1[3:6]).max(0) > 0.95 * vmax) | (np.abs(xa[3:6]).max(0) > 0.95 * vmax) | (-x1[2] < 1.0) | \
                (np.abs(x1[7]) > P[L.FD_P_MAX_PITCH_RAD] - 1e-3) | (np.abs(x1[9:12]).max(0) > P[L.FD_P_MAX_RATE_RAD] - 1e-3)
        excluded |= clamp | acc
        e = rel_err(x1.T, xb.T, STATE_ANGLE_COLS).max(1)
        worst = np.where(excluded, worst, np.maximum(worst, e))
        # the next step starts from the kernel's state (no error accumulation)
    kept = ~excluded
    print(f"\n[dr wind] {precision}: worst per-step rel err {worst[kept].max():.3e} over {kept.sum()} envs x {steps} steps "
          f"({excluded.sum()} excluded for a clamp)")
    assert kept.sum() > n // 4
    assert worst[kept].max() < tol


def test_gust_process_statistics():
    n, steps = 65536, 500
    d = Disturbances(turbulence_intensity=(0.05, 0.3), gust_length=(30.0, 300.0), wind_speed=(0.0, 5.0),
                     wind_direction=(0.0, 2 * np.pi))
    env = GpuRateVecEnv(n, "medium", 10.0, 0.02, "step", seed=77, precision="mixed", disturbances=d)
    env.reset()
    dr = env.dr
    A, B = dr[L.FD_DR_GUST_A].clone(), dr[L.FD_DR_GUST_B].clone()
    sigma = B / torch.sqrt(1 - A * A)
    g0 = dr[L.FD_DR_GUST_N:L.FD_DR_GUST_D + 1] / sigma
    assert abs(g0.mean().item()) < 0.01 and abs(g0.var().item() - 1) < 0.02
    g = dr[L.FD_DR_GUST_N:L.FD_DR_GUST_D + 1].clone()
    s1 = torch.zeros(3, dtype=torch.float64, device=dr.device)
    s2, lag, cross = s1.clone(), s1.clone(), s1.clone()
    prev = None
    sub = torch.randperm(n, generator=torch.Generator().manual_seed(0))[:2000].to(dr.device)
    hist = []
    for k in range(steps):
        env.step_device(_actions(n, k, 0.2), auto_reset=False)
        gn = dr[L.FD_DR_GUST_N:L.FD_DR_GUST_D + 1].clone()
        z = (gn - A * g) / B                              # the normals the kernel drew
        s1 += z.sum(1)
        s2 += (z * z).sum(1)
        cross += torch.stack([(z[0] * z[1]).sum(), (z[1] * z[2]).sum(), (z[0] * z[2]).sum()])
        if prev is not None:
            lag += (z * prev).sum(1)
        hist.append(z[:, sub].T.cpu())
        prev, g = z, gn
    m = n * steps
    mean, var = (s1 / m).cpu().numpy(), (s2 / m).cpu().numpy()
    lag1, xc = (lag / (n * (steps - 1))).cpu().numpy(), (cross / m).cpu().numpy()
    bound = 5 / np.sqrt(m)
    print(f"\n[dr gust] mean {mean}, var {var}, lag-1 {lag1}, cross {xc}")
    assert np.all(np.abs(mean) < bound) and np.all(np.abs(var - 1) < 10 * bound)
    assert np.all(np.abs(lag1) < bound * 1.5) and np.all(np.abs(xc) < bound * 1.5)
    h = torch.stack(hist, 0).numpy()                       # [steps][2000][3]
    x = h[:, :, 0]
    rng = np.random.default_rng(0)
    pairs = rng.choice(2000, size=(1000, 2), replace=True)
    pairs = pairs[pairs[:, 0] != pairs[:, 1]]
    c = np.array([np.corrcoef(x[:, i], x[:, j])[0, 1] for i, j in pairs])
    print(f"[dr gust] env pairs: mean corr {c.mean():.4f}, max |corr| {np.abs(c).max():.3f}")
    assert abs(c.mean()) < 5 / np.sqrt(steps * len(c)) and np.abs(c).max() < 6 / np.sqrt(steps)


def test_reset_draws():
    n = 65536
    env = GpuRateVecEnv(n, "medium", 10.0, 0.02, "step", seed=3, precision="f64", disturbances=DOC)
    env.reset()
    dr = env.dr.cpu().numpy()
    x = env.x.cpu().numpy()
    W = dr[0:3]
    spd = np.hypot(W[0], W[1])
    assert spd.min() >= 0 and spd.max() <= 5 + 1e-9 and np.all(W[2] == 0)
    airspeed = np.linalg.norm(x[3:6] - _body(x, _air(env)), axis=0)           # the record's airspeed, air-relative
    assert airspeed.min() >= 15 - 1e-9 and airspeed.max() <= 30 + 1e-9
    A, B = dr[L.FD_DR_GUST_A], dr[L.FD_DR_GUST_B]
    sigma = B / np.sqrt(1 - A * A)
    intensity, Lg = sigma / airspeed, -0.02 * airspeed / np.log(A)
    assert intensity.min() >= -1e-12 and intensity.max() <= 0.3 + 1e-9
    assert np.allclose(Lg, 100.0, rtol=1e-9)
    for slot, (lo, hi) in [(L.FD_DR_MASS_S, DOC.mass), (L.FD_DR_IXX_S, DOC.inertia_xx), (L.FD_DR_IYY_S, DOC.inertia_yy),
                           (L.FD_DR_IZZ_S, DOC.inertia_zz), (L.FD_DR_RHO_S, DOC.air_density)]:
        assert dr[slot].min() >= lo and dr[slot].max() <= hi and np.ptp(dr[slot]) > 0.9 * (hi - lo)
    # same seed, same draws; a new episode, new draws
    env2 = GpuRateVecEnv(n, "medium", 10.0, 0.02, "step", seed=3, precision="f64", disturbances=DOC)
    env2.reset()
    assert torch.equal(env.dr, env2.dr) and torch.equal(env.x, env2.x)
    env2.reset()
    assert np.mean(env2.dr.cpu().numpy()[L.FD_DR_MASS_S] == dr[L.FD_DR_MASS_S]) < 0.01
    # IC and command draws are those of the plain env
    plain = GpuRateVecEnv(n, "medium", 10.0, 0.02, "step", seed=3, precision="f64")
    plain.reset()
    keep = [0, 1, 2, 6, 7, 8, 9, 10, 11]
    assert torch.equal(plain.x[keep], env.x[keep]) and torch.equal(plain.e, env.e) and torch.equal(plain.ei, env.ei)
    assert np.allclose(airspeed, plain.x[3].cpu().numpy(), rtol=1e-12)
    # REDRAW = 0: host-written rows survive resets
    fixed = Disturbances(redraw=False)
    env.set_disturbances(fixed)
    rows = env.dr.clone()
    rows[L.FD_DR_WIND_N] = 3.0
    rows[L.FD_DR_MASS_S] = 1.05
    env.dr.copy_(rows)
    env.reset()
    assert torch.equal(env.dr, rows)
    # parity sampling: obs[9] is the pool's airspeed
    par = GpuRateVecEnv(1024, "medium", 10.0, 0.02, "step", seed=4, precision="f64", sampling="parity", pool_depth=2,
                        disturbances=DOC)
    obs = par.reset().cpu().numpy()
    pool = par.pool.cpu().numpy()
    assert np.allclose(obs[:, 9], pool[:, 0, L.FD_R_AIRSPEED].astype(np.float32), rtol=1e-6)


def test_air_relative_observation_and_stall():
    d = Disturbances(redraw=False)
    env = GpuRateVecEnv(64, "easy", 10.0, 0.02, "step", seed=1, precision="f64", disturbances=d)
    env.reset()
    env.dr[L.FD_DR_WIND_N] = 6.0                        # 6 m/s tailwind (the air moves north, the aircraft flies north)
    env.dr[L.FD_DR_GUST_N:L.FD_DR_GUST_B + 1] = 0.0
    env.x.zero_()
    env.x[2] = -100.0
    env.x[3] = 13.0                                     # ground speed 13 m/s, heading north, level
    env.step_device(torch.tensor([[0.0, 0.0, 0.0, 0.5]] * 64, device=env.device), auto_reset=False)
    obs = env.obs.cpu().numpy()
    assert np.allclose(obs[:, 9], 7.0, atol=0.2), obs[:, 9]
    assert env.terminated.bool().all()
    # the same state in still air flies on
    env.dr[L.FD_DR_WIND_N] = 0.0
    env.x.zero_()
    env.x[2] = -100.0
    env.x[3] = 13.0
    env.step_device(torch.tensor([[0.0, 0.0, 0.0, 0.5]] * 64, device=env.device), auto_reset=False)
    assert np.allclose(env.obs.cpu().numpy()[:, 9], 13.0, atol=0.3) and not env.terminated.bool().any()


@pytest.mark.parametrize("n", [4096, 65536 + 256])
def test_graph_capture_equals_eager(n):
    envs = [GpuRateVecEnv(n, "medium", 10.0, 0.02, "step", seed=12, precision="mixed", disturbances=DOC) for _ in range(2)]
    for e in envs:
        e.reset()
    acts = [_actions(n, k) for k in range(50)]
    act_buf = acts[0].clone()
    eager, graphed = envs
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                          # warm-up outside the capture on a scratch env
        w = GpuRateVecEnv(n, "medium", 10.0, 0.02, "step", seed=12, precision="mixed", disturbances=DOC)
        w.reset()
        w.step_device(act_buf)
    torch.cuda.current_stream().wait_stream(s)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        graphed.step_device(act_buf)
    for k in range(50):
        eager.step_device(acts[k])
        act_buf.copy_(acts[k])
        gr.replay()
    torch.cuda.synchronize()
    for t in ("x", "e", "ei", "dr", "obs", "rewards_full", "terminated", "truncated"):
        assert torch.equal(getattr(eager, t), getattr(graphed, t)), t


def test_disturbances_degrade_pid_tracking():
    from hcrl_amd.eval_metrics import evaluate_pid_controller
    m_calm, _ = evaluate_pid_controller(n_episodes=4096, difficulty="medium", seed=2, precision="mixed")
    m_dr, _ = evaluate_pid_controller(n_episodes=4096, difficulty="medium", seed=2, precision="mixed", disturbances=DOC)
    r_calm = m_calm[L.FD_M_RMSE].mean().item()
    r_dr = m_dr[L.FD_M_RMSE].mean().item()
    print(f"\n[dr effect] PID tracking RMSE medium/mixed: calm {r_calm:.4f}, design-doc ranges {r_dr:.4f}")
    assert r_dr > r_calm


def test_argument_errors():
    lib = _lib.load()
    env = GpuRateVecEnv(256, "easy", 10.0, 0.02, "step", seed=0, precision="mixed", disturbances=NEUTRAL)
    env.reset()
    p = _lib.ptr
    base = [p(env.x), p(env.e), p(env.ei), None, None, p(env.env_consts), None, 0, 0, p(env.obs)]
    rc = lib.fdyn_rate_env_reset_dr_mixed(*base, env.n, None, p(env.dr_consts), None)
    assert rc == _lib.FDYN_ERR_NULL
    rc = lib.fdyn_rate_env_reset_dr_mixed(*base, env.n, p(env.dr), None, None)
    assert rc == _lib.FDYN_ERR_NULL
    assert lib.fdyn_rate_env_reset_dr_mixed(*base, 0, p(env.dr), p(env.dr_consts), None) == _lib.FDYN_OK
    act = torch.zeros((256, 4), device=env.device)
    step = [p(env.x), p(env.e), p(env.ei), None, p(env.params), 1, p(env.env_consts), p(act), None, None, None, None, None,
            None, 0, 0, 1, 0.0, p(env.obs), p(env.rewards), None, p(env.terminated), p(env.truncated), None, None, None, None, 0]
    assert lib.fdyn_rate_env_step_dr_mixed(*step, env.n, None, p(env.dr_consts), None) == _lib.FDYN_ERR_NULL
    assert lib.fdyn_rate_env_step_dr_mixed(*step, env.n, p(env.dr), None, None) == _lib.FDYN_ERR_NULL
    assert lib.fdyn_rate_env_step_dr_mixed(*step, 0, p(env.dr), p(env.dr_consts), None) == _lib.FDYN_OK
    assert lib.fdyn_rate_env_step_dr_mixed(*step, env.n, p(env.dr), p(env.dr_consts), None) == _lib.FDYN_OK
    torch.cuda.synchronize()

"""Every in-kernel Philox draw replayed against the host model (tests/philox_numpy.py, itself pinned by
tests/test_device_draw_model.py): the reset record of the rate env on all four reset paths, the random-walk command increment,
the randomisation rows and gusts, the sensor layer's Philox mode and the action noise of the three head kernels.  A wrong counter
word, step, episode, key half or decode still gives well-distributed numbers -- only a value-by-value comparison sees it.

Sizes: n = 1000 (15 full waves and a 40-lane tail, no multiple of the 256-lane block) and n = 65 (one full wave and one lane).

Tolerances.
  * `a + b u` words (fp32, possibly contracted to one FMA): 2 fp32 ulps of max(|a|, |a + b|), half an ulp more for a word that
    is narrowed to an fp32 env row.  Discrete outcomes (count, axes, signs) exactly -- the model reports no lane whose decode sits
    within 2^-20 of a boundary for the seeds used here, and the tests assert that.
  * sqrtf / logf / cosf site (random walk): 1e-5 absolute on the recovered normal: a few fp32 ulps at |z| <= 6 plus the fp32
    rounding of 2 pi u; with fp32 env words, half an ulp of the stored command over the increment's scale on top.
  * fast-intrinsic sites (__logf, __cosf / __sinf, the polynomial sincos): not derivable.  MEASURED below holds the worst
    |z_device - z_model| observed on the MI355X against the float64 model over every case of this file; each bound is 4 x that
    figure and must stay under 1e-2 (a wrong counter moves most lanes by O(1)).  The recovered z of the fp32 rows also carries
    the rounding of the stored word over its sigma (observe: an O(1) fp32 observation over sigma = 0.01).  Every test prints
    its figure before asserting.

MEASURED (worst case on MI355X / bound = 4 x / ceiling 1e-2):
  gust_z        initial gust and gust update, recovered z                 8.3e-07 / 3.3e-06 / 1e-2
  wind_dir      wind direction atan2(E, N) against lo + (hi - lo) u, rad  2.9e-07 / 1.2e-06 / 1e-2
  wind_speed    hypot(N, E) against lo + (hi - lo) u, relative            6.8e-08 / 2.7e-07 / 1e-2
  sensor_f64    NoisySensorInterface f64, recovered z                     2.6e-06 / 1e-05 / 1e-2
  sensor_f32    NoisySensorInterface f32, recovered z                     2.8e-06 / 1.1e-05 / 1e-2
  observe       ObservationNoise.apply (fp32 rows), recovered z           2.2e-05 / 8.8e-05 / 1e-2
  head          the three head kernels, recovered z                       1.7e-06 / 6.8e-06 / 1e-2
"""
import math

import numpy as np
import pytest
import torch

import philox_numpy as pn
from hcrl_amd import _lib, layout as L

gpu = pytest.mark.gpu

MEASURED = {"gust_z": 8.3e-7, "wind_dir": 2.9e-7, "wind_speed": 6.8e-8, "sensor_f64": 2.6e-6, "sensor_f32": 2.8e-6,
            "observe": 2.2e-5, "head": 1.7e-6}

SEEDS = [3, (1 << 40) + 3, 2 ** 63 - 1]                       # the second shares its low key half with the first
SCALES = {"easy": 0.3, "medium": 0.5, "hard": 0.7}
CMDS = {"step": pn.CMD_STEP, "ramp": pn.CMD_RAMP, "sine": pn.CMD_SINE, "random": pn.CMD_RANDOM_WALK}
DT = 0.02
F64 = torch.float64


def _bound(name, worst):
    """Print the figure, then hold it to 4 x the recorded worst case (which itself stays under the 1e-2 ceiling)."""
    bound = 4.0 * MEASURED[name]
    print(f"MEASURED {name}: worst {worst:.4g} (recorded {MEASURED[name]:.4g}, bound {bound:.4g})")
    assert bound < 1e-2, name
    assert worst <= bound, (name, worst, bound)


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _spacing32(v):
    return np.spacing(np.asarray(v, np.float64).astype(np.float32)).astype(np.float64)


def _env(n, difficulty, cmd, seed, precision, episode_time=10.0, **kw):
    from hcrl_amd.rate_env import GpuRateVecEnv
    return GpuRateVecEnv(n, difficulty, episode_time, DT, cmd, seed=seed, precision=precision, sampling="device", **kw)


def _max_rates(env):
    return env.env_consts_host[[L.FD_EC_MAX_RATE_P, L.FD_EC_MAX_RATE_Q, L.FD_EC_MAX_RATE_R]]


# ---- 1. reset records ---------------------------------------------------------------------------------------------------------
def _check_reset(env, key_episode, where):
    """State, env words and counters of the whole fleet right after a reset against the record keyed by `key_episode` [n] (the
    FD_EI_EPISODE each lane had when it was reset)."""
    n, seed, cmd = env.n, env.seed_value, CMDS[env.command_type]
    rec = pn.reset_record(seed, np.arange(n), key_episode, cmd, SCALES[env.difficulty], _max_rates(env))
    assert not rec.ambiguous.any(), (where, "choose another seed: a decode sits on a boundary")
    if seed >> 32:                                              # the model itself depends on the high key half
        low = pn.reset_record(seed & 0xFFFFFFFF, np.arange(n), key_episode, cmd, SCALES[env.difficulty], _max_rates(env))
        assert np.abs(low.rec[:, 0] - rec.rec[:, 0]).max() > 1.0
    torch.cuda.synchronize()
    x, e, ei = _np(env.x), _np(env.e), env.ei.cpu().numpy()
    assert np.array_equal(ei[L.FD_EI_STEP], np.zeros(n, np.int32)), where
    assert np.array_equal(ei[L.FD_EI_EPISODE], key_episode + 1), where
    # state: x[2] = -altitude, x[3] = airspeed, x[6..8] attitude, x[9..11] rates, the rest exactly zero
    want = {L.FD_X_D: (-rec.rec[:, L.FD_R_ALTITUDE], rec.span[:, L.FD_R_ALTITUDE]), L.FD_X_U: (rec.rec[:, L.FD_R_AIRSPEED], rec.span[:, L.FD_R_AIRSPEED])}
    for k in range(6):
        want[L.FD_X_ROLL + k] = (rec.rec[:, L.FD_R_ROLL + k], rec.span[:, L.FD_R_ROLL + k])
    for row in range(L.FD_NX):
        if row not in want:
            assert not x[row].any(), (where, "state row", row)
            continue
        val, span = want[row]
        over = np.abs(x[row] - val) - 2.0 * _spacing32(span)
        assert over.max() <= 0.0, (where, "state row", row, "lane", int(over.argmax()), x[row][over.argmax()], val[over.argmax()])
    # command words: FD_E_CMD_* for a step command, FD_E_SCHED* for ramp / sine, nothing for the random walk
    ulps = 2.0 + (0.5 if env.e.dtype == torch.float32 else 0.0)
    got_cmd, got_sched = e[L.FD_E_CMD_P:L.FD_E_CMD_R + 1].T, e[L.FD_E_SCHED0:L.FD_E_SCHED3 + 1].T
    if cmd == pn.CMD_STEP:
        got, other = np.concatenate([got_cmd, np.zeros((n, 1))], 1), got_sched
    elif cmd in (pn.CMD_RAMP, pn.CMD_SINE):
        got, other = got_sched, got_cmd
    else:
        got, other = np.zeros((n, 4)), np.concatenate([got_cmd, got_sched], 1)
    assert not other.any(), (where, "command words of another command type are set")
    model, span = rec.rec[:, L.FD_R_CMD0:], rec.span[:, L.FD_R_CMD0:]
    active = rec.position < rec.count[:, None]
    # discrete outcomes first, exactly: how many axes, which, and their signs
    assert np.array_equal((got[:, :3] != 0.0).sum(1), rec.count), (where, "number of active axes")
    assert np.array_equal(got[:, :3] != 0.0, active), (where, "which axes are active")
    assert np.array_equal(got[:, :3] < 0.0, rec.negative & active), (where, "signs")
    over = np.abs(got - model) - ulps * _spacing32(span)
    assert over.max() <= 0.0, (where, "command word", np.unravel_index(int(over.argmax()), over.shape))
    assert np.array_equal(got[span == 0.0], np.zeros(int((span == 0.0).sum()))), where
    # the other per-episode words of the reset
    assert np.array_equal(e[L.FD_E_PREV_THR], np.full(n, 0.5)) and not e[L.FD_E_TIME].any() and not e[L.FD_E_EP_RETURN].any(), where


@gpu
@pytest.mark.parametrize("n,seed", [(1000, SEEDS[0]), (1000, SEEDS[1]), (1000, SEEDS[2]), (65, SEEDS[0])],
                         ids=["n1000-seed3", "n1000-seed2p40p3", "n1000-seed2p63m1", "n65-seed3"])
@pytest.mark.parametrize("difficulty", ["easy", "hard"])
@pytest.mark.parametrize("cmd", ["step", "ramp", "sine", "random"])
@pytest.mark.parametrize("precision", ["f64", "mixed"])
def test_reset_records_match_the_model_on_every_reset_path(precision, cmd, difficulty, n, seed):
    """reset(), a second reset(), a masked reset (only the masked lanes draw and advance their episode) and the in-kernel
    auto-reset of the step kernel (episode_time 0.06 s: every lane truncates at its third step), each against the record the
    model draws for (seed, lane, the FD_EI_EPISODE the lane had).  Exact: counters, zero rows, number / choice / signs of the
    active axes.  Continuous words: 2 fp32 ulps of max(|a|, |a + b|), +0.5 for fp32 env rows."""
    env = _env(n, difficulty, cmd, seed, precision, episode_time=0.06)
    assert int(env.env_consts_host[L.FD_EC_MAX_STEPS]) == 3
    env.reset()
    _check_reset(env, np.zeros(n, np.int64), "first reset")
    env.reset()
    _check_reset(env, np.ones(n, np.int64), "second reset")
    mask = (np.arange(n) % 3 == 0)
    env.reset(torch.as_tensor(mask, device=env.device))
    key = np.where(mask, 2, 1).astype(np.int64)
    _check_reset(env, key, "masked reset")
    zero = torch.zeros((n, L.FD_ACT_DIM), device=env.device)
    for k in range(3):
        env.step_device(zero, auto_reset=True)
        torch.cuda.synchronize()
        trunc, term = env.truncated.cpu().numpy(), env.terminated.cpu().numpy()
        assert not term.any() and np.array_equal(trunc, np.full(n, int(k == 2), np.uint8)), ("step", k)
    _check_reset(env, key + 1, "auto-reset in the step kernel")


# ---- 2. random-walk increments -----------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("seed", SEEDS, ids=["seed3", "seed2p40p3", "seed2p63m1"])
@pytest.mark.parametrize("difficulty", ["easy", "hard"])
@pytest.mark.parametrize("precision,n", [("f64", 1000), ("mixed", 1000), ("f64", 65)])
def test_random_walk_increments_match_the_model(precision, n, difficulty, seed):
    """command_type "random", rw_delta = None, no auto-reset, zero actions: three steps in the first episode, a reset, two steps in
    the second.  cmd' = clip(cmd + delta) with delta = z 0.1 sqrt(dt) scale max_rate and z keyed by (lane, FD_EI_EPISODE as
    stored, FD_EI_STEP after the increment, word 7).  The recovered z against the model to 1e-5 (fp32 env rows: plus half an ulp
    of the stored command over the increment's scale); lanes the model clips are left out, at most 5 %."""
    env = _env(n, difficulty, "random", seed, precision)
    mr, scale = _max_rates(env), SCALES[difficulty]
    unit = (0.1 * math.sqrt(DT) * scale) * mr[None, :]
    zero = torch.zeros((n, L.FD_ACT_DIM), device=env.device)
    lanes = np.arange(n)
    env.reset()
    seen, worst, left_out = [], 0.0, 0
    for k in range(5):
        if k == 3:
            env.reset()
        torch.cuda.synchronize()
        cmd0, ei0 = _np(env.e[L.FD_E_CMD_P:L.FD_E_CMD_R + 1]).T, env.ei.cpu().numpy()
        assert np.array_equal(ei0[L.FD_EI_EPISODE], np.full(n, 1 if k < 3 else 2)) and np.array_equal(ei0[L.FD_EI_STEP], np.full(n, k % 3))
        env.step_device(zero, auto_reset=False)
        torch.cuda.synchronize()
        assert not env.terminated.any() and not env.truncated.any()
        cmd1 = _np(env.e[L.FD_E_CMD_P:L.FD_E_CMD_R + 1]).T
        z = pn.random_walk_normals(seed, lanes, ei0[L.FD_EI_EPISODE], ei0[L.FD_EI_STEP] + 1)
        seen.append(z)
        free = (np.abs(cmd0 + z * unit) < mr[None, :]).all(1)
        left_out += int((~free).sum())
        tol = 1e-5 + (0.5 * _spacing32(np.abs(cmd1)) / unit if env.e.dtype == torch.float32 else 0.0)
        err = np.abs((cmd1 - cmd0) / unit - z) - tol
        assert err[free].max() <= 0.0, ("step", k, "lane", int(err.max(1).argmax()))
        worst = max(worst, float(np.abs((cmd1 - cmd0) / unit - z)[free].max()))
        direct = np.abs(cmd1 - np.clip(cmd0 + z * unit, -mr, mr)) - tol * unit
        assert direct.max() <= 0.0, ("step", k)
    print(f"random walk: worst |z_device - z_model| = {worst:.3g}")
    assert left_out <= 0.05 * 5 * n
    for a in range(5):                                          # five different blocks: neither the step nor the episode stands still
        for b in range(a + 1, 5):
            assert np.abs(seen[a] - seen[b]).max() > 1.0


# ---- 3. randomisation rows and gusts ------------------------------------------------------------------------------------------
def _gust_coefficients(v, V0):
    a = np.exp(-DT * V0 / v[:, 4])
    return a, v[:, 3] * V0 * np.sqrt(1.0 - a * a)


@gpu
@pytest.mark.parametrize("seed", SEEDS, ids=["seed3", "seed2p40p3", "seed2p63m1"])
def test_randomisation_rows_and_gusts_match_the_model(seed):
    """The documented ranges, f64, n = 1000: reset, three steps, reset, two steps (zero actions, no auto-reset).
    Multipliers and vertical wind are `lo + (hi - lo) double(u)` stored as they are: relative 1e-12.  The wind's speed and
    direction reach the rows through the fp32 polynomial sincos (N = speed cos, E = speed sin), so hypot and atan2 of the rows
    are held to the measured rule, like the normals of the initial gust (g0 / sigma, sigma from the stored A and B) and of each
    gust update ((g' - A g) / B).  A and B must lie between their values at the model airspeed -+ 2 fp32 ulps.
    Measured on MI355X (worst / bound 4 x / ceiling): recovered z 8.3e-7 / 3.3e-6 / 1e-2, direction 2.9e-7 / 1.2e-6 / 1e-2 rad,
    speed 6.8e-8 / 2.7e-7 / 1e-2 relative."""
    from hcrl_amd.disturbances import Disturbances
    n, lanes = 1000, np.arange(1000)
    d = Disturbances.design_doc()
    env = _env(n, "medium", "step", seed, "f64", disturbances=d)
    consts = d.block()
    zero = torch.zeros((n, L.FD_ACT_DIM), device=env.device)
    worst = {"gust_z": 0.0, "wind_dir": 0.0, "wind_speed": 0.0}
    step_z = []
    for episode_key in (0, 1):
        env.reset()
        torch.cuda.synchronize()
        dr, ei = _np(env.dr), env.ei.cpu().numpy()
        assert np.array_equal(ei[L.FD_EI_EPISODE], np.full(n, episode_key + 1))
        v = pn.dr_reset_values(seed, lanes, episode_key, consts)
        for row, col in ((L.FD_DR_MASS_S, 5), (L.FD_DR_IXX_S, 6), (L.FD_DR_IYY_S, 7), (L.FD_DR_IZZ_S, 8), (L.FD_DR_RHO_S, 9),
                         (L.FD_DR_WIND_D, 2)):
            over = np.abs(dr[row] - v[:, col]) - 1e-12 * np.abs(v[:, col])
            assert over.max() <= 0.0, ("row", row, "episode", episode_key, int(over.argmax()))
        speed, direction = np.hypot(dr[L.FD_DR_WIND_N], dr[L.FD_DR_WIND_E]), np.arctan2(dr[L.FD_DR_WIND_E], dr[L.FD_DR_WIND_N])
        worst["wind_speed"] = max(worst["wind_speed"], float((np.abs(speed - v[:, 0]) / v[:, 0]).max()))
        dd = (direction - v[:, 1] + np.pi) % (2 * np.pi) - np.pi
        worst["wind_dir"] = max(worst["wind_dir"], float(np.abs(dd).max()))
        # gust coefficients: exp and sqrt in fp64 on the record's fp32 airspeed
        rec = pn.reset_record(seed, lanes, episode_key, pn.CMD_STEP, SCALES["medium"], _max_rates(env))
        V0, dV = rec.rec[:, L.FD_R_AIRSPEED], 2.0 * _spacing32(rec.span[:, L.FD_R_AIRSPEED])
        (a_hi, b_lo), (a_lo, b_hi) = _gust_coefficients(v, V0 - dV), _gust_coefficients(v, V0 + dV)
        A, B = dr[L.FD_DR_GUST_A], dr[L.FD_DR_GUST_B]
        assert np.all(A >= a_lo * (1 - 1e-12)) and np.all(A <= a_hi * (1 + 1e-12)), ("gust A", episode_key)
        assert np.all(B >= b_lo * (1 - 1e-12)) and np.all(B <= b_hi * (1 + 1e-12)), ("gust B", episode_key)
        z0 = dr[L.FD_DR_GUST_N:L.FD_DR_GUST_D + 1].T * (np.sqrt(1.0 - A * A) / B)[:, None]
        worst["gust_z"] = max(worst["gust_z"], float(np.abs(z0 - pn.dr_initial_gust_normals(seed, lanes, episode_key)).max()))
        for k in range(3 if episode_key == 0 else 2):
            g0 = _np(env.dr[L.FD_DR_GUST_N:L.FD_DR_GUST_D + 1]).T
            env.step_device(zero, auto_reset=False)
            torch.cuda.synchronize()
            assert not env.terminated.any() and not env.truncated.any()
            dr1 = _np(env.dr)
            assert np.array_equal(dr1[L.FD_DR_GUST_A], A) and np.array_equal(dr1[L.FD_DR_MASS_S:], dr[L.FD_DR_MASS_S:])
            z = (dr1[L.FD_DR_GUST_N:L.FD_DR_GUST_D + 1].T - A[:, None] * g0) / B[:, None]
            zm = pn.gust_normals(seed, lanes, episode_key + 1, k + 1)       # stored episode, step after the increment
            step_z.append(zm)
            worst["gust_z"] = max(worst["gust_z"], float(np.abs(z - zm).max()))
    for name in ("wind_speed", "wind_dir", "gust_z"):
        _bound(name, worst[name])
    for a in range(5):
        for b in range(a + 1, 5):
            assert np.abs(step_z[a] - step_z[b]).max() > 1.0


# ---- 4. sensor layer, Philox mode ---------------------------------------------------------------------------------------------
X_CONST = [1.5, -2.5, -3.0, 2.0, 0.5, -0.25, 0.1, -0.2, 0.3, 0.01, -0.02, 0.03]        # altitude 3 m, airspeed sqrt(4.3125)


@gpu
@pytest.mark.parametrize("seed", [SEEDS[0], SEEDS[1]], ids=["seed3", "seed2p40p3"])
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_sensor_update_normals_match_the_model(precision, seed):
    """NoisySensorInterface.update on a constant state, n = 1000, three updates: all 20 normals recovered -- 14 from the
    measurement rows (the gyro rows after taking off the bias the model accumulated over the earlier updates), 6 from the
    increments of the two bias walks -- against the model keyed by (row, update count including this update).
    Measured on MI355X (worst / bound 4 x / ceiling): f64 2.6e-6 / 1.0e-5 / 1e-2, f32 2.8e-6 / 1.1e-5 / 1e-2."""
    from hcrl_amd.sensors import NoisySensorInterface, noise_block
    n, rows = 1000, np.arange(1000)
    s = NoisySensorInterface({"seed": seed}, n, precision)
    cfg = noise_block({"seed": seed})
    dt = s.dtype
    x = torch.tensor(X_CONST, dtype=F64)[:, None].repeat(1, n).to(dt).cuda().contiguous()
    xv = _np(x)[:, 0]
    airspeed = float(torch.tensor(math.sqrt(xv[3] ** 2 + xv[4] ** 2 + xv[5] ** 2), dtype=F64).to(dt))
    truth = np.concatenate([xv, [airspeed, -xv[2]]])
    sigma = np.array([cfg[L.FD_SN_GPS_POS]] * 3 + [cfg[L.FD_SN_GPS_VEL]] * 3 + [cfg[L.FD_SN_ATTITUDE]] * 3 + [cfg[L.FD_SN_GYRO]] * 3
                     + [cfg[L.FD_SN_AIRSPEED], cfg[L.FD_SN_ALTITUDE]])
    zcol = list(range(L.FD_SZ_POS, L.FD_SZ_POS + 3)) + list(range(L.FD_SZ_VEL, L.FD_SZ_VEL + 3)) + \
        list(range(L.FD_SZ_ATT, L.FD_SZ_ATT + 3)) + list(range(L.FD_SZ_GYRO, L.FD_SZ_GYRO + 3)) + [L.FD_SZ_AIRSPEED, L.FD_SZ_ALTITUDE]
    walk = np.array([cfg[L.FD_SN_GYRO_BIAS_WALK]] * 3 + [cfg[L.FD_SN_ACCEL_BIAS_WALK]] * 3)
    bias_model, bias_prev, worst, blocks = np.zeros((6, n)), np.zeros((6, n)), 0.0, []
    for t in range(3):
        s.update(x)
        torch.cuda.synchronize()
        assert int(s._step) == t + 1
        zm = pn.sensor_normals(seed, rows, t + 1)                              # [n, 20]
        blocks.append(zm)
        meas, bias = _np(s.get_state()), _np(s._bias)
        shift = np.zeros((L.FD_NMS, n))
        shift[L.FD_X_P:L.FD_X_R + 1] = bias_model[:3]                          # the gyro bias of the earlier updates
        z_meas = (meas - truth[:, None] - shift) / sigma[:, None]
        worst = max(worst, float(np.abs(z_meas.T - zm[:, zcol]).max()))
        z_bias = (bias - bias_prev) / walk[:, None]
        worst = max(worst, float(np.abs(z_bias.T - zm[:, L.FD_SZ_GYRO_BIAS:L.FD_SZ_GYRO_BIAS + 6]).max()))
        bias_model += walk[:, None] * zm[:, L.FD_SZ_GYRO_BIAS:L.FD_SZ_GYRO_BIAS + 6].T
        bias_prev = bias
    _bound("sensor_" + precision, worst)
    assert np.abs(blocks[0] - pn.sensor_normals(seed, rows, 0)).max() > 1.0                  # first update: step 1, not 0
    assert np.abs(blocks[0] - blocks[1]).max() > 1.0 and np.abs(blocks[1] - blocks[2]).max() > 1.0


@gpu
@pytest.mark.parametrize("n", [1000, 65])
def test_observation_noise_normals_match_the_model(n):
    """ObservationNoise.apply without z on an asymmetric random observation block, twice, the second time with a reset mask (a
    masked lane starts from a zero gyro bias): the ten normals it consumes recovered from the changed columns and the bias
    increment; the rate errors are recomputed from the noisy rates exactly; the columns it does not own are untouched.
    Measured on MI355X (worst / bound 4 x / ceiling): 2.2e-5 / 8.8e-5 / 1e-2 (the fp32 rounding of an O(1) row over sigma 0.01)."""
    from hcrl_amd.sensors import ObservationNoise, noise_block
    seed, rows = SEEDS[1], np.arange(n)
    cfg = noise_block({"seed": seed})
    on = ObservationNoise({"seed": seed}, n)
    g = torch.Generator().manual_seed(77 + n)
    on.gyro_bias.copy_((torch.randn(3, n, generator=g) * 2e-4).cuda())
    worst = 0.0
    for t in range(2):
        obs0 = (torch.randn(n, L.FD_OBS_DIM, generator=g) * 0.7 + 0.2).cuda().contiguous()
        mask = None if t == 0 else (torch.arange(n) % 4 == 1).to(torch.uint8).cuda()
        bias0 = _np(on.gyro_bias)
        if mask is not None:
            bias0 = np.where(_np(mask)[None, :] != 0, 0.0, bias0)
        obs = on.apply(obs0.clone(), mask)
        torch.cuda.synchronize()
        o0, o1, bias1 = _np(obs0), _np(obs), _np(on.gyro_bias)
        zm = pn.sensor_normals(seed, rows, t + 1)
        z_gyro = (o1[:, 0:3] - bias0.T - o0[:, 0:3]) / cfg[L.FD_SN_GYRO]
        z_att = (o1[:, 11:14] - o0[:, 11:14]) / cfg[L.FD_SN_ATTITUDE]
        z_as, z_alt = (o1[:, 9] - o0[:, 9]) / cfg[L.FD_SN_AIRSPEED], (o1[:, 10] - o0[:, 10]) / cfg[L.FD_SN_ALTITUDE]
        z_walk = (bias1 - bias0).T / cfg[L.FD_SN_GYRO_BIAS_WALK]
        for got, col in ((z_gyro, L.FD_SZ_GYRO), (z_att, L.FD_SZ_ATT), (z_walk, L.FD_SZ_GYRO_BIAS)):
            worst = max(worst, float(np.abs(got - zm[:, col:col + 3]).max()))
        worst = max(worst, float(np.abs(z_as - zm[:, L.FD_SZ_AIRSPEED]).max()), float(np.abs(z_alt - zm[:, L.FD_SZ_ALTITUDE]).max()))
        assert torch.equal(obs[:, 6:9], obs0[:, 3:6] - obs[:, 0:3])
        keep = [3, 4, 5, 14, 15, 16, 17]
        assert torch.equal(obs[:, keep], obs0[:, keep])
    _bound("observe", worst)


# ---- 5. action noise ----------------------------------------------------------------------------------------------------------
LOG_STD = [0.0, -0.5, 0.3, -1.0]
HEAD_SEED = (0x5eed << 32) + 1234
SENT = 768.0
STEP_WORDS = [pytest.param(0, id="step0"), pytest.param(1, id="step1"), pytest.param(0xFFFFFFFF, id="step_all_ones"),
              pytest.param(None, id="null_pointer")]


def _p(t):
    return None if t is None else t.data_ptr()


def _head_inputs(kind, B):
    """Operands of one head kernel with O(1) means: (arguments in front of log_std, has a value output)."""
    g = torch.Generator().manual_seed(4100 + B)
    r = lambda *s: torch.randn(*s, generator=g)                                  # noqa: E731
    BF = torch.bfloat16
    if kind in ("gaussian_f32", "gaussian_bf16"):
        mean = r(B, 4) * 1.3 + 0.4
        return [(mean.to(BF) if kind == "gaussian_bf16" else mean).cuda().contiguous()]
    Wa = (r(4, 64) * 0.1 * torch.tensor([0.5, 1.0, 1.7, 2.6])[:, None]).to(BF)
    ba, wv, bv = torch.tensor([0.3, -0.7, 1.1, -0.2]).to(BF), (r(64) * 0.2).to(BF), torch.tensor([0.45]).to(BF)
    if kind == "heads":
        lat = [(r(B, 64) * 0.7 + 0.3).to(BF) for _ in range(2)]
        return [t.cuda().contiguous() for t in (lat[0], lat[1], Wa, ba, wv, bv)]
    from hcrl_amd.policy import _KPERM16
    perm = torch.tensor([16 * (k // 16) + _KPERM16[k % 16] for k in range(128)])
    h = [(r(B, 256) * 0.6).to(BF) for _ in range(2)]
    W1, b1 = (r(2, 128, 256) * 0.08).to(BF), r(2, 128) * 0.2
    W2, b2 = (r(2, 64, 128) * 0.1).to(BF), r(2, 64) * 0.2
    return [t.cuda().contiguous() for t in (h[0], h[1], W1, b1, W2[:, :, perm], b2, Wa, ba, wv, bv)]


def _run_head(kind, args, step_t, det, B):
    lib, st = _lib.load(), _lib.current_stream()
    ls = torch.tensor(LOG_STD, device="cuda")
    a, lp, v = (torch.full(s, SENT, device="cuda") for s in ((B, 4), (B,), (B,)))
    if kind.startswith("gaussian"):
        rc = lib.fdyn_gaussian_head(_p(args[0]), int(kind == "gaussian_bf16"), _p(ls), HEAD_SEED, _p(step_t), det, _p(a), _p(lp), B, st)
    elif kind == "heads":
        rc = lib.fdyn_policy_heads(*(_p(t) for t in args), _p(ls), HEAD_SEED, _p(step_t), det, _p(a), _p(lp), _p(v), B, st)
    else:
        rc = lib.fdyn_policy_trunks_heads(*(_p(t) for t in args), _p(ls), HEAD_SEED, _p(step_t), det, _p(a), _p(lp), _p(v), B, st)
    assert rc == 0
    torch.cuda.synchronize()
    return _np(a), _np(lp)


@gpu
@pytest.mark.parametrize("step", STEP_WORDS)
@pytest.mark.parametrize("kind,B", [("gaussian_f32", 300), ("gaussian_bf16", 300), ("heads", 300), ("trunks_heads", 77)])
def test_action_noise_matches_the_model(kind, B, step):
    """fdyn_gaussian_head (fp32 and bf16 means), fdyn_policy_heads (B = 300) and fdyn_policy_trunks_heads (B = 77): the kernel's
    own mean from a deterministic call, then z = (a - mean) / exp(log_std) of a sampled call against the model keyed by (row,
    the word the step pointer holds: 0, 1, all ones, or no pointer = 0); logp against the closed form of the model's z to 1e-3
    (the figure tests/test_gpu_policy_kernels.py uses).
    Measured on MI355X (worst / bound 4 x / ceiling): 1.7e-6 / 6.8e-6 / 1e-2 over the four kernels and step words."""
    args = _head_inputs(kind, B)
    step_t = None if step is None else torch.tensor([step - (1 << 32) if step >= 1 << 31 else step], dtype=torch.int32, device="cuda")
    word = 0 if step is None else step
    mean, lp_det = _run_head(kind, args, step_t, 1, B)
    a, lp = _run_head(kind, args, step_t, 0, B)
    assert np.abs(mean).max() > 1.0 and np.abs(mean).max() < 100.0                # every row written, visible means
    std = np.exp(np.array(LOG_STD))
    z, zm = (a - mean) / std[None, :], pn.head_normals(HEAD_SEED, np.arange(B), word)
    closed = (-0.5 * zm ** 2 - np.array(LOG_STD)[None, :] - 0.5 * math.log(2 * math.pi)).sum(1)
    worst = float(np.abs(z - zm).max())
    _bound("head", worst)
    assert np.abs(lp - closed).max() < 1e-3
    assert np.abs(lp_det - (-np.array(LOG_STD) - 0.5 * math.log(2 * math.pi)).sum()).max() < 1e-3
    # the model's blocks of neighbouring steps, of step 0 under the low key half alone, and of the row above are all different
    for other in (pn.head_normals(HEAD_SEED, np.arange(B), (word + 1) & 0xFFFFFFFF), pn.head_normals(HEAD_SEED & 0xFFFFFFFF, np.arange(B), word),
                  pn.head_normals(HEAD_SEED, np.arange(B) + 1, word)):
        assert np.abs(other - zm).max() > 1.0

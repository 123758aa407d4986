"""Host model of every in-kernel random draw (`sampling="device"`, the Philox mode of the sensor layer, the policy's action
noise): Philox-4x32-10 written from the published algorithm (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as
1, 2, 3", SC'11 -- the Random123 philox4x32 with 10 rounds) and one function per consumer that returns what the kernel must
produce for a given key and counter.  NumPy only; nothing here imports the product package, so the model cannot inherit a
mistake from it.  Uniforms are float32 exactly as the device forms them; everything after them is float64.

Counter layouts (the key is always the 64-bit seed: low half k0, high half k1):

  consumer                         c0       c1        c2     c3                 step / episode that keys the draw
  reset record (IC + command)      env      episode   0      0..3               episode = FD_EI_EPISODE BEFORE the reset
  randomisation rows at a reset    env      episode   0      16..18             (the reset then stores episode + 1)
  initial gust at a reset          env      episode   0      19
  random-walk command increment    env      episode   step   7                  episode = FD_EI_EPISODE as stored (so: the
  gust update                      env      episode   step   20                 record's episode + 1); step = FD_EI_STEP
                                                                                AFTER this step's increment: 1, 2, 3, ...
  action noise (three heads)       row lo   row hi    step   0x51               step = the word `*step` holds at launch
                                                                                (null pointer: 0); the policy advances it
                                                                                once per rollout step
  sensor normals, block b = 0..4   row lo   row hi    step   0x60 + b           step = update count INCLUDING this update:
                                                                                the host classes add 1 before the launch,
                                                                                so the first update draws with step 1
"""
import numpy as np

U32 = np.uint32
M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)          # the two multipliers of the round function
W0, W1 = 0x9E3779B9, 0xBB67AE85                                # key schedule: golden ratio, sqrt(3) - 1
MASK = np.uint64(0xFFFFFFFF)
SH = np.uint64(32)

# fourth counter word per consumer (include/fdyn_layout.h names the same values FD_PHX_*)
W_RESET, W_RANDOM_WALK, W_DR_RESET, W_DR_GUST0, W_GUST, W_ACTION, W_SENSOR = 0, 7, 16, 19, 20, 0x51, 0x60

CMD_STEP, CMD_RAMP, CMD_SINE, CMD_RANDOM_WALK = 0, 1, 2, 3
AMBIGUOUS = 2.0 ** -20                                         # u * m this close to an integer: the fp32 product may floor either way


def philox(seed, c0, c1, c2, c3):
    """Philox-4x32-10 block(s): key = (seed & 0xffffffff, seed >> 32), counter = (c0, c1, c2, c3), broadcast -> uint32[..., 4]."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    c = [np.asarray(v).astype(np.uint64) & MASK for v in np.broadcast_arrays(c0, c1, c2, c3)]
    for rnd in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]                          # 32 x 32 -> 64-bit products: no overflow in uint64
        key0, key1 = np.uint64((k0 + rnd * W0) & 0xFFFFFFFF), np.uint64((k1 + rnd * W1) & 0xFFFFFFFF)
        c = [(p1 >> SH) ^ c[1] ^ key0, p1 & MASK, (p0 >> SH) ^ c[3] ^ key1, p0 & MASK]
    return np.stack(c, axis=-1).astype(U32)


ONE_BELOW = np.nextafter(np.float32(1.0), np.float32(0.0))     # 0x1.fffffep-1


def u01_unclamped(r):
    """(float(r >> 8) + 0.5f) * 2^-24 in float32 arithmetic: the library's formula before the top-end fix (returns 1.0 for
    r >> 8 == 0xFFFFFF, because 16777215.5 rounds to 2^24)."""
    r = np.asarray(r, dtype=U32)
    return ((r >> U32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 16777216.0)


def u01(r):
    """The device's word -> uniform conversion (csrc/philox.hpp, philox_u01): float32, strictly inside (0, 1)."""
    return np.minimum(u01_unclamped(r), ONE_BELOW)


def _f32(v):
    return float(np.float32(v))


def _row_words(rows):
    rows = np.asarray(rows, dtype=np.int64)
    return (rows & 0xFFFFFFFF).astype(np.uint64), ((rows >> 32) & 0xFFFFFFFF).astype(np.uint64)


# ---- counters, one enumerator per consumer (what test_device_draw_model checks for disjointness) -----------------------------
def reset_counters(env, episode):
    """[..., 4 blocks, 4 words]: the record's blocks.  `episode` is FD_EI_EPISODE before the reset."""
    env, episode = np.broadcast_arrays(np.asarray(env, np.int64), np.asarray(episode, np.int64))
    w = np.arange(4, dtype=np.int64) + W_RESET
    return np.stack(np.broadcast_arrays(env[..., None], episode[..., None], 0, w), -1)


def dr_reset_counters(env, episode):
    """[..., 4 blocks, 4 words]: three blocks of range draws and the initial-gust block; `episode` as reset_counters."""
    env, episode = np.broadcast_arrays(np.asarray(env, np.int64), np.asarray(episode, np.int64))
    w = np.array([W_DR_RESET, W_DR_RESET + 1, W_DR_RESET + 2, W_DR_GUST0], dtype=np.int64)
    return np.stack(np.broadcast_arrays(env[..., None], episode[..., None], 0, w), -1)


def step_counters(env, episode, step, word):
    """[..., 4 words] of a per-step env draw (word = W_RANDOM_WALK or W_GUST): `episode` is FD_EI_EPISODE as the step kernel
    loads it, `step` is FD_EI_STEP after the step's increment (>= 1)."""
    return np.stack(np.broadcast_arrays(np.asarray(env, np.int64), np.asarray(episode, np.int64), np.asarray(step, np.int64),
                                        np.int64(word)), -1)


def row_counters(rows, step, word, blocks=1):
    """[..., blocks, 4 words] of a row-keyed draw (W_ACTION: one block, W_SENSOR: five)."""
    lo, hi = _row_words(rows)
    w = np.arange(blocks, dtype=np.int64) + word
    return np.stack(np.broadcast_arrays(lo.astype(np.int64)[..., None], hi.astype(np.int64)[..., None],
                                        np.int64(int(step) & 0xFFFFFFFF), w), -1)


def _blocks(seed, ctr):
    return philox(seed, ctr[..., 0], ctr[..., 1], ctr[..., 2], ctr[..., 3])


# ---- Box-Muller, float64 on the fp32 uniforms ------------------------------------------------------------------------------
def _two_pi(const):
    return float(np.float32(const))                            # the kernels' fp32 literal, widened


def normals4(r, two_pi=6.283185307):
    """Four normals of one block as the row kernels pair them: (r0, r1) -> cos, sin ; (r2, r3) -> cos, sin."""
    u = u01(r).astype(np.float64)
    ra, rb = np.sqrt(-2.0 * np.log(u[..., 0])), np.sqrt(-2.0 * np.log(u[..., 2]))
    a, b = _two_pi(two_pi) * u[..., 1], _two_pi(two_pi) * u[..., 3]
    return np.stack([ra * np.cos(a), ra * np.sin(a), rb * np.cos(b), rb * np.sin(b)], -1)


def normals3(r, two_pi):
    """Three normals of one block as the env kernels pair them: (r0, r1) -> cos, sin ; (r2, r3) -> cos."""
    return normals4(r, two_pi)[..., :3]


# ---- consumers -------------------------------------------------------------------------------------------------------------
class ResetRecord:
    """What device_reset_record must produce for lanes `env` at `episode`.

    rec        [n, 12] float64, FD_R_* order (command words already times max_rate, zero where the axis is idle)
    span       [n, 12] max(|a|, |a + b|) of the word's `a + b u` (the scale of its fp32 rounding), 0 for exact zeros
    count      [n] number of active axes; first / second [n] the first two entries of the axis permutation
    position   [n, 3] place of axis a in the permutation (0, 1, 2); active = position < count
    negative   [n, 3] sign bit of axis a (bit `position` of word 2 of block 2; never set for sine)
    ambiguous  [n] a discrete draw whose u * m lies within 2^-20 of an integer (fp32 could floor it either way)
    """


def reset_blocks(seed, env, episode):
    """uint32 [n, 4, 4]: the four Philox blocks of the record (they do not depend on the command type or the difficulty)."""
    return _blocks(seed, reset_counters(np.asarray(env, np.int64), episode))


def reset_record(seed, env, episode, cmd_type, scale, max_rates, rate_dtype=np.float64, blocks=None):
    """`episode` = FD_EI_EPISODE before the reset.  `scale` = difficulty scale, `max_rates` [3] fp64 env constants;
    `rate_dtype` = the state dtype the kernel narrows them to; `blocks` = reset_blocks(seed, env, episode) if already at hand."""
    env = np.asarray(env, np.int64)
    r = reset_blocks(seed, env, episode) if blocks is None else blocks
    u = u01(r).astype(np.float64)
    n = env.shape[0]
    d15 = _f32(0.26179938779914943)
    ab = np.zeros((12, 2))
    ab[0], ab[1] = (_f32(15.0), _f32(15.0)), (_f32(50.0), _f32(150.0))
    ab[2] = ab[3] = (-d15, 2.0 * d15)
    ab[4] = (0.0, _f32(6.283185307179586))
    ab[5] = ab[6] = ab[7] = (_f32(-0.1), _f32(0.2))
    out = ResetRecord()
    out.rec, out.span = np.zeros((n, 12)), np.zeros((n, 12))
    for k in range(8):
        out.rec[:, k] = ab[k, 0] + ab[k, 1] * u[:, k // 4, k % 4]
        out.span[:, k] = max(abs(ab[k, 0]), abs(ab[k, 0] + ab[k, 1]))
    out.count = np.zeros(n, np.int64)
    out.first = out.second = np.zeros(n, np.int64)
    out.position = np.tile(np.arange(3), (n, 1))
    out.negative = np.zeros((n, 3), bool)
    out.ambiguous = np.zeros(n, bool)
    if cmd_type == CMD_RANDOM_WALK:
        return out
    sine = cmd_type == CMD_SINE
    m = 2.0 if sine else 3.0
    ck, cp = u[:, 2, 0] * m, u[:, 2, 1] * 6.0
    out.ambiguous = (np.abs(ck - np.rint(ck)) < AMBIGUOUS) | (np.abs(cp - np.rint(cp)) < AMBIGUOUS)
    out.count = np.minimum(1 + np.floor(ck).astype(np.int64), 2 if sine else 3)
    perm = np.floor(cp).astype(np.int64) % 6
    # the permutation (first, second, third) of the axes: `first` = perm // 2, and the low bit picks which of the other two
    # axes comes second -- the one after `first` (cyclically) when clear, the one before when set
    out.first = perm // 2
    out.second = np.where(perm & 1 == 1, (out.first + 2) % 3, (out.first + 1) % 3)
    axes = np.arange(3)[None, :]
    out.position = np.where(axes == out.first[:, None], 0, np.where(axes == out.second[:, None], 1, 2))
    bits = (r[:, 2, 2][:, None].astype(np.int64) >> out.position) & 1
    out.negative = (bits == 1) & (not sine)
    um = np.take_along_axis(u[:, 3, :3], out.position, axis=1)                  # magnitude uniform of each axis' place
    sc = _f32(scale) * (0.5 if sine else 1.0)
    mr = np.asarray(max_rates, np.float64).astype(rate_dtype).astype(np.float64)[None, :]
    active = out.position < out.count[:, None]
    mag = (_f32(0.3) + _f32(0.7) * um) * sc * mr
    out.rec[:, 8:11] = np.where(active, np.where(out.negative, -mag, mag), 0.0)
    out.span[:, 8:11] = np.where(active, (_f32(0.3) + _f32(0.7)) * sc * mr, 0.0)
    if sine:
        out.rec[:, 11] = _f32(0.1) + _f32(1.9) * u[:, 2, 3]
        out.span[:, 11] = _f32(0.1) + _f32(1.9)
    return out


def random_walk_normals(seed, env, episode, step):
    """[n, 3] normals of the random-walk increment (sqrtf / logf / cosf site).  `episode` = FD_EI_EPISODE as stored during the
    episode, `step` = FD_EI_STEP after the increment (the first step of an episode draws with 1)."""
    return normals3(_blocks(seed, step_counters(env, episode, step, W_RANDOM_WALK)), 6.283185307)


def random_walk_delta(seed, env, episode, step, dt, scale, max_rates):
    """[n, 3] increment of the command: normal * 0.1 sqrt(dt) scale * max_rate."""
    return random_walk_normals(seed, env, episode, step) * (0.1 * np.sqrt(dt) * scale) * np.asarray(max_rates, np.float64)[None, :]


def dr_reset_values(seed, env, episode, dr_consts):
    """[n, 10] the ten range draws lo + (hi - lo) u in the order of the FD_DC_* pairs (wind speed, direction, vertical wind,
    turbulence intensity, gust length, mass, ixx, iyy, izz, air density).  `episode` = FD_EI_EPISODE before the reset."""
    r = _blocks(seed, dr_reset_counters(env, episode))[:, :3, :].reshape(-1, 12)[:, :10]
    u = u01(r).astype(np.float64)
    c = np.asarray(dr_consts, np.float64)
    lo, hi = c[0:20:2][None, :], c[1:20:2][None, :]
    return lo + (hi - lo) * u


def dr_initial_gust_normals(seed, env, episode):
    """[n, 3] normals of g0 (fast-intrinsic site); `episode` = FD_EI_EPISODE before the reset."""
    return normals3(_blocks(seed, dr_reset_counters(env, episode))[:, 3, :], 6.283185307179586)


def gust_normals(seed, env, episode, step):
    """[n, 3] normals of the gust update g <- A g + B z (fast-intrinsic site); episode / step as random_walk_normals."""
    return normals3(_blocks(seed, step_counters(env, episode, step, W_GUST)), 6.283185307179586)


def sensor_normals(seed, rows, step):
    """[n, 20] normals of one sensor update in FD_SZ_* order.  `step` = the update count including this update (the host classes
    increment before launching: 1 for the first update)."""
    return normals4(_blocks(seed, row_counters(rows, step, W_SENSOR, 5))).reshape(len(np.atleast_1d(rows)), 20)


def head_normals(seed, rows, step):
    """[n, 4] action-noise normals of the three head kernels.  `step` = the word the step pointer holds at launch (0 for a null
    pointer)."""
    return normals4(_blocks(seed, row_counters(rows, step, W_ACTION, 1))[:, 0, :])

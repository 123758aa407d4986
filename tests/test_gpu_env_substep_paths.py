"""The two sub-step loops of the benched env build against each other.

`fdyn_rate_env_step_img_mixed` (one wave per SIMD, still air) holds the RK4 sub-step loop twice: the general one, and one whose
dynamics evaluation has no rare block -- taken when the image's FD_ECD_SMALL_STEPS word says that no Euler angle can move by more
than 0.125 rad within a sub-step (Params::euler_increment_bound) and no type needs atan2.  The plain entry point
(`fdyn_rate_env_step_mixed`) has only the general loop.  Both must compute the same bits: two envs from one seed, the same
starting state written into both, 60 steps, and after every step the 12 state words, env words, integer words, observations,
rewards, flags, shard counters and episode-end records (sorted by env) are compared for equality.

The starting states put the fleet where the loops differ in code: at the pitch clamp (the `ang` fix-up and the rebuild of the
carried sin / cos), at the body-rate clamp, at the yaw wrap, on the ground; two types for which the word must be 0 (and both
entry points run the general loop); a fleet mixing such a type with the default one; and rates written from outside beyond
the clamp, which the bound does not cover (the wave holding them must fall back to the general loop).
"""
import dataclasses

import numpy as np
import pytest
import torch

from hcrl_amd import layout as L
from hcrl_amd.params import AircraftParams
from hcrl_amd.rate_env import GpuRateVecEnv

pytestmark = pytest.mark.gpu

STEPS = 60
SIZES = [1, 63, 64, 65, 257]            # below / at / above one wave, more than one workgroup
BASE = AircraftParams()
FAST_RATES = dataclasses.replace(BASE, max_angular_rate=2.0 * BASE.max_angular_rate)     # bound 0.224 rad: word 0
WIDE_ALPHA = dataclasses.replace(BASE, max_alpha=40.0)                                   # tan(40 deg) > 0.7: needs atan2, word 0


def _start_random(x, n):
    pass


def _start_pitch_clamp(x, n):
    sgn = torch.where(torch.arange(n, device=x.device) % 2 == 0, 1.0, -1.0).to(x.dtype)
    x[7] = sgn * np.radians(84.9)
    x[10] = sgn * 3.0                    # 0.1 deg at 3 rad/s: in the clamp within the first sub-step, and pushed back into it
    x[6] = 0.0


def _start_rate_clamp(x, n):
    k = torch.arange(n, device=x.device)
    r = np.radians(BASE.max_angular_rate)
    x[9] = torch.where(k % 2 == 0, r, -r).to(x.dtype)
    x[10] = torch.where(k % 3 == 0, r, -r).to(x.dtype)
    x[11] = torch.where(k % 5 == 0, -r, r).to(x.dtype)


def _start_yaw_wrap(x, n):
    sgn = torch.where(torch.arange(n, device=x.device) % 2 == 0, 1.0, -1.0).to(x.dtype)
    x[8] = sgn * (np.pi - 1e-3)
    x[11] = sgn * 1.0


def _start_ground(x, n):
    x[2] = -0.1                          # NED: 0.1 m above the ground
    x[5] = 10.0                          # sinking: 0.1 m in about one env step


def _start_outside(x, n):
    _start_rate_clamp(x, n)
    x[9:12] *= 2.0                       # written from outside: beyond the clamp the bound rests on


# name -> (types, types dealt out env by env?, start state, auto_reset, expected FD_ECD_SMALL_STEPS)
CASES = {
    "random": ((BASE,), False, _start_random, True, 1.0),
    "pitch_clamp": ((BASE,), False, _start_pitch_clamp, False, 1.0),
    "rate_clamp": ((BASE,), False, _start_rate_clamp, False, 1.0),
    "yaw_wrap": ((BASE,), False, _start_yaw_wrap, False, 1.0),
    "ground": ((BASE,), False, _start_ground, False, 1.0),
    "outside_limits": ((BASE,), False, _start_outside, False, 1.0),
    "fast_rates_type": ((FAST_RATES,), False, _start_rate_clamp, False, 0.0),
    "wide_alpha_type": ((WIDE_ALPHA,), False, _start_random, True, 0.0),
    "mixed_fleet": ((BASE, FAST_RATES), True, _start_rate_clamp, True, 0.0),
}


def _make(n, types, mixed):
    ti = (np.arange(n) % len(types)).astype(np.uint8) if mixed else None
    return GpuRateVecEnv(n, "medium", 2.0, 0.02, "step", seed=23, precision="mixed", sampling="device", types=types, type_index=ti)


def _bits(t):
    return t.contiguous().view(torch.uint8)


def _same(a, b, what, k):
    assert torch.equal(_bits(a), _bits(b)), f"step {k}: {what} differs between the general and the block-free sub-step loop"


def _sorted_events(env):
    ints, flts = env.episode_events()
    order = torch.argsort(ints[:, L.FD_EV_ENV])
    return ints[order], flts[order]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("case", list(CASES))
def test_substep_loops_bit_equal(case, n):
    types, mixed, start, auto_reset, word = CASES[case]
    a, b = _make(n, types, mixed), _make(n, types, mixed)
    plain = a.lib.fdyn_rate_env_step_mixed
    a._step_fn = lambda *args: plain(*args[:-2], args[-1])             # same arguments, the image dropped: the general loop
    assert float(b.launch_image()[L.FD_IMG_EC + L.FD_ECD_SMALL_STEPS]) == word
    a.reset(); b.reset()
    start(a.x, n)
    b.x.copy_(a.x)
    g = torch.Generator(device=a.device).manual_seed(7)
    for k in range(STEPS):
        act = torch.rand((n, 4), device=a.device, generator=g) * 2.0 - 1.0
        a.step_device(act, auto_reset=auto_reset); b.step_device(act, auto_reset=auto_reset)
        for name in ("x", "e", "ei", "obs", "rewards", "rewards_full", "terminated", "truncated", "_ev_cur"):
            _same(getattr(a, name), getattr(b, name), name, k)
        (ia, fa), (ib, fb) = _sorted_events(a), _sorted_events(b)
        _same(ia, ib, "event records (int)", k)
        _same(fa, fb, "event records (float)", k)
    assert torch.isfinite(b.x).all()


def test_starting_states_reach_what_they_aim_at():
    """The pitch start is still at the pitch clamp after a step, the ground start reaches the ground, the yaw start wraps: the
    fix-ups the cases above are about do run."""
    n = 64
    env = _make(n, (BASE,), False)
    act = torch.zeros((n, 4), device=env.device)
    env.reset(); _start_pitch_clamp(env.x, n)
    act[:, 1] = torch.where(torch.arange(n, device=env.device) % 2 == 0, -1.0, 1.0)      # elevator pushing the way the rate goes
    env.step_device(act, auto_reset=False)
    assert (env.x[7].abs() > np.radians(84.0)).any()
    env.reset(); _start_ground(env.x, n)
    for _ in range(5):
        env.step_device(act, auto_reset=False)
    assert (env.x[2] == 0.0).any()
    env.reset(); _start_yaw_wrap(env.x, n)
    env.step_device(act, auto_reset=False)
    assert (env.x[8].abs() <= np.pi).all() and ((env.x[8] * env.x[11]) < 0).any()         # wrapped to the other side

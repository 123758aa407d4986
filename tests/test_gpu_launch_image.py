"""The prepared launch image (fdyn_rate_env_image + fdyn_rate_env_step_img_* / _dr_img_*) against the plain entry points.

Nothing in the image path changes an arithmetic instruction, so the check is bit equality, not a tolerance: two envs built from
the same seed, one stepped through the plain entry point and one through the image one, for 320 steps with auto-reset; after
every step the state, env words, integer words, observations, rewards, flags, PID state, disturbance rows, shard counters and
the episode-end records (sorted by env: the order of records inside a shard is the order waves arrive in) must be identical.
"""
import dataclasses

import numpy as np
import pytest
import torch

from hcrl_amd import layout as L
from hcrl_amd.disturbances import Disturbances
from hcrl_amd.params import AircraftParams
from hcrl_amd.rate_env import GpuRateVecEnv

pytestmark = pytest.mark.gpu

N, STEPS = 4000, 320          # 4000: the last workgroup is partly filled


def _types(n_types):
    base = AircraftParams()
    return tuple(dataclasses.replace(base, mass=base.mass * (1.0 + 0.07 * k), inertia_xx=base.inertia_xx * (1.0 + 0.05 * k),
                                     max_alpha=base.max_alpha + 0.5 * k, max_pitch_angle=base.max_pitch_angle - 0.5 * k)
                 for k in range(n_types))


def _make(precision, command, n_types, dr):
    ti = None if n_types == 1 else (np.arange(N) * 7 % n_types).astype(np.uint8)
    dist = None
    if dr:
        dist = Disturbances(wind_speed=(0.0, 6.0), wind_direction=(0.0, 6.28), turbulence_intensity=(0.0, 0.15), mass=(0.8, 1.2),
                            air_density=(0.9, 1.1))
    return GpuRateVecEnv(N, "medium", 2.0, 0.02, command, seed=11, precision=precision, sampling="device", types=_types(n_types),
                         type_index=ti, disturbances=dist)


def _use_plain_entry_point(env):
    """Step this env through the entry point without an image: same arguments, the image dropped."""
    fn = getattr(env.lib, f"fdyn_rate_env_step_{'dr_' if env.dr is not None else ''}{env.precision}")
    env._step_fn = lambda *a: fn(*a[:-2], a[-1])


def _bits(t):
    t = t.contiguous()
    return t.view(torch.uint8)


def _same(a, b, what, k):
    assert torch.equal(_bits(a), _bits(b)), f"step {k}: {what} differs between the plain and the image entry point"


def _sorted_events(env):
    ints, flts = env.episode_events()
    order = torch.argsort(ints[:, L.FD_EV_ENV])
    return ints[order], flts[order]


def _run(precision, command, n_types, dr, pid):
    a, b = _make(precision, command, n_types, dr), _make(precision, command, n_types, dr)
    _use_plain_entry_point(a)
    a.reset(); b.reset()
    g = torch.Generator(device=a.device).manual_seed(5)
    ended = 0
    for k in range(STEPS):
        act = None if pid else (torch.rand((N, 4), device=a.device, generator=g) * 2.0 - 1.0)
        a.step_device(act); b.step_device(act)
        for name in ("x", "e", "ei", "obs", "rewards", "rewards_full", "terminated", "truncated", "pid_state", "_ev_cur"):
            _same(getattr(a, name), getattr(b, name), name, k)
        if pid:
            _same(a.actions_taken, b.actions_taken, "actions_taken", k)
        if dr:
            _same(a.dr, b.dr, "dr", k)
        (ia, fa), (ib, fb) = _sorted_events(a), _sorted_events(b)
        _same(ia, ib, "event records (int)", k)
        _same(fa, fb, "event records (float)", k)
        ended += ia.shape[0]
    assert ended >= N, f"only {ended} episodes ended in {STEPS} steps: the auto-reset and the records were hardly exercised"
    assert b._image.fills == 1


@pytest.mark.parametrize("n_types", [1, 8])
@pytest.mark.parametrize("command", ["step", "sine"])
@pytest.mark.parametrize("precision", ["mixed", "f64"])
def test_image_entry_point_bit_equal(precision, command, n_types):
    _run(precision, command, n_types, dr=False, pid=False)


@pytest.mark.parametrize("precision", ["mixed", "f64"])
def test_image_entry_point_bit_equal_dr(precision):
    _run(precision, "step", 8, dr=True, pid=False)


@pytest.mark.parametrize("precision", ["mixed", "f64"])
def test_image_entry_point_bit_equal_pid_mode(precision):
    _run(precision, "step", 1, dr=False, pid=True)


def test_image_entry_point_bit_equal_f32():
    _run("f32", "step", 8, dr=False, pid=False)


def test_image_follows_env_consts_and_params():
    """A curriculum switch writes env_consts in place; the next step must run with the new constants (here: 10 instead of 100
    steps per episode), as an env built with them does."""
    from hcrl_amd.samplers import env_consts
    a = GpuRateVecEnv(512, "medium", 2.0, 0.02, "step", seed=3, precision="mixed", sampling="device")
    b = GpuRateVecEnv(512, "easy", 0.2, 0.02, "step", seed=3, precision="mixed", sampling="device")
    a.env_consts.copy_(torch.as_tensor(env_consts("easy", 0.2, 0.02, "step"), device=a.device))
    a.reset(); b.reset()
    act = torch.zeros((512, 4), device=a.device); act[:, 3] = 0.5
    for k in range(12):
        a.step_device(act); b.step_device(act)
        _same(a.x, b.x, "x", k); _same(a.truncated, b.truncated, "truncated", k); _same(a.obs, b.obs, "obs", k)
    assert a._image.fills == 2 and b._image.fills == 1
    heavier = torch.as_tensor(dataclasses.replace(AircraftParams(), mass=AircraftParams().mass * 1.5).to_block(), device=a.device)
    a.params[0].copy_(heavier)
    c = GpuRateVecEnv(512, "easy", 0.2, 0.02, "step", seed=3, precision="mixed", sampling="device",
                      types=(dataclasses.replace(AircraftParams(), mass=AircraftParams().mass * 1.5),))
    for env in (a, c):
        env.x.copy_(b.x); env.e.copy_(b.e); env.ei.copy_(b.ei)
    a.step_device(act); c.step_device(act)
    _same(a.x, c.x, "x after a parameter change", 0)
    assert a._image.fills == 3


def test_library_loaded_before_the_first_gpu_call_still_launches():
    """A fresh process that loads the HIP library BEFORE the framework has touched the GPU (what build() followed by smoke() does)
    fills a launch image and steps: loaded ahead of the runtime's start-up, every launch of the library returned
    hipErrorNoDevice while the framework's own kernels ran."""
    import os
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import hcrl_amd, torch\n"
            "from hcrl_amd import _lib\n"
            "assert not torch.cuda.is_initialized()\n"
            "_lib.load()\n"
            "from hcrl_amd.rate_env import GpuRateVecEnv\n"
            "env = GpuRateVecEnv(256, 'medium', 10.0, 0.02, 'step', seed=0, precision='f64', sampling='device')\n"
            "env.reset()\n"
            "env.step_device(torch.zeros(256, 4, device=env.device), auto_reset=False)\n"
            "torch.cuda.synchronize()\n"
            "assert bool(torch.isfinite(env.x).all())\n"
            "print('ok')\n")
    proc = subprocess.run([sys.executable, "-c", code], cwd=repo, capture_output=True, text=True, timeout=120)
    assert proc.returncode == 0 and proc.stdout.strip().endswith("ok"), proc.stderr[-2000:]

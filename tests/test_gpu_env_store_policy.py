"""The store policy of the image entry points (write-through stores at one wave per SIMD) against the plain entry points.

A store's cache policy changes no value, so the check is bit equality: two envs built from the same seed, one stepped through
the plain entry point (plain stores) and one through the image one, as in test_gpu_launch_image.py.  After every step the state,
env words, integer words, observations, rewards, flags, shard counters and the episode-end records (sorted by env) must be
identical.  Sizes: a lone lane, a partial wave, one full wave (the 16-byte tile path), a full wave plus one lane (tile path and
tile fallback in one launch) and a partly filled second workgroup.  Episodes last 20 steps, so in 50 steps every env ends at
least twice: the auto-reset, the records and the state stores of finished lanes all run.

The graph test replays captured launches back to back with no host synchronisation in between: every launch loads what the
launch before it stored, which is where a write-through byte that had not reached memory would show.
"""
import numpy as np
import pytest
import torch

from hcrl_amd import layout as L
from hcrl_amd.disturbances import Disturbances
from hcrl_amd.rate_env import GpuRateVecEnv

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 257]
STEPS, EPISODE_S, DT = 50, 0.4, 0.02          # 20 steps per episode
NAMES = ("x", "e", "ei", "obs", "rewards", "rewards_full", "terminated", "truncated", "pid_state", "_ev_cur")


def _make(n, precision, dr=False):
    dist = None
    if dr:
        dist = Disturbances(wind_speed=(0.0, 6.0), wind_direction=(0.0, 6.28), turbulence_intensity=(0.0, 0.15), mass=(0.8, 1.2),
                            air_density=(0.9, 1.1))
    return GpuRateVecEnv(n, "medium", EPISODE_S, DT, "step", seed=11, precision=precision, sampling="device", disturbances=dist)


def _use_plain_entry_point(env):
    """Step this env through the entry point without an image: same arguments, the image dropped."""
    fn = getattr(env.lib, f"fdyn_rate_env_step_{'dr_' if env.dr is not None else ''}{env.precision}")
    env._step_fn = lambda *a: fn(*a[:-2], a[-1])


def _bits(t):
    return t.contiguous().view(torch.uint8)


def _same(a, b, what, k):
    assert torch.equal(_bits(a), _bits(b)), f"step {k}: {what} differs between the plain and the image entry point"


def _sorted_events(env):
    ints, flts = env.episode_events()
    order = torch.argsort(ints[:, L.FD_EV_ENV])
    return ints[order], flts[order]


def _compare(a, b, k, pid=False, dr=False):
    for name in NAMES:
        _same(getattr(a, name), getattr(b, name), name, k)
    if pid:
        _same(a.actions_taken, b.actions_taken, "actions_taken", k)
    if dr:
        _same(a.dr, b.dr, "dr", k)
    (ia, fa), (ib, fb) = _sorted_events(a), _sorted_events(b)
    _same(ia, ib, "event records (int)", k)
    _same(fa, fb, "event records (float)", k)
    return ia[:, L.FD_EV_ENV]


def _bit31(nbytes, dev):
    """A 16-byte aligned device buffer whose address has bit 31 set (any 3 GiB range holds one).  The 16-byte write-through
    stores go through a buffer descriptor assembled from the two halves of a pointer: a low half with its top bit set is
    the case in which a sign extension there would spoil the high half."""
    big = torch.empty(3 << 30, dtype=torch.uint8, device=dev)
    p = big.data_ptr()
    off = 0 if p & (1 << 31) else (((p >> 31) + 1) << 31) - p
    assert (p + off) & (1 << 31) and (p + off) % 16 == 0 and off + nbytes <= big.numel()
    return big[off:off + nbytes]


def _run(n, precision, pid=False, dr=False, stagger=False, high=False):
    a, b = _make(n, precision, dr), _make(n, precision, dr)
    _use_plain_entry_point(a)
    if high:
        for env in (a, b):
            env.obs = _bit31(n * L.FD_OBS_DIM * 4, env.device).view(torch.float32).view(n, L.FD_OBS_DIM)
            env.actions_taken = _bit31(n * L.FD_ACT_DIM * 4, env.device).view(torch.float32).view(n, L.FD_ACT_DIM)
    a.reset(); b.reset()
    if stagger:
        # episodes end at a different step in neighbouring lanes: every wave holds finished and unfinished lanes in the
        # same launch, at every step
        for env in (a, b):
            env.ei[L.FD_EI_STEP].copy_((torch.arange(n, device=env.device) * 7 % 20).to(torch.int32))
    g = torch.Generator(device=a.device).manual_seed(5)
    ended = torch.zeros(n, dtype=torch.int64, device=a.device)
    for k in range(STEPS):
        act = None if pid else (torch.rand((n, 4), device=a.device, generator=g) * 2.0 - 1.0)
        a.step_device(act); b.step_device(act)
        envs = _compare(a, b, k, pid, dr)
        ended += torch.bincount(envs.long(), minlength=n)
        if stagger and n >= 2 and 0 < k < 20:
            done = (b.terminated | b.truncated).bool()
            assert bool(done.any()) and not bool(done.all()), f"step {k}: finished and unfinished lanes do not share a wave"
    assert int(ended.min()) >= 2, f"an env ended only {int(ended.min())} times in {STEPS} steps"


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("precision", ["mixed", "f64"])
def test_store_policy_bit_equal(precision, n):
    _run(n, precision)


@pytest.mark.parametrize("n", SIZES)
def test_store_policy_bit_equal_mixed_waves(n):
    _run(n, "mixed", stagger=True)


@pytest.mark.parametrize("n", SIZES)
def test_store_policy_bit_equal_pid_mode(n):
    _run(n, "mixed", pid=True)


@pytest.mark.parametrize("n", SIZES)
def test_store_policy_bit_equal_dr(n):
    _run(n, "mixed", dr=True)


@pytest.mark.parametrize("n", [64, 257])
def test_store_policy_bit_equal_address_bit_31(n):
    """Observations and actions_out (the two outputs written by 16-byte buffer stores) at addresses with bit 31 set."""
    _run(n, "mixed", pid=True, high=True)


@pytest.mark.parametrize("n", [65, 257])
@pytest.mark.parametrize("precision", ["mixed", "f64"])
def test_store_policy_graph_replay(precision, n):
    """Two graphs of four steps, one per event-counter parity, captured the way bench.py captures them; five replays with no
    host synchronisation in between (an eager step flips the parity between the third and the fourth), against the same steps
    launched eagerly through the plain entry point."""
    a, b = _make(n, precision), _make(n, precision)
    _use_plain_entry_point(a)
    a.reset(); b.reset()
    g = torch.Generator(device=a.device).manual_seed(7)
    acts = [(torch.rand((n, 4), device=a.device, generator=g) * 2.0 - 1.0).contiguous() for _ in range(8)]
    GS = 4
    count, played = 0, []                          # `played`: the action index of every step b has really executed

    def eager():
        nonlocal count
        b.step_device(acts[count % 8])
        played.append(count % 8)
        count += 1

    for _ in range(4):
        eager()
    torch.cuda.synchronize()
    graphs, captured = {}, {}
    for _ in range(2):
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            for j in range(GS):
                b.step_device(acts[(count + j) % 8])
        # the capture flipped the env's host-side counter parity GS times: even, so it is where it was
        graphs[count % 2], captured[count % 2] = gr, [(count + j) % 8 for j in range(GS)]
        eager()
    torch.cuda.synchronize()

    def replay():
        nonlocal count
        # a graph replays the action batches it was captured with, whatever the step count is now
        graphs[count % 2].replay()
        played.extend(captured[count % 2])
        count += GS

    for _ in range(3):
        replay()
    eager()
    for _ in range(2):
        replay()
    for idx in played:
        a.step_device(acts[idx])
    torch.cuda.synchronize()
    assert len(played) == 4 + 2 + 5 * GS + 1
    assert int(b.ei[L.FD_EI_EPISODE].min()) >= 2, "no episode ended inside the replays"
    # a replay moves no host-side view: the counters of the last step are the set the graph's last launch appended to
    b._ev_cur = b._ev_counts[1 - b._ev_slot]
    _compare(a, b, len(played))

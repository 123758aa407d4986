"""Hybrid cascade fleets (fdyn_hybrid_step_* / hcrl_amd.hybrid): PID outer loops over a learned or PID rate loop per aircraft,
switched live -- the composition of controllers/attitude_agent.py:67,152 with controllers/learned_rate_agent.py:128-198 and
gui/simulation_worker_learned.py:51-118.  PID lanes must fly exactly the cascade; learned lanes exactly the host composition
(BatchedLearnedRateAgent fed the rate command the fleet hands out)."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from hcrl_amd import _lib, layout as L, config as cfgmod
from hcrl_amd.agents import AgentFleet, AttitudeAgent
from hcrl_amd.fleet import BatchedCascade
from hcrl_amd.flight_types import AircraftState, ControlCommand, ControlMode, ControllerConfig
from hcrl_amd.hybrid import HybridFleet
from hcrl_amd.learned_rate_agent import BatchedLearnedRateAgent, LearnedRateAgent
from hcrl_amd.params import param_table
from hcrl_amd.policy import RateLSTMPolicy

pytestmark = pytest.mark.gpu

DT = 0.01


def _policy(seed=0):
    torch.manual_seed(seed)
    pol = RateLSTMPolicy(compute_dtype=torch.bfloat16).cuda()
    with torch.no_grad():
        pol.action_net.weight.mul_(30.0)                      # make the random policy move the surfaces (and hit the clip)
    pol.prepare_inference()
    return pol


_POL = {}


def _shared_policy():
    if "p" not in _POL:
        _POL["p"] = _policy()
    return _POL["p"]


def _setup(n, seed=0):
    """cfg-3 square mission; initial conditions: the cfg-3 one with N, E ~ U(+-20) m and yaw ~ U(+-10 deg)."""
    g = load_golden("cfg3_waypoint_square.npz")
    rs = np.random.RandomState(seed)
    x0 = np.repeat(g["x0"][None], n, 0).astype(np.float64)
    x0[:, L.FD_X_N] += rs.uniform(-20, 20, n)
    x0[:, L.FD_X_E] += rs.uniform(-20, 20, n)
    x0[:, L.FD_X_YAW] += np.radians(rs.uniform(-10, 10, n))
    fc = cfgmod.load_controller_config("cascaded_pid.yaml")
    mc = cfgmod.load_mission_config("square_pattern.yaml")
    wps = cfgmod.square_mission(mc.pattern_size, mc.altitude, mc.speed)
    return x0, fc, wps, float(g["radius"])


def _commands(level, n, seed=1):
    rs = np.random.RandomState(seed)
    if level == "hsa":
        return np.stack([rs.uniform(-np.pi, np.pi, n), rs.uniform(15, 25, n), rs.uniform(80, 120, n), np.zeros(n)])
    yaw = np.where(rs.rand(n) < 0.5, np.nan, rs.uniform(-0.5, 0.5, n))
    return np.stack([rs.uniform(-0.4, 0.4, n), rs.uniform(-0.15, 0.2, n), yaw, rs.uniform(0.3, 0.8, n)])


LEVEL_ID = {"hsa": L.FD_LEVEL_HSA, "attitude": L.FD_LEVEL_ATTITUDE}


def _hybrid(n, level, precision, x0, fc, wps, radius, guidance="PP", pol=None, cmd=None, **kw):
    pol = pol or _shared_policy()
    if level == "mission":
        hf = HybridFleet(n, pol, "waypoint", wps, precision, ControllerConfig(), fc, guidance_type=guidance,
                         acceptance_radius=radius, dt=DT, **kw)
    else:
        hf = HybridFleet(n, pol, level, None, precision, ControllerConfig(), fc, dt=DT, **kw)
        hf.set_command(cmd)
    hf.reset(x0)
    return hf


class _Reference:
    """The PID fleet a hybrid all-PID run must equal: BatchedCascade.run(dt, 1) (mission) or AgentFleet.run(level, cmd, dt, 1)."""

    def __init__(self, n, level, precision, x0, fc, wps, radius, guidance="PP", cmd=None):
        self.level, self.cmd = level, cmd
        if level == "mission":
            self.f = BatchedCascade(n, wps, precision, ControllerConfig(), fc, guidance_type=guidance, acceptance_radius=radius)
        else:
            self.f = AgentFleet(n, precision, ControllerConfig(), fc)
        self.f.reset(x0)

    def step(self):
        if self.level == "mission":
            self.f.run(DT, 1)
        else:
            self.f.run(LEVEL_ID[self.level], self.cmd, DT, 1)


def _check_aligned(hf, ref, outer_only=False):
    """After ref.step(): the hybrid fleet (which ran its outer loops on the same state at the end of its previous launch) holds
    the same PID states, mission progress and the surfaces it is about to apply."""
    rows = slice(3 * L.FD_NPS, None) if outer_only else slice(None)
    assert torch.equal(hf.pid_state[rows], ref.f.pid_state[rows])
    if ref.level == "mission":
        assert torch.equal(hf.wp_idx, ref.f.wp_idx) and torch.equal(hf.reached_total, ref.f.reached_total)


# ---- 1. all-PID hybrid = the cascade, bit for bit -----------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "mixed"])
@pytest.mark.parametrize("level,guidance", [("mission", "PP"), ("mission", "LOS"), ("hsa", "PP"), ("attitude", "PP")])
def test_all_pid_equals_cascade(level, guidance, precision):
    n, steps = 4096, 1000
    x0, fc, wps, radius = _setup(n)
    cmd = None if level == "mission" else _commands(level, n)
    hf = _hybrid(n, level, precision, x0, fc, wps, radius, guidance, cmd=cmd, learned=False)
    ref = _Reference(n, level, precision, x0, fc, wps, radius, guidance, cmd)
    for k in range(steps):
        assert torch.equal(hf.x, ref.f.x), k
        ref.step()
        _check_aligned(hf, ref)
        assert torch.equal(hf.surfaces, ref.f.surfaces), k
        hf.run(DT, 1)
    assert torch.equal(hf.x, ref.f.x)
    if level == "mission":
        assert int(hf.reached_total.sum()) >= n           # every aircraft reached the first waypoint
    if precision == "f64" and level == "mission":       # fp64: K one-step launches == one K-step launch
        one = BatchedCascade(n, wps, "f64", ControllerConfig(), fc, guidance_type=guidance, acceptance_radius=radius)
        one.reset(x0)
        one.run(DT, steps)
        assert torch.equal(hf.x, one.x)


# ---- 2. injected PID actions through the learned path = the cascade -------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "mixed"])
@pytest.mark.parametrize("level", ["mission", "hsa", "attitude"])
def test_injected_pid_actions_equal_cascade(level, precision):
    n, steps = 2048, 400
    x0, fc, wps, radius = _setup(n)
    cmd = None if level == "mission" else _commands(level, n)
    hf = _hybrid(n, level, precision, x0, fc, wps, radius, cmd=cmd, learned=True, throttle="outer")
    ref = _Reference(n, level, precision, x0, fc, wps, radius, cmd=cmd)
    shadow = AgentFleet(n, precision, ControllerConfig(), fc)          # its own rate-PID state: the host's inner loop
    for k in range(steps):
        assert torch.equal(hf.x, ref.f.x), k
        ref.step()
        _check_aligned(hf, ref, outer_only=True)
        shadow.x.copy_(hf.x)
        rc = torch.cat([hf.rate_cmd[0:3].to(hf.dtype), hf.surfaces[L.FD_U_THROTTLE:]]).contiguous()
        s = shadow.compute_action(L.FD_LEVEL_RATE, rc, DT)
        assert torch.equal(shadow.pid_state[0:3 * L.FD_NPS], ref.f.pid_state[0:3 * L.FD_NPS]), k
        assert torch.equal(s, ref.f.surfaces), k
        act = torch.stack([s[L.FD_U_AILERON], s[L.FD_U_ELEVATOR], s[L.FD_U_RUDDER], s[L.FD_U_THROTTLE]], 1).float()
        hf.apply(act, DT)
    assert torch.equal(hf.x, ref.f.x)


# ---- 3. policy in the loop = host composition -----------------------------------------------------------------------------
def _ulps(a, b):
    """Largest distance between two fp32 tensors in units of the fp32 spacing at the larger magnitude."""
    a, b = a.float(), b.float()
    m = torch.maximum(a.abs(), b.abs())
    sp = (torch.nextafter(m, torch.full_like(m, float("inf"))) - m).double()
    return float(((a.double() - b.double()).abs() / sp).max())


@pytest.mark.parametrize("throttle", ["policy", "outer"])
@pytest.mark.parametrize("level", ["mission", "attitude"])
@pytest.mark.parametrize("B", [65536, 300])
def test_policy_in_loop_equals_host_composition(B, level, throttle, monkeypatch):
    if B == 300:
        monkeypatch.setenv("FDYN_NO_MFMA", "1")            # the policy's plain torch path
    pol = _shared_policy()
    x0, fc, wps, radius = _setup(B)
    cmd = None if level == "mission" else _commands(level, B)
    hf = _hybrid(B, level, "mixed", x0, fc, wps, radius, pol=pol, cmd=cmd, learned=True, throttle=throttle)
    assert hf.fused() == (B == 65536)
    agent = BatchedLearnedRateAgent(pol, B, ControllerConfig())
    exact, worst = True, 0.0
    for k in range(200):
        x_before = hf.x.clone()
        a = agent.compute_actions(hf.rate_cmd[0:3].T, hf.x)
        u = _ulps(hf.obs, agent.obs)
        worst = max(worst, u)
        assert u <= 1.0, (k, u)
        exact = exact and torch.equal(hf.obs, agent.obs)
        hf.run(DT, 1)
        if exact:
            assert torch.equal(hf.prev_action, a), k
        else:
            assert torch.allclose(hf.prev_action, a, atol=2e-2), k
        assert not torch.equal(hf.x, x_before)
    print(f"\n[hybrid] B={B} {level} throttle={throttle}: obs max {worst:.1f} ulp, bit-exact throughout: {exact}")


# ---- 4. mixed mask: lanes are independent ---------------------------------------------------------------------------------
def test_mixed_mask_lanes_equal_pure_runs():
    n, steps = 4096, 300
    x0, fc, wps, radius = _setup(n)
    mask = torch.as_tensor(np.random.RandomState(3).rand(n) < 0.5, device="cuda")
    runs = {}
    for name, learned in (("pid", False), ("learned", True), ("mixed", mask)):
        hf = _hybrid(n, "mission", "mixed", x0, fc, wps, radius, learned=learned)
        hf.run(DT, steps)
        runs[name] = hf
    m, p = mask, ~mask
    mx = runs["mixed"]
    for t in ("x", "pid_state", "surfaces"):
        assert torch.equal(getattr(mx, t)[:, p], getattr(runs["pid"], t)[:, p]), t
        assert torch.equal(getattr(mx, t)[:, m], getattr(runs["learned"], t)[:, m]), t
    assert torch.equal(mx.wp_idx[p], runs["pid"].wp_idx[p]) and torch.equal(mx.wp_idx[m], runs["learned"].wp_idx[m])
    assert torch.equal(mx.obs[m], runs["learned"].obs[m]) and torch.equal(mx.prev_action[m], runs["learned"].prev_action[m])
    assert not torch.equal(runs["pid"].x[:, m], runs["learned"].x[:, m])


# ---- 5. live switch -----------------------------------------------------------------------------------------------------------
def test_live_switch_resets_like_the_reference():
    n, s = 4096, 300
    x0, fc, wps, radius = _setup(n)
    rs = np.random.RandomState(4)
    mask0 = rs.rand(n) < 0.5
    hf = _hybrid(n, "mission", "mixed", x0, fc, wps, radius, learned=mask0)
    hf.run(DT, s - 1)
    snap_pid, snap_wp, snap_reached = hf.pid_state.clone(), hf.wp_idx.clone(), hf.reached_total.clone()
    hf.run(DT, 1)
    flip = rs.rand(n) < 0.3
    mask1 = mask0 ^ flip
    to_pid = torch.as_tensor(np.nonzero(flip & mask0)[0], device="cuda")
    to_learned = torch.as_tensor(np.nonzero(flip & ~mask0)[0], device="cuda")
    assert to_pid.numel() > 100 and to_learned.numel() > 100
    hf.set_learned(mask1)
    # lanes now learned: a new policy episode, prev_action = [0, 0, 0, 0.5] in the observation in hand
    pa = torch.tensor([0.0, 0.0, 0.0, 0.5], device="cuda")
    assert torch.equal(hf.obs[to_learned, 14:18], pa.expand(to_learned.numel(), 4))
    assert bool((hf.start[to_learned] == 1).all()) and bool((hf.start[torch.as_tensor(~flip, device="cuda")] == 0).all())
    pol = hf.policy
    with torch.no_grad():
        a_ref, _, _, _ = pol.step(hf.obs[to_learned].contiguous(), pol.initial_state(to_learned.numel(), "cuda"),
                                  torch.ones(to_learned.numel(), device="cuda"), deterministic=True)
    # lanes now PID: a cascade started from this step's state, outer-loop PID states and mission progress, rate-PID rows zeroed
    m = to_pid.numel()
    c = BatchedCascade(m, wps, "mixed", ControllerConfig(), fc, guidance_type="PP", acceptance_radius=radius)
    c.reset(hf.x[:, to_pid].T.double().cpu().numpy())
    c.pid_state.copy_(snap_pid[:, to_pid]); c.pid_state[0:3 * L.FD_NPS] = 0.0
    c.wp_idx.copy_(snap_wp[to_pid])
    for k in range(200):
        assert torch.equal(hf.x[:, to_pid], c.x), k
        c.run(DT, 1)
        assert torch.equal(hf.pid_state[:, to_pid], c.pid_state), k
        assert torch.equal(hf.surfaces[:, to_pid], c.surfaces), k
        assert torch.equal(hf.wp_idx[to_pid], c.wp_idx), k
        assert torch.equal(hf.reached_total[to_pid] - snap_reached[to_pid], c.reached_total), k
        hf.run(DT, 1)
        if k == 0:
            assert torch.allclose(hf.actions[to_learned], a_ref.float(), atol=2e-2)


# ---- 6. graph replay = eager ------------------------------------------------------------------------------------------------
def test_graph_equals_eager():
    n = 65536
    x0, fc, wps, radius = _setup(n)
    mask = np.random.RandomState(5).rand(n) < 0.75
    eager = _hybrid(n, "mission", "mixed", x0, fc, wps, radius, learned=mask)
    graph = _hybrid(n, "mission", "mixed", x0, fc, wps, radius, learned=mask, use_graph=True)
    assert graph.fused()
    eager.run(DT, 50)
    graph.run(DT, 50)
    for t in ("x", "pid_state", "wp_idx", "surfaces", "obs", "prev_action", "rate_cmd"):
        assert torch.equal(getattr(eager, t), getattr(graph, t)), t
    for a, b in zip(eager.states, graph.states):
        assert torch.equal(a, b)


# ---- 7. the single-aircraft drop-in: attitude_agent.rate_agent = LearnedRateAgent(...) -------------------------------------
def test_single_aircraft_rate_agent_dropin():
    pol = _shared_policy()
    cfg = ControllerConfig()
    x0 = np.zeros(12)
    x0[L.FD_X_D], x0[L.FD_X_U] = -100.0, 20.0
    cmd = np.array([0.3, 0.05, 0.2, 0.6])
    hf = HybridFleet(1, pol, "attitude", None, "f64", cfg, throttle="policy", dt=DT)
    hf.set_command(cmd)
    hf.reset(x0[None])
    agent = AttitudeAgent(cfg)
    assert agent.rate_agent is None
    agent.rate_agent = LearnedRateAgent(None, cfg, fallback_to_pid=False, policy=pol)
    command = ControlCommand(mode=ControlMode.ATTITUDE, roll_angle=cmd[0], pitch_angle=cmd[1], yaw_angle=cmd[2], throttle=cmd[3])
    plain, fleet = AttitudeAgent(cfg), AgentFleet(1, "f64", cfg)
    for k in range(60):
        xv = hf.x[:, 0].cpu().numpy()
        state = AircraftState.from_vector(xv, derived=(np.sqrt(xv[3] * xv[3] + xv[4] * xv[4] + xv[5] * xv[5]), -xv[2], 0.0, 0.0))
        s = agent.compute_action(command, state, dt=DT)
        assert np.array_equal(agent.rate_agent.obs, hf.obs[0].cpu().numpy()), k
        hf.run(DT, 1)
        got = np.array([s.aileron, s.elevator, s.rudder, s.throttle])
        assert np.array_equal(got, hf.prev_action[0].double().cpu().numpy()), (k, got, hf.prev_action[0])
        # the default rate_agent: today's PID path, unchanged
        fleet.x.copy_(torch.as_tensor(xv, device="cuda").reshape(12, 1))
        sp = plain.compute_action(command, state, dt=DT)
        ref = fleet.compute_action(L.FD_LEVEL_ATTITUDE, cmd, DT)[:, 0].cpu().numpy()
        assert np.array_equal([sp.elevator, sp.aileron, sp.rudder, sp.throttle], ref), k
    agent.reset()
    assert np.array_equal(agent.rate_agent.prev_action, [0.0, 0.0, 0.0, 0.5])
    assert not bool(agent._fleet.pid_state.any())


# ---- 8. argument errors ---------------------------------------------------------------------------------------------------------
def test_argument_errors_return_codes_without_launching():
    lib = _lib.load()
    fn = lib.fdyn_hybrid_step_mixed
    n = 256
    x0, fc, wps, radius = _setup(n)
    x = torch.as_tensor(x0.T.copy(), device="cuda").contiguous()
    ps = torch.zeros((27, n), dtype=torch.float32, device="cuda")
    idx = torch.zeros(n, dtype=torch.int32, device="cuda")
    params = torch.as_tensor(param_table(("rc_plane",)), device="cuda")
    cfg = torch.as_tensor(cfgmod.pid_table(ControllerConfig(), fc), device="cuda")
    consts = torch.as_tensor(cfgmod.cascade_consts(ControllerConfig(), fc, "PP"), device="cuda")
    W = torch.as_tensor(cfgmod.waypoint_table(wps), device="cuda")
    cmd = torch.zeros((4, n), dtype=torch.float64, device="cuda")
    act = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
    prev = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
    obs = torch.zeros((n, 18), dtype=torch.float32, device="cuda")
    surf = torch.zeros((4, n), dtype=torch.float64, device="cuda")
    p = _lib.ptr
    s = _lib.current_stream()

    def call(level=L.FD_LEVEL_WAYPOINT, cmd_=None, wps_=W, n_wp=len(wps), prev_=prev, obs_=obs, surf_=surf, nn=n, x_=x,
             act_=act, thr=0):
        return fn(level, p(x_), p(ps), p(idx), None, p(params), 1, p(cfg), p(consts), p(cmd_), p(wps_), n_wp, p(act_), None, thr,
                  p(prev_), p(obs_), None, p(surf_), None, nn, DT, s)

    before = x.clone()
    assert call(obs_=None) == _lib.FDYN_ERR_NULL
    assert call(surf_=None) == _lib.FDYN_ERR_NULL
    assert call(prev_=None) == _lib.FDYN_ERR_NULL
    assert call(level=L.FD_LEVEL_RATE) == _lib.FDYN_ERR_BAD_SIZE
    assert call(level=0) == _lib.FDYN_ERR_BAD_SIZE
    assert call(level=L.FD_LEVEL_HSA) == _lib.FDYN_ERR_BAD_SIZE                       # wps with a non-waypoint level
    assert call(n_wp=17) == _lib.FDYN_ERR_BAD_SIZE
    assert call(n_wp=0) == _lib.FDYN_ERR_BAD_SIZE
    assert call(cmd_=cmd) == _lib.FDYN_ERR_BAD_SIZE                                   # wps and cmd together
    assert call(level=L.FD_LEVEL_HSA, wps_=None, n_wp=0) == _lib.FDYN_ERR_NULL        # no command at all
    assert call(thr=2) == _lib.FDYN_ERR_BAD_SIZE
    torch.cuda.synchronize()
    assert torch.equal(x, before) and not bool(obs.any()) and not bool(prev.any())     # nothing launched
    assert fn(L.FD_LEVEL_WAYPOINT, None, None, None, None, None, 1, None, None, None, None, 0, None, None, 0, None, None, None,
              None, None, 0, DT, s) == _lib.FDYN_OK                                    # n = 0: a no-op
    assert call() == _lib.FDYN_OK
    torch.cuda.synchronize()
    assert not torch.equal(x, before) and bool(obs.any())

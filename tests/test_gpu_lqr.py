"""fdyn_lqr_design / fdyn_lqr_step_* and hcrl_amd.lqr on the device.

Reference on the box: the NumPy restatement of both (tests/lqr_numpy.py) -- the design on the 288 linearisations of
tests/golden/trim_reference.npz, the closed loop over the CPU oracle's RK4 step -- computed once per session.

Gates (none derived from what the kernels return unless said so):
  K            1e-9 max(1, |K|): fp64 on both sides, no shared elimination code (the gate test_gpu_trim.py uses for x0);
               iteration counts and status equal, residual <= 1e-10
  controls     n_steps = 0 against u0 - K delta clipped: 1e-15
  closed loop  500 steps against the NumPy loop over the oracle: 1e-9 (the f64 physics matches the oracle to 2e-12 per
               trajectory and the loop contracts); saturated-step counts equal
  recovery     deviation <= 1e-4 after 20 s, controls held at u0 >= 0.1 away: as tests/test_lqr_oracle.py
  mixed, f32   see test_reduced_precision_fleets_fly_beside_f64
"""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, rel_err, STATE_ANGLE_COLS
import lqr_numpy as ln
import trim_numpy as tn
from hcrl_amd import _lib, layout as L
from hcrl_amd import lqr as Q
from hcrl_amd import trim as T
from hcrl_amd.agents import LQRAgent
from hcrl_amd.fleet import BatchedCascade, BatchedSixDOF
from hcrl_amd.flight_types import AircraftState, Waypoint
from hcrl_amd.hybrid import HybridFleet
from hcrl_amd.params import param_table

pytestmark = pytest.mark.gpu

SENTINEL = -12345.678
ISENT = -1234567
PAD = 96
DEV = "cuda"


def _dev(a, dtype=None):
    t = torch.as_tensor(np.array(a, order="C"), device=DEV)
    return t if dtype is None else t.to(dtype)


def _padded(rows, n, dtype=torch.float64, fill=SENTINEL):
    return torch.full((rows * n + PAD,), fill, dtype=dtype, device=DEV)


def _design(A, B, w):
    """A [n][12][12], B [n][12][4], w [12] or [n][12] (host) -> dict of host arrays (K [n][16], residual, iters, status); every
    output buffer has a sentinel pad behind it, asserted untouched."""
    n = len(A)
    A_d, B_d = _dev(np.transpose(A, (1, 2, 0))), _dev(np.transpose(B, (1, 2, 0)))
    w = np.asarray(w, np.float64)
    w_d = _dev(w if w.ndim == 1 else w.T)
    K, res = _padded(L.FD_NLQK, n), _padded(1, n)
    it, st = _padded(1, n, torch.int32, ISENT), _padded(1, n, torch.int32, ISENT)
    rc = _lib.load().fdyn_lqr_design(_lib.ptr(A_d), _lib.ptr(B_d), _lib.ptr(w_d), int(w.ndim == 2), n, _lib.ptr(K), _lib.ptr(res),
                                     _lib.ptr(it), _lib.ptr(st), _lib.current_stream())
    _lib.check(rc, "fdyn_lqr_design")
    torch.cuda.synchronize()
    for buf, rows, sent in ((K, L.FD_NLQK, SENTINEL), (res, 1, SENTINEL), (it, 1, ISENT), (st, 1, ISENT)):
        assert bool((buf[rows * n:] == sent).all()), "wrote behind an output buffer"
    return dict(K=K[:L.FD_NLQK * n].reshape(L.FD_NLQK, n).T.cpu().numpy(), residual=res[:n].cpu().numpy(), iters=it[:n].cpu().numpy(),
                status=st[:n].cpu().numpy())


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same_bits(a, b):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in ("K", "residual")) and \
        np.array_equal(a["iters"], b["iters"]) and np.array_equal(a["status"], b["status"])


def _take(r, idx):
    return {k: v[idx] for k, v in r.items()}


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "trim_reference.npz"))


@pytest.fixture(scope="module")
def want(golden):
    return ln.design_many(golden["A"], golden["B"], ln.default_weights())


@pytest.fixture(scope="module")
def grid(golden):
    """The 288 linearisations in ONE launch with shared weights."""
    return _design(golden["A"], golden["B"], ln.default_weights())


def _assert_matches(got, ref, what):
    assert np.array_equal(got["status"], ref["status"]), (what, got["status"], ref["status"])
    assert np.array_equal(got["iters"], ref["iters"]), (what, got["iters"], ref["iters"])
    err = np.abs(got["K"] - ref["K"]) / np.maximum(1.0, np.abs(ref["K"]))
    print(f"{what}: worst K deviation {err.max():.3e}, exact in {int((got['K'] == ref['K']).sum())} of {got['K'].size} words")
    assert err.max() <= 1e-9, (what, err.max())


def test_grid_matches_the_restatement(grid, want):
    assert len(grid["status"]) == 288 and not grid["status"].any(), np.flatnonzero(grid["status"])
    print(f"residual: worst {grid['residual'].max():.3e}; iterations {grid['iters'].min()}..{grid['iters'].max()}")
    assert grid["residual"].max() <= 1e-10
    _assert_matches(grid, want, "288 aircraft")


@pytest.mark.parametrize("n", [1, 63, 65, 257])
def test_shapes_and_lane_position(n, grid, golden):
    idx = (np.arange(n) * 7 + 3) % 288
    got = _design(golden["A"][idx], golden["B"][idx], ln.default_weights())
    assert _same_bits(got, _take(grid, idx)), "a lane's result depends on where it sits in the launch"


def test_shared_weights_equal_the_same_weights_per_lane(grid, golden):
    per_lane = _design(golden["A"], golden["B"], np.tile(ln.default_weights(), (288, 1)))
    assert _same_bits(per_lane, grid)


def test_a_weight_sweep_in_one_launch(golden, want):
    """Three weight sets on one aircraft, per lane: each equals the restatement with those weights, and they differ."""
    i = 40
    maxima = np.tile(ln.DEFAULT_MAXIMA, (3, 1))
    maxima[1, 3], maxima[2, 8:] = 0.05, 0.6
    w = 1.0 / maxima ** 2
    got = _design(np.repeat(golden["A"][i:i + 1], 3, 0), np.repeat(golden["B"][i:i + 1], 3, 0), w)
    ref = ln.design_many(np.repeat(golden["A"][i:i + 1], 3, 0), np.repeat(golden["B"][i:i + 1], 3, 0), w)
    _assert_matches(got, ref, "weight sweep")
    assert np.abs(got["K"][1] - got["K"][0]).max() > 1e-3 and np.abs(got["K"][2] - got["K"][0]).max() > 1e-3


def test_bad_lanes_and_their_neighbours(grid, golden):
    keep = np.arange(0, 288, 6)                                          # 48 good aircraft, both airframes
    w0 = ln.default_weights()
    A, B, W, kind = [], [], [], []
    rs = np.random.RandomState(2)
    for j, i in enumerate(keep):
        A.append(golden["A"][i]); B.append(golden["B"][i]); W.append(w0); kind.append(0)
        if j % 3 == 2:
            a, b, w = golden["A"][i].copy(), golden["B"][i].copy(), w0.copy()
            k = 1 + (j // 3) % 4
            if k == 1:                                                   # a NaN word in a block of A
                a[L.FD_X_V, L.FD_X_R] = np.nan
            elif k == 2:                                                 # a bad weight
                w[rs.randint(12)] = (0.0, -2.0, np.nan, np.inf)[(j // 12) % 4]
            elif k == 3:                                                 # an unstabilisable longitudinal block
                for r in T.LONGITUDINAL_STATES:
                    a[r, :] = 0.0
                    a[r, r] = 0.5
                    b[r, :] = 0.0
            else:                                                        # an infinite word of B
                b[L.FD_X_Q, L.FD_U_ELEVATOR] = -np.inf
            A.append(a); B.append(b); W.append(w); kind.append(k)
    A, B, W, kind = np.array(A), np.array(B), np.array(W), np.array(kind)
    assert all((kind == k).sum() >= 3 for k in (1, 2, 3, 4))
    mixed = _design(A, B, W)
    assert _same_bits(_take(mixed, kind == 0), _take(grid, keep)), "a good lane changed because of its neighbour"
    bad = _take(mixed, kind != 0)
    assert not bad["K"].any() and np.array_equal(_bits(bad["K"]), np.zeros_like(bad["K"], dtype=np.uint64)), "a bad lane kept a gain"
    assert (mixed["status"][np.isin(kind, (1, 2, 4))] == L.FD_LQR_BAD_INPUT).all()
    assert np.isnan(mixed["residual"][np.isin(kind, (1, 2, 4))]).all() and not mixed["iters"][np.isin(kind, (1, 2, 4))].any()
    assert (mixed["status"][kind == 3] & L.FD_LQR_NOT_CONVERGED).all()
    ref = ln.design_many(A[kind != 0], B[kind != 0], W[kind != 0])
    assert np.array_equal(bad["status"], ref["status"]) and np.array_equal(bad["iters"], ref["iters"])
    print(f"bad lanes: status {sorted(set(bad['status'].tolist()))}, iterations of the unstabilisable block {set(mixed['iters'][kind == 3].tolist())}")


# ---- the closed loop -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def flights():
    return ln.oracle_flights()


def _fleet(f, precision="f64", x=None):
    """A fleet of the reference's aircraft at `x` (default: the perturbed start) and a design holding the REFERENCE's gains and
    trim points, so the step kernels are compared on identical inputs."""
    n = len(f["type"])
    fleet = BatchedSixDOF(n, precision, types=tn.TYPES, type_index=f["type"])
    fleet.reset(f["x_start"] if x is None else x)
    design = Q.LqrDesign(_dev(f["K"].T), torch.zeros(n, dtype=torch.float64, device=DEV), torch.zeros(n, dtype=torch.int32, device=DEV),
                         torch.zeros(n, dtype=torch.int32, device=DEV), _dev(f["x0"].T), _dev(f["u0"].T))
    return fleet, design


def _deviation(fleet, f):
    x = fleet.state_numpy()
    return np.array([ln.deviation(x[i], f["x0"][i]) for i in range(len(x))])


def test_controls_only(flights):
    f = flights["all"]
    n = len(f["type"])
    fleet, design = _fleet(f)
    x_before = fleet.x.clone()
    surf, sat = _padded(L.FD_NU, n), _padded(1, n, torch.int32, 0)
    Q.step_into("f64", fleet.x, design, fleet.params, fleet.type_index, ln.DT, 0, surf, sat)
    torch.cuda.synchronize()
    assert bool((surf[L.FD_NU * n:] == SENTINEL).all()) and torch.equal(fleet.x, x_before) and not bool(sat.any())
    got = surf[:L.FD_NU * n].reshape(L.FD_NU, n).T.cpu().numpy()
    ref = np.array([ln.clip_controls(ln.controls(f["K"][i], f["x0"][i], f["u0"][i], f["x_start"][i]))[0] for i in range(n)])
    print(f"controls at the perturbed start: worst |device - NumPy| = {np.abs(got - ref).max():.3e}")
    assert np.abs(got - ref).max() <= 1e-15
    assert (np.abs(ref) == 1.0).any() or (ref[:, 3] == 0.0).any()              # the clip is exercised


def test_five_hundred_steps_against_the_numpy_closed_loop(flights):
    f = flights["all"]
    fleet, design = _fleet(f)
    fleet.step_lqr(design, ln.STEPS_COMPARE, ln.DT)
    torch.cuda.synchronize()
    err = rel_err(fleet.state_numpy(), f["x_500"], STATE_ANGLE_COLS)
    print(f"500 closed-loop steps, 10 aircraft: worst |device - NumPy over the oracle| = {err.max():.3e}; "
          f"controls {np.abs(fleet.u.T.cpu().numpy() - f['u_500']).max():.3e}; saturated steps {fleet.lqr_saturated_steps.cpu().tolist()}")
    assert err.max() <= 1e-9
    assert np.abs(fleet.u.T.cpu().numpy() - f["u_500"]).max() <= 1e-9
    assert np.array_equal(fleet.lqr_saturated_steps.cpu().numpy(), f["sat_500"])
    assert fleet.time == pytest.approx(ln.STEPS_COMPARE * ln.DT)
    # the count accumulates over launches, and many short launches equal one long one to the bit
    again, _ = _fleet(f)
    for _ in range(5):
        again.step_lqr(design, 100, ln.DT)
    assert torch.equal(again.x, fleet.x) and torch.equal(again.lqr_saturated_steps, fleet.lqr_saturated_steps)


def test_recovery_and_the_open_loop_contrast(flights):
    f = flights["listed"]
    fleet, design = _fleet(f)
    fleet.step_lqr(design, ln.STEPS_20S, ln.DT)
    dev = _deviation(fleet, f)
    held, _ = _fleet(f)
    held.set_controls(f["u0"])
    for _ in range(ln.STEPS_20S):
        held.step(ln.DT)
    open_dev = _deviation(held, f)
    print(f"after 20 s: LQR {dev.max():.3e} from trim (NumPy over the oracle {f['dev'][:, 2].max():.3e}), controls held at u0 "
          f"{open_dev.min():.2f}..{open_dev.max():.2f}; saturated steps {fleet.lqr_saturated_steps.cpu().tolist()}")
    assert dev.max() <= 1e-4
    assert open_dev.min() >= 0.1
    assert np.array_equal(fleet.lqr_saturated_steps.cpu().numpy(), f["sat"])


MEASURED_MIXED, MEASURED_F32 = 6.819e-6, 1.208e-4      # first run on MI355X


def test_reduced_precision_fleets_fly_beside_f64(flights):
    """The mixed and f32 fleets fly the 20 s recovery of the ten aircraft beside the f64 fleet, compared every second on the eight
    regulated words.  Measured on the first run on MI355X: mixed 6.819e-06, f32 1.208e-04 (the f32 fleet stores its state in
    fp32: 1e-6 of a 20 m/s velocity per step, regulated away by the loop).  Gate: ten times those values, which is below 1e-2
    (one sixtieth of the smallest open-loop drift, 0.6)."""
    f = flights["all"]
    fleets = {p: _fleet(f, p) for p in ("f64", "mixed", "f32")}
    worst = {p: 0.0 for p in ("mixed", "f32")}
    words = list(ln.DELTA_STATES)
    for _ in range(20):
        for fleet, design in fleets.values():
            fleet.step_lqr(design, 100, ln.DT)
        ref = fleets["f64"][0].x[words]
        for p in worst:
            d = fleets[p][0].x[words].to(torch.float64) - ref
            d = torch.remainder(d + np.pi, 2 * np.pi) - np.pi
            worst[p] = max(worst[p], float(d.abs().max()))
    print(f"worst difference to the f64 fleet over 20 s: mixed {worst['mixed']:.3e}, f32 {worst['f32']:.3e}")
    assert 10 * MEASURED_MIXED < 1e-2 and 10 * MEASURED_F32 < 1e-2
    assert worst["mixed"] <= 10 * MEASURED_MIXED and worst["f32"] <= 10 * MEASURED_F32


def test_zero_gain_at_trim_is_the_plain_step_to_the_bit():
    """A trimmed lane whose design failed (K = 0) holds u0: 100 LQR steps in one launch equal 100 calls of step() bit for bit --
    the integrator is the fleets' own, not a copy."""
    n = 70
    ty = (np.arange(n) % 2).astype(np.uint8)
    V_ = 15.0 + 0.2 * np.arange(n)
    a, b = (BatchedSixDOF(n, "f64", types=tn.TYPES, type_index=ty) for _ in range(2))
    for fl in (a, b):
        fl.trim(V_, turn_rate=0.1)
    w = ln.default_weights()
    w[4] = np.nan
    design = a.design_lqr(weights=w, strict=False)
    assert bool((design.status == L.FD_LQR_BAD_INPUT).all()) and not bool(design.K.any())
    with pytest.raises(ValueError, match=rf"{n} of {n} aircraft.*invalid model or weights"):
        a.design_lqr(weights=w)
    a.step_lqr(design, 100, 0.01)
    for _ in range(100):
        b.step(0.01)
    assert torch.equal(a.x, b.x) and torch.equal(a.u, b.u) and not bool(a.lqr_saturated_steps.any())


def test_fleet_design_matches_the_oracle_design(flights):
    """BatchedSixDOF.trim -> design_lqr on the device against trim -> linearise -> design in NumPy over the oracle; a design without
    a trim raises."""
    f = flights["all"]
    n = len(f["type"])
    fleet = BatchedSixDOF(n, "f64", types=tn.TYPES, type_index=f["type"])
    with pytest.raises(ValueError, match="has no trim"):
        fleet.design_lqr()
    fleet.trim(f["spec"][:, 0], f["spec"][:, 1], f["spec"][:, 2], ln.ALTITUDE, ln.HEADING)
    d = fleet.design_lqr()
    assert bool(d.ok.all()) and d.count_not_ok() == 0 and d.x0 is not None and torch.equal(d.x0, fleet.x)
    # A and B come from two central differences of two implementations of the dynamics (1.8e-10 apart), so the
    # gains are compared at the linearisation's own gate of 1e-6, not the solver's
    err = np.abs(d.K.T.cpu().numpy() - f["K"]) / np.maximum(1.0, np.abs(f["K"]))
    print(f"fleet design against the oracle design: worst K deviation {err.max():.3e}")
    assert err.max() <= 1e-6
    A, B = fleet.linearize()
    cl = d.closed_loop(A, B).permute(2, 0, 1).cpu().numpy()
    words = list(ln.DELTA_STATES)
    worst = max(np.linalg.eigvals(cl[i][np.ix_(words, words)]).real.max() for i in range(n))
    print(f"coupled 8-state closed loop of the ten aircraft: worst pole real part {worst:.3f}")
    assert worst < 0.0
    sweep = fleet.design_lqr(weights=Q.LqrWeights(theta=np.linspace(0.05, 0.2, n)))
    assert bool(sweep.ok.all()) and float((sweep.K - d.K).abs().max()) > 1e-3


def test_lqr_agent_is_lane_zero_of_the_fleet_call(flights):
    f = flights["all"]
    fleet, design = _fleet(f)
    fleet.step_lqr(design, 0)
    want = fleet.u[:, 0].cpu().numpy()
    state = AircraftState.from_vector(f["x_start"][0])
    for agent in (LQRAgent(design), LQRAgent(f["K"][0], f["x0"][0], f["u0"][0])):
        s = agent.compute_action(None, state, 0.01)
        assert [s.elevator, s.aileron, s.rudder, s.throttle] == want.tolist()
        agent.reset()
        assert agent.get_control_level().name == "SURFACE"
    moved = LQRAgent(design).compute_action((f["x0"][2], f["u0"][2]), state)       # a new trim point as the command
    ref = ln.clip_controls(ln.controls(f["K"][0], f["x0"][2], f["u0"][2], f["x_start"][0]))[0]
    assert np.abs(np.array([moved.elevator, moved.aileron, moved.rudder, moved.throttle]) - ref).max() <= 1e-15
    with pytest.raises(ValueError):
        LQRAgent(f["K"][0])


def test_cascade_and_hybrid_fleets_inherit_both_methods(flights):
    f = flights["listed"]
    assert HybridFleet.design_lqr is BatchedSixDOF.design_lqr and HybridFleet.step_lqr is BatchedSixDOF.step_lqr
    assert BatchedCascade.design_lqr is BatchedSixDOF.design_lqr and BatchedCascade.step_lqr is BatchedSixDOF.step_lqr
    n = len(f["type"])
    plain = BatchedSixDOF(n, "mixed", types=tn.TYPES, type_index=f["type"])
    casc = BatchedCascade(n, [Waypoint(100.0, 0.0, -100.0)], "mixed", types=tn.TYPES, type_index=f["type"])
    out = []
    for fleet in (plain, casc):
        fleet.trim(f["spec"][:, 0], f["spec"][:, 1], f["spec"][:, 2])
        d = fleet.design_lqr()
        fleet.x.copy_(_dev(f["x_start"].T))
        fleet.step_lqr(d, 200, ln.DT)
        out.append((d.K.clone(), fleet.x.clone()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


def test_graph_replay_equals_eager(golden, flights):
    A, B, w = _dev(np.transpose(golden["A"], (1, 2, 0))), _dev(np.transpose(golden["B"], (1, 2, 0))), _dev(ln.default_weights())
    eager = Q.lqr_into(A, B, w)
    f = flights["all"]
    n = len(f["type"])
    fe, design = _fleet(f)
    fg, _ = _fleet(f)
    se, sg = torch.zeros((L.FD_NU, n), dtype=torch.float64, device=DEV), torch.zeros((L.FD_NU, n), dtype=torch.float64, device=DEV)
    ce, cg = torch.zeros(n, dtype=torch.int32, device=DEV), torch.zeros(n, dtype=torch.int32, device=DEV)
    Q.step_into("f64", fe.x, design, fe.params, fe.type_index, ln.DT, 50, se, ce)
    out = Q.LqrDesign(torch.zeros_like(eager.K), torch.zeros_like(eager.residual), torch.zeros_like(eager.iterations),
                      torch.zeros_like(eager.status))
    scratch = fg.x.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                                 # warm-up outside the capture, on a copy of the state
        Q.lqr_into(A, B, w, out)
        Q.step_into("f64", scratch, design, fg.params, fg.type_index, ln.DT, 50, sg, cg)
    torch.cuda.current_stream().wait_stream(s)
    for t in (out.K, out.residual, out.iterations, out.status, sg, cg):
        t.zero_()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        Q.lqr_into(A, B, w, out)
        Q.step_into("f64", fg.x, design, fg.params, fg.type_index, ln.DT, 50, sg, cg)
    gr.replay()
    torch.cuda.synchronize()
    for a, b in ((eager.K, out.K), (eager.residual, out.residual), (eager.iterations, out.iterations), (eager.status, out.status),
                 (fe.x, fg.x), (se, sg), (ce, cg)):
        assert torch.equal(a, b)

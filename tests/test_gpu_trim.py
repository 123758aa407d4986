"""fdyn_trim / fdyn_linearize and hcrl_amd.trim on the device.

Reference on the box: the NumPy restatement of the two algorithms (tests/trim_numpy.py) over the CPU oracle's dynamics, solved
once per session, and tests/golden/trim_reference.npz (the same algorithm over the reference's own `_dynamics`).

Gates (none derived from what the kernels return):
  z, x0, u0   1e-9: both sides find the root of one function up to libm rounding (~1e-15) amplified by |J^-1|
  iterations  within one of the reference's; residual <= 1e-10 (the oracle reaches 1.4e-14 on every feasible point)
  A, B        1e-6 max(1, |value|): rounding of one derivative (a few 1e-14) over a step of 2e-5 is ~1e-9; perturbing x_dot by
              4e-16 relative moved A by 1.2e-8 at a step of 1e-6 on the CPU
  hold        1e-6 over 30 s; the oracle stays within 1e-13
Measured on MI355X (recorded in DESIGN.md §7d): worst |z - oracle| 8.9e-16, |x0 - oracle| 3.6e-15, residual 1.4e-14; worst A / B
deviation 1.8e-10 at the trims and 1.4e-9 away from them; hold over 30 s: altitude 1.2e-11 m, everything else below 3e-13.
"""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import trim_numpy as tn
from hcrl_amd import _lib, layout as L
from hcrl_amd import trim as T
from hcrl_amd import validation as V
from hcrl_amd.backend import SimulationAircraftBackend
from hcrl_amd.fleet import BatchedSixDOF
from hcrl_amd.params import param_table

pytestmark = pytest.mark.gpu

SENTINEL = -12345.678
ISENT = -1234567
PAD = 96
DEV = "cuda"


def _dev(a, dtype=None):
    return torch.as_tensor(np.array(a, order="C"), device=DEV) if dtype is None else torch.as_tensor(np.array(a, order="C"), device=DEV).to(dtype)


def _params(types=tn.TYPES):
    return _dev(param_table(types))


def _padded(rows, n, dtype=torch.float64, fill=SENTINEL):
    return torch.full((rows * n + PAD,), fill, dtype=dtype, device=DEV)


def _trim(spec, ty=None, scales=None, params=None):
    """spec [n][5] (host), ty [n] or None, scales [n][5] or None -> dict of host arrays (z, x0 [n][12], u0 [n][4], ...);
    every output buffer has a sentinel pad behind it, asserted untouched."""
    n = len(spec)
    params = _params() if params is None else params
    spec_d = _dev(np.asarray(spec, np.float64).T)
    ty_d = None if ty is None else _dev(np.asarray(ty, np.uint8))
    sc_d = None if scales is None else _dev(np.asarray(scales, np.float64).T)
    x0, u0, res = _padded(L.FD_NX, n), _padded(L.FD_NU, n), _padded(1, n)
    it, st = _padded(1, n, torch.int32, ISENT), _padded(1, n, torch.int32, ISENT)
    rc = _lib.load().fdyn_trim(_lib.ptr(spec_d), _lib.ptr(ty_d), _lib.ptr(sc_d), _lib.ptr(params), int(params.shape[0]), n,
                               _lib.ptr(x0), _lib.ptr(u0), _lib.ptr(res), _lib.ptr(it), _lib.ptr(st), _lib.current_stream())
    _lib.check(rc, "fdyn_trim")
    torch.cuda.synchronize()
    for buf, rows, sent in ((x0, L.FD_NX, SENTINEL), (u0, L.FD_NU, SENTINEL), (res, 1, SENTINEL), (it, 1, ISENT), (st, 1, ISENT)):
        assert bool((buf[rows * n:] == sent).all()), "wrote behind an output buffer"
    x0h = x0[:L.FD_NX * n].reshape(L.FD_NX, n).T.cpu().numpy()
    u0h = u0[:L.FD_NU * n].reshape(L.FD_NU, n).T.cpu().numpy()
    z = np.concatenate([np.arctan2(x0h[:, L.FD_X_W], x0h[:, L.FD_X_U])[:, None], x0h[:, [L.FD_X_PITCH, L.FD_X_ROLL]], u0h], axis=1)
    return dict(z=z, x0=x0h, u0=u0h, residual=res[:n].cpu().numpy(), iters=it[:n].cpu().numpy(), status=st[:n].cpu().numpy())


def _linearize(x, u, ty=None, scales=None, params=None, f32=False):
    """x [n][12], u [n][4] (host) -> A [n][12][12], B [n][12][4]; pads asserted untouched."""
    n = len(x)
    params = _params() if params is None else params
    dt = torch.float32 if f32 else torch.float64
    x_d, u_d = _dev(np.asarray(x, np.float64).T, dt).contiguous(), _dev(np.asarray(u, np.float64).T, dt).contiguous()
    ty_d = None if ty is None else _dev(np.asarray(ty, np.uint8))
    sc_d = None if scales is None else _dev(np.asarray(scales, np.float64).T)
    A, B = _padded(L.FD_NX * L.FD_NX, n), _padded(L.FD_NX * L.FD_NU, n)
    rc = _lib.load().fdyn_linearize(_lib.ptr(x_d), _lib.ptr(u_d), int(f32), _lib.ptr(ty_d), _lib.ptr(sc_d), _lib.ptr(params),
                                    int(params.shape[0]), n, _lib.ptr(A), _lib.ptr(B), _lib.current_stream())
    _lib.check(rc, "fdyn_linearize")
    torch.cuda.synchronize()
    assert bool((A[144 * n:] == SENTINEL).all()) and bool((B[48 * n:] == SENTINEL).all()), "wrote behind an output buffer"
    return (A[:144 * n].reshape(12, 12, n).permute(2, 0, 1).cpu().numpy(), B[:48 * n].reshape(12, 4, n).permute(2, 0, 1).cpu().numpy())


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same_bits(a, b):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in ("x0", "u0", "residual")) and \
        np.array_equal(a["iters"], b["iters"]) and np.array_equal(a["status"], b["status"])


def _take(r, idx):
    return {k: v[idx] for k, v in r.items()}


@pytest.fixture(scope="module")
def ref():
    return tn.oracle_reference()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "trim_reference.npz"))


@pytest.fixture(scope="module")
def grid(ref):
    """The 288 aircraft of the feasible grid in ONE launch with a type index and mass scales."""
    f = ref["feasible"]
    return _trim(f["spec"], f["type"], f["scales"])


def _assert_matches(got, want, what):
    """Converged lanes: status equal, iterations within one, z / x0 / u0 within 1e-9."""
    assert np.array_equal(got["status"], want["status"]), (what, got["status"], want["status"])
    assert np.abs(got["iters"].astype(int) - want["iters"].astype(int)).max() <= 1, what
    for k in ("z", "x0", "u0"):
        worst = np.abs(got[k] - want[k]).max()
        print(f"{what} {k}: worst |device - reference| = {worst:.3e}")
        assert worst <= 1e-9, (what, k, worst)


def test_feasible_grid(grid, ref, golden):
    f = ref["feasible"]
    assert len(grid["status"]) == 288 and not grid["status"].any(), np.flatnonzero(grid["status"])
    print(f"residual: worst {grid['residual'].max():.3e}; iterations {grid['iters'].min()}..{grid['iters'].max()}")
    assert grid["residual"].max() <= 1e-10
    _assert_matches(grid, f, "oracle")
    _assert_matches(grid, {k: golden[k] for k in ("z", "x0", "u0", "iters", "status")}, "golden")


def test_infeasible_lanes_and_their_neighbours(ref):
    f, inf = ref["feasible"], ref["infeasible"]
    n_bad = len(inf["type"])
    keep = np.arange(0, 288, 6)                                          # 48 feasible aircraft, both airframes
    alone = _trim(f["spec"][keep], f["type"][keep], f["scales"][keep])
    # one infeasible lane after every third feasible one
    spec, ty, scales, is_bad = [], [], [], []
    for j, i in enumerate(keep):
        spec.append(f["spec"][i]); ty.append(f["type"][i]); scales.append(f["scales"][i]); is_bad.append(-1)
        if j % 3 == 2 and j // 3 < n_bad:
            b = j // 3
            spec.append(inf["spec"][b]); ty.append(inf["type"][b]); scales.append(inf["scales"][b]); is_bad.append(b)
    is_bad = np.array(is_bad)
    assert (is_bad >= 0).sum() == n_bad
    mixed = _trim(np.array(spec), np.array(ty), np.array(scales))
    assert _same_bits(_take(mixed, is_bad < 0), alone), "a feasible lane changed because of its neighbour"
    got = _take(mixed, is_bad >= 0)
    for b, (must_set, must_clear) in enumerate(inf["want"]):
        s = int(got["status"][b])
        print(f"infeasible {b:2d}: status {s:2d} ({T.describe_status(s)}), iterations {got['iters'][b]}")
        assert s & must_set == must_set and not s & must_clear, (b, s)
    conv = (inf["status"] & (tn.NOT_CONVERGED | tn.BAD_SPEC)) == 0            # bits 1 and 2: roots like any other
    _assert_matches(_take(got, conv), {k: inf[k][conv] for k in ("z", "x0", "u0", "iters", "status")}, "infeasible, converged")
    bad_spec = (inf["status"] & tn.BAD_SPEC) != 0
    assert np.array_equal(got["status"][bad_spec], inf["status"][bad_spec]) and not got["iters"][bad_spec].any()


@pytest.mark.parametrize("n", [1, 63, 65, 257])
def test_shapes_and_null_arguments(n, grid, ref):
    f = ref["feasible"]
    rc = np.flatnonzero((f["type"] == 0) & (f["scales"][:, 0] == 1.0))        # rc_plane at nominal mass: what NULL, NULL means
    idx = rc[np.arange(n) % len(rc)]
    null = _trim(f["spec"][idx])
    explicit = _trim(f["spec"][idx], np.zeros(n, np.uint8), np.ones((n, 5)))
    assert _same_bits(null, explicit)
    assert _same_bits(null, _take(grid, idx)), "a lane's result depends on where it sits in the launch"
    x, u = f["x0"][idx], f["u0"][idx]
    A0, B0 = _linearize(x, u)
    A1, B1 = _linearize(x, u, np.zeros(n, np.uint8), np.ones((n, 5)))
    assert np.array_equal(_bits(A0), _bits(A1)) and np.array_equal(_bits(B0), _bits(B1))


def test_scales_equal_an_edited_parameter_block(ref):
    f = ref["feasible"]
    scales = np.array([1.2, 0.9, 1.1, 1.05, 0.95])
    pick = np.flatnonzero(f["scales"][:, 0] == 1.0)[::7]                     # 14 conditions over both airframes
    for t, name in enumerate(tn.TYPES):
        idx = pick[f["type"][pick] == t]
        edited = _dev(tn.scaled_block(param_table((name,))[0], scales, L)[None])
        a = _trim(f["spec"][idx], np.full(len(idx), t, np.uint8), np.tile(scales, (len(idx), 1)))
        b = _trim(f["spec"][idx], params=edited)
        assert not a["status"].any() and np.array_equal(a["status"], b["status"])
        for k in ("x0", "u0"):
            worst = np.abs(a[k] - b[k]).max()
            print(f"{name} {k}: scales against an edited block {worst:.3e}")
            assert worst <= 1e-12, (name, k, worst)
        Aa, Ba = _linearize(a["x0"], a["u0"], np.full(len(idx), t, np.uint8), np.tile(scales, (len(idx), 1)))
        Ab, Bb = _linearize(a["x0"], a["u0"], params=edited)
        assert np.abs(Aa - Ab).max() <= 1e-12 * max(1.0, np.abs(Ab).max()) and np.abs(Ba - Bb).max() <= 1e-12 * max(1.0, np.abs(Bb).max())


HOLD = ((20.0, 0.0, 0.0), (25.0, 3.0, 0.0), (20.0, 0.0, 0.2), (18.0, 0.0, -0.3))      # V, gamma (deg), turn rate


def test_trim_holds_for_thirty_seconds():
    """The reference's own check (|dh| < 5 m in 60 s), made sharp: a trimmed f64 fleet keeps every steady quantity to 1e-6 for
    3000 steps of 0.01 s.  The mixed and f32 fleets start from the same solution rounded; their drift is printed, not gated."""
    ty = np.repeat(np.arange(2, dtype=np.uint8), len(HOLD))
    V_ = np.tile([c[0] for c in HOLD], 2)
    gam = np.radians(np.tile([c[1] for c in HOLD], 2))
    om = np.tile([c[2] for c in HOLD], 2)
    n, h, psi0, dt, steps = len(ty), 100.0, 0.3, 0.01, 3000
    fleets = {p: BatchedSixDOF(n, p, types=tn.TYPES, type_index=ty) for p in ("f64", "mixed", "f32")}
    res = {p: f.trim(V_, gam, om, altitude=h, heading=psi0) for p, f in fleets.items()}
    r = res["f64"]
    assert bool(r.ok.all())
    for p in ("mixed", "f32"):                                                # the stored state is the fp64 solution rounded
        assert torch.equal(res[p].x0, r.x0) and torch.equal(res[p].u0, r.u0)
        assert torch.equal(fleets[p].x, r.x0.to(fleets[p].dtype)) and torch.equal(fleets[p].u, r.u0.to(fleets[p].dtype))
    assert torch.equal(fleets["f64"].x, r.x0) and torch.equal(fleets["f64"].u, r.u0)
    Vt, gt, ot = _dev(V_), _dev(gam), _dev(om)
    steady = [L.FD_X_U, L.FD_X_V, L.FD_X_W, L.FD_X_ROLL, L.FD_X_PITCH, L.FD_X_P, L.FD_X_Q, L.FD_X_R]
    want = r.x0[steady].clone()
    worst = torch.zeros(4, dtype=torch.float64, device=DEV)                    # airspeed, steady words, altitude, heading
    drift = {p: torch.zeros(n, dtype=torch.float64, device=DEV) for p in ("mixed", "f32")}
    for k in range(1, steps + 1):
        for f in fleets.values():
            f.step(dt, None)
        t = k * dt
        x = fleets["f64"].x
        speed = torch.sqrt(x[L.FD_X_U] ** 2 + x[L.FD_X_V] ** 2 + x[L.FD_X_W] ** 2)
        alt = -x[L.FD_X_D] - (h + Vt * torch.sin(gt) * t)
        yaw = torch.remainder(x[L.FD_X_YAW] - psi0 - ot * t + np.pi, 2 * np.pi) - np.pi
        now = torch.stack([(speed - Vt).abs().max(), (x[steady] - want).abs().max(), alt.abs().max(), yaw.abs().max()])
        worst = torch.maximum(worst, now)
        if k == steps:
            for p in drift:
                drift[p] = (-fleets[p].x[L.FD_X_D].to(torch.float64) - (h + Vt * torch.sin(gt) * t)).abs()
    worst = worst.cpu().numpy()
    print(f"f64 hold over 30 s: airspeed {worst[0]:.3e}, u v w phi theta p q r {worst[1]:.3e}, altitude {worst[2]:.3e}, "
          f"heading {worst[3]:.3e}")
    for p, d in drift.items():
        print(f"{p} altitude drift after 30 s (not gated): worst {float(d.max()):.3e} m, per case {d.cpu().numpy().round(6).tolist()}")
    assert (worst <= 1e-6).all(), worst


def _lin_gate(got, want, what):
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    print(f"{what}: worst deviation {err.max():.3e}")
    assert err.max() <= 1e-6, (what, err.max())


def test_linearize_at_the_trims(ref, golden):
    f = ref["feasible"]
    A, B = _linearize(f["x0"], f["u0"], f["type"], f["scales"])
    _lin_gate(A, f["A"], "A at the 288 trims, oracle"); _lin_gate(B, f["B"], "B at the 288 trims, oracle")
    _lin_gate(A, golden["A"], "A at the 288 trims, golden"); _lin_gate(B, golden["B"], "B at the 288 trims, golden")


def test_linearize_away_from_trim():
    n = 32
    x = V.spread_initial_conditions(n)
    rs = np.random.RandomState(5)
    x[:, L.FD_X_V:L.FD_X_W + 1] = rs.uniform(-2.0, 2.0, (n, 2))
    u = np.concatenate([rs.uniform(-0.5, 0.5, (n, 3)), rs.uniform(0.2, 0.9, (n, 1))], axis=1)
    ty = (np.arange(n) % 2).astype(np.uint8)
    A, B = _linearize(x, u, ty)
    fs = [tn.oracle_airframe(tn.TYPES[t])[0] for t in range(2)]
    wantA, wantB = zip(*(tn.linearize(fs[ty[i]], x[i], u[i]) for i in range(n)))
    _lin_gate(A, np.array(wantA), "A at 32 non-trim states"); _lin_gate(B, np.array(wantB), "B at 32 non-trim states")
    # model-free: the first-order model predicts the oracle's own increment for a random displacement of norm 1e-4
    worst = 0.0
    for i in range(n):
        dx = rs.normal(size=12)
        dx *= 1e-4 / np.linalg.norm(dx)
        f = fs[ty[i]]
        worst = max(worst, float(np.linalg.norm(f(x[i] + dx, u[i]) - f(x[i], u[i]) - A[i] @ dx)))
    print(f"|f(x + dx) - f(x) - A dx| for |dx| = 1e-4: worst {worst:.3e}")
    assert worst <= 1e-6
    # fp32 input: the same VALUES handed over as fp32 and as fp64 give the same bits
    x32, u32 = x.astype(np.float32).astype(np.float64), u.astype(np.float32).astype(np.float64)
    A64, B64 = _linearize(x32, u32, ty)
    A32, B32 = _linearize(x32, u32, ty, f32=True)
    assert np.array_equal(_bits(A64), _bits(A32)) and np.array_equal(_bits(B64), _bits(B32))


def test_fleet_linearize_layout(ref):
    """BatchedSixDOF.linearize: [12][12][N] / [12][4][N] with A[i][j] = d xdot_i / d x_j, and the two sub-system helpers."""
    f = ref["feasible"]
    idx = np.arange(0, 288, 24)
    fleet = BatchedSixDOF(len(idx), "f64", types=tn.TYPES, type_index=f["type"][idx])
    sc = f["scales"][idx].T
    res = fleet.trim(f["spec"][idx, 0], f["spec"][idx, 1], f["spec"][idx, 2], tn.ALTITUDE, tn.HEADING, scales=sc)
    assert bool(res.ok.all()) and np.abs(res.alpha.cpu().numpy() - f["z"][idx, 0]).max() <= 1e-9
    assert np.abs(res.bank.cpu().numpy() - f["z"][idx, 2]).max() <= 1e-9
    A, B = fleet.linearize(scales=sc)
    assert tuple(A.shape) == (12, 12, len(idx)) and tuple(B.shape) == (12, 4, len(idx))
    _lin_gate(A.permute(2, 0, 1).cpu().numpy(), f["A"][idx], "fleet A"); _lin_gate(B.permute(2, 0, 1).cpu().numpy(), f["B"][idx], "fleet B")
    Al, Bl = T.longitudinal_block(A, B)
    assert tuple(Al.shape) == (4, 4, len(idx)) and tuple(Bl.shape) == (4, 2, len(idx))
    assert torch.equal(Al[1, 2], A[L.FD_X_W, L.FD_X_Q]) and torch.equal(Bl[0, 1], B[L.FD_X_U, L.FD_U_THROTTLE])
    Ad, Bd = T.lateral_block(A, B)
    assert torch.equal(Ad[3, 1], A[L.FD_X_ROLL, L.FD_X_P]) and torch.equal(Bd[1, 0], B[L.FD_X_P, L.FD_U_AILERON])


def test_strict_raises_before_touching_the_fleet():
    fleet = BatchedSixDOF(5, "f64", types=("rc_plane",))
    fleet.set_controls(np.tile([0.1, 0.0, 0.0, 0.6], (5, 1)))
    x_before, u_before, t_before = fleet.x.clone(), fleet.u.clone(), fleet.time
    with pytest.raises(ValueError, match=r"2 of 5 aircraft"):
        fleet.trim([20.0, 40.0, 20.0, 9.0, 25.0])                              # 40 m/s: throttle 1.23; 9 m/s: alpha at its limit
    assert torch.equal(fleet.x, x_before) and torch.equal(fleet.u, u_before) and fleet.time == t_before
    res = fleet.trim([20.0, 40.0, 20.0, 9.0, 25.0], strict=False)
    assert res.status.cpu().tolist() == [0, L.FD_TRIM_CONTROL_RANGE, 0, L.FD_TRIM_ALPHA_LIMIT, 0] and torch.equal(fleet.x, res.x0)


def test_single_aircraft_backend_trim():
    want = T.trim_fleet(1, 22.0, climb_angle=np.radians(2.0), turn_rate=0.1, altitude=150.0, heading=0.5, types=("cessna",))
    backend = SimulationAircraftBackend({"aircraft_type": "cessna"})
    state, surfaces = backend.trim(22.0, climb_angle=np.radians(2.0), turn_rate=0.1, altitude=150.0, heading=0.5)
    assert np.array_equal(state.to_vector(), want.x0[:, 0].cpu().numpy()) and surfaces == want.surfaces(0)
    assert state.altitude == pytest.approx(150.0) and state.airspeed == pytest.approx(22.0)
    assert backend.get_state() is state
    backend.set_controls(surfaces)
    for _ in range(100):
        s = backend.step(0.01)
    assert abs(s.airspeed - 22.0) <= 1e-6 and abs(s.altitude - (150.0 + 22.0 * np.sin(np.radians(2.0)) * 1.0)) <= 1e-6


def test_trimmed_scenario_trims_each_fleet_for_its_own_airframe():
    n = 64

    class Watch(V.TrajectoryComparison):
        worst = None

        def update_fleets(self, a, b):
            now = torch.stack([(-f.x[L.FD_X_D] - 100.0).abs().max() for f in (a, b)])
            self.worst = now if self.worst is None else torch.maximum(self.worst, now)
            return super().update_fleets(a, b)

    a, b = BatchedSixDOF(n, "f64", types=("rc_plane",)), BatchedSixDOF(n, "f64", types=("cessna",))
    scenario = V.TrimmedFlightScenario({"duration": 5.0, "airspeed": 20.0})
    watch = scenario.run_fleets(a, b, comparison=Watch(n, a.device))
    ua, ub = scenario.trims[0].u0, scenario.trims[1].u0
    assert bool(scenario.trims[0].ok.all()) and bool(scenario.trims[1].ok.all())
    assert float((ua[L.FD_U_THROTTLE] - ub[L.FD_U_THROTTLE]).abs().min()) > 1e-3 and float((ua[L.FD_U_ELEVATOR] - ub[L.FD_U_ELEVATOR]).abs().min()) > 1e-3
    assert torch.equal(a.u, ua) and torch.equal(b.u, ub)                       # each fleet holds its own controls
    worst = watch.worst.cpu().numpy()
    print(f"altitude error over 5 s: rc_plane {worst[0]:.3e}, cessna {worst[1]:.3e}")
    assert (worst <= 1e-6).all()
    m = watch.as_dict(0)
    assert m["altitude_rmse"] <= 1e-6 and m["position_3d_rmse"] <= 1e-5
    with pytest.raises(ValueError):
        scenario.run_fleets(a, b, x0=np.zeros((n, 12)))


def test_graph_replay_equals_eager(ref):
    f = ref["feasible"]
    n = 288
    params = _params()
    spec, ty, sc = _dev(f["spec"].T), _dev(f["type"]), _dev(f["scales"].T)
    eager = T.trim_into(spec, params, ty, sc)
    eA, eB = T.linearize_into(eager.x0, eager.u0, params, ty, sc)
    out = T.TrimResult(torch.zeros_like(eager.x0), torch.zeros_like(eager.u0), torch.zeros_like(eager.residual),
                       torch.zeros_like(eager.iterations), torch.zeros_like(eager.status))
    gA, gB = torch.zeros_like(eA), torch.zeros_like(eB)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                                 # warm-up outside the capture
        T.trim_into(spec, params, ty, sc, out)
        T.linearize_into(out.x0, out.u0, params, ty, sc, (gA, gB))
    torch.cuda.current_stream().wait_stream(s)
    for t in (out.x0, out.u0, out.residual, out.iterations, out.status, gA, gB):
        t.zero_()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        T.trim_into(spec, params, ty, sc, out)
        T.linearize_into(out.x0, out.u0, params, ty, sc, (gA, gB))
    gr.replay()
    torch.cuda.synchronize()
    assert n == out.n
    for a, b in ((eager.x0, out.x0), (eager.u0, out.u0), (eager.residual, out.residual), (eager.iterations, out.iterations),
                 (eager.status, out.status), (eA, gA), (eB, gB)):
        assert torch.equal(a, b)

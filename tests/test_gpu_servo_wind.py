"""fdyn_servo_step_wind_* / fdyn_servo_mission_wind_* (include/fdyn_wind.h) and their host layer on the device.

Reference on the box: the restatement tests/servo_wind_numpy.py (the Galilean map once per control step over the CPU oracle's
still-air RK4), computed once per session and shared.  tests/test_servo_wind_oracle.py shows that on every flight used here no
clamp of the integrator is active in either frame, and measures the yardstick D.

Gates (none derived from what the kernels return):
  zero rows against the still-air entries, restarted every step   fp64 words 1e-15 relative, f32 state 1 fp32 ulp, counters and wp_idx equal
  f64 against the restatement, steady wind / replayed gusts / mission   state, integrators and statistics within 10 x D of the
        word's unit (servo_wind_numpy.state_gate): the device's wind-frame RK4 and the restatement's air-frame RK4 are two
        fourth-order discretisations of one ODE, so their gap is of the order of their truncation errors -- an order argument,
        hence the factor; integer words equal
  gust rows with replayed z     bit-identical (two fp64 products and one sum, contraction off)
  in-kernel draws               (g' - A g) / B against tests/philox_numpy.py at the stated counter, 1e-5 absolute (the gate of
                                tests/test_gpu_device_draws.py at every Box-Muller site)
  split launches, lane position, complete lanes, NULL outputs, graph replay, fleet methods: bit-identical
  mixed, f32                    the behaviour gates of the CPU test (c); reached_total equal and event steps within one of f64's
"""
import numpy as np
import pytest
import torch

from conftest import rel_err, STATE_ANGLE_COLS
import lqr_numpy as ln
import servo_mission_numpy as mn
import servo_numpy as sn
import servo_wind_numpy as wn
import trim_numpy as tn
from hcrl_amd import _lib, layout as L
from hcrl_amd import servo as SV
from hcrl_amd.fleet import BatchedSixDOF

pytestmark = pytest.mark.gpu

SENTINEL = -12345.678
ISENT = -1234567
PAD = 96
DEV = "cuda"
DT = ln.DT
SEED = 0x1234_5678_9ABC_DEF1


def _dev(a, dtype=None):
    t = torch.as_tensor(np.array(a, order="C"), device=DEV)
    return t if dtype is None else t.to(dtype)


def _calm(n):
    rows = np.zeros((n, wn.NSW))
    rows[:, wn.SW_GUST_A] = 1.0
    return rows


class Run:
    """One fleet's arrays for the servo step (wps None) or the servo mission, in still air (`launch(..., wind=False)`: the plain
    entries) or in its air mass; every array a [rows][n] view of a buffer with a sentinel pad behind it.  `f`: a dict of per-aircraft
    arrays type, K, x0, u0, ref0; `lanes` picks from it lane by lane."""

    def __init__(self, f, lanes, rows, wps=None, C=None, precision="f64", x=None, ref=None, limits=sn.DEFAULT_LIMITS, step=0):
        lanes = np.asarray(lanes)
        self.n, self.precision, self.lanes, self.mission = len(lanes), precision, lanes, wps is not None
        n, sdt = self.n, _lib.state_dtype(precision)
        self.fleet = BatchedSixDOF(n, precision, types=tn.TYPES, type_index=np.asarray(f["type"])[lanes])
        self._bufs = []
        self.x = self._view(L.FD_NX, sdt, (np.asarray(f["x0"])[lanes] if x is None else np.asarray(x)).T)
        self.ref = self._view(L.FD_NSVR, torch.float64, (np.asarray(f["ref0"])[lanes] if ref is None else np.asarray(ref)).T)
        self.integ = self._view(L.FD_NSVI, torch.float64, np.zeros((L.FD_NSVI, n)))
        self.idx = self._view(1, torch.int32, np.zeros((1, n), np.int32))
        self.surf = self._view(L.FD_NU, sdt, None)
        self.err = self._view(L.FD_NSVI, torch.float64, None)
        self.sat, self.reached, self.flown = (self._view(1, torch.int32, np.zeros((1, n), np.int32)) for _ in range(3))
        self.stats = self._view(L.FD_NMST, torch.float64, np.tile(np.array(mn.STATS_START)[:, None], (1, n)))
        self.rows = self._view(L.FD_NSW, torch.float64, np.asarray(rows, np.float64).T)
        self.step = self._view(1, torch.int32, np.full((1, 1), step, np.int32), n=1)
        self.design = SV.ServoDesign(_dev(np.asarray(f["K"])[lanes].T), torch.zeros(n, dtype=torch.float64, device=DEV), torch.zeros(n, dtype=torch.int32, device=DEV),
                                     torch.zeros(n, dtype=torch.int32, device=DEV), _dev(np.asarray(f["x0"])[lanes].T), _dev(np.asarray(f["u0"])[lanes].T))
        self.limits = _dev(np.array(limits, np.float64))
        if self.mission:
            self.wps, self.C = _dev(np.asarray(wps, np.float64)), _dev(np.asarray(C, np.float64))

    def _view(self, rows, dtype, init, n=None):
        n = self.n if n is None else n
        sent = ISENT if dtype == torch.int32 else SENTINEL
        buf = torch.full((rows * n + PAD,), sent, dtype=dtype, device=DEV)
        view = buf[:rows * n].view(rows, n)
        if init is not None:
            view.copy_(_dev(np.asarray(init)).to(dtype))
        self._bufs.append((buf, rows * n, sent))
        return view

    def launch(self, n_steps, null=(), dt=DT, wind=True, z=None, seed=SEED):
        p = lambda name: None if name in null else _lib.ptr(getattr(self, name))   # noqa: E731
        fl = self.fleet
        head = [_lib.ptr(self.x), _lib.ptr(self.design.x0), _lib.ptr(self.design.u0), _lib.ptr(self.design.K), _lib.ptr(self.ref), _lib.ptr(self.integ),
                _lib.ptr(self.limits)]
        mid = [_lib.ptr(fl.type_index), _lib.ptr(fl.params), int(fl.params.shape[0]), self.n, float(dt), int(n_steps), p("surf"), p("sat"), p("err")]
        if self.mission:
            head += [_lib.ptr(self.idx), _lib.ptr(self.C), _lib.ptr(self.wps), int(self.wps.shape[0])]
            mid += [p("reached"), p("flown"), p("stats")]
        if z is not None:
            assert tuple(z.shape) == (n_steps, 3, self.n) and z.dtype == torch.float64 and z.is_contiguous()
            self._z = z                                                        # alive until the launch has run
        tail = [_lib.ptr(self.rows), seed, p("step"), _lib.ptr(z)] if wind else []
        name = f"fdyn_servo_{'mission' if self.mission else 'step'}{'_wind' if wind else ''}_{self.precision}"
        _lib.check(getattr(_lib.load(), name)(*head, *mid, *tail, _lib.current_stream()), name)
        return self

    def pads_untouched(self):
        torch.cuda.synchronize()
        return all(bool((buf[used:] == sent).all()) for buf, used, sent in self._bufs)

    ARRAYS = ("x", "ref", "integ", "idx", "surf", "err", "sat", "reached", "flown", "stats", "rows", "step")
    CARRIED = ("x", "ref", "integ", "idx", "sat", "reached", "flown", "stats")

    def snapshot(self):
        torch.cuda.synchronize()
        return {k: getattr(self, k).clone() for k in self.ARRAYS}

    def take(self, other):
        """Restart from another run's words."""
        for k in self.CARRIED:
            getattr(self, k).copy_(getattr(other, k))

    def host(self, name):
        t = getattr(self, name)
        return t.T.cpu().numpy().astype(np.float64 if t.dtype.is_floating_point else np.int64)


def _bits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else (t.view(torch.int32) if t.dtype == torch.float32 else t)


def _same(a, b, keys=Run.ARRAYS, lanes_a=None, lanes_b=None):
    """Names of the arrays that differ in any bit (NaN bits included) between two snapshots, on the given lanes."""
    bad = []
    for k in keys:
        per_lane = a[k].shape[-1] != 1 or k != "step"
        ta = a[k] if lanes_a is None or not per_lane else a[k][:, lanes_a]
        tb = b[k] if lanes_b is None or not per_lane else b[k][:, lanes_b]
        if not torch.equal(_bits(ta), _bits(tb)):
            bad.append(k)
    return bad


@pytest.fixture(scope="module")
def f():
    return sn.compare_flights()


@pytest.fixture(scope="module")
def gate():
    """(state [12], integrators [3]) of the step flights: 10 x D, D measured on the CPU (test_servo_wind_oracle.py (e))."""
    return wn.state_gate(wn.yardstick_groups())


def _state_diff(x_dev, x_ref):
    d = np.asarray(x_dev, np.float64) - np.asarray(x_ref, np.float64)
    for c in STATE_ANGLE_COLS:
        d[..., c] = (d[..., c] + np.pi) % (2 * np.pi) - np.pi
    return np.abs(d)


def _report(what, dx, di, gx, gi):
    names = ("position", "velocity", "angle", "rate")
    worst = {k: float(dx[:, s].max()) for k, s in wn.GROUPS.items()}
    print(f"{what}: worst |device - restatement| " + ", ".join(f"{k} {worst[k]:.3e} (gate {gx[wn.GROUPS[k]][0]:.3e})" for k in names)
          + f"; integrators {di.max(axis=0)} (gates {gi})")


# ---- zero rows: the still-air entries ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", _lib.PRECISIONS)
@pytest.mark.parametrize("mission", [False, True], ids=["step", "mission"])
def test_zero_rows_fly_the_still_air_entries(mission, precision, f):
    """200 steps, one per launch, the wind entry restarted from the plain entry's words every step."""
    short = mn.short_flights()
    kw = dict(wps=short["wps"], C=short["C"]) if mission else dict(ref=np.array([sn.commanded(r) for r in f["ref0"]]))
    plain = Run(f, np.arange(10), _calm(10), precision=precision, **kw)
    windy = Run(f, np.arange(10), _calm(10), precision=precision, **kw)
    worst64 = worst_ulp = 0.0
    identical = True
    for s in range(200):
        windy.take(plain)
        plain.launch(1, wind=False)
        windy.launch(1)
        a, b = plain.snapshot(), windy.snapshot()
        for k in ("idx", "sat", "reached", "flown"):
            assert torch.equal(a[k], b[k]), (s, k)
        for k in ("x", "ref", "integ", "surf", "err", "stats"):
            if mission or k != "stats":
                identical = identical and torch.equal(_bits(a[k]), _bits(b[k]))
                ta, tb = a[k].double(), b[k].double()
                if a[k].dtype == torch.float32:
                    ulp = torch.abs(ta - tb) / torch.maximum(torch.abs(tb), torch.tensor(2.0 ** -126, device=DEV, dtype=torch.float64))
                    worst_ulp = max(worst_ulp, float((ulp / 2.0 ** -23).max()))
                else:
                    fin = torch.isfinite(tb)
                    assert torch.equal(fin, torch.isfinite(ta))
                    worst64 = max(worst64, float((torch.abs(ta - tb)[fin] / torch.clamp(torch.abs(tb[fin]), min=1.0)).max()))
        assert not b["rows"][L.FD_SW_GUST_N:L.FD_SW_GUST_N + 3].any()
    print(f"zero rows, {'mission' if mission else 'step'} {precision}: bit-identical to the still-air entry over 200 steps: {identical}; "
          f"worst fp64 word {worst64:.3e} relative, worst f32 word {worst_ulp:.2f} fp32 ulp")
    assert worst64 <= 1e-15 and worst_ulp <= 1.0
    assert plain.pads_untouched() and windy.pads_untouched()


# ---- f64 against the restatement --------------------------------------------------------------------------------------------------
def test_steady_wind_against_the_restatement(f, gate):
    c = wn.compare_flights()
    run = Run(f, np.arange(10), c["rows0"], x=c["x_start"]).launch(100)
    run.ref.copy_(_dev(c["ref_cmd"].T))
    run.launch(400)
    assert run.pads_untouched()
    dx, di = _state_diff(run.host("x"), c["x_500"]), np.abs(run.host("integ") - c["integ_500"])
    _report("steady wind, 10 aircraft, 500 steps", dx, di, *gate)
    assert np.array_equal(run.host("rows"), c["rows0"])                       # B = 0: the gust rows are rewritten with themselves
    assert (dx <= gate[0]).all() and (di <= gate[1]).all(), (dx.max(axis=0), di.max(axis=0))


def test_replayed_gusts_against_the_restatement(f, gate):
    c = wn.compare_flights(gusts=True)
    z = _dev(c["z"])
    run = Run(f, np.arange(10), c["rows0"], x=c["x_start"]).launch(100, z=z[:100].contiguous())
    run.ref.copy_(_dev(c["ref_cmd"].T))
    run.launch(200, z=z[100:300].contiguous())
    rows = np.array(c["rows0"])
    for s in range(300):
        rows[:, 3:6] = wn.gust_update(rows[:, 3:6], rows[:, 6:7], rows[:, 7:8], c["z"][s].T)
    assert np.array_equal(run.host("rows").view(np.uint64), rows.view(np.uint64)), "gust rows after 300 steps"
    run.launch(200, z=z[300:].contiguous())
    assert run.pads_untouched()
    assert np.array_equal(run.host("rows").view(np.uint64), np.ascontiguousarray(c["rows_500"]).view(np.uint64)), "gust rows after 500 steps"
    dx, di = _state_diff(run.host("x"), c["x_500"]), np.abs(run.host("integ") - c["integ_500"])
    _report("replayed gusts, 10 aircraft, 500 steps", dx, di, *gate)
    assert (dx <= gate[0]).all() and (di <= gate[1]).all(), (dx.max(axis=0), di.max(axis=0))


def _gusty(f, n, sigma=1.0):
    rs = np.random.RandomState(11)
    rows = np.tile(wn.steady_rows(*wn.STEADY), (n, 1))
    rows[:, 3:6] = rs.normal(0, 0.5, (n, 3))
    rows[:, wn.SW_GUST_A] = np.exp(-DT * np.asarray(f["spec"])[np.arange(n) % 10, 0] / wn.GUST_LENGTH)
    rows[:, wn.SW_GUST_B] = sigma * np.sqrt(1.0 - rows[:, wn.SW_GUST_A] ** 2)
    return rows


def test_in_kernel_draws_against_the_host_model(f):
    n = 257
    lanes = np.arange(n) % 10
    for mission, start in ((False, 0), (True, 41)):
        short = mn.short_flights()
        kw = dict(wps=short["wps"], C=short["C"]) if mission else {}
        run = Run(f, lanes, _gusty(f, n), step=start, **kw)
        for k in range(3):
            before = run.host("rows")
            run.launch(1)
            after = run.host("rows")
            got = (after[:, 3:6] - before[:, 6:7] * before[:, 3:6]) / before[:, 7:8]
            want = wn.gust_normals(SEED, np.arange(n), start + k + 1)
            err = np.abs(got - want).max()
            print(f"in-kernel gust normals, {'mission' if mission else 'step'}, counter step {start + k + 1}: worst |recovered - host model| {err:.3e}")
            assert err <= 1e-5
            assert np.array_equal(after[:, [0, 1, 2, 6, 7]], before[:, [0, 1, 2, 6, 7]])
            run.step += 1                                                      # the caller advances it
        assert run.pads_untouched()
    # a NULL step pointer draws with 0
    a, b = Run(f, lanes, _gusty(f, n)).launch(3), Run(f, lanes, _gusty(f, n)).launch(3, null=("step",))
    assert _same(a.snapshot(), b.snapshot()) == []


def test_two_launches_with_the_counter_advanced_are_one(f):
    one = Run(f, np.arange(10), _gusty(f, 10)).launch(100)
    two = Run(f, np.arange(10), _gusty(f, 10)).launch(50)
    two.step += 50
    two.launch(50)
    a, b = one.snapshot(), two.snapshot()
    assert _same(a, b, [k for k in Run.ARRAYS if k != "step"]) == []
    assert a["rows"][3:6].abs().max() > 0 and not torch.equal(a["rows"][3:6], _dev(_gusty(f, 10).T)[3:6])


# ---- the mission in the chosen crosswind ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cross():
    assert wn.chosen_crosswind() == 8.0
    return wn.mission_flights(wn.chosen_crosswind())


def _mission_run(cross, lanes=np.arange(10), rows=None, precision="f64", **kw):
    f = cross["f"]
    lanes = np.asarray(lanes)
    rows = np.tile(cross["wind"], (len(lanes), 1)) if rows is None else rows
    x = np.array([wn.to_ground(f["x0"][i], wn.air_mass(cross["wind"])) for i in lanes])
    return Run(f, lanes, rows, wps=cross["wps"], C=cross["C"], precision=precision, x=x, limits=wn.MISSION_LIMITS, **kw)


@pytest.fixture(scope="module")
def ten(cross):
    run = _mission_run(cross).launch(mn.SHORT_STEPS)
    assert run.pads_untouched()
    return run.snapshot()


def test_mission_in_the_crosswind_against_the_restatement(ten, cross):
    rows = cross["rows"]
    h = lambda k: ten[k].T.cpu().numpy()   # noqa: E731
    for k, key in (("idx", "idx"), ("reached", "reached"), ("flown", "flown"), ("sat", "sat")):
        assert np.array_equal(h(k)[:, 0], [r[key] for r in rows]), (k, h(k)[:, 0].tolist(), [r[key] for r in rows])
    g = wn.mission_yardstick_groups()
    gx, gi = wn.state_gate(g)
    dx, di = _state_diff(h("x"), np.array([r["x"] for r in rows])), np.abs(h("integ") - np.array([r["integ"] for r in rows]))
    _report("mission, 8 m/s from abeam, 10 aircraft, 1500 steps", dx, di, gx, gi)
    ds = np.abs(h("stats") - np.array([r["stats"] for r in rows]))
    gs = 10.0 * np.array([g["position"], g["angle"], g["velocity"], g["position"]])     # altitude error, roll, airspeed, cross-track
    print(f"mission statistics: worst |device - restatement| {ds.max(axis=0)} (gates {gs})")
    assert (dx <= gx).all() and (di <= gi).all() and (ds <= gs).all(), (dx.max(axis=0), di.max(axis=0), ds.max(axis=0))


def test_complete_lanes_and_controls_only(cross, f):
    # every word of a complete lane, its gust rows included, is untouched by a further launch (gusts drawn in the kernel)
    run = _mission_run(cross, rows=_gusty(f, 10)).launch(mn.SHORT_STEPS)
    run.step += mn.SHORT_STEPS
    a = run.snapshot()
    done = torch.nonzero(a["idx"][0] >= 3)[:, 0]
    assert len(done) >= 1
    b = run.launch(20).snapshot()
    assert _same(a, b, lanes_a=done, lanes_b=done) == []
    assert run.pads_untouched()
    # n_steps = 0 writes nothing but surf_out, and its controls are those of a lane of an n_steps = 1 launch
    for mission in (False, True):
        mk = (lambda: _mission_run(cross, rows=_gusty(f, 10))) if mission else (lambda: Run(f, np.arange(10), _gusty(f, 10), x=wn.compare_flights()["x_start"]))
        zero, one = mk(), mk()
        before = zero.snapshot()
        after = zero.launch(0).snapshot()
        assert _same(before, after, [k for k in Run.ARRAYS if k != "surf"]) == []
        first = one.launch(1).snapshot()
        assert bool(torch.isfinite(after["surf"]).all())
        if mission:                                                            # one call site of guidance and law per kernel: to the bit
            assert _same(after, first, ["surf"]) == []
        else:                                                                  # tests/test_gpu_servo.py's gate for the plain entry
            assert float((after["surf"] - first["surf"]).abs().max()) <= 1e-15
        assert zero.pads_untouched()


@pytest.mark.parametrize("n", [1, 63, 65, 257])
def test_shapes_and_lane_position(n, ten, cross, f):
    lanes = np.arange(n) % 10
    run = _mission_run(cross, lanes).launch(mn.SHORT_STEPS)
    assert run.pads_untouched(), "wrote behind an array"
    assert _same(run.snapshot(), ten, lanes_b=torch.as_tensor(lanes, device=DEV)) == [], "a lane's result depends on where it sits in the launch"
    # the step entry with replayed normals: z is indexed [s][k][lane]
    z10 = _dev(wn.replay_normals(60, 10))
    base = Run(f, np.arange(10), _gusty(f, 10)).launch(60, z=z10).snapshot()
    run = Run(f, lanes, _gusty(f, 10)[lanes]).launch(60, z=z10[:, :, torch.as_tensor(lanes, device=DEV)].contiguous())
    assert run.pads_untouched(), "wrote behind an array"
    assert _same(run.snapshot(), base, lanes_b=torch.as_tensor(lanes, device=DEV)) == []


# ---- interface --------------------------------------------------------------------------------------------------------------------
def test_null_outputs_leave_the_rest_alone(cross, f):
    full = _mission_run(cross, rows=_gusty(f, 10)).launch(300).snapshot()
    for name in ("surf", "sat", "err", "reached", "flown", "stats"):
        run = _mission_run(cross, rows=_gusty(f, 10))
        before = run.snapshot()
        got = run.launch(300, null=(name,)).snapshot()
        assert _same(got, full, [k for k in Run.ARRAYS if k != name]) == [], name
        assert _same(got, before, [name]) == [], name
        assert run.pads_untouched()
    full = Run(f, np.arange(10), _gusty(f, 10)).launch(100).snapshot()
    for name in ("surf", "sat", "err"):
        got = Run(f, np.arange(10), _gusty(f, 10)).launch(100, null=(name,)).snapshot()
        assert _same(got, full, [k for k in Run.ARRAYS if k != name]) == [], name


def _method_fleet(f, x, precision="f64"):
    n = len(f["type"])
    fleet = BatchedSixDOF(n, precision, types=tn.TYPES, type_index=f["type"])
    fleet.reset(np.asarray(x))
    fleet._servo = SV.ServoDesign(_dev(f["K"].T), torch.zeros(n, dtype=torch.float64, device=DEV), torch.zeros(n, dtype=torch.int32, device=DEV),
                                  torch.zeros(n, dtype=torch.int32, device=DEV), _dev(f["x0"].T), _dev(f["u0"].T))
    fleet.servo = SV.ServoState.at_trim(fleet._servo.x0)
    return fleet


def test_graph_replay_equals_eager_launches(f):
    x0 = wn.compare_flights()["x_start"]
    fe, we = _method_fleet(f, x0), SV.ServoWind(_dev(_gusty(f, 10).T), seed=SEED)
    fg, wg = _method_fleet(f, x0), SV.ServoWind(_dev(_gusty(f, 10).T), seed=SEED)
    for _ in range(10):
        fe.step_servo(5, DT, wind=we)
    carried = lambda fl, w: (fl.x, fl.servo.ref, fl.servo.integ, fl._saturated_steps(), w.rows, w.step)   # noqa: E731
    saved = [t.clone() for t in carried(fg, wg)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                                 # warm-up outside the capture
        fg.step_servo(5, DT, wind=wg)
    torch.cuda.current_stream().wait_stream(s)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        fg.step_servo(5, DT, wind=wg)
    for t, v in zip(carried(fg, wg), saved):                                   # start over: the warm-up flew
        t.copy_(v)
    for _ in range(10):
        gr.replay()
    torch.cuda.synchronize()
    assert int(wg.step) == int(we.step) == 50                                  # the counter's increment is part of the graph
    for a, b in zip(carried(fe, we) + (fe.u, fe.servo.err), carried(fg, wg) + (fg.u, fg.servo.err)):
        assert torch.equal(_bits(a), _bits(b))
    assert not torch.equal(we.rows[3:6], _dev(_gusty(f, 10).T)[3:6])           # the replays drew gusts


class _Spy:
    def __init__(self, lib):
        self.lib, self.names = lib, []

    def __getattr__(self, name):
        if name.startswith("fdyn_servo_"):                                     # building a fleet calls other entries
            self.names.append(name)
        return getattr(self.lib, name)


def test_fleet_methods_route_by_the_wind(cross, f, monkeypatch):
    c = wn.compare_flights()
    spy = _Spy(_lib.load())
    monkeypatch.setattr(_lib, "_lib", spy)
    # step_servo(wind=) is step_into(wind=)
    fleet, wind = _method_fleet(f, c["x_start"]), SV.ServoWind(_dev(_gusty(f, 10).T), seed=SEED)
    fleet.step_servo(40, DT, wind=wind)
    run = Run(f, np.arange(10), _gusty(f, 10), x=c["x_start"])
    w2 = SV.ServoWind(run.rows, seed=SEED, step=run.step[0])
    SV.step_into("f64", run.x, run.design, SV.ServoState(run.ref, run.integ, run.limits, run.err), run.fleet.params, run.fleet.type_index, DT, 40,
                 run.surf, run.sat, run.err, wind=w2)
    torch.cuda.synchronize()
    assert spy.names == ["fdyn_servo_step_wind_f64"] * 2 and int(wind.step) == int(run.step) == 40
    for a, b in ((fleet.x, run.x), (fleet.servo.ref, run.ref), (fleet.servo.integ, run.integ), (wind.rows, run.rows), (fleet.u, run.surf), (fleet.servo.err, run.err)):
        assert torch.equal(_bits(a), _bits(b))
    # fly_servo_mission(wind=) is mission_into(wind=), here the `ten` of the restatement test
    del spy.names[:]
    x = np.array([wn.to_ground(f["x0"][i], wn.air_mass(cross["wind"])) for i in range(10)])
    fleet = _method_fleet(f, x)
    fleet.servo.limits.copy_(_dev(np.array(wn.MISSION_LIMITS)))
    m = fleet.start_servo_mission(cross["wps"], acceptance_radius=mn.RADIUS)
    wind = SV.ServoWind(_dev(np.tile(cross["wind"], (10, 1)).T), seed=SEED)
    fleet.fly_servo_mission(900, DT, wind=wind)
    fleet.fly_servo_mission(600, DT, wind=wind)
    torch.cuda.synchronize()
    assert spy.names == ["fdyn_servo_mission_wind_f64"] * 2 and int(wind.step) == 1500 and bool(fleet.servo_mission_complete().all())
    ten_ = _mission_run(cross).launch(mn.SHORT_STEPS).snapshot()
    for a, b in ((fleet.x, ten_["x"]), (fleet.servo.integ, ten_["integ"]), (m.wp_idx, ten_["idx"][0]), (m.steps_flown, ten_["flown"][0]),
                 (m.reached_total, ten_["reached"][0]), (m.stats, ten_["stats"]), (fleet.lqr_saturated_steps, ten_["sat"][0])):
        assert torch.equal(_bits(a), _bits(b))
    # wind=None: the old calls
    del spy.names[:]
    fleet = _method_fleet(f, f["x0"])
    fleet.step_servo(3, DT)
    fleet.start_servo_mission(cross["wps"], acceptance_radius=mn.RADIUS)
    fleet.fly_servo_mission(3, DT)
    assert spy.names == ["fdyn_servo_step_f64", "fdyn_servo_mission_f64"]
    with pytest.raises(ValueError, match="there is none"):
        SV.step_into("f64", run.x, run.design, SV.ServoState(run.ref, run.integ, run.limits, run.err), run.fleet.params, run.fleet.type_index, DT, 1,
                     z=torch.zeros((1, 3, 10), dtype=torch.float64, device=DEV))


# ---- mixed and f32 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "mixed", "f32"])
def test_references_are_held_in_wind_and_downdraft(precision):
    """The CPU test (c) on the device: the four probe conditions, 40 s, the wind from abeam and the downdraft switched on at 1 s by
    changing the rows.  The end errors are formed on the host in fp64 from the final state, references and rows."""
    for r in wn.probe_flights():
        d = {k: np.array([r[k]]) for k in ("type", "K", "x0", "u0")}
        d["ref0"] = np.array([sn.reference_at(r["x0"])])
        n1, n2 = int(round(sn.T_COMMAND / r["dt"])), int(round((sn.T_END - sn.T_COMMAND) / r["dt"]))
        run = Run(d, [0], _calm(1), precision=precision).launch(n1, dt=r["dt"])
        run.rows.copy_(_dev(r["wind"][:, None]))
        run.launch(n2, dt=r["dt"])
        assert run.pads_untouched()
        err = wn.errors(run.host("x")[0], run.host("ref")[0], wn.air_mass(r["wind"]))
        print(f"{precision}, {r['dt']}: end errors {err} (restatement {r['err']})")
        assert abs(err[0]) <= sn.GATE_V and abs(err[1]) <= sn.GATE_H and abs(err[2]) <= sn.GATE_PSI, (precision, err)


def test_reduced_precision_fleets_fly_beside_f64(cross):
    """reached_total equal and each event step within one step of the f64 fleet's; the state difference at step 300 (before any
    second event) is printed, not gated."""
    fig = {}
    for p in ("f64", "mixed", "f32"):
        run = _mission_run(cross, precision=p)
        counts, x300 = [], None
        for s in range(1000):
            if s == 300:
                x300 = run.x.clone()
            run.launch(1)
            counts.append(run.reached[0].clone())
        counts = torch.stack(counts).cpu().numpy()
        events = np.array([[int(np.argmax(counts[:, i] >= k)) for k in (1, 2, 3)] for i in range(10)])
        fig[p] = (events, counts[-1], x300.T.cpu().numpy().astype(np.float64))
        assert run.pads_untouched()
    e64, r64, x64 = fig["f64"]
    assert np.array_equal(e64, [r["events"] for r in cross["rows"]]) and (r64 == 3).all()
    for p in ("mixed", "f32"):
        ev, reached, x300 = fig[p]
        print(f"{p}: worst |event step - f64's| {int(np.abs(ev - e64).max())}; state at step 300: worst rel_err to the f64 fleet "
              f"{rel_err(x300, x64, STATE_ANGLE_COLS).max():.3e}")
        assert np.array_equal(reached, r64) and np.abs(ev - e64).max() <= 1, (p, ev.tolist(), e64.tolist())

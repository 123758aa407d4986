"""fdyn_servo_lqg_mission_* (include/fdyn_servo_lqg_mission.h) and its host layer on the device.

Reference on the box: the restatement tests/servo_lqg_mission_numpy.py flown over the CPU oracle's RK4 on replayed Philox normals,
computed once per session and shared; tests/test_servo_lqg_mission_oracle.py shows that no waypoint switch of those flights is
within 1e-6 m of the acceptance radius (asserted again here before comparing), which is what lets the f64 test demand EQUAL counters.

Gates (none derived from what the kernels return):
  feedback = truth against fdyn_servo_mission_*   bit-identical in all three precisions
  f64 against the restatement, z replayed         counters equal; x, xhat, phat, du_prev, integ, ref, the five accumulators, stats 1e-9
                                                  (the project's gate for the same law and filter)
  mixed, f32 against the f64 fleet                tests/test_gpu_servo_mission.py's comparison and its GATES
  in-kernel draws against philox_numpy            1e-5 (the gate of the servo estimator's draws: fp32 Box-Muller)
  controls, n_steps = 0                           1e-13: a heading command a few ulp (4e-16) off the restatement's, times the heading gains
  split launches, graph replay, lane position, complete lanes, NULL outputs, refusals, fleet methods: bit-identical
  behaviour on in-kernel draws                    the CPU gates of tests/test_servo_lqg_mission_oracle.py, in all three precisions
"""
import numpy as np
import pytest
import torch

from conftest import rel_err, STATE_ANGLE_COLS
import lqr_numpy as ln
import servo_lqg_mission_numpy as lm
import servo_lqg_numpy as lq
import servo_mission_numpy as mn
import servo_numpy as sn
import trim_numpy as tn
from hcrl_amd import _lib, layout as L
from hcrl_amd import servo as SV
from hcrl_amd import servo_lqg as SL
from hcrl_amd import servo_lqg_mission as SM
from hcrl_amd.fleet import BatchedSixDOF
from test_gpu_servo_mission import GATES, Run as MissionRun, _same as _same_mission

pytestmark = pytest.mark.gpu

SENTINEL = -12345.678
ISENT = -1234567
PAD = 96
DEV = "cuda"
DT = ln.DT
FB = {"estimate": lm.ESTIMATE, "measurement": lm.MEASUREMENT, "truth": lm.TRUTH}


def _dev(a, dtype=None):
    t = torch.as_tensor(np.array(a, order="C"), device=DEV)
    return t if dtype is None else t.to(dtype)


class Run:
    """One fleet's arrays for fdyn_servo_lqg_mission_*, every written array a [rows][n] view of a buffer with a sentinel pad behind
    it.  `lanes` picks the aircraft of lm.setup() lane by lane."""
    OPTIONAL = ("surf", "sat", "err", "reached", "flown", "stats", "err_est", "err_meas", "chatter", "meas", "err_pos")
    ARRAYS = ("x", "ref", "integ", "idx", "surf", "err", "sat", "reached", "flown", "stats", "xhat", "du", "err_est", "err_meas",
              "chatter", "meas", "phat", "err_pos")

    def __init__(self, su, lanes, precision="f64", gain=None, C=None, seed=lm.SEED):
        f = su["f"]
        lanes = np.asarray(lanes)
        self.n, self.precision, self.lanes, self.seed = len(lanes), precision, lanes, seed
        n, sdt, f64, i32 = self.n, _lib.state_dtype(precision), torch.float64, torch.int32
        self.fleet = BatchedSixDOF(n, precision, types=tn.TYPES, type_index=f["type"][lanes])
        self._bufs = []
        zeros = lambda rows, dt=np.float64: np.zeros((rows, n), dt)   # noqa: E731
        self.x = self._view(L.FD_NX, sdt, f["x0"][lanes].T)
        self.ref = self._view(L.FD_NSVR, f64, f["ref0"][lanes].T)
        self.integ = self._view(L.FD_NSVI, f64, zeros(L.FD_NSVI))
        self.idx, self.sat, self.reached, self.flown = (self._view(1, i32, zeros(1, np.int32)) for _ in range(4))
        self.surf = self._view(L.FD_NU, sdt, None)
        self.err = self._view(L.FD_NSVI, f64, None)
        self.stats = self._view(L.FD_NMST, f64, np.tile(np.array(mn.STATS_START)[:, None], (1, n)))
        self.xhat, self.err_est, self.err_meas = (self._view(L.FD_NSKX, f64, zeros(L.FD_NSKX)) for _ in range(3))
        self.du, self.chatter = (self._view(L.FD_NU, f64, zeros(L.FD_NU)) for _ in range(2))
        self.meas = self._view(L.FD_NSKX, f64, None)
        self.phat = self._view(2, f64, f["x0"][lanes].T[:2])
        self.err_pos = self._view(2, f64, zeros(2))
        self.step = torch.zeros(1, dtype=i32, device=DEV)
        self.K, self.x0, self.u0 = _dev(f["K"][lanes].T), _dev(f["x0"][lanes].T), _dev(f["u0"][lanes].T)
        self.F, self.sigma = _dev(su["F"][lanes].T), _dev(np.array(lq.DEFAULT_SIGMA))
        self.limits = _dev(np.array(sn.DEFAULT_LIMITS))
        self.wps, self.C = _dev(np.asarray(su["wps"], np.float64)), _dev(np.asarray(su["C"] if C is None else C, np.float64))
        self.pos = _dev(lm.position_words(gain=gain, dt=DT))

    def _view(self, rows, dtype, init):
        sent = ISENT if dtype == torch.int32 else SENTINEL
        buf = torch.full((rows * self.n + PAD,), sent, dtype=dtype, device=DEV)
        view = buf[:rows * self.n].view(rows, self.n)
        if init is not None:
            view.copy_(_dev(np.asarray(init)).to(dtype))
        self._bufs.append((buf, rows * self.n, sent))
        return view

    def call(self, n_steps, feedback="estimate", null=(), z=None, dt=DT, **over):
        """The entry's return code; `over` replaces arguments by name (n, n_wp, n_types); feedback a name or the integer itself."""
        p = lambda name: None if name in null else _lib.ptr(getattr(self, name))   # noqa: E731
        fl, fb = self.fleet, feedback if isinstance(feedback, int) else FB[feedback]
        return getattr(_lib.load(), f"fdyn_servo_lqg_mission_{self.precision}")(
            p("x"), p("x0"), p("u0"), p("K"), p("ref"), p("integ"), p("limits"), p("idx"), p("C"), p("wps"), over.get("n_wp", int(self.wps.shape[0])),
            _lib.ptr(fl.type_index), _lib.ptr(fl.params), over.get("n_types", int(fl.params.shape[0])), over.get("n", self.n), float(dt), int(n_steps),
            p("surf"), p("sat"), p("err"), p("reached"), p("flown"), p("stats"), p("F"), p("sigma"), p("xhat"), p("du"), self.seed, p("step"),
            _lib.ptr(z), fb, p("err_est"), p("err_meas"), p("chatter"), p("meas"), p("pos"), p("phat"),
            p("err_pos"), _lib.current_stream())

    def launch(self, n_steps, feedback="estimate", null=(), z=None):
        _lib.check(self.call(n_steps, feedback, null, z), "fdyn_servo_lqg_mission")
        if n_steps > 0 and "step" not in null:
            self.step += int(n_steps)
        return self

    def pads_untouched(self):
        torch.cuda.synchronize()
        return all(bool((buf[used:] == sent).all()) for buf, used, sent in self._bufs)

    def snapshot(self):
        torch.cuda.synchronize()
        return {k: getattr(self, k).clone() for k in self.ARRAYS}

    def host(self, name):
        return getattr(self, name).T.cpu().numpy().astype(np.float64 if getattr(self, name).dtype.is_floating_point else np.int64)


def _same(a, b, keys=Run.ARRAYS, lanes_a=None, lanes_b=None):
    return _same_mission(a, b, keys, lanes_a, lanes_b)


@pytest.fixture(scope="module")
def su():
    return lm.setup()


def _z(su, lanes, steps=lm.STEPS):
    """[steps][12][n] on the device: the setup's replayed normals, lane by lane."""
    return _dev(np.ascontiguousarray(su["z"][:steps][:, np.asarray(lanes) % 10, :].transpose(0, 2, 1)))


@pytest.fixture(scope="module")
def ten(su):
    """The ten aircraft in ONE launch of 1500 steps on the device under the estimate, f64, z replayed: {feedback: snapshot}."""
    out = {}
    for fb in FB:
        run = Run(su, np.arange(10)).launch(lm.STEPS, fb, z=_z(su, np.arange(10)))
        assert run.pads_untouched()
        out[fb] = run.snapshot()
    return out


# ---- feedback = truth is the mission kernel ------------------------------------------------------------------------------------------
TRUTH_KEYS = ("x", "ref", "integ", "idx", "reached", "flown", "stats", "surf", "sat", "err")


def _truth_pair(su, precision):
    lanes = np.arange(257) % 10
    mine, theirs = Run(su, lanes, precision), MissionRun(su["f"], lanes, su["wps"], su["C"], precision)
    for _ in range(15):
        mine.launch(100, "truth")
        theirs.launch(100)
    assert mine.pads_untouched() and theirs.pads_untouched()
    return mine.snapshot(), theirs.snapshot()


@pytest.mark.parametrize("precision", ["f64", "mixed", "f32"])
def test_truth_is_the_mission_kernel_bit_for_bit(precision, su):
    """In f64 too: the true state's errors are formed after the law (DESIGN section 7m's placement), and no word differs."""
    a, b = _truth_pair(su, precision)
    assert bool((b["idx"] == 3).all()) and _same(a, b, TRUTH_KEYS) == []


# ---- f64 against the restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("feedback", ["estimate", "measurement", "truth"])
def test_f64_against_the_restatement_on_replayed_normals(feedback, ten, su):
    rows, records = lm.short_flights(FB[feedback])
    margin = min(abs(d - mn.RADIUS) for rec in records for d, _ in rec if not np.isnan(d))
    assert margin > 1e-6, "a waypoint switch of the reference flight rests on rounding"
    s = ten[feedback]
    h = lambda k: s[k].T.cpu().numpy()   # noqa: E731
    for k, key in (("idx", "idx"), ("reached", "reached"), ("flown", "flown"), ("sat", "sat")):
        assert np.array_equal(h(k)[:, 0], [r[key] for r in rows]), (k, h(k)[:, 0].tolist(), [r[key] for r in rows])
    want = lambda key: np.array([r[key] for r in rows])   # noqa: E731
    errs = {"x": rel_err(h("x"), want("x"), STATE_ANGLE_COLS).max()}
    for k, key in (("xhat", "xhat"), ("phat", "phat"), ("du", "du_prev"), ("integ", "integ"), ("err_est", "err_est"), ("err_meas", "err_meas"),
                   ("chatter", "chatter"), ("err_pos", "err_pos"), ("stats", "stats")):
        errs[k] = (np.abs(h(k) - want(key)) / np.maximum(1.0, np.abs(want(key)))).max()
    er = np.abs(h("ref") - want("ref"))
    er[:, L.FD_SVR_HEADING] = np.abs(ln.wrap_angle(er[:, L.FD_SVR_HEADING]))
    errs["ref"] = er.max()
    print(f"{feedback}: smallest |distance - radius| {margin:.2e} m; worst |device - restatement|: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(v <= 1e-9 for v in errs.values()), errs
    assert all(r["reached"] == 3 and r["flown"] < lm.STEPS for r in rows)


# ---- reduced precision ---------------------------------------------------------------------------------------------------------
def test_reduced_precision_fleets_fly_beside_f64(su):
    """tests/test_gpu_servo_mission.py's comparison on the estimate with the normals replayed: reached_total at step 1500 equal, each
    event step within its band of the f64 fleet's, the state at step 300 within its gate (GATES: event steps 1, rel_err mixed 3e-06,
    f32 2e-04)."""
    z, fig = _z(su, np.arange(10)), {}
    for p in ("f64", "mixed", "f32"):
        run = Run(su, np.arange(10), p)
        counts, x300 = [], None
        for s in range(lm.STEPS):
            if s == 300:
                x300 = run.x.clone()
            run.launch(1, "estimate", z=z[s:s + 1])
            counts.append(run.reached[0].clone())
        counts = torch.stack(counts).cpu().numpy()
        events = np.array([[int(np.argmax(counts[:, i] >= k)) for k in (1, 2, 3)] for i in range(10)])
        fig[p] = (events, counts[-1], x300.T.cpu().numpy().astype(np.float64))
        assert run.pads_untouched()
    e64, r64, x64 = fig["f64"]
    assert np.array_equal(e64, [r["events"] for r in lm.short_flights(lm.ESTIMATE)[0]])
    got = {}
    for p in ("mixed", "f32"):
        ev, reached, x300 = fig[p]
        got[p] = (int(np.abs(ev - e64).max()), float(rel_err(x300, x64, STATE_ANGLE_COLS).max()))
        print(f"{p}: worst |event step - f64's| = {got[p][0]} steps; state at step 300: worst rel_err to the f64 fleet {got[p][1]:.3e}")
    for p in ("mixed", "f32"):
        assert np.array_equal(fig[p][1], r64), (p, fig[p][1], r64)
        assert got[p][0] <= GATES[p][0] and got[p][1] <= GATES[p][1], (p, got[p], GATES[p])


# ---- the draws -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", [0, 41, None])
def test_in_kernel_draws_are_the_host_models(step, su):
    """One step from the trim (d = 0) with g = 1 (phat = y_p): meas_out / sigma are the ten normals, (phat - p) / sigma_p the two."""
    lanes = np.arange(65) % 10
    run = Run(su, lanes, gain=1.0)
    if step is not None:
        run.step.fill_(step)
    run.launch(1, "estimate", null=() if step is not None else ("step",))
    got = np.concatenate([run.host("meas") / np.array(lq.DEFAULT_SIGMA), (run.host("phat") - su["f"]["x0"][lanes][:, :2]) / lm.SIGMA_POS], axis=1)
    want = lm.normals(lm.SEED, np.arange(65), (step or 0) + 1)
    print(f"step word {step}: worst |in-kernel normal - philox_numpy's| = {np.abs(got - want).max():.2e} (ten words {np.abs(got - want)[:, :10].max():.2e}, "
          f"position {np.abs(got - want)[:, 10:].max():.2e})")
    assert np.abs(got - want).max() <= 1e-5 and run.pads_untouched()


def test_split_launches_are_the_single_launch(su):
    one, two = Run(su, np.arange(10)), Run(su, np.arange(10))
    one.launch(100)
    two.launch(50).launch(50)
    assert int(one.step) == int(two.step) == 100 and _same(one.snapshot(), two.snapshot()) == []
    assert bool(one.err_pos.all()) and one.pads_untouched() and two.pads_untouched()


@pytest.mark.parametrize("n", [1, 63, 65, 257])
def test_shapes_and_lane_position(n, ten, su):
    lanes = np.arange(n) % 10
    run = Run(su, lanes).launch(lm.STEPS, "estimate", z=_z(su, lanes))
    assert run.pads_untouched(), "wrote behind an array"
    assert _same(run.snapshot(), ten["estimate"], lanes_b=torch.as_tensor(lanes, device=DEV)) == [], "a lane's result depends on where it sits in the launch"


# ---- completion ----------------------------------------------------------------------------------------------------------------------
KEPT = ("x", "ref", "integ", "du", "stats", "sat", "err", "surf", "flown")        # what a completing step leaves as it was


def test_complete_lanes(ten, su):
    """After 900 steps some aircraft have completed.  A further launch changes NOTHING of theirs, in any array.  A lane launched for
    exactly the steps it flies and then for one more: that step marks it complete, its measurement, filters and accounting stand,
    and the words of KEPT stay; the single launch of 1500 holds the same words."""
    flown = ten["estimate"]["flown"][0].cpu().numpy()
    done = np.flatnonzero(flown < 900)
    assert 0 < len(done) < 10
    z = _z(su, np.arange(10))
    run = Run(su, np.arange(10)).launch(900, z=z[:900])
    at900 = run.snapshot()
    assert at900["flown"][0].cpu().tolist() == np.minimum(flown, 900).tolist()
    run.launch(20, z=z[900:920])
    at920 = run.snapshot()
    d = torch.as_tensor(done, device=DEV)
    assert _same(at920, at900, lanes_a=d, lanes_b=d) == []
    assert _same(ten["estimate"], at900, lanes_a=d, lanes_b=d) == []
    flying = torch.as_tensor(np.flatnonzero(flown >= 920), device=DEV)
    assert bool((at920["flown"][0, flying] == 920).all()) and not torch.equal(at920["xhat"][:, flying], at900["xhat"][:, flying])
    lane, k = int(done[0]), int(flown[done[0]])
    alone = Run(su, np.arange(10)).launch(k, z=z[:k])
    before = alone.snapshot()
    assert int(before["idx"][0, lane]) == 2 and int(before["flown"][0, lane]) == k
    after = alone.launch(1, z=z[k:k + 1]).snapshot()
    assert int(after["idx"][0, lane]) == 3 and int(after["reached"][0, lane]) == int(before["reached"][0, lane]) + 1
    assert _same(after, before, KEPT + ("chatter",), [lane], [lane]) == []
    assert set(_same(after, before, ("xhat", "phat", "err_est", "err_meas", "err_pos", "meas"), [lane], [lane])) == \
        {"xhat", "phat", "err_est", "err_meas", "err_pos", "meas"}
    assert _same(after, ten["estimate"], Run.ARRAYS, [lane], [lane]) == []
    assert run.pads_untouched() and alone.pads_untouched()


def test_restart_keeps_flying(su):
    run = Run(su, np.arange(10), C=mn.consts("PP", mn.RADIUS, "restart")).launch(lm.STEPS)
    s = run.snapshot()
    assert bool((s["flown"] == lm.STEPS).all()) and bool((s["reached"] >= 3).all()) and bool((s["idx"] < 3).all()) and run.pads_untouched()


def test_controls_only(ten, su):
    """n_steps = 0 on states out of a flight: only surf_out is written; the controls are the restatement's from the stored estimate
    and position estimate; under truth they are, to the bit, those of the next launch of one step; a complete lane writes nothing."""
    z = _z(su, np.arange(10))
    for fb in ("estimate", "measurement", "truth"):
        run = Run(su, np.arange(10)).launch(900, fb, z=z[:900])
        before = run.snapshot()
        assert 0 < int((before["idx"][0] < 3).sum()) < 10
        live = []
        run.surf.fill_(SENTINEL)
        run.launch(0, fb)
        after = run.snapshot()
        assert _same(after, before, [k for k in Run.ARRAYS if k != "surf"]) == [] and run.pads_untouched() and int(run.step) == 900
        f, got = su["f"], run.host("surf")
        for i in range(10):
            u = lm.controls_from(f["K"][i], f["x0"][i], f["u0"][i], run.host("x")[i], run.host("xhat")[i], run.host("phat")[i], run.host("integ")[i],
                                 su["wps"], su["C"], int(before["idx"][0, i]), FB[fb])
            live.append(u is not None)
            if u is None:
                assert (got[i] == SENTINEL).all(), "a complete lane's controls were written"
            else:
                assert np.abs(got[i] - ln.clip_controls(u)[0]).max() <= 1e-13, (fb, i)
        assert 0 < sum(live) < 10
        if fb == "truth":
            nxt = run.launch(1, fb, z=z[900:901]).snapshot()
            lv = torch.as_tensor(np.flatnonzero(np.array(live) & (nxt["flown"][0].cpu().numpy() > before["flown"][0].cpu().numpy())), device=DEV)
            assert len(lv) and torch.equal(nxt["surf"][:, lv], after["surf"][:, lv])


def test_null_for_each_optional_output_leaves_the_others(su):
    base = Run(su, np.arange(10)).launch(450).snapshot()
    assert bool((base["reached"] == 2).any()) and bool(base["sat"].any())
    for name in Run.OPTIONAL:
        run = Run(su, np.arange(10))
        untouched = getattr(run, name).clone()
        got = run.launch(450, null=(name,)).snapshot()
        assert _same(got, base, [k for k in Run.ARRAYS if k != name]) == [], name
        assert torch.equal(got[name], untouched) and run.pads_untouched(), name
    got = Run(su, np.arange(10)).launch(450, null=("step",)).snapshot()           # a NULL step word is 0
    assert _same(got, base) == []


def test_every_refusal_writes_nothing(su):
    run = Run(su, np.arange(10))
    before = run.snapshot()
    bad = _lib.FDYN_ERR_BAD_SIZE
    for kw, code in ((dict(n_steps=-1), bad), (dict(n_wp=0), bad), (dict(n_wp=L.FD_MAX_WAYPOINTS + 1), bad), (dict(n=-1), bad),
                     (dict(n_types=0), _lib.FDYN_ERR_BAD_TYPES), (dict(n_types=9), _lib.FDYN_ERR_BAD_TYPES), (dict(feedback=3), bad),
                     (dict(dt=2.0), _lib.FDYN_ERR_BAD_DT), (dict(dt=float("nan")), _lib.FDYN_ERR_BAD_DT)):
        kw = dict(kw)
        assert run.call(kw.pop("n_steps", 5), **kw) == code, kw
    for name in ("x", "x0", "u0", "K", "ref", "integ", "limits", "idx", "C", "wps", "F", "sigma", "xhat", "du", "pos", "phat"):
        assert run.call(5, null=(name,)) == _lib.FDYN_ERR_NULL, name
    assert run.call(5, null=("phat",), feedback=7, dt=9.0) == _lib.FDYN_ERR_NULL                # pointers before feedback before dt
    assert run.call(5, feedback=7, dt=9.0) == bad
    # the words of pos are the host layer's to refuse
    fl = _method_fleet(su)
    for kw in (dict(gain=0.0), dict(gain=1.0001), dict(gain=float("nan")), dict(sigma_pos=-0.5), dict(sigma_pos=float("inf"))):
        with pytest.raises(_lib.FdynError, match="bad size argument"):
            fl.start_servo_lqg_mission(su["wps"], acceptance_radius=mn.RADIUS, **kw)
    fl.servo_position.gain = 2.0
    x = fl.x.clone()
    with pytest.raises(_lib.FdynError, match="bad size argument"):
        fl.fly_servo_lqg_mission(5)
    assert _same(run.snapshot(), before) == [] and run.pads_untouched() and torch.equal(fl.x, x)


# ---- behaviour on in-kernel draws --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "mixed", "f32"])
def test_behaviour_gates_hold_on_in_kernel_draws(precision, su):
    s = {}
    for key, fb, gain in (("truth", "truth", None), ("est", "estimate", None), ("meas", "measurement", None), ("raw", "estimate", 1.0)):
        run = Run(su, np.arange(10), precision, gain=gain).launch(lm.STEPS, fb)
        assert run.pads_untouched()
        s[key] = {k: v.cpu().numpy() for k, v in run.snapshot().items()}
    for key in ("truth", "est", "meas"):
        assert (s[key]["idx"][0] == 3).all() and (s[key]["reached"][0] == 3).all(), key
    steps = np.abs(s["est"]["flown"][0] - s["truth"]["flown"][0]) / s["truth"]["flown"][0]
    ratio = s["est"]["err_pos"][0] / s["est"]["err_pos"][1]
    lat = lambda key: s[key]["chatter"][[L.FD_U_AILERON, L.FD_U_RUDDER]]   # noqa: E731
    print(f"{precision}: steps flown, worst |estimate - truth| / truth {steps.max():.4f}; err_pos ratio {ratio.min():.3f} .. {ratio.max():.3f}; lateral "
          f"chatter estimate / truth {(lat('est') / lat('truth')).min():.2f} .. {(lat('est') / lat('truth')).max():.2f}, estimate / (g = 1) "
          f"{(lat('est') / lat('raw')).min():.2f} .. {(lat('est') / lat('raw')).max():.2f}, (g = 1) / truth {(lat('raw') / lat('truth')).min():.2f} .. "
          f"{(lat('raw') / lat('truth')).max():.2f}")
    assert steps.max() <= lm.GATE_STEPS and ratio.max() <= lm.GATE_POS_RATIO
    assert (lat("est") <= lm.GATE_CHATTER * lat("truth")).all()
    assert (lat("est") <= lm.GATE_RAW * lat("raw")).all() and (lat("raw") > lm.GATE_CHATTER * lat("truth")).all()


# ---- plumbing ------------------------------------------------------------------------------------------------------------------
def _method_fleet(su, precision="f64", **kw):
    """A BatchedSixDOF holding the reference's gains, filters and trim points, with a mission started through its own method."""
    f, n = su["f"], su["n"]
    fleet = BatchedSixDOF(n, precision, types=tn.TYPES, type_index=f["type"])
    fleet.reset(f["x0"])
    zi = lambda: torch.zeros(n, dtype=torch.int32, device=DEV)   # noqa: E731
    zd = lambda: torch.zeros(n, dtype=torch.float64, device=DEV)   # noqa: E731
    fleet._servo = SV.ServoDesign(_dev(f["K"].T), zd(), zi(), zi(), _dev(f["x0"].T), _dev(f["u0"].T))
    fleet.servo = SV.ServoState.at_trim(fleet._servo.x0)
    fleet._servo_kalman = SL.ServoKalmanDesign(_dev(su["F"].T), zd(), zi(), zi(), dt=DT, sigma=_dev(np.array(lq.DEFAULT_SIGMA)))
    fleet.servo_lqg = SL.ServoLqgState.zeros(n, DEV, seed=lm.SEED)
    if kw.pop("start", True):
        fleet.start_servo_lqg_mission(su["wps"], acceptance_radius=mn.RADIUS, **kw)
    return fleet


def _carried(fl):
    m, q, p = fl.servo_mission, fl.servo_lqg, fl.servo_position_state
    return (fl.x, fl.servo.ref, fl.servo.integ, m.wp_idx, m.reached_total, m.steps_flown, m.stats, fl._saturated_steps(), q.xhat, q.du_prev,
            q.step, q.err_est, q.err_meas, q.chatter, p.phat, p.err_pos)


def test_fleet_methods_agree_with_the_entry_point(su):
    bare = _method_fleet(su, start=False)
    with pytest.raises(ValueError, match="start_servo_lqg_mission"):
        bare.fly_servo_lqg_mission(1)
    bare._servo_kalman = None
    with pytest.raises(ValueError, match="no servo filter"):
        bare.start_servo_lqg_mission(su["wps"])
    fleet = _method_fleet(su)
    assert fleet.servo_position.words.tolist() == lm.position_words(dt=DT).tolist()
    assert torch.equal(fleet.servo_position_state.phat, fleet.x[:2]) and not bool(fleet.servo_mission_complete().any())
    fleet.fly_servo_lqg_mission(900)
    assert 0 < int(fleet.servo_mission_complete().sum()) < 10
    fleet.fly_servo_lqg_mission(600)
    run = Run(su, np.arange(10)).launch(900).launch(600)
    s = run.snapshot()
    m, q, p = fleet.servo_mission, fleet.servo_lqg, fleet.servo_position_state
    for got, k in ((fleet.x, "x"), (fleet.u, "surf"), (fleet.servo.ref, "ref"), (fleet.servo.integ, "integ"), (fleet.servo.err, "err"), (m.wp_idx, "idx"),
                   (m.reached_total, "reached"), (m.steps_flown, "flown"), (m.stats, "stats"), (fleet.lqr_saturated_steps, "sat"), (q.xhat, "xhat"),
                   (q.du_prev, "du"), (q.err_est, "err_est"), (q.err_meas, "err_meas"), (q.chatter, "chatter"), (q.meas, "meas"), (p.phat, "phat"),
                   (p.err_pos, "err_pos")):
        assert torch.equal(got.reshape(s[k].shape), s[k]), k
    assert bool(fleet.servo_mission_complete().all()) and fleet.time == pytest.approx(1500 * DT) and int(q.step) == 1500
    direct = _method_fleet(su)                                                 # the same arrays handed to lqg_mission_into: no fleet bookkeeping
    for k in (900, 600):
        SM.lqg_mission_into("f64", direct.x, direct._servo, direct._servo_kalman, direct.servo, direct.servo_lqg, direct.servo_mission,
                            direct.servo_position, direct.servo_position_state, direct.params, direct.type_index, DT, k, "estimate", None, direct.u,
                            direct._saturated_steps(), direct.servo.err)
    torch.cuda.synchronize()
    for a, b in zip(_carried(direct) + (direct.u, direct.servo.err), _carried(fleet) + (fleet.u, fleet.servo.err)):
        assert torch.equal(a, b)
    assert direct.time == 0.0
    with pytest.raises(ValueError, match="mission of that fleet"):
        SM.lqg_mission_into("f64", direct.x[:, :4].contiguous(), direct._servo, direct._servo_kalman, direct.servo, direct.servo_lqg,
                            direct.servo_mission, direct.servo_position, direct.servo_position_state, direct.params, None, DT, 1)
    with pytest.raises(ValueError, match=r"\[1\]\[12\]\[10\]"):
        fleet.fly_servo_lqg_mission(1, z=torch.zeros((1, 10, 10), dtype=torch.float64, device=DEV))


def test_graph_replay_equals_eager(su):
    fe, fg = _method_fleet(su), _method_fleet(su)
    for _ in range(10):
        fe.fly_servo_lqg_mission(50)
    saved = [t.clone() for t in _carried(fg)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                                 # warm-up outside the capture
        fg.fly_servo_lqg_mission(50)
    torch.cuda.current_stream().wait_stream(s)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        fg.fly_servo_lqg_mission(50)
    for t, v in zip(_carried(fg), saved):                                      # start over: the warm-up and the capture's bookkeeping
        t.copy_(v)
    for _ in range(10):
        gr.replay()
    torch.cuda.synchronize()
    for a, b in zip(_carried(fe) + (fe.u, fe.servo.err), _carried(fg) + (fg.u, fg.servo.err)):
        assert torch.equal(a, b)
    assert bool((fe.servo_mission.reached_total == 2).all()) and int(fg.servo_lqg.step) == 500

"""fdyn_loop_margins and hcrl_amd.margins on the device.

Reference on the box: the NumPy restatement (tests/margin_numpy.py) on the designs the LQR and Kalman restatements make of the 288
linearisations of tests/golden/trim_reference.npz, computed once per session.

Gates (none derived from what the kernel returns):
  grid          every word of curve, alpha_s, alpha_t, idx_s, idx_t and status BIT-IDENTICAL to the restatement at dt 0.01 and 0.02
                under estimate and truth feedback (fp64 on both sides, one rounding per operation in the same order; the one
                operation the earlier bit-identical kernels did not use is the fp64 square root)
  shapes        n = 1, 63, 65, 257 with sentinel pads behind every output; curve = NULL leaves the rest bit-equal; lane position
                is irrelevant;  n_omega = 1, 7, 64, 256;  0 and 257 are refused
  bad lanes     every kind of margin_numpy.bad_cases interleaved among good lanes: the good lanes bit-identical to a launch
                without them, the bad lanes exactly the restatement's status, NaNs and -1 indices
  graph         replay bit-equal to eager
  fleet         BatchedSixDOF.trim -> design_lqr -> design_kalman -> loop_margins on the device against the same chain in NumPy
                over the CPU oracle (the ten aircraft of lqr_numpy.oracle_flights): alpha within 1e-9 relative; and bit-identical
                to the restatement on the fleet's own K and F read back
  flight        the golden aircraft with the smallest lateral alpha_s at dt 0.02 (status 0) flies fdyn_lqr_step_f64 for 500 steps of
                0.02 s from 0.1 x lqr_numpy.PERTURBATION and ends closer to trim than it started
"""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import kf_numpy as kn
import lqr_numpy as ln
import margin_numpy as mn
import trim_numpy as tn
from hcrl_amd import _lib, layout as L
from hcrl_amd import lqr as Q
from hcrl_amd import margins as M
from hcrl_amd.fleet import BatchedSixDOF
from hcrl_amd.params import param_table

pytestmark = pytest.mark.gpu

SENTINEL = -12345.678
ISENT = -1234567
PAD = 96
DEV = "cuda"
FEEDBACKS = (mn.ESTIMATE, mn.TRUTH)
KEYS = ("alpha_s", "idx_s", "alpha_t", "idx_t", "curve", "status")


def _dev(a, dtype=None):
    t = torch.as_tensor(np.array(a, order="C"), device=DEV)
    return t if dtype is None else t.to(dtype)


def _padded(rows, n, dtype=torch.float64, fill=SENTINEL):
    return torch.full((rows * n + PAD,), fill, dtype=dtype, device=DEV)


def _margins(K, F, feedback, zre, zim, curve=True, n_omega=None, expect_rc=0):
    """K [n][16], F [n][80] (host) -> dict of host arrays shaped as margin_numpy.loop_margins shapes them; every output buffer has
    a sentinel pad behind it, asserted untouched."""
    n, W = len(K), len(zre) if n_omega is None else n_omega
    K_d, F_d, zr, zi = _dev(np.asarray(K).T), _dev(np.asarray(F).T), _dev(zre), _dev(zim)
    a_s, a_t = _padded(2, n), _padded(2, n)
    i_s, i_t, st = _padded(2, n, torch.int32, ISENT), _padded(2, n, torch.int32, ISENT), _padded(1, n, torch.int32, ISENT)
    cv = _padded(2 * max(W, 1), n)
    rc = _lib.load().fdyn_loop_margins(_lib.ptr(K_d), _lib.ptr(F_d), int(feedback), _lib.ptr(zr), _lib.ptr(zi), W, n, _lib.ptr(a_s), _lib.ptr(i_s),
                                       _lib.ptr(a_t), _lib.ptr(i_t), _lib.ptr(cv) if curve else None, _lib.ptr(st), _lib.current_stream())
    torch.cuda.synchronize()
    assert rc == expect_rc, rc
    if rc:
        for buf, sent in ((a_s, SENTINEL), (a_t, SENTINEL), (cv, SENTINEL), (i_s, ISENT), (i_t, ISENT), (st, ISENT)):
            assert bool((buf == sent).all()), "a refused launch wrote something"
        return None
    for buf, rows, sent in ((a_s, 2, SENTINEL), (a_t, 2, SENTINEL), (i_s, 2, ISENT), (i_t, 2, ISENT), (st, 1, ISENT), (cv, 2 * W if curve else 0, SENTINEL)):
        assert bool((buf[rows * n:] == sent).all()), "wrote behind an output buffer"
    two = lambda t: t[:2 * n].reshape(2, n).T.cpu().numpy()
    return dict(alpha_s=two(a_s), idx_s=two(i_s), alpha_t=two(a_t), idx_t=two(i_t), status=st[:n].cpu().numpy(),
                curve=cv[:2 * W * n].reshape(2, W, n).permute(2, 0, 1).cpu().numpy() if curve else None)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same(a, b, keys=KEYS):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in keys)


def _take(r, idx):
    return {k: (None if r[k] is None else r[k][idx]) for k in KEYS}


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "trim_reference.npz"))


@pytest.fixture(scope="module")
def designs(golden):
    return mn.golden_designs(golden)


@pytest.fixture(scope="module")
def grids():
    return {dt: mn.unit_circle(mn.default_omega(dt), dt) for dt in mn.DTS}


@pytest.fixture(scope="module")
def want(designs, grids):
    return {(dt, fb): mn.loop_margins(designs["K"], designs["F"][dt], fb, *grids[dt]) for dt in mn.DTS for fb in FEEDBACKS}


@pytest.fixture(scope="module")
def grid_est(designs, grids):
    """The 288 aircraft at dt 0.01 under estimate feedback in ONE launch: what the shape tests compare with."""
    return _margins(designs["K"], designs["F"][0.01], mn.ESTIMATE, *grids[0.01])


# ---- the kernel against the restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", mn.DTS)
@pytest.mark.parametrize("fb", FEEDBACKS)
def test_grid_is_bit_identical_to_the_restatement(designs, grids, want, dt, fb):
    got, ref = _margins(designs["K"], designs["F"][dt], fb, *grids[dt]), want[dt, fb]
    assert got["status"].shape == (288,) and not got["status"].any(), np.flatnonzero(got["status"])
    for k in ("curve", "alpha_s", "alpha_t"):
        diff = _bits(got[k]) != _bits(ref[k])
        ulp = np.abs(_bits(got[k]).astype(np.int64) - _bits(ref[k]).astype(np.int64)).max()
        print(f"dt {dt} feedback {fb}: {k}: {int(diff.sum())} of {diff.size} words differ from the restatement's, worst {int(ulp)} ulp")
    a = got["alpha_s"]
    print(f"dt {dt} feedback {fb}: alpha_s lon {a[:, 0].min():.4f}..{a[:, 0].max():.4f}, lat {a[:, 1].min():.4f}..{a[:, 1].max():.4f}")
    assert _same(got, ref)


@pytest.mark.parametrize("n", [1, 63, 65, 257])
def test_shapes_lane_position_and_no_curve(n, grid_est, designs, grids):
    idx = (np.arange(n) * 7 + 3) % 288
    K, F = designs["K"][idx], designs["F"][0.01][idx]
    got = _margins(K, F, mn.ESTIMATE, *grids[0.01])
    assert _same(got, _take(grid_est, idx)), "a lane's result depends on where it sits in the launch"
    bare = _margins(K, F, mn.ESTIMATE, *grids[0.01], curve=False)
    assert bare["curve"] is None and _same(bare, got, [k for k in KEYS if k != "curve"])


@pytest.mark.parametrize("n_omega", [1, 7, 64, 256])
def test_grid_sizes(n_omega, designs):
    idx = np.arange(0, 288, 9)
    omega = np.geomspace(1e-2, np.pi / 0.01, n_omega) if n_omega > 1 else np.array([np.pi / 0.01])
    omega[-1] = np.pi / 0.01
    zre, zim = mn.unit_circle(omega, 0.01)
    K, F = designs["K"][idx], designs["F"][0.01][idx]
    for fb in (mn.ESTIMATE, mn.MEASUREMENT):
        got = _margins(K, F, fb, zre, zim)
        assert got["curve"].shape == (len(idx), 2, n_omega) and not got["status"].any()
        assert _same(got, mn.loop_margins(K, F, fb, zre, zim))


@pytest.mark.parametrize("n_omega", [0, 257, -1])
def test_grid_sizes_outside_1_to_256_are_refused(n_omega, designs):
    z = np.full(300, 0.5)
    assert _margins(designs["K"][:5], designs["F"][0.01][:5], mn.ESTIMATE, z, z, n_omega=n_omega, expect_rc=_lib.FDYN_ERR_BAD_SIZE) is None


def test_measurement_feedback_is_truth_feedback_and_feedback_is_checked(designs, grids):
    K, F = designs["K"][:65], designs["F"][0.02][:65]
    assert _same(_margins(K, F, mn.MEASUREMENT, *grids[0.02]), _margins(K, F, mn.TRUTH, *grids[0.02]))
    assert _margins(K, F, 3, *grids[0.02], expect_rc=_lib.FDYN_ERR_BAD_SIZE) is None


@pytest.mark.parametrize("fb", FEEDBACKS)
def test_bad_lanes_and_their_neighbours(fb, designs):
    zre, zim = mn.unit_circle(mn.default_omega(0.01, 7), 0.01)
    keep = np.arange(0, 288, 4)                                          # 72 good aircraft, both airframes
    K, F, kind = [], [], []
    n_kinds = len(mn.bad_cases(designs["K"][0], designs["F"][0.01][0]))
    for j, i in enumerate(keep):
        K.append(designs["K"][i]); F.append(designs["F"][0.01][i]); kind.append(-1)
        if j % 3 == 2:
            c = (j // 3) % n_kinds
            _, k, f, _, _ = mn.bad_cases(designs["K"][i], designs["F"][0.01][i])[c]
            K.append(k); F.append(f); kind.append(c)
    K, F, kind = np.array(K), np.array(F), np.array(kind)
    assert all((kind == c).sum() >= 2 for c in range(n_kinds))
    mixed = _margins(K, F, fb, zre, zim)
    alone = _margins(designs["K"][keep], designs["F"][0.01][keep], fb, zre, zim)
    assert not alone["status"].any()
    assert _same(_take(mixed, kind < 0), alone), "a good lane changed because of its neighbour"
    ref = mn.loop_margins(K, F, fb, zre, zim)
    assert _same(mixed, ref)
    col = 3 if fb == mn.ESTIMATE else 4
    for c, case in enumerate(mn.bad_cases(designs["K"][0], designs["F"][0.01][0])):
        st = mixed["status"][kind == c]
        dead = (st & (mn.SINGULAR | mn.BAD_INPUT)) != 0
        if case[col] is None:
            assert ((st & mn.SINGULAR) != 0).all() and ((st & mn.BAD_INPUT) == 0).all(), (case[0], st)
        else:
            assert (st == case[col]).all(), (case[0], st)
        rows = _take(mixed, kind == c)
        assert np.isnan(rows["alpha_s"][dead]).all() and np.isnan(rows["alpha_t"][dead]).all() and np.isnan(rows["curve"][dead]).all()
        assert (rows["idx_s"][dead] == -1).all() and (rows["idx_t"][dead] == -1).all()
        assert np.isfinite(rows["alpha_s"][~dead]).all() and np.isfinite(rows["curve"][~dead]).all()
        if case[0] == "the pass-through filter":
            assert (st == mn.NOT_STABLE).all() and (rows["alpha_s"] == 1.0).all()


def test_graph_replay_equals_eager(designs, grids):
    K, F = _dev(designs["K"].T), _dev(designs["F"][0.02].T)
    zre, zim = (_dev(v) for v in grids[0.02])
    eager = M.margins_into(K, F, zre, zim, "estimate", curve=True)
    out = M.margins_into(K, F, zre, zim, "truth", curve=True)            # other values, then overwritten by the replay
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                                 # warm-up outside the capture
        M.margins_into(K, F, zre, zim, "truth", out)
    torch.cuda.current_stream().wait_stream(s)
    assert not torch.equal(out.alpha_s, eager.alpha_s)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        M.margins_into(K, F, zre, zim, "estimate", out)
    gr.replay()
    torch.cuda.synchronize()
    for a, b in ((eager.alpha_s, out.alpha_s), (eager.idx_s, out.idx_s), (eager.alpha_t, out.alpha_t), (eager.idx_t, out.idx_t),
                 (eager.status, out.status)):
        assert torch.equal(a, b)
    assert np.array_equal(_bits(eager.curve.cpu().numpy()), _bits(out.curve.cpu().numpy()))


# ---- the fleet -----------------------------------------------------------------------------------------------------------------
def test_fleet_chain_against_numpy_over_the_oracle():
    """trim -> design_lqr -> design_kalman -> loop_margins on the device against the same chain in NumPy over the CPU oracle (the
    ten aircraft of lqr_numpy.oracle_flights): alpha within 1e-9 relative."""
    base = ln.oracle_flights()["all"]
    n = len(base["type"])
    fleet = BatchedSixDOF(n, "f64", types=tn.TYPES, type_index=base["type"])
    with pytest.raises(ValueError, match="no certified stabilising gain"):
        fleet.loop_margins()
    fleet.trim(base["spec"][:, 0], base["spec"][:, 1], base["spec"][:, 2], ln.ALTITUDE, ln.HEADING)
    lqr = fleet.design_lqr()
    with pytest.raises(ValueError, match="no certified stable filter"):
        fleet.loop_margins()
    for dt in mn.DTS:
        kal = fleet.design_kalman(dt)
        F_ref = kn.design_many(base["A"], base["B"], dt, kn.default_noise())["F"]
        omega = mn.default_omega(dt)
        for name, fb in (("estimate", mn.ESTIMATE), ("truth", mn.TRUTH)):
            m = fleet.loop_margins(name, curve=True)
            ref = mn.loop_margins(base["K"], F_ref, fb, *mn.unit_circle(omega, dt))
            own = mn.loop_margins(lqr.K.T.cpu().numpy(), kal.F.T.cpu().numpy(), fb, *mn.unit_circle(omega, dt))
            assert bool(m.ok.all()) and not ref["status"].any() and m.dt == dt and m.feedback == fb
            assert np.array_equal(_bits(m.alpha_s.T.cpu().numpy()), _bits(own["alpha_s"])) and np.array_equal(m.idx_s.T.cpu().numpy(), own["idx_s"])
            err_s = np.abs(m.alpha_s.T.cpu().numpy() / ref["alpha_s"] - 1.0).max()
            err_t = np.abs(m.alpha_t.T.cpu().numpy() / ref["alpha_t"] - 1.0).max()
            print(f"dt {dt} {name}: alpha_s {float(m.alpha_s.min()):.4f}..{float(m.alpha_s.max()):.4f}; fleet chain against NumPy over the "
                  f"oracle: alpha_s {err_s:.3e}, alpha_t {err_t:.3e}")
            assert err_s <= 1e-9 and err_t <= 1e-9
            assert np.array_equal(m.omega_s.cpu().numpy(), omega[m.idx_s.cpu().numpy()]) and np.array_equal(m.omega.cpu().numpy(), M.default_grid(dt))
            low, high = m.gain_margin()
            assert bool((low < 1.0).all()) and bool((high > 1.0).all()) and bool((m.phase_margin_deg() > 0.0).all())
            assert tuple(m.curve.shape) == (2, 64, n)
    few = fleet.loop_margins("estimate", omega=[1.0, 10.0, 100.0])
    assert few.curve is None and int(few.idx_s.max()) <= 2 and bool(few.ok.all())


def test_the_least_robust_certified_loop_flies_stably(golden, designs, want):
    """The golden aircraft with the smallest lateral alpha_s at dt 0.02 under state feedback, K as designed, status 0: flown by
    fdyn_lqr_step_f64 for 500 steps of 0.02 s from a tenth of lqr_numpy.PERTURBATION it ends closer to trim than it started."""
    dt = 0.02
    ref = want[dt, mn.TRUTH]
    i = int(np.argmin(ref["alpha_s"][:, 1]))
    assert ref["status"][i] == 0
    name = tn.TYPES[int(golden["type"][i])]
    fleet = BatchedSixDOF(1, "f64", types=(name,))
    fleet.params = _dev(tn.scaled_block(param_table((name,))[0], golden["scales"][i], L)[None])       # the golden grid scales the mass
    x0, u0 = golden["x0"][i], golden["u0"][i]
    x = np.array(x0, np.float64)
    for k, v in ln.PERTURBATION.items():
        x[k] += 0.1 * v
    fleet.reset(x[None])
    zi, zd = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.float64, device=DEV)
    lqr = Q.LqrDesign(_dev(designs["K"][i:i + 1].T), zd, zi, zi.clone(), _dev(x0[None].T), _dev(u0[None].T))
    got = _margins(designs["K"][i:i + 1], designs["F"][dt][i:i + 1], mn.TRUTH, *mn.unit_circle(mn.default_omega(dt), dt))
    assert got["status"][0] == 0 and got["alpha_s"][0, 1] == ref["alpha_s"][i, 1]
    start = ln.deviation(x, x0)
    fleet.step_lqr(lqr, 500, dt)
    torch.cuda.synchronize()
    end = ln.deviation(fleet.state_numpy()[0], x0)
    print(f"aircraft {i} ({name}): lateral alpha_s {ref['alpha_s'][i, 1]:.4f} at dt {dt}; deviation {start:.4f} -> {end:.6f} after 500 steps")
    assert np.isfinite(end) and end < start

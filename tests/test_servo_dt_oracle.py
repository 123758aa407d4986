"""The sampled-data servo design (include/fdyn_servo_dt.h) on the CPU: the NumPy restatement (tests/servo_dt_numpy.py) on the 288
linearisations of tests/golden/trim_reference.npz at dt 0.01 and 0.02, against

  * an independent answer recorded in tests/golden/servo_dt_reference.npz: K from scipy.linalg.expm and
    scipy.linalg.solve_discrete_are (tests/golden/make_golden_servo_dt.py; no scipy is needed here);
  * the loop margins of the loop as it is flown (servo_margin_numpy.loop_margins, default 64-point grid, the Phi and Gamma of
    servo_lqg_numpy's golden filter designs at that dt), beside the continuous design's (servo_numpy.golden_designs).

Gates, none taken from what a kernel returns:
  K against scipy      measured 1.26e-12 of max(1, |K|) at dt 0.01 (7.4e-13 at dt 0.02); gate ten times that, rounded up to one
                       digit: 2e-11
  certificate          status 0, at most RIC_MAX_ITERS doubling steps, residual <= 1e-10 on all 288 at both dt
  (a) stability        every status-0 sampled design has FD_MRG_NOT_STABLE clear under truth feedback: the certificate of the design
                       and of the margins is the same matrix
  (b) per aircraft     alpha_s(sampled) / alpha_s(continuous) > 1 on every aircraft and both blocks under truth feedback.  Measured
                       worst ratio 1.00471 at dt 0.01 and 1.01988 at dt 0.02, above 1 on all; gate = the geometric mean of that worst
                       ratio and 1: 1.00235 and 1.00989
  (c) fleet worst      alpha_s of the least robust aircraft at dt 0.02, truth feedback: continuous 0.0710, sampled 0.5862; gate =
                       their geometric mean, 0.2040
Under estimate feedback the same table is printed and not gated (nobody had measured it), and so is |K_dt - K| / |K| for dt -> 0.
"""
import os

import numpy as np
import pytest

import servo_dt_numpy as sd
import servo_lqg_numpy as sl
import servo_margin_numpy as sm
import servo_numpy as sn
from conftest import GOLDEN

SCIPY_MEASURED = 1.26e-12                                        # worst |K - K_scipy| / max(1, |K_scipy|) over both dt
SCIPY_GATE = 2e-11                                               # ten times that, rounded up to one digit
ratio_gate, worst_gate = sd.ratio_gate, sd.worst_gate            # the margin gates (b) and (c), shared with the device test


def _tag(dt):
    return f"dt{dt:g}".replace(".", "p")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "trim_reference.npz"))


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "servo_dt_reference.npz"))


@pytest.fixture(scope="module")
def margins(golden, fixture):
    """{(dt, feedback): (continuous, sampled)} of servo_margin_numpy.loop_margins on the restatement's recorded gains."""
    cont = sn.golden_designs(golden)
    assert not cont["status"].any()
    x0 = np.array(golden["x0"], np.float64)
    out = {}
    for dt in sd.DTS:
        F = sl.golden_designs(golden, dt)["F"]
        zre, zim = sm.unit_circle(sm.default_omega(dt), dt)
        for fb in (sm.TRUTH, sm.ESTIMATE):
            out[dt, fb] = tuple(sm.loop_margins(K, F, x0, dt, fb, zre, zim) for K in (cont["K"], fixture[f"{_tag(dt)}_K"]))
    return out


@pytest.mark.parametrize("dt", sd.DTS)
def test_restatement_is_certified_and_equals_scipy(dt, golden, fixture):
    got = sd.golden_designs(golden, dt)
    assert len(got["status"]) == 288 and not got["status"].any(), np.flatnonzero(got["status"])
    assert got["iters"].max() <= sn.MAX_ITERS and got["residual"].max() <= 1e-10
    t = _tag(dt)
    # the fixture holds what this restatement writes: a stale file would make the device test compare against something else
    assert np.array_equal(got["K"], fixture[f"{t}_K"]) and np.array_equal(got["iters"], fixture[f"{t}_iters"])
    assert np.array_equal(got["status"], fixture[f"{t}_status"]) and np.array_equal(got["residual"], fixture[f"{t}_residual"])
    ks = fixture[f"{t}_K_scipy"]
    dev = np.abs(got["K"] - ks) / np.maximum(1.0, np.abs(ks))
    print(f"dt {dt}: doubling steps {got['iters'].min()}..{got['iters'].max()}, residual <= {got['residual'].max():.2e}, "
          f"|K - K_scipy| / max(1, |K_scipy|) <= {dev.max():.2e} (gate {SCIPY_GATE:.0e})")
    assert dev.max() <= SCIPY_GATE
    assert np.abs(got["K"] - sn.golden_designs(golden)["K"]).max() > 1e-2          # and it is not the continuous gain


@pytest.mark.parametrize("dt", sd.DTS)
def test_sampled_design_widens_every_margin_of_the_flown_loop(dt, margins, fixture):
    cont, samp = margins[dt, sm.TRUTH]
    assert not (samp["status"][fixture[f"{_tag(dt)}_status"] == 0] & sm.NOT_STABLE).any()          # (a)
    assert not samp["status"].any() and not cont["status"].any()
    worst_ratio, worst_c, worst_s = sd.margin_gates(cont["alpha_s"], samp["alpha_s"])
    for blk, name in enumerate(("lon", "lat")):
        print(f"dt {dt} truth {name}: alpha_s continuous {cont['alpha_s'][:, blk].min():.4f} .. {cont['alpha_s'][:, blk].max():.4f}, sampled "
              f"{samp['alpha_s'][:, blk].min():.4f} .. {samp['alpha_s'][:, blk].max():.4f}, worst per-aircraft ratio {worst_ratio[blk]:.5f}")
    print(f"dt {dt} truth: gate on the ratio {ratio_gate(dt):.5f}; certificate squarings at most {samp['squarings'].max()}")
    assert worst_ratio.min() > 1.0 and worst_ratio.min() >= ratio_gate(dt)                          # (b)
    if dt == 0.02:                                                                                  # (c)
        print(f"dt 0.02 truth: fleet-worst alpha_s continuous {worst_c:.4f}, sampled {worst_s:.4f}, gate {worst_gate():.4f}")
        assert worst_s >= worst_gate()
        # the continuous design's minimum sits at the Nyquist point, the last of the grid, on every aircraft: the hold eats the margin
        assert (cont["idx_s"] == cont["curve"].shape[2] - 1).all()


def test_estimate_feedback_table_is_reported(margins):
    """No gate: the table under estimate feedback, printed for DESIGN 7t.  Only that the numbers exist is asserted."""
    for dt in sd.DTS:
        cont, samp = margins[dt, sm.ESTIMATE]
        ratio = samp["alpha_s"] / cont["alpha_s"]
        for blk, name in enumerate(("lon", "lat")):
            print(f"dt {dt} estimate {name}: alpha_s continuous {cont['alpha_s'][:, blk].min():.4f} .. {cont['alpha_s'][:, blk].max():.4f}, sampled "
                  f"{samp['alpha_s'][:, blk].min():.4f} .. {samp['alpha_s'][:, blk].max():.4f}, worst per-aircraft ratio {ratio[:, blk].min():.5f}")
        assert np.isfinite(samp["alpha_s"]).all() and np.isfinite(cont["alpha_s"]).all()


def test_approach_to_the_continuous_gain_is_reported(golden):
    """No gate: |K_dt - K| / |K| (Euclidean, all 26 words) over 24 of the aircraft at dt 0.02, 0.01 and 0.005, printed for DESIGN 7t.
    Asserted only: every design is certified and the distance shrinks with dt."""
    cont, w = sn.golden_designs(golden), sn.default_weights()
    worst = []
    for dt in (0.02, 0.01, 0.005):
        rel = []
        for i in range(0, 288, 12):
            d = sd.design(golden["A"][i], golden["B"][i], golden["x0"][i], w, dt)
            assert d["status"] == 0, (dt, i, d["status"])
            rel.append(np.linalg.norm(d["K"] - cont["K"][i]) / np.linalg.norm(cont["K"][i]))
        worst.append(max(rel))
        print(f"dt {dt}: worst |K_dt - K| / |K| over 24 aircraft {worst[-1]:.3f}")
    assert worst[0] > worst[1] > worst[2]


def test_refused_lanes(golden):
    """What fdyn_servo_design refuses, and the series cap of the discretisation, per lane: BAD_INPUT, K = 0, NaN residual."""
    i, w = 40, sn.default_weights()
    A, B, x0 = golden["A"][i], golden["B"][i], golden["x0"][i]
    assert sd.design(A, B, x0, w, 0.02)["status"] == 0
    bad_w, bad_a, bad_b, still = w.copy(), A.copy(), B.copy(), x0.copy()
    bad_w[16], bad_a[sn.LAT_STATES[1], sn.LAT_STATES[2]], bad_b[sn.LON_STATES[0], 3] = -1.0, np.nan, np.inf
    still[sn.X_U] = still[sn.X_W] = 0.0
    norm = max(sl.row_norm(a) for a, _ in sl.blocks(A, B))
    over = 1.01 * sl.NORM_MAX / norm                                  # just past |a|_inf dt = 1.5
    for name, args in (("a negative weight", (A, B, x0, bad_w, 0.02)), ("a NaN word of A", (bad_a, B, x0, w, 0.02)),
                       ("an infinite word of B", (A, bad_b, x0, w, 0.02)), ("V0 = 0", (A, B, still, w, 0.02)),
                       ("dt past the series cap", (A, B, x0, w, over)), ("dt = 0", (A, B, x0, w, 0.0)), ("dt = 2", (A, B, x0, w, 2.0))):
        d = sd.design(*args)
        assert d["status"] == sd.BAD_INPUT and not d["K"].any() and np.isnan(d["residual"]) and d["iters"] == 0, name
    assert sd.design(A, B, x0, w, 0.98 * sl.NORM_MAX / norm)["status"] == 0       # and just inside it the lane is designed

"""The servo's loop margins, CPU side: the NumPy restatement of fdyn_servo_loop_margins (tests/servo_margin_numpy.py) against an
independent reference -- np.linalg.solve on the AUGMENTED complex system, where the integrators are states and not a factor
1 / (z - 1), and np.linalg.svd -- on the 288 linearisations of tests/golden/trim_reference.npz (both blocks, dt = 0.01 and 0.02,
estimate and truth feedback: 2304 cases, the default 64-point grid), the disk guarantee as a theorem test, loop recovery, and the
status bits.

Gates (none derived from what the code under test returns):
  curve, alpha_s, alpha_t   1e-9 relative against the reference, the gate of the regulators' margins
                            (measured: curve 8.5e-12, alpha_s 2.5e-14, alpha_t 6.9e-15)
  idx_s, idx_t              the reference's argmin, or the restatement's value at the reference's index within 1e-9 of its own minimum
  status                    0 on all 2304 cases; at most 30 squarings (measured 8..10)
  disk guarantee            every corner pair of channel gains g in {1 / (1 + 0.9 alpha_s), 1 / (1 - 0.9 alpha_s)}^2 leaves the perturbed
                            closed loop (plant + integrators under truth; plant + estimate + integrators under estimate, the estimator
                            fed the controller's own unperturbed du) with spectral radius < 1 under np.linalg.eigvals: 0 unstable of
                            4608 at each dt (measured worst radius 0.99817 at dt 0.01, 0.99609 at 0.02).  The factor 0.9 leaves room
                            for the grid's finite resolution: a condition, not a tolerance
  recovery                  aircraft 0, dt 0.01, process-noise rates x 1e4: |alpha_s(estimate) - alpha_s(truth)| <= 3e-8, ten times the
                            measured gap rounded up to one digit (measured 2.6e-9 longitudinal, 2.9e-9 lateral); with the default
                            noise the gap is above 1e-3 (measured 2.0e-2 and 5.4e-3)
"""
import os

import numpy as np
import pytest

from conftest import GOLDEN
import servo_lqg_numpy as sl
import servo_margin_numpy as sm

FEEDBACKS = (sm.ESTIMATE, sm.TRUTH)
RECOVERY_GATE = 3e-8


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "trim_reference.npz"))


@pytest.fixture(scope="module")
def designs(golden):
    return sm.golden_designs(golden)


@pytest.fixture(scope="module")
def restated(designs):
    """{(dt, feedback): servo_margin_numpy.loop_margins of the 288 aircraft on the default grid}"""
    out = {}
    for dt in sm.DTS:
        zre, zim = sm.unit_circle(sm.default_omega(dt), dt)
        for fb in FEEDBACKS:
            out[dt, fb] = sm.loop_margins(designs["K"], designs["F"][dt], designs["x0"], dt, fb, zre, zim)
    return out


@pytest.mark.parametrize("dt", sm.DTS)
def test_restatement_matches_the_reference_on_the_golden_grid(designs, restated, dt):
    omega = sm.default_omega(dt)
    zre, zim = sm.unit_circle(omega, dt)
    assert (zre[-1], zim[-1]) == (-1.0, 0.0)
    z = zre + 1j * zim
    rows = np.arange(288)
    for fb in FEEDBACKS:
        got = restated[dt, fb]
        assert got["status"].shape == (288,) and not got["status"].any(), np.flatnonzero(got["status"])
        assert got["squarings"].max() <= sm.MAX_SQUARINGS
        worst = dict(curve=0.0, alpha_s=0.0, alpha_t=0.0)
        for blk in range(2):
            s_ref, t_ref = sm.reference(designs["K"], designs["F"][dt], designs["x0"], dt, blk, fb == sm.ESTIMATE, z)
            worst["curve"] = max(worst["curve"], np.abs(got["curve"][:, blk] / s_ref - 1.0).max())
            worst["alpha_s"] = max(worst["alpha_s"], np.abs(got["alpha_s"][:, blk] / s_ref.min(axis=1) - 1.0).max())
            worst["alpha_t"] = max(worst["alpha_t"], np.abs(got["alpha_t"][:, blk] / t_ref.min(axis=1) - 1.0).max())
            # the index: the reference's argmin, or the restatement's own value at the reference's index within 1e-9 of its own minimum
            for idx, ref, own, alpha in ((got["idx_s"][:, blk], s_ref, got["curve"][:, blk], got["alpha_s"][:, blk]),
                                         (got["idx_t"][:, blk], t_ref, got["curve_t"][:, blk], got["alpha_t"][:, blk])):
                at = ref.argmin(axis=1)
                assert (idx >= 0).all() and (idx < 64).all() and np.array_equal(own[rows, idx], alpha)
                tie = np.abs(own[rows, at] / alpha - 1.0) <= 1e-9
                assert ((idx == at) | tie).all(), (dt, fb, blk, np.flatnonzero(~((idx == at) | tie)))
            # alpha_s is the curve's own minimum, first index
            assert np.array_equal(got["alpha_s"][:, blk], got["curve"][:, blk].min(axis=1))
            assert np.array_equal(got["idx_s"][:, blk], got["curve"][:, blk].argmin(axis=1))
        a = got["alpha_s"]
        print(f"dt {dt} feedback {fb}: alpha_s lon {a[:, 0].min():.4f} / {np.median(a[:, 0]):.4f} / {a[:, 0].max():.4f}, "
              f"lat {a[:, 1].min():.4f} / {np.median(a[:, 1]):.4f} / {a[:, 1].max():.4f}; minimum at the Nyquist point on "
              f"{int((got['idx_s'] == 63).all(axis=1).sum())} of 288; squarings {got['squarings'].min()}..{got['squarings'].max()}; "
              "against the reference: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
        assert max(worst.values()) <= 1e-9, worst


@pytest.mark.parametrize("dt", sm.DTS)
def test_the_disk_guarantee_holds_at_every_corner(designs, restated, dt):
    """With alpha_s >= a, gains of both channels inside [1 / (1 + a), 1 / (1 - a)] keep the loop stable: checked at the four
    corners of that square for a = 0.9 alpha_s on every case, by eigenvalues of the perturbed closed loop."""
    unstable, total, worst = 0, 0, 0.0
    for fb in FEEDBACKS:
        got = restated[dt, fb]
        for blk in range(2):
            for i in range(288):
                a = 0.9 * got["alpha_s"][i, blk]
                assert 0.0 < a < 1.0
                for g0 in (1.0 / (1.0 + a), 1.0 / (1.0 - a)):
                    for g1 in (1.0 / (1.0 + a), 1.0 / (1.0 - a)):
                        m = sm.perturbed_loop(designs["K"][i], designs["F"][dt][i], designs["x0"][i], dt, blk, fb == sm.ESTIMATE, (g0, g1))
                        rho = np.abs(np.linalg.eigvals(m)).max()
                        worst, total, unstable = max(worst, rho), total + 1, unstable + (not rho < 1.0)
    print(f"dt {dt}: {unstable} unstable of {total} perturbed loops, worst spectral radius {worst:.5f}")
    assert total == 4608 and unstable == 0


def test_the_perturbed_loop_at_unit_gains_is_the_certified_matrix(designs):
    """perturbed_loop is written independently of the restatement: at g = (1, 1) its truth form is the augmented matrix the
    certificate squares, and its estimate form has the eigenvalues of that matrix together with those of (I - L) Phi (separation)."""
    dt, i = 0.02, 97
    K, F, x0 = designs["K"][i:i + 1], designs["F"][dt][i:i + 1], designs["x0"][i:i + 1]
    for blk, size in ((0, 7), (1, 6)):
        b = sm.block_matrices(K, F, x0, dt, blk, True)
        d = sm.block_setup(b)
        aug = d["aug"][:size, :size, 0]
        np.testing.assert_allclose(sm.perturbed_loop(K[0], F[0], x0[0], dt, blk, False, (1.0, 1.0)), aug, rtol=0, atol=1e-15)
        full = np.linalg.eigvals(sm.perturbed_loop(K[0], F[0], x0[0], dt, blk, True, (1.0, 1.0)))
        parts = np.concatenate([np.linalg.eigvals(aug), np.linalg.eigvals(d["A1"][:, :, 0])])
        for p in parts:
            assert np.abs(full - p).min() < 1e-7, (blk, p)


def test_loop_recovery(golden, designs):
    """Process-noise rates x 1e4 drive L to I (every state is measured): the estimate loop's alpha_s returns to the sampled servo's."""
    dt = 0.01
    nz = sl.default_noise()
    nz[sl.NSKX:] *= 1.0e4
    kf = sl.design(golden["A"][0], golden["B"][0], dt, nz)
    assert kf["status"] == 0
    zre, zim = sm.unit_circle(sm.default_omega(dt), dt)
    K, x0 = designs["K"][:1], designs["x0"][:1]
    est = sm.loop_margins(K, kf["F"][None], x0, dt, sm.ESTIMATE, zre, zim)
    tru = sm.loop_margins(K, kf["F"][None], x0, dt, sm.TRUTH, zre, zim)
    nominal = sm.loop_margins(K, designs["F"][dt][:1], x0, dt, sm.ESTIMATE, zre, zim)
    gap = np.abs(est["alpha_s"][0] - tru["alpha_s"][0])
    gap0 = np.abs(nominal["alpha_s"][0] - tru["alpha_s"][0])
    print(f"alpha_s estimate {est['alpha_s'][0]}, truth {tru['alpha_s'][0]}, gap {gap}; default noise: {nominal['alpha_s'][0]}, gap {gap0}")
    assert est["status"][0] == 0 and tru["status"][0] == 0 and nominal["status"][0] == 0
    assert (gap <= RECOVERY_GATE).all()
    assert (gap0 > 1e-3).all()                                           # with the default noise the two loops differ, orders more


def test_status_bits(designs):
    zre, zim = sm.unit_circle(sm.default_omega(0.01, 7), 0.01)
    assert (zre[-1], zim[-1]) == (-1.0, 0.0)
    K, F, x0 = designs["K"][0], designs["F"][0.01][0], designs["x0"][0]
    for fb, col in ((sm.ESTIMATE, 5), (sm.TRUTH, 6), (sm.MEASUREMENT, 6)):
        good = sm.loop_margins(K[None], F[None], x0[None], 0.01, fb, zre, zim)
        assert good["status"][0] == 0 and np.isfinite(good["curve"]).all()
        names = set()
        for case in sm.bad_cases(K, F, x0):
            name, k, f, x, dt, want = case[0], case[1], case[2], case[3], case[4], case[col]
            names.add(name)
            r = sm.loop_margins(k[None], f[None], x[None], dt, fb, zre, zim)
            st = int(r["status"][0])
            assert st == want, (name, fb, st)
            if st & (sm.SINGULAR | sm.BAD_INPUT):
                assert np.isnan(r["alpha_s"]).all() and np.isnan(r["alpha_t"]).all() and np.isnan(r["curve"]).all(), name
                assert (r["idx_s"] == -1).all() and (r["idx_t"] == -1).all(), name
            else:
                assert np.isfinite(r["alpha_s"]).all() and np.isfinite(r["curve"]).all(), name
            if st == 0:                                                   # the poisoned words were not read: the good lane's result
                assert all(np.array_equal(r[key], good[key]) for key in ("alpha_s", "alpha_t", "idx_s", "idx_t", "curve")), name
            if name == "the pass-through filter":
                # Phi = I, Gamma = 0: G = 0 and L_i = 0 at every z != 1, so sigma_min(I + L_i) = 1 and 1 / sigma_max(T) = +inf on the
                # whole grid (first index); the integrators are then undamped (unit eigenvalues): never certified
                assert st == sm.NOT_STABLE and (r["alpha_s"] == 1.0).all() and (r["curve"] == 1.0).all() and (r["idx_s"] == 0).all()
                assert np.isposinf(r["alpha_t"]).all() and (r["idx_t"] == 0).all()
            if name.startswith("Kb -> -0.5 Kb"):
                assert np.abs(np.linalg.eigvals(sm.perturbed_loop(k, f, x, dt, 0, False, (1.0, 1.0)))).max() > 1.0
        assert len(names) == 13
        # a grid point at z = 1: 1 / (z - 1) is not a number, by construction
        one = sm.loop_margins(K[None], F[None], x0[None], 0.01, fb, *sm.grid_with_one())
        assert one["status"][0] == sm.SINGULAR and np.isnan(one["alpha_s"]).all() and np.isnan(one["curve"]).all() and (one["idx_s"] == -1).all()
    # the squaring certificate by itself: a contraction, a slow contraction, a rotation (never certified: the cap), an expansion, a NaN
    rot = np.eye(7)
    rot[:2, :2] = [[0.0, -1.0], [1.0, 0.0]]
    nan = 0.5 * np.eye(7)
    nan[1, 2] = np.nan
    m = np.stack([0.5 * np.eye(7), 0.999 * np.eye(7) + 0.01 * np.eye(7, k=1), rot, 1.5 * np.eye(7), nan], axis=-1)
    with np.errstate(all="ignore"):
        ok, sq = sm.schur_by_squaring(m)
    assert ok.tolist() == [True, True, False, False, False] and sq[0] == 0 and 1 <= sq[1] < sm.MAX_SQUARINGS and sq[2] == sm.MAX_SQUARINGS


def test_measurement_feedback_equals_truth_feedback_to_the_bit(designs):
    for dt in sm.DTS:
        zre, zim = sm.unit_circle(sm.default_omega(dt), dt)
        idx = np.arange(0, 288, 7)
        a = sm.loop_margins(designs["K"][idx], designs["F"][dt][idx], designs["x0"][idx], dt, sm.MEASUREMENT, zre, zim)
        b = sm.loop_margins(designs["K"][idx], designs["F"][dt][idx], designs["x0"][idx], dt, sm.TRUTH, zre, zim)
        for key in ("alpha_s", "alpha_t", "curve", "curve_t"):
            assert np.array_equal(a[key].view(np.uint64), b[key].view(np.uint64)), key
        for key in ("idx_s", "idx_t", "status"):
            assert np.array_equal(a[key], b[key]), key

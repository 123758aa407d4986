"""Loop margins, CPU side: the NumPy restatement of fdyn_loop_margins (tests/margin_numpy.py) against an independent reference --
np.linalg.solve on complex matrices and np.linalg.svd -- on the 288 linearisations of tests/golden/trim_reference.npz (both blocks,
dt = 0.01 and 0.02, estimate and truth feedback: 2304 cases, the default 64-point grid), the disk guarantee as a theorem test, loop
recovery, the status bits, and the host logic of hcrl_amd.margins that needs no device.

Gates (none derived from what the code under test returns):
  curve, alpha_s, alpha_t   1e-9 relative against the reference, the project's gate for design quantities
                            (measured: curve 1.4e-13, alpha_s 1.5e-14, alpha_t 4.2e-15)
  idx_s, idx_t              the reference's argmin, or the restatement's value at the reference's index within 1e-9 of its own minimum
  status                    0 on all 2304 cases; at most 9 squarings (measured 5..9)
  disk guarantee            every corner pair of channel gains g in {1 / (1 + 0.9 alpha_s), 1 / (1 - 0.9 alpha_s)}^2 leaves the perturbed
                            closed loop (4 x 4 under truth, 8 x 8 plant + estimator under estimate) with spectral radius < 1 under
                            np.linalg.eigvals: 0 unstable of 4608 at each dt (measured worst radius 0.99456 at dt 0.01, 0.98914 at 0.02).
                            The factor 0.9 leaves room for the grid's finite resolution: a condition, not a tolerance
  recovery                  aircraft 0, dt 0.01, process-noise rates x 1e4: |alpha_s(estimate) - alpha_s(truth)| <= 1e-6
                            (measured 2.6e-8 longitudinal, 1.5e-8 lateral)
"""
import math
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import kf_numpy as kn
import margin_numpy as mn
from hcrl_amd import layout as L
from hcrl_amd import margins as M

FEEDBACKS = (mn.ESTIMATE, mn.TRUTH)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "trim_reference.npz"))


@pytest.fixture(scope="module")
def designs(golden):
    return mn.golden_designs(golden)


@pytest.fixture(scope="module")
def restated(designs):
    """{(dt, feedback): margin_numpy.loop_margins of the 288 aircraft on the default grid}"""
    out = {}
    for dt in mn.DTS:
        zre, zim = mn.unit_circle(mn.default_omega(dt), dt)
        for fb in FEEDBACKS:
            out[dt, fb] = mn.loop_margins(designs["K"], designs["F"][dt], fb, zre, zim)
    return out


def _blocks(designs, dt, blk):
    """-> (Phi [n][4][4], Gamma [n][4][2], Kb [n][2][4], Lk [n][4][4]) of one block as stacks of matrices."""
    return tuple(np.moveaxis(m, -1, 0) for m in mn.block_matrices(designs["K"], designs["F"][dt], blk, True))


def test_constants_mirror_the_header():
    assert (mn.NOT_STABLE, mn.SINGULAR, mn.BAD_INPUT) == (L.FD_MRG_NOT_STABLE, L.FD_MRG_SINGULAR, L.FD_MRG_BAD_INPUT) == (1, 2, 4)
    assert (mn.ESTIMATE, mn.MEASUREMENT, mn.TRUTH) == (L.FD_LQG_ESTIMATE, L.FD_LQG_MEASUREMENT, L.FD_LQG_TRUTH)
    assert mn.PHI == (L.FD_KF_PHI_LON, L.FD_KF_PHI_LAT) and mn.GAMMA == (L.FD_KF_GAMMA_LON, L.FD_KF_GAMMA_LAT)
    assert mn.LG == (L.FD_KF_L_LON, L.FD_KF_L_LAT) and mn.MAX_OMEGA == M.MAX_OMEGA == 256
    assert np.array_equal(mn.pass_through_filter(), kn.pass_through())
    from hcrl_amd import _lib
    assert "fdyn_loop_margins" in _lib.SIGNATURES


@pytest.mark.parametrize("dt", mn.DTS)
def test_restatement_matches_the_reference_on_the_golden_grid(designs, restated, dt):
    omega = mn.default_omega(dt)
    zre, zim = mn.unit_circle(omega, dt)
    assert (zre[-1], zim[-1]) == (-1.0, 0.0)
    z = zre + 1j * zim
    for fb in FEEDBACKS:
        got = restated[dt, fb]
        assert got["status"].shape == (288,) and not got["status"].any(), np.flatnonzero(got["status"])
        assert got["squarings"].max() <= 9
        worst = dict(curve=0.0, alpha_s=0.0, alpha_t=0.0)
        for blk in range(2):
            s_ref, t_ref = mn.reference(*_blocks(designs, dt, blk), fb == mn.ESTIMATE, z)
            worst["curve"] = max(worst["curve"], np.abs(got["curve"][:, blk] / s_ref - 1.0).max())
            worst["alpha_s"] = max(worst["alpha_s"], np.abs(got["alpha_s"][:, blk] / s_ref.min(axis=1) - 1.0).max())
            worst["alpha_t"] = max(worst["alpha_t"], np.abs(got["alpha_t"][:, blk] / t_ref.min(axis=1) - 1.0).max())
            # the index: the reference's argmin, or the restatement's own value at the reference's index within 1e-9 of its own minimum
            rows = np.arange(288)
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
        print(f"dt {dt} feedback {fb}: alpha_s lon {a[:, 0].min():.4f}..{a[:, 0].max():.4f}, lat {a[:, 1].min():.4f}..{a[:, 1].max():.4f}; "
              f"squarings {got['squarings'].min()}..{got['squarings'].max()}; against the reference: "
              + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
        assert max(worst.values()) <= 1e-9, worst


@pytest.mark.parametrize("dt", mn.DTS)
def test_the_disk_guarantee_holds_at_every_corner(designs, restated, dt):
    """With alpha_s >= a, gains of both channels inside [1 / (1 + a), 1 / (1 - a)] keep the loop stable: checked at the four
    corners of that square for a = 0.9 alpha_s on every case, by eigenvalues of the perturbed closed loop."""
    unstable, total, worst = 0, 0, 0.0
    for fb in FEEDBACKS:
        got = restated[dt, fb]
        for blk in range(2):
            Phi, Gamma, Kb, Lk = _blocks(designs, dt, blk)
            for i in range(288):
                a = 0.9 * got["alpha_s"][i, blk]
                assert 0.0 < a < 1.0
                for g0 in (1.0 / (1.0 + a), 1.0 / (1.0 - a)):
                    for g1 in (1.0 / (1.0 + a), 1.0 / (1.0 - a)):
                        m = mn.perturbed_loop(Phi[i], Gamma[i], Kb[i], Lk[i], fb == mn.ESTIMATE, (g0, g1))
                        rho = np.abs(np.linalg.eigvals(m)).max()
                        worst, total, unstable = max(worst, rho), total + 1, unstable + (not rho < 1.0)
    print(f"dt {dt}: {unstable} unstable of {total} perturbed loops, worst spectral radius {worst:.5f}")
    assert total == 4608 and unstable == 0


def test_loop_recovery(golden, designs):
    """Process-noise rates x 1e4 drive L_kf to I (every state is measured): the LQG loop's alpha_s returns to the sampled LQR's."""
    dt = 0.01
    nz = kn.default_noise()
    nz[8:] *= 1.0e4
    kf = kn.design(golden["A"][0], golden["B"][0], dt, nz)
    assert kf["status"] == 0
    zre, zim = mn.unit_circle(mn.default_omega(dt), dt)
    est = mn.loop_margins(designs["K"][:1], kf["F"][None], mn.ESTIMATE, zre, zim)
    tru = mn.loop_margins(designs["K"][:1], kf["F"][None], mn.TRUTH, zre, zim)
    nominal = mn.loop_margins(designs["K"][:1], designs["F"][dt][:1], mn.ESTIMATE, zre, zim)
    gap = np.abs(est["alpha_s"][0] - tru["alpha_s"][0])
    print(f"alpha_s estimate {est['alpha_s'][0]}, truth {tru['alpha_s'][0]}, gap {gap}; default noise: {nominal['alpha_s'][0]}")
    assert est["status"][0] == 0 and tru["status"][0] == 0
    assert (gap <= 1e-6).all()
    assert (np.abs(nominal["alpha_s"][0] - tru["alpha_s"][0]) > 1e-3).any()        # with the default noise the two loops differ


def test_status_bits(designs):
    zre, zim = mn.unit_circle(mn.default_omega(0.01, 7), 0.01)
    assert (zre[-1], zim[-1]) == (-1.0, 0.0)
    K, F = designs["K"][0], designs["F"][0.01][0]
    for fb, col in ((mn.ESTIMATE, 3), (mn.TRUTH, 4)):
        good = mn.loop_margins(K[None], F[None], fb, zre, zim)
        assert good["status"][0] == 0 and np.isfinite(good["curve"]).all()
        for case in mn.bad_cases(K, F):
            name, k, f, want = case[0], case[1], case[2], case[col]
            r = mn.loop_margins(k[None], f[None], fb, zre, zim)
            st = int(r["status"][0])
            if want is None:
                assert st & mn.SINGULAR and not st & mn.BAD_INPUT, (name, st)
            else:
                assert st == want, (name, fb, st)
            if st & (mn.SINGULAR | mn.BAD_INPUT):
                assert np.isnan(r["alpha_s"]).all() and np.isnan(r["alpha_t"]).all() and np.isnan(r["curve"]).all(), name
                assert (r["idx_s"] == -1).all() and (r["idx_t"] == -1).all(), name
            else:
                assert np.isfinite(r["alpha_s"]).all() and np.isfinite(r["curve"]).all(), name
            if name == "the pass-through filter":
                assert st == mn.NOT_STABLE and (r["alpha_s"] == 1.0).all() and (r["curve"] == 1.0).all() and (r["idx_s"] == 0).all()
            if name.startswith("Kb -> -0.5 Kb"):
                Phi, Gamma, Kb, _ = (np.moveaxis(m, -1, 0)[0] for m in mn.block_matrices(k[None], f[None], 0, True))
                assert np.abs(np.linalg.eigvals(Phi - Gamma @ Kb)).max() > 1.0
    # the squaring certificate by itself: a contraction, a rotation (never certified: the cap), an expansion (overflows), a NaN
    rot = np.eye(4)
    rot[:2, :2] = [[0.0, -1.0], [1.0, 0.0]]
    nan = 0.5 * np.eye(4)
    nan[1, 2] = np.nan
    m = np.stack([0.5 * np.eye(4), 0.999 * np.eye(4) + 0.01 * np.eye(4, k=1), rot, 1.5 * np.eye(4), nan], axis=-1)
    with np.errstate(all="ignore"):
        ok, sq = mn.schur_by_squaring(m)
    assert ok.tolist() == [True, True, False, False, False] and sq[0] == 0 and 1 <= sq[1] < mn.MAX_SQUARINGS and sq[2] == mn.MAX_SQUARINGS


# ---- hcrl_amd.margins without a device -----------------------------------------------------------------------------------------
def test_grid_construction_and_argument_errors():
    for dt in (0.01, 0.02, 0.005):
        w = M.default_grid(dt)
        assert w.shape == (64,) and w[0] == 1e-2 and w[-1] == math.pi / dt and (np.diff(w) > 0).all()
        assert np.allclose(np.diff(np.log(w)), np.log(w[1] / w[0]), rtol=1e-12)
        zre, zim = M.unit_circle(w, dt)
        assert (zre[-1], zim[-1]) == (-1.0, 0.0) and np.allclose(zre ** 2 + zim ** 2, 1.0, atol=1e-15)
        assert np.array_equal(w, mn.default_omega(dt)) and np.array_equal(zre, mn.unit_circle(w, dt)[0]) and np.array_equal(zim, mn.unit_circle(w, dt)[1])
    assert M.default_grid(0.01, 7).shape == (7,)
    zre, zim = M.unit_circle([1.0, 10.0], 0.01)
    assert zre.tolist() == [math.cos(0.01), math.cos(0.1)] and zim.tolist() == [math.sin(0.01), math.sin(0.1)]
    for bad in ([1.0, 1.0], [2.0, 1.0], [0.0, 1.0], [-1.0, 1.0], [1.0, np.nan], [1.0, 400.0], [], np.ones((2, 2)), np.arange(1.0, 258.0)):
        with pytest.raises(ValueError):
            M.unit_circle(bad, 0.01)
    for dt, n in ((0.0, 64), (-1.0, 64), (0.01, 1), (0.01, 257)):
        with pytest.raises(ValueError):
            M.default_grid(dt, n)


def _report(alpha, idx, status, omega=None):
    a = torch.tensor(alpha, dtype=torch.float64)
    i = torch.tensor(idx, dtype=torch.int32)
    return M.LoopMargins(a, i, a.clone(), i.clone(), torch.tensor(status, dtype=torch.int32), None,
                         None if omega is None else torch.tensor(omega, dtype=torch.float64), 0.01)


def test_margin_formulas_and_index_to_omega():
    nan = float("nan")
    r = _report([[0.5, 1.0, nan], [0.087, 2.5, nan]], [[1, 0, -1], [2, 2, -1]], [0, 1, 6], [0.1, 1.0, 10.0])
    assert r.n == 3 and r.ok.tolist() == [True, False, False] and r.count_not_ok() == 2
    low, high = r.gain_margin()
    assert low[0, 0].item() == pytest.approx(1 / 1.5) and high[0, 0].item() == pytest.approx(2.0)
    assert low[1, 0].item() == pytest.approx(1 / 1.087) and high[1, 0].item() == pytest.approx(1 / 0.913)
    assert math.isinf(high[0, 1].item()) and math.isinf(high[1, 1].item()) and math.isnan(high[0, 2].item()) and math.isnan(low[1, 2].item())
    lo_db, hi_db = r.gain_margin_db()
    assert lo_db[0, 0].item() == pytest.approx(20 * math.log10(1 / 1.5)) and hi_db[0, 0].item() == pytest.approx(20 * math.log10(2.0))
    pm = r.phase_margin_deg()
    assert pm[0, 0].item() == pytest.approx(math.degrees(2 * math.asin(0.25))) and pm[1, 0].item() == pytest.approx(math.degrees(2 * math.asin(0.0435)))
    assert pm[0, 1].item() == pytest.approx(60.0) and pm[1, 1].item() == pytest.approx(180.0) and math.isnan(pm[0, 2].item())
    assert r.omega_s[:, :2].tolist() == [[1.0, 0.1], [10.0, 10.0]] and torch.isnan(r.omega_s[:, 2]).all() and torch.equal(r.omega_t[:, :2], r.omega_s[:, :2])
    assert M.describe_status(0) == "ok" and r.describe_status(6) == "a pole on a grid point, invalid gain or filter"
    assert M.describe_status(1) == "nominal loop not certified stable"
    with pytest.raises(ValueError, match="no omega grid"):
        _report([[0.5], [0.5]], [[0], [0]], [0]).omega_s


def test_margins_into_refuses_wrong_arguments():
    K, F = torch.zeros((16, 3), dtype=torch.float64), torch.zeros((80, 3), dtype=torch.float64)
    z = torch.zeros(8, dtype=torch.float64)
    for args in ((K[:15], F, z, z), (K, F[:, :2], z, z), (K, F, z, z[:7]), (K, F, z[:0], z[:0]), (K, F, torch.zeros(257, dtype=torch.float64),
                 torch.zeros(257, dtype=torch.float64)), (K.float(), F, z, z), (K, F, z.float(), z.float()), (K, F, z.reshape(2, 4), z.reshape(2, 4))):
        with pytest.raises(ValueError):
            M.margins_into(*args)
    with pytest.raises(ValueError, match="feedback"):
        M.margins_into(K, F, z, z, "guess")
    with pytest.raises(ValueError, match="feedback"):
        M.margins_into(K, F, z, z, 3)
    with pytest.raises(ValueError, match="cannot take"):
        M.margins_into(K, F, z, z, "truth", _report([[0.5] * 2] * 2, [[0] * 2] * 2, [0, 0]))
    # every tensor on one device: "meta" tensors have a device and no storage, so this needs no GPU
    meta = torch.device("meta")
    for args in ((K, F.to(meta), z, z), (K, F, z.to(meta), z), (K, F, z, z.to(meta)), (K.to(meta), F, z, z)):
        with pytest.raises(ValueError, match="one device"):
            M.margins_into(*args)
    # a caller's report: dtype, shape, device and contiguity of every word, and a curve where one is asked for
    good = lambda: _report([[0.5] * 3] * 2, [[0] * 3] * 2, [0, 0, 0])
    with pytest.raises(ValueError, match="needs a report that has a curve"):
        M.margins_into(K, F, z, z, "truth", good(), curve=True)
    for name, bad in (("alpha_s", torch.zeros((2, 3))), ("idx_t", torch.zeros((2, 3), dtype=torch.int64)), ("alpha_t", torch.zeros((2, 3), dtype=torch.float64, device=meta)),
                      ("idx_s", torch.zeros((3, 2), dtype=torch.int32).T), ("alpha_s", torch.zeros((3, 3), dtype=torch.float64))):
        r = good()
        setattr(r, name, bad)
        with pytest.raises(ValueError, match=f"out.{name}"):
            M.margins_into(K, F, z, z, "truth", r)


def test_fleet_guards_need_no_device():
    from hcrl_amd.fleet import BatchedCascade, BatchedSixDOF
    from hcrl_amd.hybrid import HybridFleet
    assert HybridFleet.loop_margins is BatchedSixDOF.loop_margins and BatchedCascade.loop_margins is BatchedSixDOF.loop_margins
    fleet = BatchedSixDOF.__new__(BatchedSixDOF)
    fleet.n = 3
    with pytest.raises(ValueError, match=r"3 of 3 aircraft have no certified stabilising gain \(call \.design_lqr\(\) first\)"):
        fleet.loop_margins()
    fleet._lqr = object()
    with pytest.raises(ValueError, match=r"3 of 3 aircraft have no certified stable filter \(call \.design_kalman\(dt\) first\)"):
        fleet.loop_margins()

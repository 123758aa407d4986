"""The restatement of the servo's flight-mode report (servo_modes_numpy, which the host build of csrc/fdyn_eig_n.hpp equals bit for
bit: test_eig_n_host.py) against LAPACK (numpy.linalg.eig) on the servo matrices of the 288 linearisations of
tests/golden/trim_reference.npz: the continuous loops, and the sampled and filter loops at dt 0.01 and 0.02 -- 2880 blocks.

Eigenvalues are matched by a minimum-cost (bottleneck) assignment, never by sorted position.  Two gates per block M (N x N):

  Bauer-Fike   |lambda - lambda_ref| <= C eps kappa_2(V) |M|_2, V LAPACK's eigenvector matrix: both solvers are backward stable, so each
               computes the exact spectrum of M + E, |E|_2 = O(eps |M|_2), and an eigenvalue of M + E lies within kappa_2(V) |E|_2 of one
               of M.  Not a flat tolerance: the sampled loop's poles cluster near z = 1 and are not well conditioned.
  trace        |sum lambda - tr M| <= C N eps |M|_2, whatever the conditioning: an orthogonal similarity moves the trace only by the
               trace of its backward error.

C = 100.  Measured on this fixture set with the host build: the worst Bauer-Fike ratio |lambda - lambda_ref| / (eps kappa_2(V) |M|_2) is 1.98
(the filter at dt 0.01; continuous 0.096, sampled 0.42 / 0.34, filter 1.98 / 1.31) and the worst trace ratio
|sum lambda - tr M| / (N eps |M|_2) is 3.35 (the filter at dt 0.02).  Ten times each, rounded up to a power of ten, is 100 for both; the
margin is for other libm / LAPACK builds, not for the solver.  A block whose kappa_2(V) exceeds 1e8 would be reported and left out of
the first gate only, at most 2 % of the blocks; on this fixture set the largest kappa_2(V) is 9.8e3 (sampled, dt 0.02) and no block
is left out, dt 0.01 included.
"""
import os

import numpy as np
import pytest

import servo_lqg_numpy as sl
import servo_margin_numpy as sm
import servo_modes_numpy as smn
import servo_numpy as sn
import lqr_numpy as ln
import trim_numpy as tn
from conftest import GOLDEN

C, EPS = 100.0, 2.0 ** -52
KAPPA_MAX, LEFT_OUT_MAX = 1e8, 0.02


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "trim_reference.npz"))


def _loops(golden):
    lo, rp = smn.golden_loops(golden), smn.golden_reports(golden)
    yield "continuous", lo["continuous"], rp["continuous"]
    for dt in smn.DTS:
        yield f"sampled dt {dt}", lo["sampled"][dt], rp["sampled"][dt]
        yield f"filter dt {dt}", lo["filter"][dt], rp["filter"][dt]


def _gates(lam, M):
    """-> (Bauer-Fike ratio or None when kappa_2(V) > KAPPA_MAX, trace ratio, kappa_2(V))"""
    ref, bf, nrm = smn.bauer_fike(M)
    trace = abs(lam.sum() - np.trace(M)) / (len(M) * EPS * nrm)
    kappa = bf / nrm
    return (None if kappa > KAPPA_MAX else smn.assignment_gap(lam, ref) / (EPS * bf)), trace, kappa


def test_every_loop_against_lapack(golden):
    blocks, left_out = 0, []
    for name, loops, rep in _loops(golden):
        assert not rep["status"].any(), (name, np.flatnonzero(rep["status"]))
        worst_bf, worst_tr, worst_kappa = 0.0, 0.0, 0.0
        for i, lane in enumerate(loops):
            at = 0
            for b, M in enumerate(lane):
                lam = rep["re"][i, at:at + len(M)] + 1j * rep["im"][i, at:at + len(M)]
                at += len(M)
                bf, tr, kappa = _gates(lam, M)
                blocks += 1
                if bf is None:
                    left_out.append((name, i, b, kappa))
                else:
                    assert bf <= C, (name, i, b, bf)
                    worst_bf = max(worst_bf, bf)
                assert tr <= C, (name, i, b, tr)
                worst_tr, worst_kappa = max(worst_tr, tr), max(worst_kappa, kappa)
        print(f"{name}: Bauer-Fike ratio {worst_bf:.3g}, trace ratio {worst_tr:.3g}, largest kappa_2(V) {worst_kappa:.3g}")
    print(f"{len(left_out)} of {blocks} blocks left out of the Bauer-Fike gate: {left_out}")
    assert blocks == 288 * 10 and len(left_out) <= LEFT_OUT_MAX * blocks


def test_the_canonical_order_and_the_summary_words(golden):
    for name, loops, rep in _loops(golden):
        sizes = [len(m) for m in loops[0]]
        at = 0
        for b, N in enumerate(sizes):
            re, im = rep["re"][:, at:at + N], rep["im"][:, at:at + N]
            at += N
            assert (np.diff(re, axis=1) <= 0.0).all(), name                                      # real part descending
            pos = im > 0.0
            assert not pos[:, -1].any()
            assert (re[:, :-1][pos[:, :-1]] == re[:, 1:][pos[:, :-1]]).all() and (im[:, 1:][pos[:, :-1]] == -im[:, :-1][pos[:, :-1]]).all(), name
            mag = np.hypot(re, im)
            s = rep["summary"][:, b]
            assert np.array_equal(s[:, smn.mo.ABSCISSA], re[:, 0]) and np.array_equal(s[:, smn.mo.N_UNSTABLE], (re > 0.0).sum(axis=1))
            assert np.array_equal(s[:, smn.mo.N_COMPLEX], (im != 0.0).sum(axis=1))
            assert np.allclose(s[:, smn.mo.RADIUS], mag.max(axis=1), rtol=1e-15, atol=0.0) and np.allclose(s[:, smn.mo.MIN_ABS], mag.min(axis=1), rtol=1e-15, atol=0.0)
            assert np.allclose(s[:, smn.mo.MIN_ZETA], (-re / mag).min(axis=1), rtol=1e-14, atol=0.0)


def test_certified_designs_have_stable_poles(golden):
    """Wherever the servo design's status is 0 the continuous abscissa is < 0; wherever the margin restatement's FD_MRG_NOT_STABLE is
    clear (truth feedback: the sampled loop; estimate feedback: the filter as well) the sampled and filter radii are < 1."""
    lo, rp = smn.golden_loops(golden), smn.golden_reports(golden)
    ok = lo["status"] == 0
    assert ok.sum() >= 280
    assert (rp["continuous"]["summary"][ok][:, :, smn.mo.ABSCISSA] < 0.0).all()
    for dt in smn.DTS:
        zre, zim = sm.unit_circle(np.array([1.0, 10.0]), dt)
        truth = sm.loop_margins(lo["K"], lo["F"][dt], lo["x0"], dt, sm.TRUTH, zre, zim)["status"]
        est = sm.loop_margins(lo["K"], lo["F"][dt], lo["x0"], dt, sm.ESTIMATE, zre, zim)["status"]
        stable, both = (truth & sm.NOT_STABLE) == 0, (est & sm.NOT_STABLE) == 0
        assert stable.sum() >= 280 and both.sum() >= 280
        assert (rp["sampled"][dt]["summary"][stable][:, :, smn.mo.RADIUS] < 1.0).all()
        assert (rp["filter"][dt]["summary"][both][:, :, smn.mo.RADIUS] < 1.0).all()


def test_separation_sampled_and_filter_poles_are_the_estimate_feedback_spectrum():
    """For the ten aircraft of lqr_numpy.oracle_flights the eigenvalues (LAPACK) of the explicitly composed 12- and 11-state
    estimate-feedback matrices -- plant, estimate and integrators, composed in NumPy from the law and the filter as
    include/fdyn_servo_lqg.h states them (servo_margin_numpy.perturbed_loop with unit gains) -- equal the restatement's sampled poles
    together with its filter poles, under the Bauer-Fike gate of the composed matrix."""
    listed = [(tn.TYPES.index(name), V, g, w) for name, V, g, w in ln.CONDITIONS]
    worst = 0.0
    for t, V, g, w in listed + [(1 - t, V, g, w) for t, V, g, w in listed]:
        d = sn.oracle_design(tn.TYPES[t], V, g, w)
        assert d["status"] == 0
        for dt in smn.DTS:
            kf = sl.design(d["A"], d["B"], dt, sl.default_noise())
            assert kf["status"] == 0
            s = smn.servo_sampled_modes(d["K"][None], kf["F"][None], d["x0"][None], dt)
            f = smn.servo_filter_modes(kf["F"][None])
            assert s["status"][0] == 0 and f["status"][0] == 0
            for blk, (srows, frows) in enumerate(((slice(0, 7), slice(0, 5)), (slice(7, 13), slice(5, 10)))):
                lam = np.concatenate([s["re"][0, srows] + 1j * s["im"][0, srows], f["re"][0, frows] + 1j * f["im"][0, frows]])
                M = sm.perturbed_loop(d["K"], kf["F"], d["x0"], dt, blk, True, (1.0, 1.0))
                assert M.shape == ((12, 12), (11, 11))[blk]
                ref, bf, _ = smn.bauer_fike(M)
                ratio = smn.assignment_gap(lam, ref) / (EPS * bf)
                worst = max(worst, ratio)
                assert ratio <= C, (t, V, g, w, dt, blk, ratio)
    print(f"separation: worst Bauer-Fike ratio {worst:.3g}")

"""The flight-mode restatement (tests/modes_numpy.py: the arithmetic of csrc/fdyn_eig.hpp on NumPy fp64 scalars) against LAPACK.

Inputs: the 288 linearisations of tests/golden/trim_reference.npz -- both blocks open loop and under lqr_numpy's default design
(1152 blocks), and the 576 x 2 filter matrices Phi (I - L) of kf_numpy's default filter at dt 0.01 and 0.02.

Gate: every eigenvalue within 1e-10 |m|_inf of np.linalg.eigvals after the nearest matching of the two multisets.  By Bauer-Fike a
backward-stable solver errs by about c eps cond(V) |m|; the worst cond(V) on these matrices is 226 and the worst |m|_inf 811, so
the gate leaves three orders over eps cond(V).  Measured on these inputs: worst gap 3.0e-15 |m| on the 1152 continuous blocks,
1.9e-14 |m| on the filter matrices; at most 16 QR sweeps per block.

The summary words are held to the same quantities formed from LAPACK's values: the three lengths and the damping ratio -Re / |.|
under the same gate (measured: 2.7e-15 |m| and 1.9e-16 |m|), the two counts exactly -- they are unambiguous here, LAPACK's poles lie
at least 5e-4 |m| apart and no real part is within 2e-6 |m| of zero.

The exceptional shifts and the sweep cap are reached by modes_numpy.shift_cases (cyclic matrices, on which the standard shifts
change nothing), counted here through a spy on the restatement's sweep.
"""
import os

import numpy as np
import pytest

import modes_numpy as mo
from conftest import GOLDEN

GATE = 1e-10


@pytest.fixture(scope="module")
def blocks():
    return mo.golden_blocks(np.load(os.path.join(GOLDEN, "trim_reference.npz")))


@pytest.fixture(scope="module")
def solved(blocks):
    return {name: (M, mo.block_modes(M)) for name, M in (("open", blocks["open"]), ("closed", blocks["closed"]),
                                                           ("filter 0.01", blocks["filter"][0.01]), ("filter 0.02", blocks["filter"][0.02]))}


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.mark.parametrize("name", ["open", "closed", "filter 0.01", "filter 0.02"])
def test_golden_blocks_against_lapack(solved, name):
    M, r = solved[name]
    assert M.shape == (288, 2, 4, 4) and not r["status"].any()
    worst, worst_sum, worst_zeta, closest = 0.0, 0.0, 0.0, np.inf
    for i in range(288):
        for b in range(2):
            m = M[i, b]
            nrm, ref = mo.norm_inf(m), np.linalg.eigvals(m)
            got = r["re"][i, b] + 1j * r["im"][i, b]
            gap = mo.match_gap(got, ref) / nrm
            worst = max(worst, gap)
            assert gap <= GATE, (name, i, b, gap)
            d = np.abs(ref[:, None] - ref[None, :])[~np.eye(4, dtype=bool)].min() / nrm
            closest = min(closest, d)
            s, mag = r["summary"][i, b], np.abs(ref)
            for word, want in ((mo.ABSCISSA, ref.real.max()), (mo.RADIUS, mag.max()), (mo.MIN_ABS, mag.min())):
                worst_sum = max(worst_sum, abs(s[word] - want) / nrm)
                assert abs(s[word] - want) <= GATE * nrm, (name, i, b, word, s[word], want)
            worst_zeta = max(worst_zeta, abs(s[mo.MIN_ZETA] - (-ref.real / mag).min()) / nrm)
            assert abs(s[mo.MIN_ZETA] - (-ref.real / mag).min()) <= GATE * nrm, (name, i, b, s[mo.MIN_ZETA])
            assert s[mo.N_UNSTABLE] == (ref.real > 0.0).sum() and s[mo.N_COMPLEX] == (ref.imag != 0.0).sum(), (name, i, b, s, ref)
    print(f"{name}: worst eigenvalue gap {worst:.3e} |m|, worst summary length {worst_sum:.3e} |m|, damping ratio {worst_zeta:.3e} |m|, closest pair of LAPACK's poles "
          f"{closest:.3e} |m|, at most {int(r['iters'].max())} sweeps")
    assert closest >= 5e-4


def test_mode_census_of_the_golden_airframes(solved):
    """These airframes do not have the textbook mode set: no yaw stiffness, so no dutch roll; the phugoid is unstable on most."""
    nc_open, nc_closed = solved["open"][1]["summary"][:, :, mo.N_COMPLEX], solved["closed"][1]["summary"][:, :, mo.N_COMPLEX]
    assert np.bincount(nc_open[:, 0].astype(int), minlength=5).tolist() == [0, 0, 36, 0, 252]
    assert (nc_open[:, 1] == 0).all()
    assert solved["open"][1]["summary"][:, :, mo.N_UNSTABLE].sum() == 356 and (solved["open"][1]["summary"][:, 1, mo.N_UNSTABLE] == 0).all()
    assert (solved["open"][1]["summary"][:, 0, mo.N_UNSTABLE] == 2).sum() == 178
    assert solved["closed"][1]["summary"][:, :, mo.N_UNSTABLE].sum() == 0 and (solved["closed"][1]["summary"][:, :, mo.ABSCISSA] < 0.0).all()
    assert np.bincount(nc_closed[:, 0].astype(int), minlength=5).tolist() == [228, 0, 48, 0, 12]
    assert np.bincount(nc_closed[:, 1].astype(int), minlength=5).tolist() == [184, 0, 104, 0, 0]
    for dt in ("filter 0.01", "filter 0.02"):                            # a certified filter is Schur
        assert (solved[dt][1]["summary"][:, :, mo.RADIUS] < 1.0).all()


def test_ordering_and_pair_conventions_bitwise(solved):
    for name, (M, r) in solved.items():
        re, im = r["re"].reshape(-1, 4), r["im"].reshape(-1, 4)
        assert (re[:, :-1] >= re[:, 1:]).all(), name                     # real part descending
        for row_re, row_im in zip(re, im):
            k = 0
            while k < 4:
                if row_im[k] != 0.0:                                     # a pair: + first, the real parts one bit pattern
                    assert row_im[k] > 0.0 and _bits(row_im[k + 1]) == _bits(-row_im[k]) and _bits(row_re[k]) == _bits(row_re[k + 1]), name
                    k += 2
                else:
                    k += 1
        assert (r["summary"][:, :, mo.ABSCISSA] == r["re"][:, :, 0]).all(), name


# ---- known answers -------------------------------------------------------------------------------------------------------------
CASES = dict(mo.degenerate_cases())


def _solve(m):
    re, im, sweeps, ok = mo.eig4(np.asarray(m, np.float64) + 0.0)
    assert ok
    return re, im, sweeps


def test_rotation_block_and_a_diagonal():
    for sigma, omega, r1, r2 in ((-0.7, 2.5, 0.3, -4.0), (0.2, 1e-3, -1.0, 5.0), (-3.0, 40.0, -3.0, 0.0)):
        m = np.zeros((4, 4))
        m[:2, :2] = [[sigma, omega], [-omega, sigma]]
        m[2, 2], m[3, 3] = r1, r2
        re, im, _ = _solve(m)
        want = np.array([sigma + 1j * omega, sigma - 1j * omega, r1, r2])
        assert mo.match_gap(re + 1j * im, want) <= 1e-13 * mo.norm_inf(m)
        P = np.eye(4)[[2, 0, 3, 1]]                                       # the same blocks scattered: the reduction has work to do
        re, im, _ = _solve(P @ m @ P.T)
        assert mo.match_gap(re + 1j * im, want) <= 1e-13 * mo.norm_inf(m)


def test_zero_diagonal_and_triangular_matrices_come_back_exactly():
    re, im, sweeps = _solve(CASES["the zero matrix"])
    assert sweeps == 0 and not _bits(re).any() and not _bits(im).any()    # +0 in every word
    for name in ("the identity", "a diagonal", "upper triangular"):
        m = CASES[name]
        re, im, sweeps = _solve(m)
        assert sweeps == 0 and np.array_equal(re, np.sort(np.diag(m))[::-1]) and not im.any(), name


def test_hessenberg_inputs_and_zero_subdiagonals():
    for name in ("already Hessenberg", "Hessenberg with a zero subdiagonal", "lower triangular", "first column already reduced",
                 "a companion matrix"):
        m = CASES[name]
        re, im, sweeps = _solve(m)
        assert mo.match_gap(re + 1j * im, np.linalg.eigvals(m)) <= 1e-13 * mo.norm_inf(m), name
    h = [[np.float64(v) for v in row] for row in CASES["already Hessenberg"]]
    mo.hessenberg4(h)
    assert np.array_equal(_bits(np.array(h)), _bits(CASES["already Hessenberg"]))      # no reflector is applied
    assert _solve(CASES["Hessenberg with a zero subdiagonal"])[2] == 0    # two 2 x 2 blocks from the start: nothing to sweep
    assert (_solve(CASES["a companion matrix"])[1] != 0.0).all()


def test_poles_that_share_a_real_part_keep_their_pairs_together():
    re, im, sweeps = _solve(CASES["two pairs on one vertical line"])
    assert sweeps == 0 and re.tolist() == [-1.0] * 4 and im.tolist() == [3.0, -3.0, 2.0, -2.0]
    re, im, _ = _solve(CASES["a pair and a real pole on one vertical line"])
    assert re.tolist() == [0.5, -1.0, -1.0, -1.0] and im.tolist() == [0.0, 2.0, -2.0, 0.0]
    P = np.eye(4)[[2, 0, 3, 1]]                                           # scattered: through the reduction and the sweeps
    re, im, _ = _solve(P @ CASES["two pairs on one vertical line"] @ P.T)
    assert np.abs(re + 1.0).max() <= 1e-13 * 4.0 and np.abs(np.abs(im) - [3.0, 3.0, 2.0, 2.0]).max() <= 1e-13 * 4.0
    for k in (0, 2):                                                      # whichever pair comes first, its members are neighbours
        assert im[k] > 0.0 and _bits(im[k + 1]) == _bits(-im[k]) and _bits(re[k]) == _bits(re[k + 1])


def test_exceptional_shifts_and_the_sweep_cap(monkeypatch):
    seen, sweep = {}, mo.francis_step

    def spy(h, its):
        seen[len(h)] = max(seen.get(len(h), -1), its)
        return sweep(h, its)
    monkeypatch.setattr(mo, "francis_step", spy)
    for name, m, size, least, converges in mo.shift_cases():
        seen.clear()
        re, im, sweeps, ok = mo.eig4(m + 0.0)
        assert ok == converges and seen[size] >= least - 1 and sweeps >= least, (name, seen, sweeps, ok)
        if converges:
            assert mo.match_gap(re + 1j * im, np.linalg.eigvals(m)) <= GATE * mo.norm_inf(m), name
    stuck = mo.shift_cases()[-1][1]
    r = mo.block_modes(np.array([[CASES["already Hessenberg"], stuck], [CASES["already Hessenberg"]] * 2]))
    assert r["status"].tolist() == [mo.NOT_CONVERGED, 0] and r["iters"].tolist() == [30, 7]
    assert np.isnan(r["re"][0]).all() and np.isnan(r["im"][0]).all() and np.isnan(r["summary"][0]).all() and np.isfinite(r["re"][1]).all()
    for loop, i, b in mo.SLOW_GOLDEN:                                     # and the golden blocks the host file takes past sweep 10
        seen.clear()
        mo.eig4(mo.golden_blocks(np.load(os.path.join(GOLDEN, "trim_reference.npz")))[loop][i, b] + 0.0)
        assert seen[4] >= 10, (loop, i, b, seen)


def test_jordan_block_and_a_diagonal():
    m = CASES["Jordan block and a diagonal"]
    r = mo.block_modes(np.array([[m, m.T]]))
    assert r["status"][0] == 0
    for b in range(2):
        assert mo.match_gap(r["re"][0, b] + 1j * r["im"][0, b], np.array([-1.5, -1.5, 0.4, -3.0])) <= 1e-7


def test_a_nan_word_gives_status_2_and_nan_everywhere():
    good = CASES["already Hessenberg"]
    for bad_value in (np.nan, np.inf, -np.inf):
        for b in range(2):
            M = np.array([[good, good]])
            M[0, b, 2, 1] = bad_value
            r = mo.block_modes(M)
            assert r["status"][0] == mo.BAD_INPUT and r["iters"][0] == 0
            assert np.isnan(r["re"]).all() and np.isnan(r["im"]).all() and np.isnan(r["summary"]).all()


def test_summary_words_of_known_spectra():
    s = mo.summary(np.array([0.5, -1.0, -1.0, -2.0]), np.array([0.0, 1.0, -1.0, 0.0]))
    assert s[mo.ABSCISSA] == 0.5 and s[mo.RADIUS] == 2.0 and s[mo.MIN_ABS] == 0.5 and s[mo.MIN_ZETA] == -1.0
    assert s[mo.N_UNSTABLE] == 1.0 and s[mo.N_COMPLEX] == 2.0
    s = mo.summary(np.array([0.0, -3.0, -3.0, -5.0]), np.array([0.0, 4.0, -4.0, 0.0]))
    assert s[mo.MIN_ZETA] == 0.0 and s[mo.MIN_ABS] == 0.0 and s[mo.RADIUS] == 5.0 and s[mo.N_UNSTABLE] == 0.0     # zeta of 0 is 0
    s = mo.summary(np.array([-3.0, -3.0, -4.0, -5.0]), np.array([4.0, -4.0, 0.0, 0.0]))
    assert s[mo.MIN_ZETA] == 0.6 and s[mo.ABSCISSA] == -3.0

"""csrc/fdyn_eig_n.hpp -- the N x N Hessenberg reduction, the windowed double-shift QR sweeps, the eigenvalues written back into the
word store, the sorting network, the summary words and the three compositions that the servo-modes kernels compile -- run on the
host: a stand-alone program (tests/host/eig_n_check.cpp) built with the host compiler, once plain and once under AddressSanitizer
and UBSan, solves a file of lanes, and every word it writes (eigenvalues, summary, iters, status) must equal the NumPy model's
(servo_modes_numpy) BIT FOR BIT.  Both sides are IEEE fp64 with one rounding per operation in the same order, and the host's sqrt is
correctly rounded as np.sqrt is, so nothing but equality is expected.

Lanes: servo_modes_numpy.degenerate_cases and shift_cases at every N = 2 .. 7 through the square entry; the servo matrices of all
288 linearisations of tests/golden/trim_reference.npz composed from A, B, x0, K and F by the three composition routines themselves
(continuous; sampled and filter at dt 0.01 and 0.02); one servo loop of a 65 536-aircraft fleet that ends at the sweep cap; and lanes
the compositions refuse.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import servo_modes_numpy as smn
from conftest import GOLDEN

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORDS = 2 * smn.NEIG + 2 * smn.NMO + 2


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _expected(rep, i, n_eig, n_blocks):
    row = np.full(WORDS, -7.0)
    row[0:n_eig], row[smn.NEIG:smn.NEIG + n_eig] = rep["re"][i], rep["im"][i]
    row[2 * smn.NEIG:2 * smn.NEIG + n_blocks * smn.NMO] = rep["summary"][i].reshape(-1)
    row[-2], row[-1] = rep["iters"][i], rep["status"][i]
    return row


@pytest.fixture(scope="module")
def lanes():
    """-> list of (name, record words, expected output row)"""
    golden = np.load(os.path.join(GOLDEN, "trim_reference.npz"))
    out = []
    for N in range(smn.MIN_N, smn.MAX_N + 1):
        cases = smn.degenerate_cases(N) + [(name, m) for name, m, _, _ in smn.shift_cases(N)]
        rep = smn.square_modes([m for _, m in cases])
        out += [(f"{N} x {N} {name}", np.concatenate([[0.0, float(N)], np.asarray(m, np.float64).ravel()]), _expected(rep, i, N, 1))
                for i, (name, m) in enumerate(cases)]
    rep = smn.square_modes([smn.STALLED_LOOP])
    out.append(("a servo loop of a spread fleet that ends at the cap", np.concatenate([[0.0, 7.0], smn.STALLED_LOOP.ravel()]), _expected(rep, 0, 7, 1)))
    lo, rp = smn.golden_loops(golden), smn.golden_reports(golden)
    A, B = np.asarray(golden["A"], np.float64), np.asarray(golden["B"], np.float64)
    K, x0 = lo["K"], lo["x0"]
    for i in range(len(A)):
        out.append((f"aircraft {i} continuous", np.concatenate([[1.0, 0.0], A[i].ravel(), B[i].ravel(), x0[i], K[i]]), _expected(rp["continuous"], i, 13, 2)))
        for dt in smn.DTS:
            F = lo["F"][dt][i]
            out.append((f"aircraft {i} sampled dt {dt}", np.concatenate([[2.0, dt], K[i], F, x0[i]]), _expected(rp["sampled"][dt], i, 13, 2)))
            out.append((f"aircraft {i} filter dt {dt}", np.concatenate([[3.0, 0.0], F]), _expected(rp["filter"][dt], i, 10, 2)))
    # what the compositions refuse, and what they do not read
    a, b, k, x, f = A[5].copy(), B[5].copy(), K[5].copy(), x0[5].copy(), lo["F"][0.02][5].copy()
    bad = []
    for name, kind, words in (("K NaN", 1, (a, b, x, np.where(np.arange(26) == 20, np.nan, k))),
                              ("V0 = 0", 1, (a, b, np.where(np.isin(np.arange(12), (3, 5)), 0.0, x), k)),
                              ("A inf inside a block", 1, (np.where(np.arange(144).reshape(12, 12) == 3 * 12 + 5, np.inf, a), b, x, k)),
                              ("A NaN outside the blocks: not read", 1, (np.where(np.arange(144).reshape(12, 12) == 0 * 12 + 1, np.nan, a), b, x, k)),
                              ("x0 NaN outside u, w: not read", 1, (a, b, np.where(np.isin(np.arange(12), (3, 5)), x, np.nan), k))):
        rep = smn.servo_flight_modes(words[0][None], words[1][None], words[2][None], words[3][None])
        bad.append((name, np.concatenate([[1.0, 0.0]] + [np.ravel(w) for w in words]), _expected(rep, 0, 13, 2)))
    for name, dt, kk, ff, xx in (("dt = 0", 0.0, k, f, x), ("dt = 2", 2.0, k, f, x), ("Gamma NaN", 0.02, k, np.where(np.arange(120) == 55, np.nan, f), x),
                                 ("L NaN: not read by the sampled loop", 0.02, k, np.where(np.arange(120) == 100, np.nan, f), x),
                                 ("-0.5 K: positive feedback", 0.02, -0.5 * k, f, x)):
        rep = smn.servo_sampled_modes(kk[None], ff[None], xx[None], dt)
        bad.append((name, np.concatenate([[2.0, dt], kk, ff, xx]), _expected(rep, 0, 13, 2)))
    for name, ff in (("L inf", np.where(np.arange(120) == 71, np.inf, f)), ("Gamma NaN: not read by the filter", np.where(np.arange(120) == 55, np.nan, f)),
                     ("the pass-through filter", smn.sl.pass_through())):
        rep = smn.servo_filter_modes(ff[None])
        bad.append((name, np.concatenate([[3.0, 0.0], ff]), _expected(rep, 0, 10, 2)))
    assert [int(r[2][-1]) for r in bad] == [2, 2, 2, 0, 0, 2, 2, 2, 0, 0, 2, 0, 0]
    return out + bad


@pytest.mark.parametrize("flags", (["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]),
                         ids=("plain", "asan-ubsan"))
def test_every_output_word_equals_the_model_bit_for_bit(tmp_path, lanes, flags):
    fin, fout, exe = str(tmp_path / "lanes.f64"), str(tmp_path / "out.f64"), str(tmp_path / "eig_n_check")
    np.concatenate([[float(len(lanes))]] + [rec for _, rec, _ in lanes]).tofile(fin)
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler: the CPU oracle cannot be built without one either"
    subprocess.run([cxx, *flags, "-std=c++17", "-ffp-contract=off", os.path.join(REPO, "tests", "host", "eig_n_check.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    run = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stdout, run.stderr)
    got = np.fromfile(fout, dtype=np.float64).reshape(len(lanes), WORDS)
    for (name, _, want), row in zip(lanes, got):
        assert np.array_equal(_bits(row), _bits(want)), (name, row, want)
    # the file exercises the sweeps, the cap, the refusals and the complex branch
    status, iters = got[:, -1].astype(int), got[:, -2].astype(int)
    capped = [name for (name, _, _), s in zip(lanes, status) if s == smn.NOT_CONVERGED]
    assert capped == [f"{N} x {N} weighted cyclic {N} x {N} to the cap" for N in range(3, 8)] + ["a servo loop of a spread fleet that ends at the cap"]
    assert (status == smn.BAD_INPUT).sum() == 3 * 6 + 7 and iters.max() >= 30 and iters.min() == 0
    assert (got[status == 0][:, smn.NEIG:2 * smn.NEIG] > 0.0).sum() >= 1000


def test_the_shift_cases_reach_the_exceptional_shifts():
    """Per N a matrix past sweep 10 of one deflation, one past sweep 20 and one at the cap (N = 2 has nothing to sweep)."""
    assert smn.shift_cases(2) == []
    for N in range(3, smn.MAX_N + 1):
        seen = []
        for name, m, least, converges in smn.shift_cases(N):
            most, ok = smn.sweeps_of(m)
            assert most >= least and ok == converges, (name, most, ok)
            seen.append(least)
        assert sorted(seen) == [11, 21, 30], (N, seen)


def test_a_real_servo_loop_at_the_cap_reports_not_converged():
    """The limit DESIGN.md 7o records: the second deflation of this loop runs 30 sweeps on a window of two complex pairs (LAPACK
    finds them) and the lane answers FD_MO_NOT_CONVERGED with NaN words, never a pole."""
    trace = []
    re, im, sweeps, ok = smn.eig_n(smn.STALLED_LOOP + 0.0, trace)
    assert not ok and trace == [4, 30] and sweeps == 34 and np.isnan(re).all() and np.isnan(im).all()
    lam = np.linalg.eigvals(smn.STALLED_LOOP)
    assert (lam.real < 0.0).all() and (lam.imag > 0.0).sum() == 2
    rep = smn.square_modes([smn.STALLED_LOOP])
    assert rep["status"][0] == smn.NOT_CONVERGED and rep["iters"][0] == 34 and np.isnan(rep["summary"][0]).all()


def test_the_sweep_cap_is_far_from_the_servo_matrices():
    """What decides that the search for two small consecutive subdiagonals stays out (csrc/fdyn_eig_n.hpp): no deflation of any of
    the 288 x 10 servo matrices reaches the cap of 30 sweeps (the slowest takes 15: the first exceptional shift is used)."""
    lo = smn.golden_loops(np.load(os.path.join(GOLDEN, "trim_reference.npz")))
    most = 0
    for loops in (lo["continuous"], *lo["sampled"].values(), *lo["filter"].values()):
        for lane in loops:
            for m in lane:
                s, ok = smn.sweeps_of(m)
                assert ok
                most = max(most, s)
    print("most sweeps of one deflation on the fixture set:", most)
    assert 10 < most < smn.MAX_SWEEPS

"""csrc/fdyn_stein_n.hpp -- the Smith doubling for X = A X B^T + Q, its residual and stopping rule, the three equations per block and
the 34 report words that the servo-covariance kernels compile -- run on the host: a stand-alone program (tests/host/stein_check.cpp,
its own main) built with the host compiler, once plain and once under AddressSanitizer and UBSan, solves a file of lanes, and every
word it writes (X or report and cov, residual, iteration count, status) must equal the NumPy model's (servo_cov_numpy) BIT FOR BIT.
Both sides are IEEE fp64 with one rounding per operation in the same order, so nothing but equality is expected.

Lanes: both blocks of the golden aircraft 0, 97, 200 and 287 at dt 0.01 and 0.02 under all three feedbacks, without and with process
noise (every solve of both blocks is in cov); the general solver at (N, M) = (1,1), (2,7), (5,5), (7,5), (7,7); a NaN word; a
non-Schur A (the squares overflow); a cap case; and lanes the report refuses (a NaN word, sigma < 0, the zero gain, the pass-through
filter).
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import servo_cov_numpy as sc
import servo_lqg_numpy as sl
import servo_margin_numpy as sm
from conftest import GOLDEN

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORDS = sc.NSCV + sc.NSCC + 3
AIRCRAFT = (0, 97, 200, 287)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _stein_lane(name, A, B, Q):
    A, B, Q = (np.asarray(v, np.float64) for v in (A, B, Q))
    r = sc.stein_solve(A, B, Q)
    row = np.full(WORDS, -7.0)
    row[:Q.size] = r["X"].reshape(-1)
    row[-3:] = r["residual"], r["iters"], r["status"]
    return name, np.concatenate([[0.0, float(len(A)), float(len(B))], A.ravel(), B.ravel(), Q.ravel()]), row


def _report_lane(name, K, F, x0, dt, sigma, rates, fb):
    r = sc.servo_covariance(K, F, x0, dt, sigma, rates, fb)
    row = np.concatenate([r["report"], r["cov"], [r["residual"], r["iters"], r["status"]]])
    rec = np.concatenate([[1.0, dt, float(fb)], K, F, x0, sigma, [0.0 if rates is None else 1.0], np.zeros(10) if rates is None else rates])
    return name, rec, row


@pytest.fixture(scope="module")
def lanes():
    """-> list of (name, record words, expected output row)"""
    d = sm.golden_designs(np.load(os.path.join(GOLDEN, "trim_reference.npz")))
    sigma, rates = np.array(sl.DEFAULT_SIGMA), np.array(sl.DEFAULT_RATES)
    out = []
    for i in AIRCRAFT:
        for dt in sc.DTS:
            for fb in sc.FEEDBACKS:
                for w in (None, rates):
                    out.append(_report_lane(f"aircraft {i} dt {dt} feedback {fb} {'W' if w is not None else 'no W'}", d["K"][i], d["F"][dt][i],
                                            d["x0"][i], dt, sigma, w, fb))
    assert all(int(r[2][-1]) == 0 for r in out)
    for (N, M), (A, B, Q) in sc.stein_cases().items():
        out.append(_stein_lane(f"stein {N} x {M}", A, B, Q))
    A, B, Q = sc.stein_cases()[7, 5]
    out.append(_stein_lane("stein: a NaN word of Q", A, B, np.where(np.arange(35).reshape(7, 5) == 11, np.nan, Q)))
    out.append(_stein_lane("stein: an infinite word of B", A, np.where(np.arange(25).reshape(5, 5) == 3, np.inf, B), Q))
    out.append(_stein_lane("stein: a non-Schur A", 3.0 * A, 2.0 * B, Q))
    out.append(_stein_lane("stein: the cap", *sc.cap_case()))
    out.append(_stein_lane("stein: Q = 0", A, B, np.zeros((7, 5))))
    K, F, x0 = d["K"][97], d["F"][0.01][97], d["x0"][97]
    bad = [("a NaN word of K", np.where(np.arange(26) == 9, np.nan, K), F, x0, 0.01, sigma, None),
           ("an infinite word of L", K, np.where(np.arange(120) == 101, np.inf, F), x0, 0.01, sigma, None),
           ("sigma < 0", K, F, x0, 0.01, np.where(np.arange(10) == 4, -0.5, sigma), None),
           ("a NaN rate", K, F, x0, 0.01, sigma, np.where(np.arange(10) == 2, np.nan, rates)),
           ("dt = 0", K, F, x0, 0.0, sigma, None),
           ("V0 = 0", K, F, np.where(np.isin(np.arange(12), (3, 5)), 0.0, x0), 0.01, sigma, None),
           ("the zero gain of a failed servo design", np.zeros(26), F, x0, 0.01, sigma, None),
           ("the pass-through filter", K, sl.pass_through(), x0, 0.01, sigma, None),
           ("-0.5 K: positive feedback", -0.5 * K, F, x0, 0.01, sigma, None),
           ("sigma = 0: allowed", K, F, x0, 0.01, np.zeros(10), rates)]
    rows = [_report_lane(name, k, f, x, dt, s, w, sc.ESTIMATE) for name, k, f, x, dt, s, w in bad]
    assert [int(r[2][-1]) for r in rows] == [4, 4, 4, 4, 4, 4, 2, 2, 2, 0]
    return out + rows


@pytest.mark.parametrize("flags", (["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]),
                         ids=("plain", "asan-ubsan"))
def test_every_output_word_equals_the_model_bit_for_bit(tmp_path, lanes, flags):
    fin, fout, exe = str(tmp_path / "lanes.f64"), str(tmp_path / "out.f64"), str(tmp_path / "stein_check")
    np.concatenate([[float(len(lanes))]] + [rec for _, rec, _ in lanes]).tofile(fin)
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler: the CPU oracle cannot be built without one either"
    subprocess.run([cxx, *flags, "-std=c++17", "-ffp-contract=off", os.path.join(REPO, "tests", "host", "stein_check.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    run = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stdout, run.stderr)
    got = np.fromfile(fout, dtype=np.float64).reshape(len(lanes), WORDS)
    for (name, _, want), row in zip(lanes, got):
        differ = np.nonzero(_bits(row) != _bits(want))[0]
        assert differ.size == 0, (name, differ[:8], row[differ[:8]], want[differ[:8]])
    # the file exercises the doubling, the cap, the overflow, the refusals and an X that is exactly zero
    status, iters = got[:, -1].astype(int), got[:, -2].astype(int)
    by_name = {name: k for k, (name, _, _) in enumerate(lanes)}
    assert status[by_name["stein: the cap"]] == sc.NOT_CONVERGED and iters[by_name["stein: the cap"]] == sc.MAX_DOUBLINGS
    assert status[by_name["stein: a non-Schur A"]] == sc.NOT_CONVERGED and iters[by_name["stein: a non-Schur A"]] < sc.MAX_DOUBLINGS
    assert status[by_name["stein: a NaN word of Q"]] == sc.BAD_INPUT and np.isnan(got[by_name["stein: a NaN word of Q"], :35]).all()
    zero = by_name["stein: Q = 0"]
    assert status[zero] == 0 and iters[zero] == 1 and got[zero, -3] == 0.0 and not got[zero, :35].any()
    good = [k for name, k in by_name.items() if name.startswith("aircraft")]
    assert 9 <= iters[good].min() and iters[good].max() <= 20


def test_truth_feedback_without_process_noise_is_exactly_zero():
    """X = 0 is the one case the residual's denominator vanishes in: residual 0, status 0, and only the estimate's words non-zero."""
    d = sm.golden_designs(np.load(os.path.join(GOLDEN, "trim_reference.npz")))
    r = sc.servo_covariance(d["K"][0], d["F"][0.01][0], d["x0"][0], 0.01, sl.DEFAULT_SIGMA, None, sc.TRUTH)
    assert r["status"] == 0 and np.isfinite(r["residual"])
    rest = np.delete(r["report"], np.arange(sc.VAR_EST, sc.VAR_EST + 10))
    assert not rest.any() and (r["report"][sc.VAR_EST:sc.VAR_EST + 10] > 0.0).all()
    assert not r["cov"][sc.CC_XE[0]:].any()

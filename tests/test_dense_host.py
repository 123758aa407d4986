"""csrc/fdyn_dense.hpp -- the elimination both design kernels compile (gauss_solve<7, 1> for the trim Newton step, gauss_solve<4, 4>
against the identity for the LQR inverses) -- run on the host: a stand-alone program (tests/host/dense_check.cpp) built with the
host compiler under UBSan solves a file of systems, and every solution and flag must equal the NumPy model's
(trim_numpy.gauss_solve) BIT FOR BIT.  Both sides are IEEE fp64 with one rounding per operation in the same order, so nothing
but equality is expected: every word is compared through its integer view, NaNs included.
"""
import functools
import os
import shutil
import subprocess

import numpy as np

import trim_numpy as tn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIVOT_REL = 1e-14                            # TRIM_PIVOT_REL and LQR_PIVOT_REL of the kernels
N_RANDOM = 12


def _systems(n):
    """-> list of (name, a [n][n], b [n], ok expected or None)."""
    rs = np.random.RandomState(100 + n)
    out = [(f"random {k}", rs.normal(size=(n, n)) + 3.0 * np.eye(n), rs.normal(size=n), True) for k in range(N_RANDOM)]
    # a swap at every column: entries in [-1, 1] under a sub-diagonal of 10.  At column k the candidates are the row swapped down
    # at k - 1 (entries <= 1 + 0.1 in size after one update by a multiplier <= 0.1) and 10 one row below: the lower row wins.
    a = rs.uniform(-1.0, 1.0, size=(n, n))
    a[np.arange(1, n), np.arange(n - 1)] = 10.0
    out.append(("swap at every column", a, rs.normal(size=n), True))
    a = rs.normal(size=(n, n))
    a[:, n // 2] = 0.0
    out.append(("zero pivot column", a, rs.normal(size=n), False))
    # the relative floor is PIVOT_REL * max|a| = 1e-14 exactly (max|a| = 1): one pivot a hair under it, its twin a hair over
    for name, last, ok in (("pivot under the floor", 0.99e-14, False), ("pivot over the floor", 1.01e-14, True)):
        a = np.eye(n)
        a[n - 1, n - 1] = last
        a[0, 1:] = 0.5
        out.append((name, a, rs.normal(size=n), ok))
    a = rs.normal(size=(n, n))
    a[1, n - 2] = np.nan
    out.append(("NaN entry", a, rs.normal(size=n), False))
    return out


@functools.lru_cache(maxsize=None)
def _host_results(tmp):
    s7, s4 = _systems(7), _systems(4)
    words = [np.array([len(s7), len(s4), PIVOT_REL])]
    words += [np.concatenate([a.ravel(), b]) for _, a, b, _ in s7] + [a.ravel() for _, a, _, _ in s4]
    src, exe = os.path.join(REPO, "tests", "host", "dense_check.cpp"), os.path.join(tmp, "dense_check")
    fin, fout = os.path.join(tmp, "systems.f64"), os.path.join(tmp, "solutions.f64")
    np.concatenate(words).astype(np.float64).tofile(fin)
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler: the CPU oracle cannot be built without one either"
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=undefined", "-fno-sanitize-recover=undefined",
                    src, "-o", exe], check=True, capture_output=True, text=True)
    run = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stdout, run.stderr)
    got = np.fromfile(fout, dtype=np.float64)
    assert got.size == len(s7) * 8 + len(s4) * 17
    return s7, s4, got[:len(s7) * 8].reshape(-1, 8), got[len(s7) * 8:].reshape(-1, 17)


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float64).view(np.uint64), np.ascontiguousarray(b, np.float64).view(np.uint64))


def test_gauss_solve_7x1_equals_the_model_bit_for_bit(tmp_path_factory):
    s7, _, got, _ = _host_results(str(tmp_path_factory.getbasetemp()))
    for (name, a, b, ok_want), row in zip(s7, got):
        x, ok = tn.gauss_solve(a, b, PIVOT_REL)
        assert ok == bool(row[7]) == ok_want, (name, ok, row[7])
        assert _same_bits(row[:7], x), (name, row[:7], x)
        if ok:
            assert np.abs(a @ x - b).max() <= 1e-9 * max(1.0, np.abs(x).max()), name


def test_gauss_solve_4x4_against_the_identity_equals_the_model_bit_for_bit(tmp_path_factory):
    _, s4, _, got = _host_results(str(tmp_path_factory.getbasetemp()))
    for (name, a, _, ok_want), row in zip(s4, got):
        x, ok = tn.gauss_solve(a, np.eye(4), PIVOT_REL)
        assert ok == bool(row[16]) == ok_want, (name, ok, row[16])
        assert _same_bits(row[:16].reshape(4, 4), x), (name, row[:16], x)
        if ok:
            assert np.abs(a @ x - np.eye(4)).max() <= 1e-9 * max(1.0, np.abs(x).max()), name

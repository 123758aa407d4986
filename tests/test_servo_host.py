"""csrc/fdyn_riccati_n.hpp -- the Riccati solver the LQ-servo design kernel compiles at N = 7 and N = 6 (products, inverse, L D L^T
test, Cayley start, doubling loop, gain and residual) -- run on the host: a stand-alone program (tests/host/servo_check.cpp) built
with the host compiler under AddressSanitizer and UBSan solves a file of blocks, and every word it writes must equal the NumPy
restatement's (servo_numpy.care_solve) BIT FOR BIT.  Both sides are IEEE fp64 with one rounding per operation in the same order,
so nothing but equality is expected.
"""
import os
import shutil
import subprocess

import numpy as np

import servo_numpy as sn
from conftest import GOLDEN

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _blocks():
    """(name, a, b, q, r): the augmented blocks of golden aircraft, and the degenerate ends of the solver."""
    g = np.load(os.path.join(GOLDEN, "trim_reference.npz"))
    w = sn.block_weights(sn.default_weights())
    out = []
    for i in (0, 97, 200, 287):
        for k, ((a, b), (q, r)) in enumerate(zip(sn.augmented_blocks(g["A"][i], g["B"][i], g["x0"][i]), w)):
            out.append((f"aircraft {i} block {k}", a, b, q, r))
    (a7, b7), (a6, b6) = sn.augmented_blocks(g["A"][0], g["B"][0], g["x0"][0])
    nan = a7.copy()
    nan[2, 1] = np.nan
    out.append(("a NaN word", nan, b7, *w[0]))
    out.append(("b = 0, longitudinal: the integrators cannot be stabilised", a7, np.zeros_like(b7), *w[0]))
    out.append(("b = 0, lateral", a6, np.zeros_like(b6), *w[1]))
    # a - gamma I singular: a = diag(1, 0, ...) has |a|_inf = 1 = gamma, so the first pivot of the start is exactly zero
    sing = np.zeros((6, 6))
    sing[0, 0] = 1.0
    out.append(("a singular start", sing, b6, *w[1]))
    return out


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float64).view(np.uint64), np.ascontiguousarray(b, np.float64).view(np.uint64))


def test_solver_equals_the_restatement_bit_for_bit(tmp_path):
    blocks = _blocks()
    fin, fout, exe = str(tmp_path / "blocks.f64"), str(tmp_path / "out.f64"), str(tmp_path / "servo_check")
    words = [[float(len(blocks))]]
    for _, a, b, q, r in blocks:
        words += [[float(len(a))], a.ravel(), b.ravel(), q, r]
    np.concatenate([np.asarray(w, np.float64) for w in words]).tofile(fin)
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler: the CPU oracle cannot be built without one either"
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(REPO, "tests", "host", "servo_check.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    run = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stdout, run.stderr)
    got = np.fromfile(fout, dtype=np.float64)
    at, seen = 0, []
    for name, a, b, q, r in blocks:
        N = len(a)
        row = got[at:at + N * N + 2 * N + 5]
        at += len(row)
        ref = sn.care_solve(a, b, q, r)
        flags = (int(row[-4]), bool(row[-3]), bool(row[-2]), bool(row[-1]))
        assert flags == (ref["iters"], ref["failed"], ref["converged"], ref["positive"]), (name, flags, ref)
        assert _same_bits(row[:N * N].reshape(N, N), ref["X"]), name
        assert _same_bits(row[N * N:N * N + 2 * N].reshape(2, N), ref["K"]), name
        assert _same_bits(row[-5], ref["residual"]), name
        seen.append(ref["status"])
    assert at == len(got)
    assert not any(seen[:8]) and all(sn.care_solve(*blk[1:])["iters"] <= 12 for blk in blocks[:8])     # the golden blocks are certified
    assert all(seen[8:]), seen                                              # every degenerate block is refused a certificate
    assert seen[8] & sn.NOT_CONVERGED and seen[11] & sn.NOT_CONVERGED       # the NaN word and the singular start fail outright

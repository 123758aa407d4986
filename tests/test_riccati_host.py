"""csrc/fdyn_riccati.hpp -- the 4 x 4 matrix products, inverse, L D L^T test and doubling loop that both design kernels compile
(fdyn_lqr_design after its Cayley transform, fdyn_kf_design on the discrete filter equation) -- run on the host: a stand-alone
program (tests/host/riccati_check.cpp) built with the host compiler under AddressSanitizer and UBSan runs the loop on a file of
start triples, and every word it writes must equal the NumPy model's (kf_numpy.doubling, lqr_numpy.inv4 / ldl_positive) BIT FOR
BIT.  Both sides are IEEE fp64 with one rounding per operation in the same order, so nothing but equality is expected.
"""
import os
import shutil
import subprocess

import numpy as np

import kf_numpy as kn
import lqr_numpy as ln
from conftest import GOLDEN

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _triples():
    """(name, A_0, G_0, H_0): the filter problem of golden aircraft at two step sizes, and the degenerate ends of the loop."""
    g = np.load(os.path.join(GOLDEN, "trim_reference.npz"))
    nz = kn.default_noise()
    out = []
    for i in (0, 97, 200, 287):
        for dt in (0.01, 0.02):
            for k, (a, b) in enumerate(ln.blocks(g["A"][i], g["B"][i])):
                Phi, _ = kn.discretise(a, b, dt)
                out.append((f"aircraft {i} block {k} dt {dt}", Phi.T.copy(), np.diag(1.0 / nz[4 * k:4 * k + 4] ** 2),
                            np.diag(nz[8 + 4 * k:12 + 4 * k] ** 2 * dt)))
    out.append(("unstable and undetected: hits the cap or overflows", 1.5 * np.eye(4), np.zeros((4, 4)), np.eye(4)))
    out.append(("singular I + G H", np.eye(4), -np.eye(4), np.eye(4)))
    nan = np.eye(4)
    nan[2, 1] = np.nan
    out.append(("a NaN word", nan, np.eye(4), np.eye(4)))
    out.append(("already converged", np.zeros((4, 4)), np.eye(4), np.eye(4)))
    return out


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float64).view(np.uint64), np.ascontiguousarray(b, np.float64).view(np.uint64))


def test_doubling_loop_inverse_and_ldl_equal_the_model_bit_for_bit(tmp_path):
    triples = _triples()
    fin, fout, exe = str(tmp_path / "triples.f64"), str(tmp_path / "out.f64"), str(tmp_path / "riccati_check")
    np.concatenate([[float(len(triples))]] + [np.concatenate([a.ravel(), g.ravel(), h.ravel()]) for _, a, g, h in triples]).tofile(fin)
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler: the CPU oracle cannot be built without one either"
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(REPO, "tests", "host", "riccati_check.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    run = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stdout, run.stderr)
    got = np.fromfile(fout, dtype=np.float64).reshape(len(triples), 37)
    seen = set()
    with np.errstate(all="ignore"):
        for (name, a, g, h), row in zip(triples, got):
            H, it, failed, converged = kn.doubling(a, g, h)
            assert (it, failed, converged) == (int(row[16]), bool(row[17]), bool(row[18])), (name, it, failed, converged, row[16:19])
            assert _same_bits(row[:16].reshape(4, 4), H), name
            assert bool(row[19]) == ln.ldl_positive(0.5 * (H + H.T)), name
            inv, ok = ln.inv4(np.eye(4) + ln.mm(g, h))
            assert ok == bool(row[36]) and _same_bits(row[20:36].reshape(4, 4), inv), name
            seen.add((failed, converged))
    assert seen == {(False, True), (True, False)} or seen == {(False, True), (True, False), (False, False)}
    assert all(bool(r[18]) and r[16] <= 12 for r in got[:16])            # the sixteen filter problems converge

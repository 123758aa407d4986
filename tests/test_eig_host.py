"""csrc/fdyn_eig.hpp -- the Hessenberg reduction, the double-shift QR sweeps, the closed-form 2 x 2 blocks, the sorting network and
the summary words that the flight-modes kernel compiles -- run on the host: a stand-alone program (tests/host/eig_check.cpp) built
with the host compiler under AddressSanitizer and UBSan solves a file of matrices, and every word it writes must equal the NumPy
model's (modes_numpy.eig4 / summary) BIT FOR BIT.  Both sides are IEEE fp64 with one rounding per operation in the same order, and
the host's sqrt is correctly rounded as np.sqrt is, so nothing but equality is expected.

Matrices: both blocks of golden aircraft 0, 37, 97, 150, 200 and 287 open loop, under the restatement's default LQR and as the
filter's Phi (I - L) at dt 0.01 and 0.02; the two golden blocks that need more than 10 sweeps of one deflation; every degenerate case
of modes_numpy.degenerate_cases; and modes_numpy.shift_cases, which take both stages past the exceptional shifts at sweeps 10 and 20
and one matrix to the sweep cap (not converged on both sides, the words the arithmetic left still equal).
"""
import os
import shutil
import subprocess

import numpy as np

import modes_numpy as mo
from conftest import GOLDEN

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLE = (0, 37, 97, 150, 200, 287)


def _matrices():
    bl = mo.golden_blocks(np.load(os.path.join(GOLDEN, "trim_reference.npz")))
    out = []
    for name, M in (("open loop", bl["open"]), ("closed loop", bl["closed"]), ("filter dt 0.01", bl["filter"][0.01]),
                    ("filter dt 0.02", bl["filter"][0.02])):
        out += [(f"aircraft {i} block {b} {name}", M[i, b]) for i in SAMPLE for b in range(2)]
    out += [(f"aircraft {i} block {b} {loop} loop: more than 10 sweeps", bl[loop][i, b]) for loop, i, b in mo.SLOW_GOLDEN]
    return out + mo.degenerate_cases() + [(name, m) for name, m, _, _, _ in mo.shift_cases()]


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def test_every_output_word_equals_the_model_bit_for_bit(tmp_path):
    mats = _matrices()
    fin, fout, exe = str(tmp_path / "matrices.f64"), str(tmp_path / "out.f64"), str(tmp_path / "eig_check")
    np.concatenate([[float(len(mats))]] + [np.asarray(m, np.float64).ravel() for _, m in mats]).tofile(fin)
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler: the CPU oracle cannot be built without one either"
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(REPO, "tests", "host", "eig_check.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    run = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stdout, run.stderr)
    got = np.fromfile(fout, dtype=np.float64).reshape(len(mats), 8 + mo.NMO + 2)
    sweeps, pairs, capped = [], 0, []
    for (name, m), row in zip(mats, got):
        re, im, it, ok = mo.eig4(np.asarray(m) + 0.0)
        assert (it, ok) == (int(row[-2]), bool(row[-1])), (name, it, ok, row[-2:])
        if not ok:
            capped.append(name)
        assert np.array_equal(_bits(row[0:4]), _bits(re)) and np.array_equal(_bits(row[4:8]), _bits(im)), (name, row[:8], re, im)
        assert np.array_equal(_bits(row[8:8 + mo.NMO]), _bits(mo.summary(re, im))), name
        sweeps.append(it)
        pairs += int((im > 0.0).sum())
    assert max(sweeps) == 30 and min(sweeps) == 0 and pairs >= 20           # the file exercises the sweeps and the complex branch
    assert capped == ["weighted cyclic 4 x 4 to the cap"]

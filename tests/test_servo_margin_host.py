"""csrc/fdyn_servo_margin.hpp -- Kc(z), the complex F_c(z), the squaring certificate on the augmented words and the lane's grid loop
and status logic that the servo margin kernel compiles -- run on the host: a stand-alone program (tests/host/servo_margin_check.cpp)
built with the host compiler under AddressSanitizer and UBSan computes the margins of a file of lanes, and every word it writes must
equal the NumPy model's (servo_margin_numpy.loop_margins) BIT FOR BIT.  Both sides are IEEE fp64 with one rounding per operation in
the same order, and the host's sqrt is correctly rounded as np.sqrt is, so nothing but equality is expected.

Lanes: golden aircraft 0, 97, 200 and 287 at dt 0.01 and 0.02 under estimate and truth feedback (both blocks of each, the default
64-point grid); every bad case of servo_margin_numpy.bad_cases under the three feedbacks on a 7-point grid that holds z = (-1, 0);
and a good lane on a 7-point grid that holds z = (1, 0).
"""
import os
import shutil
import subprocess

import numpy as np

import servo_margin_numpy as sm
from conftest import GOLDEN

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lanes():
    d = sm.golden_designs(np.load(os.path.join(GOLDEN, "trim_reference.npz")))
    out = []
    for dt in sm.DTS:
        zre, zim = sm.unit_circle(sm.default_omega(dt), dt)
        for i in (0, 97, 200, 287):
            for fb in (sm.ESTIMATE, sm.TRUTH):
                out.append((f"aircraft {i} dt {dt} feedback {fb}", d["K"][i], d["F"][dt][i], d["x0"][i], dt, fb, zre, zim))
    zre, zim = sm.unit_circle(sm.default_omega(0.01, 7), 0.01)
    for name, K, F, x0, dt, _, _ in sm.bad_cases(d["K"][0], d["F"][0.01][0], d["x0"][0]):
        for fb in (sm.ESTIMATE, sm.TRUTH, sm.MEASUREMENT):
            out.append((f"{name}, feedback {fb}", K, F, x0, dt, fb, zre, zim))
    for fb in (sm.ESTIMATE, sm.TRUTH):
        out.append((f"a grid point at z = 1, feedback {fb}", d["K"][97], d["F"][0.01][97], d["x0"][97], 0.01, fb, *sm.grid_with_one()))
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def test_every_output_word_equals_the_model_bit_for_bit(tmp_path):
    lanes = _lanes()
    fin, fout, exe = str(tmp_path / "lanes.f64"), str(tmp_path / "out.f64"), str(tmp_path / "servo_margin_check")
    np.concatenate([[float(len(lanes))]] + [np.concatenate([[float(fb), float(len(zre)), dt], K, F, x0, zre, zim])
                                            for _, K, F, x0, dt, fb, zre, zim in lanes]).tofile(fin)
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler: the CPU oracle cannot be built without one either"
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(REPO, "tests", "host", "servo_margin_check.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    run = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stdout, run.stderr)
    got = np.fromfile(fout, dtype=np.float64)
    at, seen = 0, set()
    for name, K, F, x0, dt, fb, zre, zim in lanes:
        W = len(zre)
        row, at = got[at:at + 9 + 2 * W], at + 9 + 2 * W
        want = sm.loop_margins(K[None], F[None], x0[None], dt, fb, zre, zim)
        assert int(row[8]) == want["status"][0], (name, row[8], want["status"][0])
        assert np.array_equal(row[2:4].astype(np.int32), want["idx_s"][0]) and np.array_equal(row[6:8].astype(np.int32), want["idx_t"][0]), name
        assert np.array_equal(_bits(row[0:2]), _bits(want["alpha_s"][0])), (name, row[0:2], want["alpha_s"][0])
        assert np.array_equal(_bits(row[4:6]), _bits(want["alpha_t"][0])), (name, row[4:6], want["alpha_t"][0])
        assert np.array_equal(_bits(row[9:]), _bits(want["curve"][0].reshape(-1))), name
        seen.add(int(row[8]))
    assert at == got.size
    assert not got[:16 * (9 + 128)].reshape(16, -1)[:, 8].any()              # the sixteen golden lanes carry the guarantee
    assert {0, sm.NOT_STABLE, sm.BAD_INPUT, sm.SINGULAR} <= seen

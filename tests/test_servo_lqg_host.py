"""csrc/fdyn_kalman_n.hpp -- the Kalman design the servo's filter kernel compiles at N = 5 (the series of the matrix exponential and
of its integral, the dual doubling loop, gain, residual and L D L^T test) -- run on the host: a stand-alone program
(tests/host/servo_lqg_check.cpp) built with the host compiler under AddressSanitizer and UBSan designs a file of blocks, and every
word it writes must equal the NumPy restatement's (servo_lqg_numpy.design_block) BIT FOR BIT.  Both sides are IEEE fp64 with one
rounding per operation in the same order, so nothing but equality is expected (a NaN equals a NaN).
"""
import os
import shutil
import subprocess

import numpy as np

import kf_numpy as kn
import lqr_numpy as ln
import servo_lqg_numpy as sl
from conftest import GOLDEN

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_GOLDEN = 16                                                  # 4 aircraft x 2 blocks x 2 steps


def _blocks():
    """(name, dt, a, b, sigma, rates): both blocks of golden aircraft at both steps, the degenerate ends, and one 4 x 4 block."""
    g = np.load(os.path.join(GOLDEN, "trim_reference.npz"))
    nz = sl.default_noise()
    out = []
    for dt in (0.01, 0.02):
        for i in (0, 97, 200, 287):
            for k, (a, b) in enumerate(sl.blocks(g["A"][i], g["B"][i])):
                out.append((f"aircraft {i} block {k} dt {dt}", dt, a, b, nz[5 * k:5 * k + 5], nz[10 + 5 * k:15 + 5 * k]))
    (a5, b5), (l5, lb5) = sl.blocks(g["A"][0], g["B"][0])
    nan = a5.copy()
    nan[2, 1] = np.nan
    out.append(("a NaN word", 0.01, nan, b5, nz[:5], nz[10:15]))
    sig0 = nz[:5].copy()
    sig0[4] = 0.0
    out.append(("sigma = 0", 0.01, a5, b5, sig0, nz[10:15]))
    big = l5 * (1.6 / (sl.row_norm(l5) * 0.01))                # |a|_inf dt = 1.6: over the kernel's cap, the header itself has none
    out.append(("|a| dt = 1.6", 0.01, big, lb5, nz[5:10], nz[15:20]))
    a4, b4 = ln.blocks(g["A"][0], g["B"][0])[0]                # fdyn_kf_design's own block: the header at N = 4 is kf_numpy
    out.append(("4 x 4", 0.01, a4, b4, np.array(kn.DEFAULT_SIGMA[:4]), np.array(kn.DEFAULT_RATES[:4])))
    return out


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64).ravel(), np.ascontiguousarray(b, np.float64).ravel()
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64))


def test_kalman_header_equals_the_restatement_bit_for_bit(tmp_path):
    blocks = _blocks()
    fin, fout, exe = str(tmp_path / "blocks.f64"), str(tmp_path / "out.f64"), str(tmp_path / "servo_lqg_check")
    words = [[float(len(blocks))]]
    for _, dt, a, b, sigma, rates in blocks:
        words += [[float(len(a)), dt], a.ravel(), b.ravel(), sigma, rates]
    np.concatenate([np.asarray(w, np.float64) for w in words]).tofile(fin)
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler: the CPU oracle cannot be built without one either"
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(REPO, "tests", "host", "servo_lqg_check.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    run = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stdout, run.stderr)
    got = np.fromfile(fout, dtype=np.float64)
    at, seen = 0, {}
    for name, dt, a, b, sigma, rates in blocks:
        N = len(a)
        row = got[at:at + 1 + 3 * N * N + 2 * N + 6]
        at += len(row)
        ref = sl.design_block(a, b, dt, sigma, rates)
        assert _same_bits(row[0], sl.row_norm(a)), name
        p = 1
        for key, size in (("Phi", N * N), ("Gamma", 2 * N), ("L", N * N), ("P", N * N)):
            assert _same_bits(row[p:p + size], ref[key]), (name, key)
            p += size
        assert _same_bits(row[p], ref["residual"]), name
        flags = (int(row[p + 1]), bool(row[p + 2]), bool(row[p + 3]), bool(row[p + 4]), bool(row[p + 5]))
        assert flags == (ref["iters"], ref["failed"], ref["converged"], ref["gain_ok"], ref["positive"]), (name, flags, ref)
        seen[name] = ref
    assert at == len(got)
    golden = [seen[b[0]] for b in blocks[:N_GOLDEN]]
    assert not any(r["status"] for r in golden) and all(1 <= r["iters"] <= 30 for r in golden)       # every golden block is certified
    assert seen["a NaN word"]["status"] & sl.NOT_CONVERGED and seen["sigma = 0"]["status"]
    assert sl.row_norm(blocks[N_GOLDEN + 2][2]) * 0.01 > sl.NORM_MAX                                 # what the kernel refuses
    # at N = 4 the header is fdyn_kf_design's arithmetic: kf_numpy's block, word for word
    name, dt, a, b, sigma, rates = blocks[-1]
    old = kn.design_block(a, b, dt, sigma, rates)
    for key in ("Phi", "Gamma", "L", "P", "residual"):
        assert _same_bits(seen[name][key], old[key]), key
    assert (seen[name]["iters"], seen[name]["status"]) == (old["iters"], old["status"])


def test_bad_inputs_are_refused_by_the_lane_rule():
    """What the kernel adds around the header: a NaN word read, sigma = 0 and |a|_inf dt = 1.6 are BAD_INPUT with the pass-through."""
    g = np.load(os.path.join(GOLDEN, "trim_reference.npz"))
    A, B = g["A"][0].copy(), g["B"][0].copy()
    ok = sl.design(A, B, 0.01, sl.default_noise())
    assert ok["status"] == 0
    nan = A.copy()
    nan[sl.EST_STATES[2], sl.EST_STATES[1]] = np.nan
    zero = sl.default_noise()
    zero[4] = 0.0
    lat = list(sl.EST_STATES[5:])
    big = A.copy()
    big[np.ix_(lat, lat)] *= 1.6 / (sl.row_norm(A[np.ix_(lat, lat)]) * 0.01)
    for r in (sl.design(nan, B, 0.01, sl.default_noise()), sl.design(A, B, 0.01, zero), sl.design(big, B, 0.01, sl.default_noise()),
              sl.design(A, B, 2.0, sl.default_noise()), sl.design(A, B, 1e-7, sl.default_noise())):
        assert r["status"] == sl.BAD_INPUT and r["iters"] == 0 and np.isnan(r["residual"]) and np.array_equal(r["F"], sl.pass_through())

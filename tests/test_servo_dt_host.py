"""csrc/fdyn_servo_dt.hpp -- the sampled-data servo design the kernel of servo_dt_kernels.hip runs per lane (discretisation, sampled
model, doubling loop, 2 x 2 inverse, gain, residual, L D L^T test and the squaring certificate) -- run on the host: a stand-alone
program (tests/host/servo_dt_check.cpp) built with the host compiler under AddressSanitizer and UBSan designs a 12-aircraft cut of
tests/golden/servo_dt_reference.npz at both recorded steps, and what it writes is compared with the restatement's recorded words:
status and iteration counts equal, K within 1e-9 max(1, |K|) (the gate of test_gpu_servo._assert_matches).  A few refused lanes ride
along: the status the restatement gives them, K = 0.
"""
import os
import shutil
import subprocess

import numpy as np

import servo_dt_numpy as sd
import servo_numpy as sn
from conftest import GOLDEN

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUT = tuple(range(0, 288, 24))                                   # 12 aircraft across both airframes


def _lanes():
    """(name, dt, A, B, x0, weights, want dict(K, iters, status)): the cut at both dt from the fixture, then refused lanes."""
    g = np.load(os.path.join(GOLDEN, "trim_reference.npz"))
    fx = np.load(os.path.join(GOLDEN, "servo_dt_reference.npz"))
    w = sn.default_weights()
    out = []
    for dt in sd.DTS:
        tag = f"dt{dt:g}".replace(".", "p")
        for i in CUT:
            out.append((f"aircraft {i} at dt {dt}", dt, g["A"][i], g["B"][i], g["x0"][i], w,
                        dict(K=fx[f"{tag}_K"][i], iters=int(fx[f"{tag}_iters"][i]), status=int(fx[f"{tag}_status"][i]))))
    i = CUT[3]
    bad_w, bad_a, still = w.copy(), g["A"][i].copy(), g["x0"][i].copy()
    bad_w[5], bad_a[5, 3], still[sn.X_U], still[sn.X_W] = np.nan, np.nan, 0.0, 0.0
    for name, dt, A, x0, ww in (("a NaN weight", 0.02, g["A"][i], g["x0"][i], bad_w), ("a NaN word of A", 0.02, bad_a, g["x0"][i], w),
                                ("V0 = 0", 0.02, g["A"][i], still, w), ("|a| dt over the series cap", 0.05, 40.0 * g["A"][i], g["x0"][i], w)):
        ref = sd.design(A, g["B"][i], x0, ww, dt)
        assert ref["status"] == sd.BAD_INPUT, name
        out.append((name, dt, A, g["B"][i], x0, ww, ref))
    return out


def test_header_on_the_host_matches_the_restatement(tmp_path):
    lanes = _lanes()
    fin, fout, exe = str(tmp_path / "lanes.f64"), str(tmp_path / "out.f64"), str(tmp_path / "servo_dt_check")
    words = [[float(len(lanes))]]
    for _, dt, A, B, x0, w, _ in lanes:
        words += [[dt], np.ravel(A), np.ravel(B), x0, w]
    np.concatenate([np.asarray(v, np.float64) for v in words]).tofile(fin)
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler: the CPU oracle cannot be built without one either"
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(REPO, "tests", "host", "servo_dt_check.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    run = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stdout, run.stderr)
    got = np.fromfile(fout, dtype=np.float64).reshape(len(lanes), sn.NSVK + 3)
    worst, exact = 0.0, 0
    for row, (name, dt, _, _, _, _, want) in zip(got, lanes):
        assert (int(row[-1]), int(row[-2])) == (want["status"], want["iters"]), (name, row[-2:], want)
        err = np.abs(row[:sn.NSVK] - want["K"]) / np.maximum(1.0, np.abs(want["K"]))
        worst, exact = max(worst, float(err.max())), exact + int((row[:sn.NSVK] == want["K"]).sum())
        assert err.max() <= 1e-9, (name, err.max())
        if want["status"]:
            assert not row[:sn.NSVK].any() and np.isnan(row[-3]) and row[-2] == 0.0, name
        else:
            assert row[-3] <= 1e-10, (name, row[-3])
    print(f"host build against the restatement: worst K deviation {worst:.3e}, exact in {exact} of {got[:, :sn.NSVK].size} words")
    assert not any(want["status"] for *_, want in lanes[:2 * len(CUT)])          # the cut is certified at both steps

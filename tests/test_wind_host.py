"""csrc/fdyn_wind.hpp -- the air-relative body velocity and the gust update the servo's wind entries add to the servo step -- run on
the host: a stand-alone program (tests/host/wind_check.cpp) built with the host compiler under AddressSanitizer and UBSan works
through a file of records, and every word it writes must equal the NumPy restatement's (servo_wind_numpy.air_relative_sc,
gust_update) BIT FOR BIT.  Both sides are IEEE arithmetic with one rounding per operation in the same order (contraction off), in
fp64 and in fp32, so nothing but equality is expected.  The sines and cosines are inputs: the two sides' libraries may differ.
"""
import os
import shutil
import subprocess

import numpy as np

import servo_wind_numpy as wn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _records():
    """[count][20]: v [3], sin / cos of roll, pitch, yaw [6], W [3], g [3], A, B, n [3]; the named ends first, then random ones."""
    rs = np.random.RandomState(3)

    def rec(v=(20.0, 0.5, 1.5), ang=(0.3, 0.1, 2.0), W=(3.0, -4.0, 0.5), g=(0.4, -0.3, 0.2), A=0.99, B=0.14, n=(0.5, -1.2, 2.0)):
        sc = [f(a) for a in ang for f in (np.sin, np.cos)]
        return np.array([*v, *sc, *W, *g, A, B, *n], np.float64)

    named = [("zero wind", rec(W=(0.0, 0.0, 0.0), g=(0.0, 0.0, 0.0), B=0.0)),
             ("zero wind, negative zeros", rec(W=(-0.0, 0.0, -0.0), g=(-0.0, -0.0, 0.0), B=0.0)),
             ("a NaN row", rec(W=(np.nan, 1.0, 0.0), g=(np.nan, 0.0, 1.0))),
             ("A = 1, B = 0: the gust holds", rec(A=1.0, B=0.0)),
             ("A = 0: white noise", rec(A=0.0, B=1.5)),
             ("an infinite normal", rec(n=(np.inf, -np.inf, 0.0)))]
    for k in range(200):
        named.append((f"random {k}", rec(v=rs.normal(0, 15, 3), ang=rs.uniform(-3.1, 3.1, 3), W=rs.normal(0, 8, 3), g=rs.normal(0, 2, 3),
                                         A=rs.uniform(0, 1), B=rs.uniform(0, 2), n=rs.standard_normal(3))))
    return named


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def test_wind_header_equals_the_restatement_bit_for_bit(tmp_path):
    recs = _records()
    fin, fout, exe = str(tmp_path / "records.f64"), str(tmp_path / "out.f64"), str(tmp_path / "wind_check")
    np.concatenate([[float(len(recs))]] + [r for _, r in recs]).tofile(fin)
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler: the CPU oracle cannot be built without one either"
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(REPO, "tests", "host", "wind_check.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    run = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stdout, run.stderr)
    got = np.fromfile(fout, dtype=np.float64).reshape(len(recs), 9)
    for (name, r), row in zip(recs, got):
        with np.errstate(all="ignore"):
            a64 = wn.air_relative_sc(r[0:3], r[3:9], r[9:12])
            r32 = r.astype(np.float32)
            a32 = r32[0:3] - wn.body_wind_sc(*r32[3:9], r32[9:12])
            g = wn.gust_update(r[12:15], r[15], r[16], r[17:20])
        assert a32.dtype == np.float32
        assert np.array_equal(_bits(row[0:3]), _bits(a64)), name
        assert np.array_equal(_bits(row[3:6].astype(np.float32)), _bits(a32)), name
        assert np.array_equal(_bits(row[6:9]), _bits(g)), name
    # what the named ends are there for
    by = {name: row for (name, _), row in zip(recs, got)}
    r0 = recs[0][1]
    assert np.array_equal(_bits(by["zero wind"][0:3]), _bits(r0[0:3])) and not by["zero wind"][6:9].any()       # v comes back, g stays 0
    assert np.array_equal(by["zero wind, negative zeros"][0:3], r0[0:3])
    assert np.isnan(by["a NaN row"][0:3]).all() and np.isnan(by["a NaN row"][6]) and np.isfinite(by["a NaN row"][7:9]).all()
    assert np.array_equal(_bits(by["A = 1, B = 0: the gust holds"][6:9]), _bits(np.array([0.4, -0.3, 0.2])))
    assert np.array_equal(by["A = 0: white noise"][6:9], 1.5 * np.array([0.5, -1.2, 2.0]))

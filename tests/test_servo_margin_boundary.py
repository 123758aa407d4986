"""CPU-side checks of the servo margins' boundary: include/fdyn_servo_margins.h parses under the strict header parser into a table of
its own of exactly one entry, the built library exports and `_lib.load()` binds it, the six older tables are what they were, every
refused call returns its code before anything is launched, and `servo_margins_into` refuses host tensors and wrong shapes or dtypes.
No compute calls (there is no GPU in the build container)."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

from conftest import REPO
from hcrl_amd import _lib, layout as L

_P, _I, _I64, _D = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double
NAME = "fdyn_servo_loop_margins"


def _header():
    return open(os.path.join(REPO, "include", "fdyn_servo_margins.h")).read()


def test_header_parses_into_its_own_table():
    table, consts = _lib._parse_header(_header(), "include/fdyn_servo_margins.h")
    assert table == _lib.SERVO_MARGIN_SIGNATURES and consts == {}
    assert list(table) == [NAME] and len(table) == 1
    #                        K   F   x0  dt  fb  zre zim n_omega n    a_s i_s a_t i_t curve status stream
    assert table[NAME] == (_I, [_P, _P, _P, _D, _I, _P, _P, _I, _I64, _P, _P, _P, _P, _P, _P, _P])
    # fdyn_loop_margins' list with x0 and dt put in: the same outputs in the same order
    old = _lib.SIGNATURES["fdyn_loop_margins"][1]
    assert table[NAME][1][-9:] == old[-9:]
    older = (_lib.SIGNATURES, _lib.MODES_SIGNATURES, _lib.SERVO_SIGNATURES, _lib.MISSION_SIGNATURES, _lib.WIND_SIGNATURES, _lib.SERVO_LQG_SIGNATURES)
    assert tuple(len(t) for t in older) == (82, 2, 4, 3, 6, 5)
    assert not any(set(table) & set(t) for t in older)
    assert "oracle" not in _header().lower()


def test_library_exports_and_binds_the_prototype():
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call([sys.executable, "-c", "import __graft_entry__ as g; g.build()"], cwd=REPO)
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert set(re.findall(r"\b(?:int|int64_t)\s+(fdyn_\w+)\s*\(", src)) == {NAME}
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME), f"{NAME} declared in include/fdyn_servo_margins.h but not exported"
    fn = getattr(_lib.load(), NAME)
    res, args = _lib.SERVO_MARGIN_SIGNATURES[NAME]
    assert fn.restype is res and list(fn.argtypes) == args


def test_constants_are_mirrored():
    import servo_margin_numpy as sm
    import servo_numpy as sn
    assert (sm.NOT_STABLE, sm.SINGULAR, sm.BAD_INPUT) == (L.FD_MRG_NOT_STABLE, L.FD_MRG_SINGULAR, L.FD_MRG_BAD_INPUT) == (1, 2, 4)
    assert (sm.ESTIMATE, sm.MEASUREMENT, sm.TRUTH) == (L.FD_LQG_ESTIMATE, L.FD_LQG_MEASUREMENT, L.FD_LQG_TRUTH)
    assert sm.K_AT == (L.FD_SVK_LON, L.FD_SVK_LAT) and sm.N == L.FD_SK_NB and sn.NSVK == L.FD_NSVK == 26
    assert sm.PHI == (L.FD_SKF_PHI_LON, L.FD_SKF_PHI_LAT) and sm.GAMMA == (L.FD_SKF_GAMMA_LON, L.FD_SKF_GAMMA_LAT)
    assert sm.LG == (L.FD_SKF_L_LON, L.FD_SKF_L_LAT) and L.FD_NSKF == 120
    assert (sn.X_U, sn.X_W) == (L.FD_X_U, L.FD_X_W)
    from hcrl_amd import margins as M, servo_margins as SM
    assert SM.LoopMargins is M.LoopMargins and SM.default_grid is M.default_grid and SM.unit_circle is M.unit_circle
    assert sm.MAX_OMEGA == SM.MAX_OMEGA == 256


def test_refused_calls_need_no_device():
    """FDYN_ERR_BAD_SIZE for n_omega outside 1..256, an unknown feedback and n < 1, FDYN_ERR_NULL for every required pointer: each
    with no launch (the pointers are never dereferenced)."""
    fn = getattr(_lib.load(), NAME)
    one = ctypes.c_void_p(8)
    #       K    F    x0   dt    fb zre  zim  n_omega n  a_s  i_s  a_t  i_t  curve status stream
    call = [one, one, one, 0.01, 0, one, one, 64, 5, one, one, one, one, None, one, None]

    def with_(at, v):
        args = list(call)
        args[at] = v
        return args

    for n_omega in (0, 257, -1):
        assert fn(*with_(7, n_omega)) == _lib.FDYN_ERR_BAD_SIZE
    for fb in (-1, 3):
        assert fn(*with_(4, fb)) == _lib.FDYN_ERR_BAD_SIZE
    for n in (0, -1, 1 << 31):
        assert fn(*with_(8, n)) == _lib.FDYN_ERR_BAD_SIZE
    for hole in (0, 1, 2, 5, 6, 9, 10, 11, 12, 14):
        assert fn(*with_(hole, None)) == _lib.FDYN_ERR_NULL, hole
    args = with_(0, None)                                                 # sizes before pointers
    args[8] = 0
    assert fn(*args) == _lib.FDYN_ERR_BAD_SIZE


def _report(n, curve=None):
    a, i = torch.zeros((2, n), dtype=torch.float64), torch.zeros((2, n), dtype=torch.int32)
    from hcrl_amd.margins import LoopMargins
    return LoopMargins(a, i, a.clone(), i.clone(), torch.zeros(n, dtype=torch.int32), curve)


def test_servo_margins_into_refuses_wrong_arguments():
    from hcrl_amd import servo_margins as SM
    f64 = torch.float64
    K, F, x0, z = torch.zeros((26, 3), dtype=f64), torch.zeros((120, 3), dtype=f64), torch.zeros((12, 3), dtype=f64), torch.zeros(8, dtype=f64)
    big = torch.zeros(257, dtype=f64)
    for args in ((K[:25], F, x0, 0.01, z, z), (K, F[:, :2], x0, 0.01, z, z), (K, F[:80], x0, 0.01, z, z), (K, F, x0[:11], 0.01, z, z),
                 (K, F, x0, 0.01, z, z[:7]), (K, F, x0, 0.01, z[:0], z[:0]), (K, F, x0, 0.01, big, big), (K.float(), F, x0, 0.01, z, z),
                 (K, F, x0.float(), 0.01, z, z), (K, F, x0, 0.01, z.float(), z.float()), (K, F, x0, 0.01, z.reshape(2, 4), z.reshape(2, 4)),
                 (K[:, :0], F[:, :0], x0[:, :0], 0.01, z, z)):
        with pytest.raises(ValueError):
            SM.servo_margins_into(*args)
    with pytest.raises(ValueError, match="on the GPU"):                  # host tensors, everything else in order
        SM.servo_margins_into(K, F, x0, 0.01, z, z)
    meta = torch.device("meta")
    for args in ((K, F.to(meta), x0, z, z), (K, F, x0.to(meta), z, z), (K, F, x0, z.to(meta), z), (K, F, x0, z, z.to(meta)), (K.to(meta), F, x0, z, z)):
        with pytest.raises(ValueError, match="one device"):
            SM.servo_margins_into(*args[:3], 0.01, *args[3:])
    with pytest.raises(ValueError, match="feedback"):
        SM.servo_margins_into(K, F, x0, 0.01, z, z, "guess")
    with pytest.raises(ValueError, match="feedback"):
        SM.servo_margins_into(K, F, x0, 0.01, z, z, 3)
    # a caller's report: size, dtype, shape, device and contiguity of every word, and a curve where one is asked for
    with pytest.raises(ValueError, match="cannot take"):
        SM.servo_margins_into(K, F, x0, 0.01, z, z, "truth", _report(2))
    with pytest.raises(ValueError, match="cannot take"):
        SM.servo_margins_into(K, F, x0, 0.01, z, z, "truth", _report(3, torch.zeros((2, 7, 3), dtype=f64)))
    with pytest.raises(ValueError, match="needs a report that has a curve"):
        SM.servo_margins_into(K, F, x0, 0.01, z, z, "truth", _report(3), curve=True)
    for name, bad in (("alpha_s", torch.zeros((2, 3))), ("idx_t", torch.zeros((2, 3), dtype=torch.int64)), ("alpha_t", torch.zeros((2, 3), dtype=f64, device=meta)),
                      ("idx_s", torch.zeros((3, 2), dtype=torch.int32).T), ("alpha_s", torch.zeros((3, 3), dtype=f64))):
        r = _report(3)
        setattr(r, name, bad)
        with pytest.raises(ValueError, match=f"out.{name}"):
            SM.servo_margins_into(K, F, x0, 0.01, z, z, "truth", r)
    with pytest.raises(ValueError, match="on the GPU"):                  # a good report on the host: still refused, nothing launched
        SM.servo_margins_into(K, F, x0, 0.01, z, z, "truth", _report(3, torch.zeros((2, 8, 3), dtype=f64)), curve=True)


def test_fleet_guards_need_no_device():
    from hcrl_amd.fleet import BatchedCascade, BatchedSixDOF
    from hcrl_amd.hybrid import HybridFleet
    assert HybridFleet.servo_loop_margins is BatchedSixDOF.servo_loop_margins and BatchedCascade.servo_loop_margins is BatchedSixDOF.servo_loop_margins
    fleet = BatchedSixDOF.__new__(BatchedSixDOF)
    fleet.n = 3
    with pytest.raises(ValueError, match=r"3 of 3 aircraft have no certified stabilising servo gain \(call \.design_servo\(\) first\)"):
        fleet.servo_loop_margins()
    fleet._servo = object()
    with pytest.raises(ValueError, match=r"3 of 3 aircraft have no certified stable servo filter \(call \.design_servo_kalman\(dt\) first\)"):
        fleet.servo_loop_margins()

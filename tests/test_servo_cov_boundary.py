"""CPU-side checks of the servo covariance report's boundary: include/fdyn_servo_covariance.h parses under the strict header parser
into a table of its own of exactly two entries, the built library exports and `_lib.load()` binds them, the nine older tables are
what they were and share no name with it, the layout constants agree between header, layout.py and the restatement, every refused
call returns its code in the documented order before anything is launched, and the host functions refuse host tensors, wrong
shapes and dtypes.  No compute calls (there is no GPU in the build container)."""
import ctypes
import math
import os
import re
import subprocess
import sys

import pytest
import torch

from conftest import REPO
from hcrl_amd import _lib, layout as L

_P, _I, _I64, _D = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double
NAMES = ("fdyn_servo_covariance", "fdyn_stein_solve")


def _header():
    return open(os.path.join(REPO, "include", "fdyn_servo_covariance.h")).read()


def test_header_parses_into_its_own_table():
    table, consts = _lib._parse_header(_header(), "include/fdyn_servo_covariance.h")
    assert table == _lib.SERVO_COVARIANCE_SIGNATURES and consts == {}
    assert tuple(table) == NAMES
    # K, F, x0, dt, sigma, sigma_per_lane, w_rate, w_rate_per_lane, feedback, n, report, cov, residual, iters, status, stream
    assert table[NAMES[0]] == (_I, [_P, _P, _P, _D, _P, _I, _P, _I, _I, _I64, _P, _P, _P, _P, _P, _P])
    # A, B, Q, N, M, n, X, residual, iters, status, stream
    assert table[NAMES[1]] == (_I, [_P, _P, _P, _I, _I, _I64, _P, _P, _P, _P, _P])
    older = (_lib.SIGNATURES, _lib.MODES_SIGNATURES, _lib.SERVO_SIGNATURES, _lib.MISSION_SIGNATURES, _lib.WIND_SIGNATURES, _lib.SERVO_LQG_SIGNATURES,
             _lib.SERVO_MARGIN_SIGNATURES, _lib.SERVO_MODES_SIGNATURES, _lib.SERVO_LQG_MISSION_SIGNATURES)
    assert tuple(len(t) for t in older[:8]) == (82, 2, 4, 3, 6, 5, 1, 4)
    assert not any(set(table) & set(t) for t in older)
    assert "oracle" not in _header().lower()


def test_library_exports_and_binds_every_prototype():
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call([sys.executable, "-c", "import __graft_entry__ as g; g.build()"], cwd=REPO)
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert set(re.findall(r"\b(?:int|int64_t)\s+(fdyn_\w+)\s*\(", src)) == set(NAMES)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), f"{name} declared in include/fdyn_servo_covariance.h but not exported"
        fn = getattr(_lib.load(), name)
        res, args = _lib.SERVO_COVARIANCE_SIGNATURES[name]
        assert fn.restype is res and list(fn.argtypes) == args


def test_constants_are_mirrored():
    import servo_cov_numpy as sc
    assert (L.FD_SCV_VAR_X, L.FD_SCV_VAR_EST, L.FD_SCV_VAR_ERR, L.FD_SCV_VAR_INTEG, L.FD_SCV_VAR_U, L.FD_SCV_VAR_DU, L.FD_NSCV) == \
        (sc.VAR_X, sc.VAR_EST, sc.VAR_ERR, sc.VAR_INTEG, sc.VAR_U, sc.VAR_DU, sc.NSCV) == (0, 10, 20, 23, 26, 30, 34)
    assert ((L.FD_SCC_E_LON, L.FD_SCC_E_LAT), (L.FD_SCC_XE_LON, L.FD_SCC_XE_LAT), (L.FD_SCC_X_LON, L.FD_SCC_X_LAT), L.FD_NSCC) == \
        (sc.CC_E, sc.CC_XE, sc.CC_X, sc.NSCC)
    nb, na = L.FD_SK_NB, (L.FD_SV_NLON, L.FD_SV_NLAT)
    assert L.FD_NSCC == 2 * nb * nb + sum(a * nb for a in na) + sum(a * a for a in na) == 200
    assert L.FD_SCV_VAR_EST - L.FD_SCV_VAR_X == L.FD_NSKX and L.FD_NSCV - L.FD_SCV_VAR_DU == L.FD_NU
    assert (L.FD_SCV_NOT_CONVERGED, L.FD_SCV_UNSTABLE, L.FD_SCV_BAD_INPUT) == (sc.NOT_CONVERGED, sc.UNSTABLE, sc.BAD_INPUT) == (1, 2, 4)
    assert (L.FD_SCV_MIN_N, L.FD_SCV_MAX_N) == (sc.MIN_N, sc.MAX_N) == (1, 7)
    assert (sc.ESTIMATE, sc.MEASUREMENT, sc.TRUTH) == (L.FD_LQG_ESTIMATE, L.FD_LQG_MEASUREMENT, L.FD_LQG_TRUTH)
    assert sc.CONTROLS == ((L.FD_U_ELEVATOR, L.FD_U_THROTTLE), (L.FD_U_AILERON, L.FD_U_RUDDER))
    for name in ("FD_SCV_VAR_DU", "FD_NSCV", "FD_SCC_X_LAT", "FD_NSCC", "FD_SCV_UNSTABLE", "FD_SCV_MAX_N"):
        assert re.search(rf"\b{name}\b", _header()) and name in L.__all__
    # the solver's constants, header text against restatement
    hpp = open(os.path.join(REPO, "hybrid-classical-and-reinforcement-learning-aircraft-controllers_amd", "csrc", "fdyn_stein_n.hpp")).read()
    assert f"STEIN_MAX_DOUBLINGS = {sc.MAX_DOUBLINGS};" in hpp and "STEIN_TOL = 1e-17;" in hpp and "STEIN_RES_MAX = 1e-9;" in hpp
    assert (sc.MAX_DOUBLINGS, sc.STEIN_TOL, sc.RES_MAX) == (40, 1e-17, 1e-9)
    from hcrl_amd import servo_covariance as SC
    assert SC.describe_status(0) == "ok" and "not certified stable" in SC.describe_status(L.FD_SCV_UNSTABLE)
    assert SC.CONTROL_LOW[L.FD_U_THROTTLE] == 0.0 and SC.CONTROL_LOW[L.FD_U_ELEVATOR] == -1.0 and set(SC.CONTROL_HIGH) == {1.0}


def test_refused_calls_need_no_device():
    """FDYN_ERR_BAD_SIZE (n < 1, an unknown feedback, N or M outside 1 .. 7), then FDYN_ERR_NULL, then FDYN_ERR_BAD_DT: each with no
    launch (the pointers are never dereferenced).  cov, iters and w_rate may be NULL."""
    lib = _lib.load()
    one = ctypes.c_void_p(8)
    #       K    F    x0   dt    sigma pl w_rate pl fb n  report cov   resid iters status stream
    good = [one, one, one, 0.01, one, 0, None, 0, 0, 5, one, None, one, None, one, None]
    fn = lib.fdyn_servo_covariance

    def with_(at, v, call=good):
        args = list(call)
        args[at] = v
        return args
    for n in (0, -1, 1 << 31):
        assert fn(*with_(9, n)) == _lib.FDYN_ERR_BAD_SIZE, n
    for fb in (-1, 3, 99):
        assert fn(*with_(8, fb)) == _lib.FDYN_ERR_BAD_SIZE, fb
    for hole in (0, 1, 2, 4, 10, 12, 14):
        assert fn(*with_(hole, None)) == _lib.FDYN_ERR_NULL, hole
    for dt in (0.0, 1e-6, 1.5, -0.01, float("nan")):
        assert fn(*with_(3, dt)) == _lib.FDYN_ERR_BAD_DT, dt
    # the order: size before pointer before dt
    assert fn(*with_(9, 0, with_(0, None, with_(3, 0.0)))) == _lib.FDYN_ERR_BAD_SIZE
    assert fn(*with_(8, 7, with_(0, None))) == _lib.FDYN_ERR_BAD_SIZE
    assert fn(*with_(0, None, with_(3, 0.0))) == _lib.FDYN_ERR_NULL

    #        A    B    Q    N  M  n  X    resid iters status stream
    sgood = [one, one, one, 7, 5, 5, one, None, None, one, None]
    fs = lib.fdyn_stein_solve
    for n in (0, -1, 1 << 31):
        assert fs(*with_(5, n, sgood)) == _lib.FDYN_ERR_BAD_SIZE, n
    for at in (3, 4):
        for size in (0, 8, -2):
            assert fs(*with_(at, size, sgood)) == _lib.FDYN_ERR_BAD_SIZE, (at, size)
    for hole in (0, 1, 2, 6, 9):
        assert fs(*with_(hole, None, sgood)) == _lib.FDYN_ERR_NULL, hole
    assert fs(*with_(3, 9, with_(0, None, sgood))) == _lib.FDYN_ERR_BAD_SIZE


def test_host_functions_refuse_wrong_arguments():
    from hcrl_amd import servo_covariance as SC
    f64, meta, n = torch.float64, torch.device("meta"), 3
    K, F, x0 = torch.zeros((26, n), dtype=f64), torch.zeros((120, n), dtype=f64), torch.zeros((12, n), dtype=f64)
    sigma = torch.full((10,), 0.1, dtype=f64)
    for bad in ((K[:25], F, x0, 0.01, sigma), (K, F[:80], x0, 0.01, sigma), (K, F, x0[:, :2], 0.01, sigma), (K.float(), F, x0, 0.01, sigma),
                (K, F, x0, 0.01, sigma[:9]), (K, F, x0, 0.01, torch.zeros((10, n + 1), dtype=f64)), (K, F, x0, 0.01, None),
                (K[:, :0], F[:, :0], x0[:, :0], 0.01, sigma), (K, F, x0, 0.01, sigma.float())):
        with pytest.raises(ValueError):
            SC.servo_covariance_into(*bad)
    with pytest.raises(ValueError, match="w_rate"):
        SC.servo_covariance_into(K, F, x0, 0.01, sigma, torch.zeros((9,), dtype=f64))
    with pytest.raises(ValueError, match="feedback must be one of"):
        SC.servo_covariance_into(K, F, x0, 0.01, sigma, None, "open")
    with pytest.raises(ValueError, match="expected a tensor on"):
        SC.servo_covariance_into(K, F.to(meta), x0, 0.01, sigma)
    with pytest.raises(ValueError, match="on the GPU"):                  # host tensors, everything else in order
        SC.servo_covariance_into(K, F, x0, 0.01, sigma)
    with pytest.raises(ValueError, match="on the GPU"):
        SC.servo_covariance_into(K, F, x0, 0.01, sigma, out=SC.empty(n, "cpu"))
    for name, bad in (("report", torch.zeros((34, n))), ("cov", torch.zeros((200, n + 1), dtype=f64)), ("residual", torch.zeros(2 * n, dtype=f64)[::2]),
                      ("iterations", torch.zeros(n, dtype=torch.int64)), ("status", torch.zeros(n, dtype=torch.int32, device=meta))):
        r = SC.empty(n, "cpu")
        setattr(r, name, bad)
        with pytest.raises(ValueError, match=f"out.{name}"):
            SC.servo_covariance_into(K, F, x0, 0.01, sigma, out=r)
    A, B, Q = torch.zeros((7, 7, n), dtype=f64), torch.zeros((5, 5, n), dtype=f64), torch.zeros((7, 5, n), dtype=f64)
    for bad in ((A[:6], B, Q), (A, B, Q[:, :4]), (torch.zeros((8, 8, n), dtype=f64), B, torch.zeros((8, 5, n), dtype=f64)), (A.float(), B, Q),
                (A[..., 0], B[..., 0], Q[..., 0]), (A[..., :0], B[..., :0], Q[..., :0])):
        with pytest.raises(ValueError):
            SC.stein_solve(*bad)
    with pytest.raises(ValueError, match="on the GPU"):
        SC.stein_solve(A, B, Q)


def test_a_design_without_sigma_is_refused_not_given_a_default():
    """servo_covariance takes the noise the loop applies from the Kalman design; a design that carries none (one made by
    servo_kalman_into, whose caller never set `.sigma`) is refused instead of being given the sensor defaults."""
    from types import SimpleNamespace
    from hcrl_amd import servo_covariance as SC
    f64, n = torch.float64, 3
    servo = SimpleNamespace(n=n, K=torch.zeros((26, n), dtype=f64), x0=torch.zeros((12, n), dtype=f64))
    kalman = SimpleNamespace(n=n, F=torch.zeros((120, n), dtype=f64), dt=0.01, sigma=None)
    with pytest.raises(ValueError, match="carries no measurement noise"):
        SC.servo_covariance(servo, kalman)
    with pytest.raises(ValueError, match="on the GPU"):                  # with a sigma given it goes on to the launch's own checks
        SC.servo_covariance(servo, kalman, sigma=torch.full((10,), 0.1, dtype=f64))
    kalman.sigma = torch.full((10,), 0.1, dtype=f64)
    with pytest.raises(ValueError, match="on the GPU"):
        SC.servo_covariance(servo, kalman)
    with pytest.raises(ValueError, match="designed at dt"):
        SC.servo_covariance(servo, kalman, dt=0.02)


def test_helpers_follow_their_definitions_on_the_host():
    from hcrl_amd import servo_covariance as SC
    r = SC.empty(2, "cpu")
    r.report[:] = torch.arange(34, dtype=torch.float64)[:, None] * torch.tensor([1.0, 4.0], dtype=torch.float64)[None, :]
    assert torch.equal(r.rms_state(), torch.sqrt(r.report[0:10])) and torch.equal(r.rms_estimate_error(), torch.sqrt(r.report[10:20]))
    assert torch.equal(r.rms_tracking(), torch.sqrt(r.report[20:23])) and torch.equal(r.rms_integrators(), torch.sqrt(r.report[23:26]))
    assert torch.equal(r.rms_control(), torch.sqrt(r.report[26:30])) and torch.equal(r.chatter(), r.report[30:34])
    est, ch = r.expected_accumulators(3000)
    assert torch.equal(est, r.report[10:20] * 3000.0) and torch.equal(ch, r.report[30:34] * 3000.0)
    u0 = torch.tensor([[0.0, 0.5], [-0.75, 0.0], [0.25, 0.0], [0.25, 0.9]], dtype=torch.float64)
    h = r.headroom(u0)
    assert h[0, 0] == 1.0 / math.sqrt(26.0) and h[1, 0] == 0.25 / math.sqrt(27.0) and h[3, 0] == 0.25 / math.sqrt(29.0)
    assert torch.allclose(h[3, 1], torch.tensor(0.1 / (4 * 29.0) ** 0.5, dtype=torch.float64), rtol=1e-14, atol=0.0)
    with pytest.raises(ValueError, match="u0"):
        r.headroom(u0[:3])
    se, sxe, sx = r.matrices(0)
    assert se.shape == (5, 5, 2) and sxe.shape == (7, 5, 2) and sx.shape == (7, 7, 2) and sx.data_ptr() == r.cov[115:].data_ptr()
    se, sxe, sx = r.matrices(1)
    assert sxe.shape == (6, 5, 2) and sx.shape == (6, 6, 2) and se.data_ptr() == r.cov[25:].data_ptr()
    with pytest.raises(ValueError, match="block must be"):
        r.matrices(2)


def test_fleet_guards_need_no_device():
    from hcrl_amd.fleet import BatchedCascade, BatchedSixDOF
    from hcrl_amd.hybrid import HybridFleet
    assert HybridFleet.servo_covariance is BatchedSixDOF.servo_covariance and BatchedCascade.servo_covariance is BatchedSixDOF.servo_covariance
    fleet = BatchedSixDOF.__new__(BatchedSixDOF)
    fleet.n = 3
    with pytest.raises(ValueError, match=r"3 of 3 aircraft have no certified stabilising servo gain \(call \.design_servo\(\) first\)"):
        fleet.servo_covariance()
    fleet._servo = object()
    with pytest.raises(ValueError, match=r"3 of 3 aircraft have no certified stable servo filter \(call \.design_servo_kalman\(dt\) first\)"):
        fleet.servo_covariance("truth")

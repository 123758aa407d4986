"""CPU-side checks of the servo estimator's boundary: include/fdyn_servo_lqg.h parses under the strict header parser into a table of
its own of exactly five entries, the built library exports and `_lib.load()` binds them, the five older tables are what they were,
the new constants are mirrored, every refused call returns its code before anything is launched, and the host layer's classes are
plain torch wherever their tensors live.  No compute calls (there is no GPU in the build container)."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO
from hcrl_amd import _lib, layout as L

_P, _I, _I64, _U64, _D = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_uint64, ctypes.c_double
STEPS = ("fdyn_servo_lqg_step_f64", "fdyn_servo_lqg_step_mixed", "fdyn_servo_lqg_step_f32", "fdyn_servo_lqg_step_f64_lds")
DESIGN = "fdyn_servo_kf_design"
TAIL = [_P, _P, _P, _P, _U64, _P, _P, _I, _P, _P, _P, _P, _P]    # F sigma xhat du_prev seed step z feedback, four optional, stream


def _header():
    return open(os.path.join(REPO, "include", "fdyn_servo_lqg.h")).read()


def test_header_parses_into_its_own_table():
    table, consts = _lib._parse_header(_header(), "include/fdyn_servo_lqg.h")
    assert table == _lib.SERVO_LQG_SIGNATURES and consts == {}
    assert set(table) == set(STEPS) | {DESIGN} and len(table) == 5
    for name in STEPS:                                                    # fdyn_servo_step_*'s list, its stream replaced by the group
        assert table[name] == (_I, _lib.SERVO_SIGNATURES[name.replace("_lqg", "").replace("_lds", "")][1][:-1] + TAIL), name
    assert table[DESIGN] == _lib.SIGNATURES["fdyn_kf_design"]             # fdyn_kf_design's list
    older = (_lib.SIGNATURES, _lib.MODES_SIGNATURES, _lib.SERVO_SIGNATURES, _lib.MISSION_SIGNATURES, _lib.WIND_SIGNATURES)
    assert tuple(len(t) for t in older) == (82, 2, 4, 3, 6)
    assert not any(set(table) & set(t) for t in older)
    assert "oracle" not in _header().lower()


def test_library_exports_and_binds_every_prototype():
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call([sys.executable, "-c", "import __graft_entry__ as g; g.build()"], cwd=REPO)
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = set(re.findall(r"\b(?:int|int64_t)\s+(fdyn_\w+)\s*\(", src))
    assert declared == set(STEPS) | {DESIGN}
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(raw, name), f"{name} declared in include/fdyn_servo_lqg.h but not exported"
    lib = _lib.load()
    for name, (res, args) in _lib.SERVO_LQG_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name


def test_constants_are_mirrored():
    import servo_lqg_numpy as sl
    assert (L.FD_SKN_SIGMA, L.FD_SKN_RATE, L.FD_NSKN) == (0, 10, 20) == (0, sl.NSKX, sl.NSKN)
    assert (L.FD_SKF_PHI_LON, L.FD_SKF_PHI_LAT, L.FD_SKF_GAMMA_LON, L.FD_SKF_GAMMA_LAT, L.FD_SKF_L_LON, L.FD_SKF_L_LAT, L.FD_NSKF) == \
        (sl.PHI_LON, sl.PHI_LAT, sl.GAMMA_LON, sl.GAMMA_LAT, sl.L_LON, sl.L_LAT, sl.NSKF) == (0, 25, 50, 60, 70, 95, 120)
    assert (L.FD_SK_NB, L.FD_NSKX) == (sl.NB, sl.NSKX) == (5, 10)
    assert L.FD_PHX_SERVO_LQG == sl.W_SERVO_LQG == 0x7A
    assert (sl.NOT_CONVERGED, sl.NO_CERTIFICATE, sl.BAD_INPUT) == (L.FD_KF_NOT_CONVERGED, L.FD_KF_NO_CERTIFICATE, L.FD_KF_BAD_INPUT)
    assert (sl.ESTIMATE, sl.MEASUREMENT, sl.TRUTH) == (L.FD_LQG_ESTIMATE, L.FD_LQG_MEASUREMENT, L.FD_LQG_TRUTH)
    # no other consumer's counter word
    others = {L.FD_PHX_RESET + k for k in range(4)} | {L.FD_PHX_RANDOM_WALK, L.FD_PHX_DR_GUST0, L.FD_PHX_GUST, L.FD_PHX_ACTION} | \
        {L.FD_PHX_DR_RESET + k for k in range(3)} | {L.FD_PHX_SENSOR + k for k in range(5)} | {L.FD_PHX_LQG + k for k in range(2)} | \
        {L.FD_PHX_SERVO_GUST}
    assert not {L.FD_PHX_SERVO_LQG + b for b in range(3)} & others
    assert sl.EST_STATES == (L.FD_X_U, L.FD_X_W, L.FD_X_Q, L.FD_X_PITCH, L.FD_X_D, L.FD_X_V, L.FD_X_P, L.FD_X_R, L.FD_X_ROLL, L.FD_X_YAW)
    assert "FD_SKF_" not in open(os.path.join(REPO, "include", "fdyn_layout.h")).read()     # they live in the header of their entries
    from hcrl_amd import servo_lqg as SL
    assert tuple(SL.servo_sensor_sigma()) == sl.DEFAULT_SIGMA and SL.DEFAULT_RATES == sl.DEFAULT_RATES
    assert np.array_equal(SL.ServoKalmanNoise().vector(), sl.default_noise())


def test_refused_calls_need_no_device():
    """The servo step's codes for its arguments in its order; FDYN_ERR_NULL for a NULL F, sigma, xhat or du_prev: each with no launch."""
    lib = _lib.load()
    one = ctypes.c_void_p(8)                                              # never dereferenced: every call below is refused
    #        x    x0   u0   K    ref  integ limits type params n_types n dt n_steps three optional, F sigma xhat du_prev seed step z fb four optional stream
    step = [one, one, one, one, one, one, one, None, one, 1, 5, 0.01, 1, None, None, None, one, one, one, one, 7, None, None, 0,
            None, None, None, None, None]
    N_TYPES, N, DT, N_STEPS, FB = 9, 10, 11, 12, 23

    def with_(call, at, v):
        args = list(call)
        args[at] = v
        return args

    for name in STEPS:
        fn = getattr(lib, name)
        assert fn(*with_(step, N, -2)) == _lib.FDYN_ERR_BAD_SIZE
        assert fn(*with_(step, N_STEPS, -1)) == _lib.FDYN_ERR_BAD_SIZE
        for n_types in (0, 9):
            assert fn(*with_(step, N_TYPES, n_types)) == _lib.FDYN_ERR_BAD_TYPES
        for dt in (2.0, 0.0, float("nan")):
            assert fn(*with_(step, DT, dt)) == _lib.FDYN_ERR_BAD_DT
        for hole in (0, 1, 2, 3, 4, 5, 6, 8, 16, 17, 18, 19):
            assert fn(*with_(step, hole, None)) == _lib.FDYN_ERR_NULL, (name, hole)
        for fb in (-1, 3):
            assert fn(*with_(step, FB, fb)) == _lib.FDYN_ERR_BAD_SIZE
        assert fn(*with_(step, N, 0)) == _lib.FDYN_OK                      # an empty fleet is done
        args = with_(step, 16, None)                                       # size before pointers before feedback before dt
        args[DT], args[FB] = 5.0, 9
        assert fn(*args) == _lib.FDYN_ERR_NULL
        args[N_STEPS] = -3
        assert fn(*args) == _lib.FDYN_ERR_BAD_SIZE
        args = with_(step, DT, 5.0)
        args[FB] = 9
        assert fn(*args) == _lib.FDYN_ERR_BAD_SIZE
    #          A    B    dt    noise per_lane n  F    residual iters status stream
    design = [one, one, 0.01, one, 0, 5, one, one, one, one, None]
    fn = getattr(lib, DESIGN)
    assert fn(*with_(design, 5, -1)) == _lib.FDYN_ERR_BAD_SIZE
    assert fn(*with_(design, 5, 0)) == _lib.FDYN_OK
    for hole in (0, 1, 3, 6, 7, 8, 9):
        assert fn(*with_(design, hole, None)) == _lib.FDYN_ERR_NULL, hole


def test_host_classes_on_host_tensors():
    import torch
    from hcrl_amd import servo_lqg as SL
    import servo_lqg_numpy as sl
    s = SL.servo_sensor_sigma({"gps_velocity_stddev": 0.2, "altitude_stddev": 0.7})
    assert s.tolist() == [0.2, 0.2, 0.01, 0.01, 0.7, 0.2, 0.01, 0.01, 0.01, 0.01]
    nz = SL.ServoKalmanNoise(rates=(0.3, 0.5, 0.1, 0.03, np.array([0.3, 0.6, 0.9]), 0.3, 0.1, 0.1, 0.03, 0.03))
    assert nz.per_lane and nz.rows(3).shape == (20, 3) and nz.rows(3)[14].tolist() == [0.3, 0.6, 0.9]
    assert not SL.ServoKalmanNoise().per_lane
    with pytest.raises(ValueError, match="10 entries"):
        SL.ServoKalmanNoise(sigma=(0.1,) * 8).vector()
    t = SL.noise_tensor(None, 3, "cpu")
    assert t.dtype == torch.float64 and tuple(t.shape) == (20,) and np.array_equal(t.numpy(), sl.default_noise())
    with pytest.raises(ValueError, match="noise"):
        SL.noise_tensor(np.zeros(16), 3, "cpu")
    # a design read back as matrices: the restatement's F of one golden aircraft in three lanes
    g = np.load(os.path.join(REPO, "tests", "golden", "trim_reference.npz"))
    ref = sl.design(g["A"][0], g["B"][0], 0.01, sl.default_noise())
    F = torch.as_tensor(np.repeat(ref["F"][:, None], 3, axis=1))
    d = SL.ServoKalmanDesign(F, torch.zeros(3, dtype=torch.float64), torch.zeros(3, dtype=torch.int32),
                             torch.as_tensor(np.array([0, 4, 3], np.int32)), dt=0.01)
    assert d.n == 3 and d.count_not_ok() == 2 and d.ok.tolist() == [True, False, False]
    assert SL.describe_status(3) == "not converged, no stability certificate" and SL.describe_status(0) == "ok"
    with pytest.raises(ValueError, match="2 of 3 aircraft have no certified stable filter"):
        SL.require_ok(d)
    (Phi0, Gam0, L0), (Phi1, Gam1, L1) = sl.matrices(ref["F"])
    assert tuple(d.phi().shape) == (2, 5, 5, 3) and tuple(d.gamma().shape) == (2, 5, 2, 3) and tuple(d.gain().shape) == (2, 5, 5, 3)
    assert np.array_equal(d.phi()[1, :, :, 2].numpy(), Phi1) and np.array_equal(d.gamma()[0, :, :, 0].numpy(), Gam0)
    assert np.array_equal(d.gain()[1, :, :, 1].numpy(), L1)
    np.testing.assert_allclose(d.filter_matrix()[0, :, :, 0].numpy(), Phi0 @ (np.eye(5) - L0), rtol=0, atol=1e-15)
    st = SL.ServoLqgState.zeros(3, "cpu", seed=9)
    assert st.seed == 9 and tuple(st.xhat.shape) == (10, 3) and tuple(st.du_prev.shape) == (4, 3) and st.step.dtype == torch.int32
    assert tuple(st.err_est.shape) == tuple(st.err_meas.shape) == tuple(st.meas.shape) == (10, 3) and tuple(st.chatter.shape) == (4, 3)
    st.xhat += 1.0
    st.step += 5
    st.steps_accumulated = 5
    st.reset(seed=11)
    assert not st.xhat.any() and st.step.tolist() == [0] and st.steps_accumulated == 0 and st.seed == 11

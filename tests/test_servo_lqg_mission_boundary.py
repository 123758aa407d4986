"""CPU-side checks of the boundary of the servo's missions on noisy sensors: include/fdyn_servo_lqg_mission.h parses under the strict
header parser into a table of its own of exactly three entries, the built library exports and `_lib.load()` binds them, the argument
list is fdyn_servo_mission_f64's followed by the estimator group of fdyn_servo_lqg_step_f64 and the position group, the new
constants reach hcrl_amd.layout, every refused call returns its code before anything is launched, and the host layer's classes are
plain torch wherever their tensors live.  No compute calls (there is no GPU in the build container)."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

from conftest import REPO
from hcrl_amd import _lib, layout as L

_P, _I, _U64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64
ENTRIES = ("fdyn_servo_lqg_mission_f64", "fdyn_servo_lqg_mission_mixed", "fdyn_servo_lqg_mission_f32")


def _header():
    return open(os.path.join(REPO, "include", "fdyn_servo_lqg_mission.h")).read()


def test_header_parses_into_its_own_table():
    table, consts = _lib._parse_header(_header(), "include/fdyn_servo_lqg_mission.h")
    assert table == _lib.SERVO_LQG_MISSION_SIGNATURES and consts == {}
    assert set(table) == set(ENTRIES) and len(table) == 3
    older = (_lib.SIGNATURES, _lib.MODES_SIGNATURES, _lib.SERVO_SIGNATURES, _lib.MISSION_SIGNATURES, _lib.WIND_SIGNATURES,
             _lib.SERVO_LQG_SIGNATURES, _lib.SERVO_MARGIN_SIGNATURES, _lib.SERVO_MODES_SIGNATURES)
    assert not any(set(table) & set(t) for t in older)
    assert "oracle" not in _header().lower()


def test_argument_list_is_the_mission_then_the_estimator_then_the_position_group():
    n_servo = len(_lib.SERVO_SIGNATURES["fdyn_servo_step_f64"][1]) - 1        # fdyn_servo_step_*'s arguments before `stream`
    for name in ENTRIES:
        res, args = _lib.SERVO_LQG_MISSION_SIGNATURES[name]
        mission = _lib.MISSION_SIGNATURES[name.replace("_lqg", "")][1][:-1]    # up to and including stats
        group = _lib.SERVO_LQG_SIGNATURES[name.replace("_mission", "_step")][1][n_servo:-1]   # F .. meas_out
        assert group == [_P, _P, _P, _P, _U64, _P, _P, _I, _P, _P, _P, _P]
        assert res is _I and args == mission + group + [_P, _P, _P] + [_P], name          # pos, phat, err_pos, stream
    # the parameter names too, in the header's own text
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    names = lambda text, fn: [p.split()[-1].lstrip("*") for p in re.search(fn + r"\s*\(([^()]*)\)", text).group(1).split(",")]   # noqa: E731
    strip = lambda path: re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", path)).read(), flags=re.S)   # noqa: E731
    mine = names(src, "fdyn_servo_lqg_mission_f64")
    mission = names(strip("fdyn_mission.h"), "fdyn_servo_mission_f64")
    lqg = names(strip("fdyn_servo_lqg.h"), "fdyn_servo_lqg_step_f64")
    assert mine[:len(mission) - 1] == mission[:-1] and mission[-2] == "stats"
    assert lqg[n_servo:-1] == ["F", "sigma", "xhat", "du_prev", "seed", "step", "z", "feedback", "err_est", "err_meas", "chatter", "meas_out"]
    assert mine[len(mission) - 1:] == lqg[n_servo:-1] + ["pos", "phat", "err_pos", "stream"]


def test_library_exports_and_binds_every_prototype():
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call([sys.executable, "-c", "import __graft_entry__ as g; g.build()"], cwd=REPO)
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = set(re.findall(r"\b(?:int|int64_t)\s+(fdyn_\w+)\s*\(", src))
    assert declared == set(ENTRIES)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(raw, name), f"{name} declared in include/fdyn_servo_lqg_mission.h but not exported"
    lib = _lib.load()
    for name, (res, args) in _lib.SERVO_LQG_MISSION_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name


def test_constants_are_mirrored():
    import servo_lqg_mission_numpy as lm
    assert L.FD_NSKZ == lm.NSKZ == 12 == L.FD_NSKX + 2
    assert (L.FD_SPF_SIGMA, L.FD_SPF_GAIN, L.FD_NSPF) == (lm.SPF_SIGMA, lm.SPF_GAIN, lm.NSPF) == (0, 1, 2)
    assert (lm.ESTIMATE, lm.MEASUREMENT, lm.TRUTH) == (L.FD_LQG_ESTIMATE, L.FD_LQG_MEASUREMENT, L.FD_LQG_TRUTH)
    layout = open(os.path.join(REPO, "include", "fdyn_layout.h")).read()
    assert "FD_SPF_" not in layout and "fdyn_servo_lqg_mission" in layout        # the words live with their entries; the Philox note names them
    from hcrl_amd import servo_lqg_mission as SM
    assert SM.default_sigma_pos() == lm.SIGMA_POS and SM.DEFAULT_RATE_POS == lm.RATE_POS
    for dt in (0.01, 0.02):
        assert SM.position_gain(dt=dt) == lm.position_gain(dt=dt)
    assert abs(SM.position_gain() - 0.0488) < 5e-5


def test_refused_calls_need_no_device():
    """fdyn_servo_mission_*'s codes in its order, then fdyn_servo_lqg_step_*'s: each with no launch."""
    lib = _lib.load()
    one = ctypes.c_void_p(8)                                              # never dereferenced: every call below is refused
    #       x    x0   u0   K    ref  integ limits wp_idx consts wps n_wp type params n_types n dt n_steps surf sat err reached flown stats
    call = [one, one, one, one, one, one, one, one, one, one, 3, None, one, 1, 5, 0.01, 1, None, None, None, None, None, None,
            # F  sigma xhat du_prev seed step z fb four optional                pos  phat err_pos stream
            one, one, one, one, 7, None, None, 0, None, None, None, None, one, one, None, None]
    N_WP, N_TYPES, N, DT, N_STEPS, FB = 10, 13, 14, 15, 16, 30

    def with_(at, v, base=None):
        args = list(call if base is None else base)
        args[at] = v
        return args

    for name in ENTRIES:
        fn = getattr(lib, name)
        assert fn(*with_(N, -2)) == _lib.FDYN_ERR_BAD_SIZE
        assert fn(*with_(N_STEPS, -1)) == _lib.FDYN_ERR_BAD_SIZE
        for n_wp in (0, L.FD_MAX_WAYPOINTS + 1):
            assert fn(*with_(N_WP, n_wp)) == _lib.FDYN_ERR_BAD_SIZE
        for n_types in (0, 9):
            assert fn(*with_(N_TYPES, n_types)) == _lib.FDYN_ERR_BAD_TYPES
        for dt in (2.0, 0.0, float("nan")):
            assert fn(*with_(DT, dt)) == _lib.FDYN_ERR_BAD_DT
        for hole in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 23, 24, 25, 26, 35, 36):      # pos and phat are required
            assert fn(*with_(hole, None)) == _lib.FDYN_ERR_NULL, (name, hole)
        for fb in (-1, 3):
            assert fn(*with_(FB, fb)) == _lib.FDYN_ERR_BAD_SIZE
        assert fn(*with_(N, 0)) == _lib.FDYN_OK                            # an empty fleet is done
        args = with_(35, None)                                             # size before pointers before feedback before dt
        args[DT], args[FB] = 5.0, 9
        assert fn(*args) == _lib.FDYN_ERR_NULL
        args[N_STEPS] = -3
        assert fn(*args) == _lib.FDYN_ERR_BAD_SIZE
        args = with_(DT, 5.0)
        args[FB] = 9
        assert fn(*args) == _lib.FDYN_ERR_BAD_SIZE


def test_host_classes_on_host_tensors():
    import torch
    from hcrl_amd import servo_lqg_mission as SM
    pf = SM.ServoPositionFilter.make("cpu")
    assert pf.sigma == 1.0 and pf.gain == SM.position_gain() and pf.words.dtype == torch.float64
    assert pf.words.tolist() == [1.0, SM.position_gain()]
    assert SM.ServoPositionFilter.make("cpu", sigma_pos=0.0, dt=0.02).gain == 1.0          # a perfect measurement is taken as it is
    assert SM.ServoPositionFilter.make("cpu", sigma_pos=2.0, gain=1.0).words.tolist() == [2.0, 1.0]
    # what the header leaves to the host: the refusal the entry cannot make on a device array
    for kw in (dict(gain=0.0), dict(gain=1.5), dict(gain=float("nan")), dict(sigma_pos=-1.0, gain=0.5), dict(sigma_pos=float("inf"), gain=0.5)):
        with pytest.raises(_lib.FdynError, match="bad size argument"):
            SM.ServoPositionFilter.make("cpu", **kw)
    with pytest.raises(ValueError, match="position_gain"):
        SM.position_gain(rate_pos=0.0)
    x = torch.arange(36, dtype=torch.float32).reshape(12, 3)
    st = SM.ServoLqgMissionState.start(x)
    assert st.phat.dtype == torch.float64 and st.phat.tolist() == [[0.0, 1.0, 2.0], [3.0, 4.0, 5.0]] and not st.err_pos.any()
    st.err_pos += torch.tensor([[1.0], [4.0]], dtype=torch.float64)
    assert st.error_ratio().tolist() == [0.25] * 3
    st.reset(x + 1.0)
    assert st.phat[0].tolist() == [1.0, 2.0, 3.0] and not st.err_pos.any()

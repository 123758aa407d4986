"""CPU-side checks of the wind entries' boundary: include/fdyn_wind.h parses under the strict header parser into a table of its own
of exactly six entries, the built library exports and `_lib.load()` binds them, the four older tables are what they were, the new
constants are mirrored, every refused call returns its code before anything is launched, and the host layer's ServoWind is plain
torch wherever its tensors live.  No compute calls (there is no GPU in the build container)."""
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
STEPS = ("fdyn_servo_step_wind_f64", "fdyn_servo_step_wind_mixed", "fdyn_servo_step_wind_f32")
MISSIONS = ("fdyn_servo_mission_wind_f64", "fdyn_servo_mission_wind_mixed", "fdyn_servo_mission_wind_f32")
TAIL = [_P, _U64, _P, _P, _P]                                             # wind, seed, step, z, stream


def _header():
    return open(os.path.join(REPO, "include", "fdyn_wind.h")).read()


def test_wind_header_parses_into_its_own_table():
    table, consts = _lib._parse_header(_header(), "include/fdyn_wind.h")
    assert table == _lib.WIND_SIGNATURES and consts == {}
    assert set(table) == set(STEPS) | set(MISSIONS) and len(table) == 6
    for name in STEPS:                                                    # fdyn_servo_step_*'s list, its stream replaced by the group
        assert table[name] == (_I, _lib.SERVO_SIGNATURES[name.replace("_wind", "")][1][:-1] + TAIL), name
    for name in MISSIONS:
        assert table[name] == (_I, _lib.MISSION_SIGNATURES[name.replace("_wind", "")][1][:-1] + TAIL), name
    assert (len(_lib.SIGNATURES), len(_lib.MODES_SIGNATURES), len(_lib.SERVO_SIGNATURES), len(_lib.MISSION_SIGNATURES)) == (82, 2, 4, 3)
    assert not set(table) & (set(_lib.SIGNATURES) | set(_lib.MODES_SIGNATURES) | set(_lib.SERVO_SIGNATURES) | set(_lib.MISSION_SIGNATURES))
    assert "oracle" not in _header().lower()


def test_library_exports_and_binds_every_wind_prototype():
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call([sys.executable, "-c", "import __graft_entry__ as g; g.build()"], cwd=REPO)
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = set(re.findall(r"\b(?:int|int64_t)\s+(fdyn_\w+)\s*\(", src))
    assert declared == set(STEPS) | set(MISSIONS)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(raw, name), f"{name} declared in include/fdyn_wind.h but not exported"
    lib = _lib.load()
    for name, (res, args) in _lib.WIND_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name


def test_constants_are_mirrored():
    rows = [L.FD_SW_WIND_N, L.FD_SW_WIND_E, L.FD_SW_WIND_D, L.FD_SW_GUST_N, L.FD_SW_GUST_E, L.FD_SW_GUST_D, L.FD_SW_GUST_A, L.FD_SW_GUST_B]
    assert rows == list(range(8)) and L.FD_NSW == 8 and L.FD_PHX_SERVO_GUST == 0x78
    # the order of the rate env's randomisation rows
    assert rows == [L.FD_DR_WIND_N, L.FD_DR_WIND_E, L.FD_DR_WIND_D, L.FD_DR_GUST_N, L.FD_DR_GUST_E, L.FD_DR_GUST_D, L.FD_DR_GUST_A, L.FD_DR_GUST_B]
    # no other consumer's counter word: the sensor's five blocks end at 0x64, the LQG step's two at 0x71
    others = {L.FD_PHX_RESET + k for k in range(4)} | {L.FD_PHX_RANDOM_WALK, L.FD_PHX_DR_GUST0, L.FD_PHX_GUST, L.FD_PHX_ACTION} | \
        {L.FD_PHX_DR_RESET + k for k in range(3)} | {L.FD_PHX_SENSOR + k for k in range(5)} | {L.FD_PHX_LQG + k for k in range(2)}
    assert L.FD_PHX_SERVO_GUST not in others
    import servo_wind_numpy as wn
    assert [wn.SW_WIND_N, wn.SW_WIND_E, wn.SW_WIND_D, wn.SW_GUST_N, wn.SW_GUST_E, wn.SW_GUST_D, wn.SW_GUST_A, wn.SW_GUST_B, wn.NSW] == rows + [L.FD_NSW]
    assert wn.W_SERVO_GUST == L.FD_PHX_SERVO_GUST
    assert "FD_SW_" not in open(os.path.join(REPO, "include", "fdyn_layout.h")).read()      # they live in the header of their entries


def test_refused_calls_need_no_device():
    """The existing codes for the existing arguments in the existing order, FDYN_ERR_NULL for wind == NULL: each with no launch."""
    lib = _lib.load()
    one = ctypes.c_void_p(8)                                              # never dereferenced: every call below is refused
    #        x    x0   u0   K    ref  integ limits type params n_types n dt  n_steps three optional, wind seed step z stream
    step = [one, one, one, one, one, one, one, None, one, 1, 5, 0.01, 1, None, None, None, one, 7, None, None, None]
    #        x    x0   u0   K    ref  integ limits wp_idx consts wps n_wp type params n_types n dt n_steps six optional, wind seed step z stream
    miss = [one, one, one, one, one, one, one, one, one, one, 3, None, one, 1, 5, 0.01, 1, None, None, None, None, None, None, one, 7, None, None, None]

    def with_(call, at, v):
        args = list(call)
        args[at] = v
        return args

    for names, call, (N_TYPES, N, DT, N_STEPS, WIND), required in ((STEPS, step, (9, 10, 11, 12, 16), (0, 1, 2, 3, 4, 5, 6, 8)),
                                                                   (MISSIONS, miss, (13, 14, 15, 16, 23), (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 12))):
        for name in names:
            fn = getattr(lib, name)
            assert fn(*with_(call, N, -2)) == _lib.FDYN_ERR_BAD_SIZE
            assert fn(*with_(call, N_STEPS, -1)) == _lib.FDYN_ERR_BAD_SIZE
            for n_types in (0, 9):
                assert fn(*with_(call, N_TYPES, n_types)) == _lib.FDYN_ERR_BAD_TYPES
            for dt in (2.0, 0.0, float("nan")):
                assert fn(*with_(call, DT, dt)) == _lib.FDYN_ERR_BAD_DT
            for hole in required:
                assert fn(*with_(call, hole, None)) == _lib.FDYN_ERR_NULL, (name, hole)
            assert fn(*with_(call, WIND, None)) == _lib.FDYN_ERR_NULL, name
            assert fn(*with_(call, N, 0)) == _lib.FDYN_OK                  # an empty fleet is done
            args = with_(call, WIND, None)                                 # size before pointers before dt
            args[DT] = 5.0
            assert fn(*args) == _lib.FDYN_ERR_NULL
            args[N_STEPS] = -3
            assert fn(*args) == _lib.FDYN_ERR_BAD_SIZE
    for name in MISSIONS:
        for n_wp in (0, -1, L.FD_MAX_WAYPOINTS + 1):
            assert getattr(lib, name)(*with_(miss, 10, n_wp)) == _lib.FDYN_ERR_BAD_SIZE, n_wp


def test_servo_wind_on_host_tensors():
    import torch
    from hcrl_amd import servo as SV
    from hcrl_amd.disturbances import Disturbances
    import servo_wind_numpy as wn
    w = SV.ServoWind.steady(3, "cpu", 6.0, [0.0, np.pi / 2, np.pi], vertical=1.0, seed=5)
    assert (w.n, w.seed) == (3, 5) and w.rows.dtype == torch.float64 and tuple(w.rows.shape) == (L.FD_NSW, 3)
    assert w.step.dtype == torch.int32 and w.step.tolist() == [0]
    np.testing.assert_allclose(w.rows[:3].numpy(), [[6.0, 0.0, -6.0], [0.0, 6.0, 0.0], [1.0, 1.0, 1.0]], atol=1e-15)
    assert not w.rows[3:6].any() and w.rows[L.FD_SW_GUST_A].tolist() == [1.0] * 3 and not w.rows[L.FD_SW_GUST_B].any()
    # ground_state is the restatement's map, and to_air undoes it
    x = torch.as_tensor(np.random.RandomState(0).normal(0, 1, (12, 3)))
    g = w.ground_state(x)
    for i in range(3):
        np.testing.assert_allclose(g[:, i].numpy(), wn.to_ground(x[:, i].numpy(), w.air_mass()[:, i].numpy()), rtol=0, atol=1e-14)
    assert g.dtype == x.dtype and w.ground_state(x.float()).dtype == torch.float32
    assert torch.equal(g[:3], x[:3]) and torch.equal(g[6:], x[6:])
    # the ranges of a Disturbances, the gust stationary at sigma = intensity x V0
    d = Disturbances(wind_speed=(2.0, 6.0), wind_direction=(0.0, 6.28), wind_vertical=(-1.0, 1.0), turbulence_intensity=(0.05, 0.1), gust_length=(100.0, 200.0))
    r = SV.ServoWind.from_disturbances(d, 4000, 20.0, 0.01, "cpu", np.random.default_rng(1)).rows.numpy()
    speed = np.hypot(r[0], r[1])
    assert speed.min() >= 2.0 - 1e-12 and speed.max() <= 6.0 + 1e-12 and np.abs(r[2]).max() <= 1.0
    A, B = r[L.FD_SW_GUST_A], r[L.FD_SW_GUST_B]
    sigma = B / np.sqrt(1.0 - A * A)
    assert (A > np.exp(-0.01 * 20.0 / 100.0) - 1e-12).all() and (A < np.exp(-0.01 * 20.0 / 200.0) + 1e-12).all()
    assert sigma.min() >= 1.0 - 1e-9 and sigma.max() <= 2.0 + 1e-9
    assert 0.8 < (r[3:6] / sigma).std() < 1.2
    calm = SV.ServoWind.from_disturbances(Disturbances(), 5, 20.0, 0.01, "cpu", np.random.default_rng(1)).rows
    assert not calm[:6].any() and not calm[L.FD_SW_GUST_B].any()
    with pytest.raises(ValueError, match="wind rows"):
        SV.ServoWind(torch.zeros((7, 3), dtype=torch.float64))
    with pytest.raises(ValueError, match="z must be"):
        w._args(3, 2, torch.zeros((2, 3, 4), dtype=torch.float64))
    with pytest.raises(ValueError, match="aircraft"):
        w._args(4, 1, None)

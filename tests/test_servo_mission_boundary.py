"""CPU-side checks of the servo missions' boundary: include/fdyn_mission.h parses under the strict header parser into a table of
its own of exactly three entries, the built library exports and `_lib.load()` binds them, the three older tables are what they
were, the new layout constants are mirrored, and every refused call returns its code before anything is launched.  No compute
calls (there is no GPU in the build container)."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO
from hcrl_amd import _lib, layout as L

_P, _I, _I64, _D = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double
MISSIONS = ("fdyn_servo_mission_f64", "fdyn_servo_mission_mixed", "fdyn_servo_mission_f32")


def _header():
    return open(os.path.join(REPO, "include", "fdyn_mission.h")).read()


def test_mission_header_parses_into_its_own_table():
    table, consts = _lib._parse_header(_header(), "include/fdyn_mission.h")
    assert table == _lib.MISSION_SIGNATURES and consts == {}
    # x, x0, u0, K, ref, integ, limits, wp_idx, consts, wps, n_wp, type, params, n_types, n, dt, n_steps, surf_out, sat_steps, err_out,
    # reached_total, steps_flown, stats, stream
    for name in MISSIONS:
        assert table[name] == (_I, [_P] * 10 + [_I, _P, _P, _I, _I64, _D, _I] + [_P] * 7), name
    assert set(table) == set(MISSIONS) and len(table) == 3
    assert (len(_lib.SIGNATURES), len(_lib.MODES_SIGNATURES), len(_lib.SERVO_SIGNATURES)) == (82, 2, 4)
    assert not set(table) & (set(_lib.SIGNATURES) | set(_lib.MODES_SIGNATURES) | set(_lib.SERVO_SIGNATURES))
    assert "oracle" not in _header().lower()


def test_library_exports_and_binds_every_mission_prototype():
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call([sys.executable, "-c", "import __graft_entry__ as g; g.build()"], cwd=REPO)
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = set(re.findall(r"\b(?:int|int64_t)\s+(fdyn_\w+)\s*\(", src))
    assert declared == set(MISSIONS)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(raw, name), f"{name} declared in include/fdyn_mission.h but not exported"
    lib = _lib.load()
    for name, (res, args) in _lib.MISSION_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name


def test_refused_calls_need_no_device():
    """A bad size (n, n_steps, n_wp), a bad type count, a missing required pointer and a bad dt are answered with no launch."""
    lib = _lib.load()
    one = ctypes.c_void_p(8)                                             # never dereferenced: every call below is refused
    #       x    x0   u0   K    ref  integ limits wp_idx consts wps n_wp type  params n_types n dt  n_steps then seven optional, stream
    call = [one, one, one, one, one, one, one, one, one, one, 3, None, one, 1, 5, 0.01, 1, None, None, None, None, None, None, None]
    N_WP, N_TYPES, N, DT, N_STEPS = 10, 13, 14, 15, 16

    def with_(at, v):
        args = list(call)
        args[at] = v
        return args

    for name in MISSIONS:
        fn = getattr(lib, name)
        assert fn(*with_(N, -2)) == _lib.FDYN_ERR_BAD_SIZE
        assert fn(*with_(N_STEPS, -1)) == _lib.FDYN_ERR_BAD_SIZE
        for n_wp in (0, -1, L.FD_MAX_WAYPOINTS + 1):
            assert fn(*with_(N_WP, n_wp)) == _lib.FDYN_ERR_BAD_SIZE, n_wp
        for n_types in (0, 9):
            assert fn(*with_(N_TYPES, n_types)) == _lib.FDYN_ERR_BAD_TYPES
        for dt in (2.0, 0.0, float("nan")):
            assert fn(*with_(DT, dt)) == _lib.FDYN_ERR_BAD_DT
        for hole in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 12):                  # wp_idx, consts and wps included
            assert fn(*with_(hole, None)) == _lib.FDYN_ERR_NULL, (name, hole)
        assert fn(*with_(N, 0)) == _lib.FDYN_OK                           # an empty fleet is done
        # the order fdyn.h's entry points report in: size, types, pointers, dt
        args = with_(N_WP, 17)
        args[0], args[DT] = None, 5.0
        assert fn(*args) == _lib.FDYN_ERR_BAD_SIZE


def test_layout_words_are_mirrored():
    assert [L.FD_MST_ALTITUDE_ERROR, L.FD_MST_ROLL, L.FD_MST_MIN_AIRSPEED, L.FD_MST_CROSS_TRACK, L.FD_NMST] == [0, 1, 2, 3, 4]
    assert (L.FD_NMS, L.FD_MS_AIRSPEED, L.FD_MS_ALTITUDE) == (14, 12, 13)          # the sensor's block keeps its names
    import servo_mission_numpy as mn
    assert [mn.MST_ALTITUDE_ERROR, mn.MST_ROLL, mn.MST_MIN_AIRSPEED, mn.MST_CROSS_TRACK, mn.NMST] == [0, 1, 2, 3, L.FD_NMST]
    assert (mn.C_GUIDANCE_TYPE, mn.C_WP_MAX_BANK, mn.C_LOS_MAX_BANK, mn.C_LOS_LEAD, mn.C_LOOKAHEAD_TIME, mn.C_LOOKAHEAD_MIN, mn.C_LOOKAHEAD_MAX,
            mn.C_PROXIMITY_SCALE, mn.C_TURN_DIST, mn.C_TURN_ANGLE, mn.C_MAX_SPEED_REDUCTION, mn.C_MIN_SPEED, mn.C_ACCEPTANCE_RADIUS, mn.C_ON_COMPLETE) == \
        (L.FD_C_GUIDANCE_TYPE, L.FD_C_WP_MAX_BANK_RAD, L.FD_C_LOS_MAX_BANK_RAD, L.FD_C_LOS_LEAD_ANGLE_RAD, L.FD_C_LOOKAHEAD_TIME, L.FD_C_LOOKAHEAD_MIN,
         L.FD_C_LOOKAHEAD_MAX, L.FD_C_PROXIMITY_SCALE, L.FD_C_TURN_THRESHOLD_DIST, L.FD_C_TURN_THRESHOLD_ANGLE_RAD, L.FD_C_MAX_SPEED_REDUCTION,
         L.FD_C_MIN_SPEED, L.FD_C_ACCEPTANCE_RADIUS, L.FD_C_ON_COMPLETE)
    assert (mn.WP_NORTH, mn.WP_EAST, mn.WP_ALTITUDE, mn.WP_SPEED) == (L.FD_WP_NORTH, L.FD_WP_EAST, L.FD_WP_ALTITUDE, L.FD_WP_SPEED)
    assert (mn.LOS, mn.PP, mn.DEFAULT) == (L.FD_GUIDANCE_LOS, L.FD_GUIDANCE_PP, L.FD_GUIDANCE_DEFAULT)
    assert (mn.D_AIRSPEED, mn.D_ALTITUDE, mn.D_GROUND_SPEED, mn.D_HEADING) == (L.FD_D_AIRSPEED, L.FD_D_ALTITUDE, L.FD_D_GROUND_SPEED, L.FD_D_HEADING)


def test_host_layer_on_host_tensors():
    """ServoMission is plain torch wherever its tensors live (here on the host); the fleet methods refuse without a design."""
    import torch
    from hcrl_amd import servo as SV
    from hcrl_amd.agents import LQServoWaypointAgent
    from hcrl_amd.config import square_mission
    from hcrl_amd.flight_types import ControlMode
    assert LQServoWaypointAgent.MODE is ControlMode.WAYPOINT
    m = SV.ServoMission.start(square_mission(300.0, 100.0, 15.0), 3, "cpu", guidance_type="LOS", acceptance_radius=25.0, on_complete="restart")
    assert (m.n, m.n_wp) == (3, 5) and m.wps.dtype == torch.float64 and tuple(m.stats.shape) == (L.FD_NMST, 3)
    assert m.wps[2].tolist() == [300.0, 300.0, 100.0, 15.0]
    assert m.consts[L.FD_C_GUIDANCE_TYPE] == L.FD_GUIDANCE_LOS and m.consts[L.FD_C_ACCEPTANCE_RADIUS] == 25.0 and m.consts[L.FD_C_ON_COMPLETE] == 1
    assert m.stats.tolist() == [[0.0] * 3, [0.0] * 3, [float("inf")] * 3, [0.0] * 3]
    assert not m.complete().any() and not m.wp_idx.any() and m.wp_idx.dtype == torch.int32
    m.wp_idx[1], m.steps_flown[1] = 5, 4410
    assert m.complete().tolist() == [False, True, False] and m.mission_time(0.01).tolist() == [0.0, 44.1, 0.0]
    table = np.array([[0.0, 0.0, 100.0, np.nan]])
    assert bool(torch.isnan(SV.ServoMission.start(table, 1, "cpu").wps[0, 3]))
    for bad in (np.zeros((0, 4)), np.zeros((17, 4)), np.zeros((3, 3))):
        with pytest.raises(ValueError, match="waypoint rows"):
            SV.ServoMission.start(bad, 1, "cpu")

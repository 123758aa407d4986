"""CPU-side checks of the LQ servo's boundary: include/fdyn_servo.h parses under the strict header parser into a table of its own,
the built library exports every prototype it declares and `_lib.load()` binds them, the tables of include/fdyn.h and
include/fdyn_modes.h are what they were, and the layout constants are mirrored.  No compute calls (there is no GPU in the build
container)."""
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
STEPS = ("fdyn_servo_step_f64", "fdyn_servo_step_mixed", "fdyn_servo_step_f32")


def _header():
    return open(os.path.join(REPO, "include", "fdyn_servo.h")).read()


def test_servo_header_parses_into_its_own_table():
    table, consts = _lib._parse_header(_header(), "include/fdyn_servo.h")
    assert table == _lib.SERVO_SIGNATURES and consts == {}
    # A, B, x0, weights, weights_per_lane, n, K, residual, iters, status, stream
    assert table["fdyn_servo_design"] == (_I, [_P, _P, _P, _P, _I, _I64, _P, _P, _P, _P, _P])
    # x, x0, u0, K, ref, integ, limits, type, params, n_types, n, dt, n_steps, surf_out, sat_steps, err_out, stream
    for name in STEPS:
        assert table[name] == (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I64, _D, _I, _P, _P, _P, _P]), name
    assert set(table) == {"fdyn_servo_design", *STEPS} and len(table) == 4
    assert len(_lib.SIGNATURES) == 82 and len(_lib.MODES_SIGNATURES) == 2
    assert not set(table) & (set(_lib.SIGNATURES) | set(_lib.MODES_SIGNATURES))
    assert "oracle" not in _header().lower()


def test_library_exports_and_binds_every_servo_prototype():
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call([sys.executable, "-c", "import __graft_entry__ as g; g.build()"], cwd=REPO)
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = set(re.findall(r"\b(?:int|int64_t)\s+(fdyn_\w+)\s*\(", src))
    assert declared == set(_lib.SERVO_SIGNATURES) and len(declared) == 4
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(raw, name), f"{name} declared in include/fdyn_servo.h but not exported"
    lib = _lib.load()
    for name, (res, args) in _lib.SERVO_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    assert lib.fdyn_abi_version() == _lib.FDYN_ABI_VERSION == 3


def test_refused_calls_need_no_device():
    """A bad size, a bad type count, a missing required pointer and a bad dt are answered before anything is launched."""
    lib = _lib.load()
    one = ctypes.c_void_p(8)                                             # never dereferenced: every call below is refused
    design = [one, one, one, one, 0, 5, one, one, one, one, None]
    assert lib.fdyn_servo_design(*design[:5], -1, *design[6:]) == _lib.FDYN_ERR_BAD_SIZE
    assert lib.fdyn_servo_design(*design[:5], 0, *design[6:]) == _lib.FDYN_OK                      # an empty fleet is done
    for hole in (0, 1, 2, 3, 6, 7, 8, 9):
        args = list(design)
        args[hole] = None
        assert lib.fdyn_servo_design(*args) == _lib.FDYN_ERR_NULL, hole
    step = [one, one, one, one, one, one, one, None, one, 1, 5, 0.01, 1, None, None, None, None]
    for name in STEPS:
        fn = getattr(lib, name)
        assert fn(*step[:10], -2, *step[11:]) == _lib.FDYN_ERR_BAD_SIZE
        assert fn(*step[:12], -1, *step[13:]) == _lib.FDYN_ERR_BAD_SIZE
        assert fn(*step[:9], 9, *step[10:]) == _lib.FDYN_ERR_BAD_TYPES
        assert fn(*step[:11], 2.0, *step[12:]) == _lib.FDYN_ERR_BAD_DT
        for hole in (0, 1, 2, 3, 4, 5, 6, 8):
            args = list(step)
            args[hole] = None
            assert fn(*args) == _lib.FDYN_ERR_NULL, (name, hole)


def test_layout_words():
    assert (L.FD_NSVK, L.FD_NSVW, L.FD_NSVR, L.FD_NSVI, L.FD_SV_NLON, L.FD_SV_NLAT) == (26, 17, 5, 3, 7, 6)
    assert (L.FD_SVK_LON, L.FD_SVK_LAT) == (0, 2 * L.FD_SV_NLON) and L.FD_NSVK == 2 * (L.FD_SV_NLON + L.FD_SV_NLAT)
    assert (L.FD_SVW_Q_LON, L.FD_SVW_Q_LAT, L.FD_SVW_R_LON, L.FD_SVW_R_LAT) == (0, 7, 13, 15)
    assert [L.FD_SVR_SPEED, L.FD_SVR_ALTITUDE, L.FD_SVR_HEADING, L.FD_SVR_CLIMB_RATE, L.FD_SVR_TURN_RATE] == list(range(5))
    assert [L.FD_SVI_SPEED, L.FD_SVI_ALTITUDE, L.FD_SVI_HEADING] == list(range(3))
    assert (L.FD_SV_NOT_CONVERGED, L.FD_SV_NO_CERTIFICATE, L.FD_SV_BAD_INPUT) == (L.FD_LQR_NOT_CONVERGED, L.FD_LQR_NO_CERTIFICATE, L.FD_LQR_BAD_INPUT)
    import servo_numpy as sn
    assert (sn.NSVK, sn.NSVW, sn.NSVR, sn.NSVI, sn.NLON, sn.NLAT) == (L.FD_NSVK, L.FD_NSVW, L.FD_NSVR, L.FD_NSVI, L.FD_SV_NLON, L.FD_SV_NLAT)
    assert sn.LON_STATES == (L.FD_X_U, L.FD_X_W, L.FD_X_Q, L.FD_X_PITCH, L.FD_X_D) and sn.LAT_STATES == (L.FD_X_V, L.FD_X_P, L.FD_X_R, L.FD_X_ROLL, L.FD_X_YAW)


def test_host_layer_on_host_tensors():
    """ServoWeights, ServoDesign's views and ServoState are plain NumPy / torch wherever their tensors live: here on the host."""
    import torch
    import servo_numpy as sn
    from hcrl_amd import servo as SV
    from hcrl_amd.agents import LQServoAgent
    from hcrl_amd.flight_types import ControlMode
    assert np.array_equal(SV.ServoWeights().vector(), sn.default_weights()) and SV.DEFAULT_LIMITS == sn.DEFAULT_LIMITS
    sweep = SV.ServoWeights(psi=np.array([0.1, 0.2, 0.4]))
    assert sweep.per_lane and sweep.rows(3).shape == (L.FD_NSVW, 3) and np.array_equal(sweep.rows(3)[11], 1.0 / np.array([0.1, 0.2, 0.4]) ** 2)
    assert SV.LONGITUDINAL_STATES == sn.LON_STATES and SV.LATERAL_STATES == sn.LAT_STATES
    assert SV.describe_status(0) == "ok" and SV.describe_status(5) == "not converged, invalid model, trim or weights"
    assert LQServoAgent.MODE is ControlMode.HSA

    g = np.load(os.path.join(REPO, "tests", "golden", "trim_reference.npz"))
    idx = [3, 150, 287]
    A, B, x0 = (torch.as_tensor(np.ascontiguousarray(np.moveaxis(g[k][idx], 0, -1))) for k in ("A", "B", "x0"))
    ref = [sn.design(g["A"][i], g["B"][i], g["x0"][i], sn.default_weights()) for i in idx]
    d = SV.ServoDesign(torch.as_tensor(np.array([r["K"] for r in ref]).T.copy()), torch.zeros(3, dtype=torch.float64),
                       torch.zeros(3, dtype=torch.int32), torch.tensor([0, 0, L.FD_SV_NO_CERTIFICATE], dtype=torch.int32), x0)
    assert d.n == 3 and d.ok.tolist() == [True, True, False] and d.count_not_ok() == 1
    with pytest.raises(ValueError, match="1 of 3 aircraft have no certified stabilising servo gain.*aircraft 2: no stability certificate"):
        SV.require_ok(d)
    lon, lat = d.closed_loop(A, B)
    assert tuple(lon.shape) == (7, 7, 3) and tuple(lat.shape) == (6, 6, 3)
    for k, i in enumerate(idx):
        want = sn.closed_loops(g["A"][i], g["B"][i], g["x0"][i], ref[k]["K"])
        assert np.abs(lon[:, :, k].numpy() - want[0]).max() <= 1e-12 and np.abs(lat[:, :, k].numpy() - want[1]).max() <= 1e-12
        assert np.linalg.eigvals(want[0]).real.max() < 0.0 and np.linalg.eigvals(want[1]).real.max() < 0.0

    st = SV.ServoState.at_trim(x0)
    want = np.array([sn.reference_at(g["x0"][i]) for i in idx]).T
    assert np.abs(st.ref.numpy() - want).max() <= 1e-12 and not st.integ.any() and st.limits.tolist() == list(sn.DEFAULT_LIMITS)
    # the trims of the golden file climb at V sin(gamma) and turn at the rate they were asked for
    spec = g["spec"][idx]
    assert np.abs(want[3] - spec[:, 0] * np.sin(spec[:, 1])).max() <= 1e-9 and np.abs(want[4] - spec[:, 2]).max() <= 1e-9
    st.command(heading=[0.5, 4.0, -0.2], speed=22.0)
    assert np.allclose(st.ref[L.FD_SVR_HEADING].numpy(), [0.5, 4.0 - 2 * np.pi, -0.2], rtol=0, atol=1e-15)
    assert st.ref[L.FD_SVR_SPEED].tolist() == [22.0] * 3 and not st.ref[L.FD_SVR_TURN_RATE].any()
    assert np.array_equal(st.ref[L.FD_SVR_CLIMB_RATE].numpy(), want[3]) and np.array_equal(st.ref[L.FD_SVR_ALTITUDE].numpy(), want[1])
    st.command(altitude=130.0)
    assert st.ref[L.FD_SVR_ALTITUDE].tolist() == [130.0] * 3 and not st.ref[L.FD_SVR_CLIMB_RATE].any()
    with pytest.raises(ValueError, match="servo command"):
        st.command(speed=[1.0, 2.0])

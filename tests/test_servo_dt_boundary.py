"""CPU-side checks of the sampled-data servo design's boundary: include/fdyn_servo_dt.h parses under the strict header parser into a
table of its own with exactly one entry, the built library exports it and `_lib.load()` binds it, refused calls need no device, and
the host layer refuses to fly or analyse a gain designed for one control step at another, while a continuous design (dt None)
passes every such check as before.  No compute calls (there is no GPU in the build container)."""
import ctypes
import os
import re
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import REPO
from hcrl_amd import _lib, layout as L
from hcrl_amd import servo as SV
from hcrl_amd import servo_covariance as SC
from hcrl_amd import servo_lqg as SL
from hcrl_amd import servo_lqg_mission as SLM
from hcrl_amd import servo_margins as SM
from hcrl_amd import servo_modes as SMO
from hcrl_amd import servo_sched as SS
from hcrl_amd import servo_sched_lqg as SQ

_P, _I, _I64, _D = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double
NAME = "fdyn_servo_design_dt"


def _header():
    return open(os.path.join(REPO, "include", "fdyn_servo_dt.h")).read()


def test_dt_header_parses_into_its_own_table_of_one():
    table, consts = _lib._parse_header(_header(), "include/fdyn_servo_dt.h")
    assert table == _lib.SERVO_DT_SIGNATURES and consts == {}
    # A, B, x0, weights, weights_per_lane, dt, n, K, residual, iters, status, stream
    assert table == {NAME: (_I, [_P, _P, _P, _P, _I, _D, _I64, _P, _P, _P, _P, _P])}
    base = _lib.SERVO_SIGNATURES["fdyn_servo_design"][1]
    assert table[NAME][1] == [*base[:5], _D, *base[5:]]                 # fdyn_servo_design's arguments with dt in front of n
    others = [_lib.SIGNATURES, _lib.MODES_SIGNATURES, _lib.SERVO_SIGNATURES, _lib.MISSION_SIGNATURES, _lib.WIND_SIGNATURES,
              _lib.SERVO_LQG_SIGNATURES, _lib.SERVO_MARGIN_SIGNATURES, _lib.SERVO_MODES_SIGNATURES, _lib.SERVO_LQG_MISSION_SIGNATURES,
              _lib.SERVO_COVARIANCE_SIGNATURES, _lib.SERVO_SCHED_SIGNATURES, _lib.SERVO_SCHED_LQG_SIGNATURES]
    assert not any(NAME in t for t in others)
    # the existing tables keep their lengths
    assert [len(t) for t in others] == [82, 2, 4, 3, 6, 5, 1, 4, 3, 2, 6, 3]
    assert "oracle" not in _header().lower()


def test_library_exports_and_binds_the_prototype():
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call([sys.executable, "-c", "import __graft_entry__ as g; g.build()"], cwd=REPO)
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert set(re.findall(r"\b(?:int|int64_t)\s+(fdyn_\w+)\s*\(", src)) == {NAME}
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME), f"{NAME} declared in include/fdyn_servo_dt.h but not exported"
    fn = getattr(_lib.load(), NAME)
    res, args = _lib.SERVO_DT_SIGNATURES[NAME]
    assert fn.restype is res and list(fn.argtypes) == args
    assert _lib.load().fdyn_abi_version() == _lib.FDYN_ABI_VERSION == 3


def test_refused_calls_need_no_device():
    """A bad size, a missing pointer and a bad dt are answered before anything is launched, in that order; an empty fleet is done."""
    fn = getattr(_lib.load(), NAME)
    one = ctypes.c_void_p(8)                                             # never dereferenced: every call below is refused
    call = [one, one, one, one, 0, 0.02, 5, one, one, one, one, None]
    assert fn(*call[:6], -1, *call[7:]) == _lib.FDYN_ERR_BAD_SIZE
    assert fn(*call[:6], (1 << 31), *call[7:]) == _lib.FDYN_ERR_BAD_SIZE
    assert fn(*call[:6], 0, *call[7:]) == _lib.FDYN_OK
    assert fn(*call[:5], 7.0, 0, *call[7:]) == _lib.FDYN_OK               # an empty fleet is done whatever dt says
    for hole in (0, 1, 2, 3, 7, 8, 9, 10):
        args = list(call)
        args[hole] = None
        assert fn(*args) == _lib.FDYN_ERR_NULL, hole
    for dt in (0.0, -0.01, 1e-6, 1.0 + 1e-9, 2.0, float("nan"), float("inf")):   # bad_dt's rule: (1e-6, 1]
        assert fn(*call[:5], dt, *call[6:]) == _lib.FDYN_ERR_BAD_DT, dt
    args = list(call)
    args[0], args[5] = None, 0.0
    assert fn(*args) == _lib.FDYN_ERR_NULL                               # the pointer is reported before the step
    with pytest.raises(ValueError, match="invalid timestep"):
        _lib.check(fn(*call[:5], 0.0, *call[6:]), NAME)


# ---- the host layer, on host tensors ---------------------------------------------------------------------------------------------
def _design(n=3, dt=None):
    g = np.load(os.path.join(REPO, "tests", "golden", "trim_reference.npz"))
    idx = [3, 150, 287][:n]
    x0 = torch.as_tensor(np.ascontiguousarray(g["x0"][idx].T))
    u0 = torch.as_tensor(np.ascontiguousarray(g["u0"][idx].T))
    return SV.ServoDesign(torch.zeros((L.FD_NSVK, n), dtype=torch.float64), torch.zeros(n, dtype=torch.float64),
                          torch.zeros(n, dtype=torch.int32), torch.zeros(n, dtype=torch.int32), x0, u0, dt)


def _flights_and_analyses(design, dt):
    """Every way of flying or analysing `design` at the step dt, as (name, call): each reaches its step check on host tensors,
    before anything is launched; what it raises afterwards (here: a wrong storage type, or nothing left to check) is not the step."""
    n = design.n
    x = torch.zeros((L.FD_NX, n), dtype=torch.float32)                   # the wrong storage type for "f64": refused after the step check
    state = SV.ServoState.at_trim(design.x0)
    kalman = SimpleNamespace(n=n, dt=dt, sigma=torch.ones(10, dtype=torch.float64), F=None)
    sched = SS.ServoSchedule.from_design(design)
    return (("step_servo", lambda: SV.step_into("f64", x, design, state, None, None, dt, 1)),
            ("fly_servo_mission", lambda: SV.mission_into("f64", x, design, state, SimpleNamespace(n=n), None, None, dt, 1)),
            ("step_servo_lqg", lambda: SL.lqg_step_into("f64", x, design, kalman, state, SimpleNamespace(xhat=x), None, None, dt, 1)),
            ("fly_servo_lqg_mission", lambda: SLM.lqg_mission_into("f64", x, design, kalman, state, SimpleNamespace(xhat=x), SimpleNamespace(n=n),
                                                                   None, SimpleNamespace(phat=x), None, None, dt, 1)),
            ("servo_loop_margins", lambda: SM.servo_loop_margins(design, kalman, omega=[1.0, 0.5])),
            ("sampled modes", lambda: SMO.sampled_poles(design, SimpleNamespace(n=n, dt=dt, F=torch.zeros((3, n), dtype=torch.float64)))),
            ("servo_covariance", lambda: SC.servo_covariance(design, SimpleNamespace(n=n, dt=dt, sigma=None))),
            ("step_servo(schedule=)", lambda: SS.sched_step_into("f64", x.double(), sched, state, None, None, dt, 1, on="nowhere")),
            ("fly_servo_mission(schedule=)", lambda: SS.sched_mission_into("f64", x.double(), sched, state, SimpleNamespace(n=n + 1), None, None, dt, 1)),
            ("step_servo_lqg(schedule=)", lambda: SQ.sched_lqg_step_into("f64", x.double(), sched, SimpleNamespace(dt=float(dt), sigma=1, n_nodes=7, n=n),
                                                                         None, state, None, None, None, dt, 1)))


def test_a_sampled_design_is_refused_at_another_step():
    design = _design(dt=0.02)
    assert design.dt == 0.02 and SS.ServoSchedule.from_design(design).dt == 0.02
    for name, call in _flights_and_analyses(design, 0.01):
        with pytest.raises(ValueError, match=r"designed for a control step of 0\.02 s and cannot run at 0\.01 s"):
            call()
    SV.check_step(design, 0.02, "at its own step")
    SV.check_step(design, 0.02 * (1.0 + 1e-15), "at its own step but for rounding")


@pytest.mark.parametrize("made", [None, 0.01])
def test_at_its_own_step_and_with_dt_none_nothing_changes(made):
    """A continuous design (dt None) at any step, and a sampled design at its own: every call passes the step check and goes on to
    what it checked before -- none of the messages below is about the step."""
    design = _design(dt=made)
    assert SS.ServoSchedule.from_design(design).dt == made
    seen = {}
    for name, call in _flights_and_analyses(design, 0.01):
        with pytest.raises(Exception) as e:
            call()
        assert "control step" not in str(e.value), (name, e.value)
        seen[name] = type(e.value).__name__
    assert len(seen) == 10


def test_design_records_carry_dt_last_and_optional():
    """ServoDesign and ServoSchedule are built positionally by existing callers: dt is the last field of both and defaults to None."""
    from dataclasses import fields
    assert [f.name for f in fields(SV.ServoDesign)][-3:] == ["x0", "u0", "dt"] and _design().dt is None
    assert [f.name for f in fields(SS.ServoSchedule)][-2:] == ["context", "dt"]
    import inspect
    from hcrl_amd.fleet import BatchedSixDOF
    for fn in (SV.design_servo, SS.design_servo_schedule, BatchedSixDOF.design_servo, BatchedSixDOF.design_servo_schedule):
        p = inspect.signature(fn).parameters
        assert list(p)[-1] == "dt" and p["dt"].default is None, fn

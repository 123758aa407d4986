"""ctypes binding of csrc/libfdyn_hip.so (the C-ABI in include/fdyn.h).

There is NO CPU fallback: if the HIP library is missing or a GPU is not present, calls fail loudly.
"""
import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FDYN_LIB", os.path.join(_HERE, "csrc", "libfdyn_hip.so"))   # FDYN_LIB: A/B experiment builds

_SCALARS = {"int": C.c_int, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "double": C.c_double, "float": C.c_float}


def _parse_header(src, header="include/fdyn.h"):
    """The text of include/fdyn.h (or of `header`, named in the errors) -> ({name: (restype, [argtypes])} of every fdyn_* prototype, {name: value} of every integer
    `#define FDYN_*`).  Strict: a parameter or a declaration it cannot type is a ValueError, never a guess."""
    src = re.sub(r"/\*.*?\*/|//[^\n]*", "", src, flags=re.S)
    consts = {name: int(val) for name, val in re.findall(r"^[ \t]*#define[ \t]+(FDYN_\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$", src, flags=re.M)}
    src = re.sub(r"^[ \t]*#define(?:.*\\\n)*.*$", "", src, flags=re.M)          # a macro body declares nothing
    table = {}
    for res, name, params in re.findall(r"\b(int|int64_t)\s+(fdyn_\w+)\s*\(([^()]*)\)\s*;", src):
        args = []
        for param in ([] if params.strip() == "void" else params.split(",")):
            words = param.replace("*", " * ").split()
            scalar = [w for w in words[:-1] if w != "const"]                  # the last word is the parameter's name
            if "*" in words:
                args.append(C.c_void_p)
            elif len(scalar) == 1 and scalar[0] in _SCALARS:
                args.append(_SCALARS[scalar[0]])
            else:
                raise ValueError(f"{header}: {name}: no ctypes type for the parameter '{param.strip()}'")
        table[name] = (_SCALARS[res], args)
    heads = re.findall(r"\b(fdyn_\w+)\s*\(", src)
    if len(heads) != len(table):                 # another return type, a function pointer, a name declared twice
        raise ValueError(f"{header}: {len(heads)} fdyn_* prototype heads, {len(table)} parsed; look at "
                         f"{sorted(set(heads) - set(table)) or sorted(h for h in set(heads) if heads.count(h) > 1)}")
    return table, consts


# name -> (restype, [argtypes]), and FDYN_OK, FDYN_ERR_*, FDYN_ABI_VERSION: read from the header the library is compiled against,
# as layout.py reads fdyn_layout.h.  Every pointer is c_void_p, the three host pointers of fdyn_device_info included: nothing in the
# repository calls it from Python.
with open(os.path.join(os.path.dirname(_HERE), "include", "fdyn.h")) as _f:
    SIGNATURES, _CONSTS = _parse_header(_f.read())
globals().update(_CONSTS)
# the flight-mode report has a header of its own (include/fdyn_modes.h), in the same prototype style: a second table, bound to the
# same library
with open(os.path.join(os.path.dirname(_HERE), "include", "fdyn_modes.h")) as _f:
    MODES_SIGNATURES = _parse_header(_f.read(), "include/fdyn_modes.h")[0]
# so has the LQ servo (include/fdyn_servo.h): a third table
with open(os.path.join(os.path.dirname(_HERE), "include", "fdyn_servo.h")) as _f:
    SERVO_SIGNATURES = _parse_header(_f.read(), "include/fdyn_servo.h")[0]
# and the waypoint missions the servo flies (include/fdyn_mission.h): a fourth
with open(os.path.join(os.path.dirname(_HERE), "include", "fdyn_mission.h")) as _f:
    MISSION_SIGNATURES = _parse_header(_f.read(), "include/fdyn_mission.h")[0]
# and the servo and its missions in wind and gusts (include/fdyn_wind.h): a fifth
with open(os.path.join(os.path.dirname(_HERE), "include", "fdyn_wind.h")) as _f:
    WIND_SIGNATURES = _parse_header(_f.read(), "include/fdyn_wind.h")[0]
# and the servo on noisy sensors, its Kalman design and its flight on the estimate (include/fdyn_servo_lqg.h): a sixth
with open(os.path.join(os.path.dirname(_HERE), "include", "fdyn_servo_lqg.h")) as _f:
    SERVO_LQG_SIGNATURES = _parse_header(_f.read(), "include/fdyn_servo_lqg.h")[0]
# and the servo's loop margins (include/fdyn_servo_margins.h): a seventh
with open(os.path.join(os.path.dirname(_HERE), "include", "fdyn_servo_margins.h")) as _f:
    SERVO_MARGIN_SIGNATURES = _parse_header(_f.read(), "include/fdyn_servo_margins.h")[0]
# and the servo's flight-mode report (include/fdyn_servo_modes.h): an eighth
with open(os.path.join(os.path.dirname(_HERE), "include", "fdyn_servo_modes.h")) as _f:
    SERVO_MODES_SIGNATURES = _parse_header(_f.read(), "include/fdyn_servo_modes.h")[0]

# and the servo's waypoint missions on noisy sensors (include/fdyn_servo_lqg_mission.h): a ninth
with open(os.path.join(os.path.dirname(_HERE), "include", "fdyn_servo_lqg_mission.h")) as _f:
    SERVO_LQG_MISSION_SIGNATURES = _parse_header(_f.read(), "include/fdyn_servo_lqg_mission.h")[0]
# and the servo's predicted covariances (include/fdyn_servo_covariance.h): a tenth
with open(os.path.join(os.path.dirname(_HERE), "include", "fdyn_servo_covariance.h")) as _f:
    SERVO_COVARIANCE_SIGNATURES = _parse_header(_f.read(), "include/fdyn_servo_covariance.h")[0]
# and the servo gain-scheduled over airspeed (include/fdyn_servo_sched.h): an eleventh
with open(os.path.join(os.path.dirname(_HERE), "include", "fdyn_servo_sched.h")) as _f:
    SERVO_SCHED_SIGNATURES = _parse_header(_f.read(), "include/fdyn_servo_sched.h")[0]
# and the scheduled servo on noisy sensors, its filter scheduled too (include/fdyn_servo_sched_lqg.h): a twelfth
with open(os.path.join(os.path.dirname(_HERE), "include", "fdyn_servo_sched_lqg.h")) as _f:
    SERVO_SCHED_LQG_SIGNATURES = _parse_header(_f.read(), "include/fdyn_servo_sched_lqg.h")[0]
# and the servo's sampled-data design (include/fdyn_servo_dt.h): a thirteenth
with open(os.path.join(os.path.dirname(_HERE), "include", "fdyn_servo_dt.h")) as _f:
    SERVO_DT_SIGNATURES = _parse_header(_f.read(), "include/fdyn_servo_dt.h")[0]

_lib = None


class FdynError(RuntimeError):
    pass


def load():
    """Load the HIP library (once).  Raises if it has not been built -- there is no fallback path."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FdynError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                            "(hipcc --offload-arch=gfx950). The batched flight-dynamics path has no CPU fallback.")
        # the framework's GPU context first.  Observed, cause inside the runtime not established: a process that loads this
        # library BEFORE torch has initialised the GPU (build() followed by smoke(), the README's command) gets hipErrorNoDevice
        # (100) from every launch of the library while torch's own kernels run; torch first, every launch works
        # (tests/test_gpu_launch_image.py: test_library_loaded_before_the_first_gpu_call_still_launches)
        import torch
        if torch.cuda.is_available():
            torch.cuda.init()
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in (*SIGNATURES.items(), *MODES_SIGNATURES.items(), *SERVO_SIGNATURES.items(), *MISSION_SIGNATURES.items(),
                                  *WIND_SIGNATURES.items(), *SERVO_LQG_SIGNATURES.items(), *SERVO_MARGIN_SIGNATURES.items(),
                                  *SERVO_MODES_SIGNATURES.items(), *SERVO_LQG_MISSION_SIGNATURES.items(),
                                  *SERVO_COVARIANCE_SIGNATURES.items(), *SERVO_SCHED_SIGNATURES.items(),
                                  *SERVO_SCHED_LQG_SIGNATURES.items(), *SERVO_DT_SIGNATURES.items()):
            fn = getattr(lib, name)          # AttributeError here = header/library drift
            fn.restype, fn.argtypes = res, args
        if lib.fdyn_abi_version() != FDYN_ABI_VERSION:
            raise FdynError("libfdyn_hip.so ABI version mismatch")
        _lib = lib
    return _lib


_SYNC_DEBUG = bool(os.environ.get("FDYN_SYNC_DEBUG"))


def check(rc, what="fdyn call"):
    if _SYNC_DEBUG:                       # debugging aid: localise an asynchronous GPU fault to one launch
        import sys
        import torch
        print(f"[fdyn] {what} rc={rc} ...", end="", file=sys.stderr, flush=True)
        torch.cuda.synchronize()
        print(" done", file=sys.stderr, flush=True)
    if rc == FDYN_OK:
        return
    if rc == FDYN_ERR_BAD_DT:
        # the reference raises ValueError for dt outside (min_timestep, max_timestep] (simplified_6dof.py:241-245)
        raise ValueError(f"{what}: invalid timestep, must be in (1e-06, 1.0]")
    names = {FDYN_ERR_BAD_TYPES: "n_types outside 1..8", FDYN_ERR_BAD_SIZE: "bad size argument",
             FDYN_ERR_NULL: "required pointer is NULL"}
    raise FdynError(f"{what}: {names.get(rc, 'HIP error ' + str(rc))}")


def ptr(t):
    """Device pointer of a torch tensor (or None -> NULL)."""
    if t is None:
        return None
    assert t.is_contiguous(), "C-ABI arrays must be contiguous"
    return t.data_ptr()


def current_stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def require_gpu():
    import torch
    if not torch.cuda.is_available():
        raise FdynError("no GPU visible: the batched flight-dynamics path runs only on the HIP device (no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


PRECISIONS = ("f64", "mixed", "f32")


def state_dtype(precision):
    import torch
    if precision not in PRECISIONS:
        raise ValueError(f"precision must be one of {PRECISIONS}")
    return torch.float32 if precision == "f32" else torch.float64

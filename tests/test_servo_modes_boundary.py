"""CPU-side checks of the servo modes' boundary: include/fdyn_servo_modes.h parses under the strict header parser into a table of its
own of exactly four entries, the built library exports and `_lib.load()` binds them, the seven older tables are what they were, the
layout constants agree between header, layout.py and the restatement, every refused call returns its code before anything is
launched, and the `*_into` functions refuse host tensors, wrong shapes, dtypes and non-contiguous outputs.  No compute calls (there
is no GPU in the build container)."""
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
NAMES = ("fdyn_servo_flight_modes", "fdyn_servo_sampled_modes", "fdyn_servo_filter_modes", "fdyn_square_modes")
OUTS = [_P, _P, _P, _P, _P, _P]                                  # eig_re, eig_im, summary, iters, status, stream


def _header():
    return open(os.path.join(REPO, "include", "fdyn_servo_modes.h")).read()


def test_header_parses_into_its_own_table():
    table, consts = _lib._parse_header(_header(), "include/fdyn_servo_modes.h")
    assert table == _lib.SERVO_MODES_SIGNATURES and consts == {}
    assert tuple(table) == NAMES
    assert table[NAMES[0]] == (_I, [_P, _P, _P, _P, _I64] + OUTS)            # A, B, x0, K, n
    assert table[NAMES[1]] == (_I, [_P, _P, _P, _D, _I64] + OUTS)            # K, F, x0, dt, n
    assert table[NAMES[2]] == (_I, [_P, _I64] + OUTS)                        # F, n
    assert table[NAMES[3]] == (_I, [_P, _I, _I64] + OUTS)                    # M, N, n
    # fdyn_modes.h's outputs in fdyn_modes.h's order
    assert _lib.MODES_SIGNATURES["fdyn_block_modes"][1][-6:] == OUTS
    older = (_lib.SIGNATURES, _lib.MODES_SIGNATURES, _lib.SERVO_SIGNATURES, _lib.MISSION_SIGNATURES, _lib.WIND_SIGNATURES, _lib.SERVO_LQG_SIGNATURES,
             _lib.SERVO_MARGIN_SIGNATURES)
    assert tuple(len(t) for t in older) == (82, 2, 4, 3, 6, 5, 1)
    assert not any(set(table) & set(t) for t in older)
    assert "oracle" not in _header().lower()


def test_library_exports_and_binds_every_prototype():
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call([sys.executable, "-c", "import __graft_entry__ as g; g.build()"], cwd=REPO)
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert set(re.findall(r"\b(?:int|int64_t)\s+(fdyn_\w+)\s*\(", src)) == set(NAMES)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), f"{name} declared in include/fdyn_servo_modes.h but not exported"
        fn = getattr(_lib.load(), name)
        res, args = _lib.SERVO_MODES_SIGNATURES[name]
        assert fn.restype is res and list(fn.argtypes) == args


def test_the_new_kernels_use_no_scratch_and_spill_no_registers(tmp_path):
    """The window position varies per lane; a matrix indexed by it in registers would become scratch.  Every kernel of
    csrc/servo_modes_kernels.hip, compiled with the library's flags: no private segment, no SGPR or VGPR spill, and the LDS the
    header states (49 words x 64 lanes x 8 B for the servo loops and N = 7)."""
    import __graft_entry__ as g
    assert os.path.exists(g.HIPCC), "no hipcc: the library cannot be built without it either"
    asm = str(tmp_path / "servo_modes.s")
    flags = [f for f in g.HIP_FLAGS if f not in ("-shared", "-fPIC")]
    subprocess.check_call([g.HIPCC, *flags, "--cuda-device-only", "-S", os.path.join(g.CSRC, "servo_modes_kernels.hip"), "-o", asm], stderr=subprocess.DEVNULL)
    text = open(asm).read()
    scratch = [int(v) for v in re.findall(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", text)]
    assert len(scratch) == 9 and not any(scratch)                # flight, sampled, filter and six sizes of the square entry
    assert [int(v) for v in re.findall(r"\.sgpr_spill_count:\s*(\d+)", text)] == [0] * 9
    assert [int(v) for v in re.findall(r"\.vgpr_spill_count:\s*(\d+)", text)] == [0] * 9
    lds = sorted(int(v) for v in re.findall(r"\.amdhsa_group_segment_fixed_size\s+(\d+)", text))
    assert lds == sorted([25088, 25088, 12800] + [N * N * 64 * 8 for N in range(2, 8)])


def test_constants_are_mirrored():
    import servo_modes_numpy as smn
    assert (L.FD_SMO_LON, L.FD_SMO_LAT, L.FD_NSMO_EIG) == (smn.SMO_LON, smn.SMO_LAT, smn.NEIG) == (0, 7, 13)
    assert (L.FD_SMO_FILTER_LON, L.FD_SMO_FILTER_LAT, L.FD_NSMO_FILTER_EIG) == (smn.SMO_FILTER_LON, smn.SMO_FILTER_LAT, smn.NFILTER) == (0, 5, 10)
    assert (L.FD_SMO_MIN_N, L.FD_SMO_MAX_N) == (smn.MIN_N, smn.MAX_N) == (2, 7)
    assert (smn.NLON, smn.NLAT, smn.NB) == (L.FD_SV_NLON, L.FD_SV_NLAT, L.FD_SK_NB)
    assert L.FD_SMO_LAT == L.FD_SV_NLON and L.FD_NSMO_EIG == L.FD_SV_NLON + L.FD_SV_NLAT and L.FD_NSMO_FILTER_EIG == 2 * L.FD_SK_NB
    assert (smn.NOT_CONVERGED, smn.BAD_INPUT, smn.NMO) == (L.FD_MO_NOT_CONVERGED, L.FD_MO_BAD_INPUT, L.FD_NMO)
    # the enums sit in the header that declares the entry points, and layout.py reads them from there
    for name in ("FD_SMO_LON", "FD_NSMO_EIG", "FD_SMO_FILTER_LAT", "FD_SMO_MAX_N"):
        assert re.search(rf"\b{name}\b", _header()) and name in L.__all__
    from hcrl_amd import servo_modes as SMO
    from hcrl_amd import modes as MO
    assert SMO.ServoModes.STATUS_BITS is MO.STATUS_BITS and SMO.LOOPS == ("continuous", "sampled", "filter")
    assert SMO.describe_status(0) == "ok" and SMO.describe_status(L.FD_MO_BAD_INPUT) == "invalid matrix"


def test_refused_calls_need_no_device():
    """FDYN_ERR_BAD_SIZE for n < 1 (fdyn_square_modes: N outside 2 .. 7 as well), FDYN_ERR_NULL for every required pointer, sizes
    before pointers: each with no launch (the pointers are never dereferenced).  summary and iters may be NULL."""
    lib = _lib.load()
    one = ctypes.c_void_p(8)
    outs = [one, one, None, None, one, None]                     # summary = iters = NULL is not an error
    calls = {NAMES[0]: ([one, one, one, one, 5] + outs, 4, (0, 1, 2, 3, 5, 6, 9)),
             NAMES[1]: ([one, one, one, 0.01, 5] + outs, 4, (0, 1, 2, 5, 6, 9)),
             NAMES[2]: ([one, 5] + outs, 1, (0, 2, 3, 6)),
             NAMES[3]: ([one, 4, 5] + outs, 2, (0, 3, 4, 7))}
    for name, (call, n_at, holes) in calls.items():
        fn = getattr(lib, name)

        def with_(at, v, call=call):
            args = list(call)
            args[at] = v
            return args
        for n in (0, -1, 1 << 31):
            assert fn(*with_(n_at, n)) == _lib.FDYN_ERR_BAD_SIZE, (name, n)
        for hole in holes:
            assert fn(*with_(hole, None)) == _lib.FDYN_ERR_NULL, (name, hole)
        args = with_(0, None)
        args[n_at] = 0
        assert fn(*args) == _lib.FDYN_ERR_BAD_SIZE, name
    for N in (1, 0, 8, -3):
        args = list(calls[NAMES[3]][0])
        args[1] = N
        assert lib.fdyn_square_modes(*args) == _lib.FDYN_ERR_BAD_SIZE, N


def test_into_functions_refuse_wrong_arguments():
    from hcrl_amd import servo_modes as SMO
    f64, meta = torch.float64, torch.device("meta")
    n = 3
    A, B = torch.zeros((12, 12, n), dtype=f64), torch.zeros((12, 4, n), dtype=f64)
    x0, K, F = torch.zeros((12, n), dtype=f64), torch.zeros((26, n), dtype=f64), torch.zeros((120, n), dtype=f64)
    M = torch.zeros((7, 7, n), dtype=f64)
    good = {"flight": (SMO.flight_modes_into, (A, B, x0, K)), "sampled": (SMO.sampled_modes_into, (K, F, x0, 0.02)),
            "filter": (SMO.filter_modes_into, (F,)), "square": (SMO.square_modes_into, (M,))}
    wrong = {"flight": ((A[:11], B, x0, K), (A, B[:, :3], x0, K), (A, B, x0[:11], K), (A, B, x0, K[:25]), (A.float(), B, x0, K), (A, B, x0, K.float()),
                        (A, B, x0, K[:, :2]), (A[..., :0], B[..., :0], x0[:, :0], K[:, :0])),
             "sampled": ((K[:25], F, x0, 0.02), (K, F[:80], x0, 0.02), (K, F, x0[:, :2], 0.02), (K, F.float(), x0, 0.02), (K[:, :0], F[:, :0], x0[:, :0], 0.02)),
             "filter": ((F[:119],), (F.float(),), (F.reshape(2, 60, n),), (F[:, :0],)),
             "square": ((M[:6],), (torch.zeros((8, 8, n), dtype=f64),), (torch.zeros((1, 1, n), dtype=f64),), (M.float(),), (M[..., 0],), (M[..., :0],))}
    for key, (fn, args) in good.items():
        for bad in wrong[key]:
            with pytest.raises(ValueError):
                fn(*bad)
        with pytest.raises(ValueError, match="on the GPU"):              # host tensors, everything else in order
            fn(*args)
    for at in range(1, 4):                                               # one device
        args = [A, B, x0, K]
        args[at] = args[at].to(meta)
        with pytest.raises(ValueError, match="expected a tensor on"):
            SMO.flight_modes_into(*args)
    # a caller's report: blocks, dtype, shape, device and contiguity of every word
    for key, sizes in (("flight", (7, 6)), ("sampled", (7, 6)), ("filter", (5, 5)), ("square", (7,))):
        fn, args = good[key]
        with pytest.raises(ValueError, match="on the GPU"):              # a good report on the host: still refused, nothing launched
            fn(*args, out=SMO.empty(n, "cpu", sizes))
        with pytest.raises(ValueError, match="cannot take blocks"):
            fn(*args, out=SMO.empty(n, "cpu", (4, 4)))
        rows = sum(sizes)
        for name, bad in (("eig_re", torch.zeros((rows, n))), ("eig_im", torch.zeros((rows, n + 1), dtype=f64)), ("eig_re", torch.zeros((n, rows), dtype=f64).T),
                          ("summary", torch.zeros((len(sizes), L.FD_NMO, n), dtype=f64, device=meta)), ("iterations", torch.zeros(n, dtype=torch.int64)),
                          ("status", torch.zeros(2 * n, dtype=torch.int32)[::2])):
            r = SMO.empty(n, "cpu", sizes)
            setattr(r, name, bad)
            with pytest.raises(ValueError, match=f"out.{name}"):
                fn(*args, out=r)
    r = SMO.empty(n, "cpu", (7, 6))
    assert r.re(0).shape == (7, n) and r.im(1).shape == (6, n) and r.lon[0].data_ptr() == r.eig_re.data_ptr() and r.eig(1).shape == (6, n)
    assert r.lat[1].data_ptr() == r.eig_im[7:].data_ptr() and r.abscissa().shape == (2, n)
    with pytest.raises(ValueError, match="block must be"):
        r.re(2)
    with pytest.raises(ValueError, match="dt > 0"):
        r.to_s_plane(0, 0.0)


def test_helpers_follow_their_definitions_on_the_host():
    """natural_frequency, damping_ratio, time_constant, time_to_double and to_s_plane are torch ops on the report's words: FleetModes'
    definitions per ragged block."""
    import math
    from hcrl_amd import servo_modes as SMO
    r = SMO.empty(2, "cpu", (7, 6))
    r.eig_re[:] = torch.tensor([[-1.0, 0.5], [-1.0, 0.0], [-2.0, -0.25], [-2.0, -0.25], [-3.0, -1.0], [-4.0, -2.0], [-5.0, -3.0]] + [[-0.5, 0.0]] * 6, dtype=torch.float64)
    r.eig_im[:] = torch.tensor([[2.0, 0.0], [-2.0, 0.0], [0.0, 1.0], [0.0, -1.0]] + [[0.0, 0.0]] * 9, dtype=torch.float64)
    wn = r.natural_frequency(0)
    assert wn[0, 0] == math.sqrt(5.0) and wn[1, 1] == 0.0
    z = r.damping_ratio(0)
    assert z[0, 0] == 1.0 / math.sqrt(5.0) and z[1, 1] == 0.0 and z[0, 1] == -1.0
    assert r.time_constant(0)[0, 0] == 1.0 and r.time_constant(0)[1, 1] == float("inf") and r.time_constant(1)[0, 0] == 2.0
    assert r.time_to_double(0)[0, 1] == math.log(2.0) / 0.5 and r.time_to_double(0)[0, 0] == float("inf")
    r.eig_re[:7, 0] = torch.tensor([0.9, 0.9, 0.5, 0.4, 0.3, 0.2, 0.1], dtype=torch.float64)
    r.eig_im[:7, 0] = torch.tensor([0.1, -0.1, 0.0, 0.0, 0.0, 0.0, 0.0], dtype=torch.float64)
    s = r.to_s_plane(0, 0.02)
    assert torch.allclose(torch.exp(s[:, 0] * 0.02), r.eig(0)[:, 0], rtol=1e-14, atol=0.0)


def test_fleet_guards_need_no_device():
    from hcrl_amd.fleet import BatchedCascade, BatchedSixDOF
    from hcrl_amd.hybrid import HybridFleet
    assert HybridFleet.servo_modes is BatchedSixDOF.servo_modes and BatchedCascade.servo_modes is BatchedSixDOF.servo_modes
    fleet = BatchedSixDOF.__new__(BatchedSixDOF)
    fleet.n = 3
    with pytest.raises(ValueError, match="loop must be one of"):
        fleet.servo_modes("open")
    for loop in ("continuous", "sampled"):
        with pytest.raises(ValueError, match=r"3 of 3 aircraft have no certified stabilising servo gain \(call \.design_servo\(\) first\)"):
            fleet.servo_modes(loop)
    with pytest.raises(ValueError, match=r"3 of 3 aircraft have no certified stable servo filter \(call \.design_servo_kalman\(dt\) first\)"):
        fleet.servo_modes("filter")
    fleet._servo = object()
    with pytest.raises(ValueError, match=r"3 of 3 aircraft have no certified stable servo filter \(call \.design_servo_kalman\(dt\) first\)"):
        fleet.servo_modes("sampled")

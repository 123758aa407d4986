"""CPU-side checks of the flight-mode report's boundary: include/fdyn_modes.h parses under the strict header parser into a table of
its own, the built library exports every prototype it declares and `_lib.load()` binds them, and the table of include/fdyn.h is what
it was.  No compute calls (there is no GPU in the build container)."""
import ctypes
import os
import re
import subprocess
import sys

from conftest import REPO
from hcrl_amd import _lib, layout as L

_P, _I, _I64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64


def _header():
    return open(os.path.join(REPO, "include", "fdyn_modes.h")).read()


def test_modes_header_parses_into_its_own_table():
    table, consts = _lib._parse_header(_header())
    assert table == _lib.MODES_SIGNATURES and consts == {}
    # A, B, K, n, eig_re, eig_im, summary, iters, status, stream
    assert table["fdyn_flight_modes"] == (_I, [_P, _P, _P, _I64, _P, _P, _P, _P, _P, _P])
    # M, n, eig_re, eig_im, summary, iters, status, stream
    assert table["fdyn_block_modes"] == (_I, [_P, _I64, _P, _P, _P, _P, _P, _P])
    assert set(table) == {"fdyn_flight_modes", "fdyn_block_modes"}
    assert len(_lib.SIGNATURES) == 82 and not set(table) & set(_lib.SIGNATURES)
    assert "oracle" not in _header().lower()


def test_library_exports_and_binds_every_modes_prototype():
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call([sys.executable, "-c", "import __graft_entry__ as g; g.build()"], cwd=REPO)
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = set(re.findall(r"\b(?:int|int64_t)\s+(fdyn_\w+)\s*\(", src))
    assert declared == set(_lib.MODES_SIGNATURES) and len(declared) == 2
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(raw, name), f"{name} declared in include/fdyn_modes.h but not exported"
    lib = _lib.load()
    for name, (res, args) in _lib.MODES_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    assert lib.fdyn_abi_version() == _lib.FDYN_ABI_VERSION == 3


def test_refused_calls_need_no_device():
    """n < 1 and a missing required pointer are answered before anything is launched."""
    lib = _lib.load()
    one = ctypes.c_void_p(8)                                             # never dereferenced: every call below is refused
    assert lib.fdyn_flight_modes(one, one, None, 0, one, one, None, None, one, None) == _lib.FDYN_ERR_BAD_SIZE
    assert lib.fdyn_flight_modes(one, one, None, -3, one, one, None, None, one, None) == _lib.FDYN_ERR_BAD_SIZE
    assert lib.fdyn_block_modes(one, 0, one, one, None, None, one, None) == _lib.FDYN_ERR_BAD_SIZE
    for hole in (0, 4, 5, 8):                                            # A, eig_re, eig_im, status
        args = [one, one, None, 5, one, one, None, None, one, None]
        args[hole] = None
        assert lib.fdyn_flight_modes(*args) == _lib.FDYN_ERR_NULL, hole
    assert lib.fdyn_flight_modes(one, None, one, 5, one, one, None, None, one, None) == _lib.FDYN_ERR_NULL      # K without B
    for hole in (0, 2, 3, 6):
        args = [one, 5, one, one, None, None, one, None]
        args[hole] = None
        assert lib.fdyn_block_modes(*args) == _lib.FDYN_ERR_NULL, hole


def test_layout_words():
    assert [L.FD_MO_ABSCISSA, L.FD_MO_RADIUS, L.FD_MO_MIN_ABS, L.FD_MO_MIN_ZETA, L.FD_MO_N_UNSTABLE, L.FD_MO_N_COMPLEX] == list(range(6))
    assert L.FD_NMO == 6 and (L.FD_MO_NOT_CONVERGED, L.FD_MO_BAD_INPUT) == (1, 2)


def test_derived_views_follow_their_definitions():
    """FleetModes' views are plain torch on whatever device the report lives on: here two aircraft on the host, one of them a
    failed lane (all NaN)."""
    import math

    import torch
    from hcrl_amd.modes import FleetModes, describe_status
    nan = float("nan")
    re = torch.tensor([[0.5, nan], [-3.0, nan], [-3.0, nan], [-4.0, nan], [0.0, nan], [-1.0, nan], [-2.0, nan], [-2.0, nan]], dtype=torch.float64)
    im = torch.tensor([[0.0, nan], [4.0, nan], [-4.0, nan], [0.0, nan], [0.0, nan], [0.0, nan], [1.5, nan], [-1.5, nan]], dtype=torch.float64)
    summary = torch.zeros((2, L.FD_NMO, 2), dtype=torch.float64)
    m = FleetModes(re, im, summary, torch.zeros(2, dtype=torch.int32), torch.tensor([0, L.FD_MO_BAD_INPUT], dtype=torch.int32))
    assert m.n == 2 and m.ok.tolist() == [True, False] and m.count_not_ok() == 1
    assert describe_status(0) == "ok" and describe_status(1) == "not converged" and describe_status(2) == "invalid matrix"
    assert tuple(m.eig.shape) == (2, 4, 2) and m.eig.dtype == torch.complex128 and m.eig[0, 1, 0] == complex(-3.0, 4.0)
    assert m.natural_frequency()[:, :, 0].tolist() == [[0.5, 5.0, 5.0, 4.0], [0.0, 1.0, 2.5, 2.5]]
    assert m.damping_ratio()[:, :, 0].tolist() == [[-1.0, 0.6, 0.6, 1.0], [0.0, 1.0, 0.8, 0.8]]                  # 0 for a pole at 0
    assert m.time_constant()[:, :, 0].tolist() == [[-2.0, 1.0 / 3.0, 1.0 / 3.0, 0.25], [math.inf, 1.0, 0.5, 0.5]]
    assert m.time_to_double()[:, :, 0].tolist() == [[math.log(2.0) / 0.5, math.inf, math.inf, math.inf], [math.inf] * 4]
    for view in (m.natural_frequency(), m.damping_ratio(), m.time_constant(), m.time_to_double()):
        assert bool(torch.isnan(view[:, :, 1]).all())                                                              # a failed lane stays NaN
    z = torch.exp(torch.complex(re[:, :1], im[:, :1]) * 0.02)
    back = FleetModes(z.real.contiguous(), z.imag.contiguous(), summary[:, :, :1], m.iterations[:1], m.status[:1]).to_s_plane(0.02)
    assert torch.allclose(back, m.eig[:, :, :1], rtol=0.0, atol=1e-12)


def test_host_tensors_are_refused_before_the_library_sees_them():
    import pytest
    import torch
    from hcrl_amd import modes as MO
    with pytest.raises(ValueError, match="A must be on the GPU"):
        MO.modes_into(torch.zeros((12, 12, 3), dtype=torch.float64), torch.zeros((12, 4, 3), dtype=torch.float64))
    with pytest.raises(ValueError, match="M must be on the GPU"):
        MO.block_modes_into(torch.zeros((2, 4, 4, 3), dtype=torch.float64))
    with pytest.raises(ValueError, match=r"include/fdyn_modes\.h: fdyn_c"):       # the parser names the header it was given
        _lib._parse_header("int fdyn_c(size_t n);", "include/fdyn_modes.h")

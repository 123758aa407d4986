"""Flight modes for whole fleets: where the poles are -- trim -> linearise -> design -> MODES -- open or closed loop, continuous
or sampled, one lane per aircraft.

The design results certify THAT a loop is stable and the margins say how ROBUST it is; `fdyn_flight_modes` and `fdyn_block_modes`
(csrc/modes_kernels.hip) say how well damped and how fast: per aircraft and per block (longitudinal | lateral) the four
eigenvalues in fp64 and six summary words (FD_MO_*).

    fleet.trim(20.0)
    fleet.modes().abscissa()                     # [2][n]: max Re of the open-loop poles of every aircraft
    m = fleet.modes(fleet.design_lqr())          # the poles of a - b K
    m.min_damping(), m.time_constant()           # [2][n], [2][4][n]
    fleet.design_kalman(0.02).filter_poles().spectral_radius()      # [2][n], < 1 for a certified filter

The report is generic -- eigenvalues in canonical order (real part descending, the member of a pair with the positive imaginary
part first) plus per-block summaries; there are no slots named after classical modes, which these airframes do not all have.
Nothing here synchronises with the device except `count_not_ok` and `describe_status` on a tensor element.
"""
import math
from dataclasses import dataclass
from typing import Optional

import torch

from . import _lib, layout as L
from . import trim as T

STATUS_BITS = ((L.FD_MO_NOT_CONVERGED, "not converged"), (L.FD_MO_BAD_INPUT, "invalid matrix"))


@dataclass
class FleetModes(T.StatusResult):
    STATUS_BITS = STATUS_BITS
    FAILURE = "have no eigenvalues"

    eig_re: torch.Tensor                    # [8][n] float64: block 0 in rows 0-3, block 1 in rows 4-7, canonical order
    eig_im: torch.Tensor                    # [8][n] float64
    summary: torch.Tensor                   # [2][FD_NMO][n] float64 (FD_MO_*)
    iterations: torch.Tensor                # [n] int32: QR sweeps of the slower block
    status: torch.Tensor                    # [n] int32: 0, FD_MO_NOT_CONVERGED or FD_MO_BAD_INPUT (every word of the lane is then NaN)

    @property
    def eig(self) -> torch.Tensor:
        """[2][4][n] complex128, assembled from the two real arrays."""
        return torch.complex(self.eig_re, self.eig_im).reshape(2, 4, self.n)

    @property
    def re(self) -> torch.Tensor:
        return self.eig_re.reshape(2, 4, self.n)

    @property
    def im(self) -> torch.Tensor:
        return self.eig_im.reshape(2, 4, self.n)

    def natural_frequency(self) -> torch.Tensor:
        """[2][4][n]: |lambda| (rad/s for a continuous-time matrix)."""
        return torch.sqrt(self.re * self.re + self.im * self.im)

    def damping_ratio(self) -> torch.Tensor:
        """[2][4][n]: -Re / |lambda|, 0 for an eigenvalue at 0 (1 = real and stable, -1 = real and unstable)."""
        wn = self.natural_frequency()
        return torch.where(wn == 0.0, torch.zeros_like(wn), -self.re / wn)

    def time_constant(self) -> torch.Tensor:
        """[2][4][n]: -1 / Re (s; negative for an unstable pole), inf where Re = 0."""
        re = self.re
        return torch.where(re == 0.0, torch.full_like(re, float("inf")), -1.0 / re)

    def time_to_double(self) -> torch.Tensor:
        """[2][4][n]: ln 2 / Re where Re > 0, else inf."""
        re = self.re
        return torch.where(re > 0.0, math.log(2.0) / re, torch.where(re == re, torch.full_like(re, float("inf")), re))

    def abscissa(self) -> torch.Tensor:
        """[2][n]: max Re (< 0: the continuous-time block is stable)."""
        return self.summary[:, L.FD_MO_ABSCISSA]

    def spectral_radius(self) -> torch.Tensor:
        """[2][n]: max |lambda| (< 1: the discrete-time block is Schur)."""
        return self.summary[:, L.FD_MO_RADIUS]

    def min_damping(self) -> torch.Tensor:
        """[2][n]: the smallest damping ratio of the block."""
        return self.summary[:, L.FD_MO_MIN_ZETA]

    def to_s_plane(self, dt: float) -> torch.Tensor:
        """[2][4][n] complex128: ln z / dt, the continuous-time poles a discrete matrix sampled at dt stands for (principal branch:
        frequencies up to the Nyquist rate pi / dt)."""
        if not dt > 0.0:
            raise ValueError(f"to_s_plane: dt > 0, got {dt}")
        return torch.log(self.eig) / float(dt)


describe_status = FleetModes.describe_status                 # 'ok' or the name of the status


def _empty(n: int, dev) -> FleetModes:
    return FleetModes(torch.empty((2 * 4, n), dtype=torch.float64, device=dev), torch.empty((2 * 4, n), dtype=torch.float64, device=dev),
                      torch.empty((2, L.FD_NMO, n), dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
                      torch.empty(n, dtype=torch.int32, device=dev))


def _check_out(out: FleetModes, n: int, dev):
    for name, t, dtype, shape in (("eig_re", out.eig_re, torch.float64, (8, n)), ("eig_im", out.eig_im, torch.float64, (8, n)),
                                  ("summary", out.summary, torch.float64, (2, L.FD_NMO, n)), ("iterations", out.iterations, torch.int32, (n,)),
                                  ("status", out.status, torch.int32, (n,))):
        if t.dtype != dtype or t.device != dev or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"out.{name}: expected a contiguous {dtype} tensor {list(shape)} on {dev}, got {t.dtype} {list(t.shape)} on {t.device}")


def _on_gpu(dev, name: str):
    if dev.type != "cuda":                                     # the kernel would take a host pointer for a device pointer
        raise ValueError(f"{name} must be on the GPU, got a tensor on {dev}")


def modes_into(A: torch.Tensor, B: torch.Tensor, K: Optional[torch.Tensor] = None, out: Optional[FleetModes] = None) -> FleetModes:
    """One launch of fdyn_flight_modes on device tensors: A [12][12][n], B [12][4][n], K [16][n] or None (the open loop), all
    float64; with `out` given nothing is allocated (the form to capture in a graph)."""
    n, dev = int(A.shape[-1]), A.device
    _on_gpu(dev, "A")
    if tuple(A.shape) != (L.FD_NX, L.FD_NX, n) or tuple(B.shape) != (L.FD_NX, L.FD_NU, n):
        raise ValueError(f"expected A [12][12][n] and B [12][4][n], got {tuple(A.shape)} and {tuple(B.shape)}")
    if K is not None and tuple(K.shape) != (L.FD_NLQK, n):
        raise ValueError(f"K: expected [{L.FD_NLQK}][{n}], got {tuple(K.shape)}")
    for name, t in (("A", A), ("B", B), ("K", K)):
        if t is not None and (t.dtype != torch.float64 or t.device != dev):
            raise ValueError(f"{name}: expected float64 on {dev}, got {t.dtype} on {t.device}")
    if out is None:
        out = _empty(n, dev)
    else:
        _check_out(out, n, dev)
    rc = _lib.load().fdyn_flight_modes(_lib.ptr(A), _lib.ptr(B), _lib.ptr(K), n, _lib.ptr(out.eig_re), _lib.ptr(out.eig_im),
                                       _lib.ptr(out.summary), _lib.ptr(out.iterations), _lib.ptr(out.status), _lib.current_stream())
    _lib.check(rc, "fdyn_flight_modes")
    return out


def block_modes_into(M: torch.Tensor, out: Optional[FleetModes] = None) -> FleetModes:
    """One launch of fdyn_block_modes: M [2][4][4][n] float64, two 4 x 4 per aircraft taken as they are (a matrix composed on the
    device, such as KalmanDesign.filter_matrix()); with `out` given nothing is allocated."""
    n, dev = int(M.shape[-1]), M.device
    _on_gpu(dev, "M")
    if tuple(M.shape) != (2, 4, 4, n) or M.dtype != torch.float64:
        raise ValueError(f"M: expected float64 [2][4][4][n], got {M.dtype} {tuple(M.shape)}")
    if out is None:
        M, out = M.contiguous(), _empty(n, dev)
    else:
        _check_out(out, n, dev)
    rc = _lib.load().fdyn_block_modes(_lib.ptr(M), n, _lib.ptr(out.eig_re), _lib.ptr(out.eig_im), _lib.ptr(out.summary),
                                      _lib.ptr(out.iterations), _lib.ptr(out.status), _lib.current_stream())
    _lib.check(rc, "fdyn_block_modes")
    return out


def fleet_modes(trim_result, params: torch.Tensor, type_index=None, scales=None, design=None) -> FleetModes:
    """Linearise every aircraft at its trim (fdyn_linearize at x0, u0), then take its poles: open loop, or under `design.K` (an
    LqrDesign).  params, type_index, scales as `lqr.design_lqr` takes them."""
    A, B = T.linearize_at_trim(trim_result, params, type_index, scales)
    if design is not None and design.n != trim_result.n:
        raise ValueError(f"the design has {design.n} aircraft, the trim {trim_result.n}")
    return modes_into(A, B, None if design is None else design.K)

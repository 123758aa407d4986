"""Flight modes of the LQ servo for whole fleets: where the poles of the servo loop are -- trim -> linearise -> design (gain and
filter) -> MODES -- continuous, as flown at dt, and of the filter's error dynamics, one lane per aircraft.

`fdyn_servo_design` certifies THAT the loop is stable and `fdyn_servo_loop_margins` says how ROBUST it is; the four entry points of
include/fdyn_servo_modes.h (csrc/servo_modes_kernels.hip) say how fast and how well damped: per aircraft the seven longitudinal and
six lateral poles of the augmented closed loop, the same loops sampled at dt with forward-Euler integrators, the five + five poles of
(I - L) Phi, and the poles of any N x N composed on the device, 2 <= N <= 7.

    fleet.trim(20.0); fleet.design_servo(); fleet.design_servo_kalman(dt=0.02)
    m = fleet.servo_modes()                      # loop="continuous" | "sampled" | "filter"
    m.abscissa(), m.min_damping()                # [2][n] each
    m.time_constant(0)                           # [7][n]: -1 / Re of the longitudinal poles, the slowest first
    fleet.servo_modes("sampled").to_s_plane(0, 0.02)   # the sampled poles mapped back: what forward Euler at dt moved

The blocks are ragged (7 | 6, 5 | 5), so the per-pole helpers take the block.  By separation the spectrum of the estimate-feedback
loop is the sampled loop's poles together with the filter's.  A lane whose QR sweeps reach the cap of 30 per deflation has status
FD_MO_NOT_CONVERGED and NaN words, never a wrong pole (about one loop in 7000 of a spread fleet: DESIGN §7o).  Nothing here
synchronises with the device except `count_not_ok` and `describe_status` on a tensor element.
"""
import math
from dataclasses import dataclass
from typing import Optional

import torch

from . import _lib, layout as L
from . import trim as T
from .modes import STATUS_BITS

LOOPS = ("continuous", "sampled", "filter")


@dataclass
class ServoModes(T.StatusResult):
    STATUS_BITS = STATUS_BITS
    FAILURE = "have no eigenvalues"

    eig_re: torch.Tensor                    # [sum of sizes][n] float64: block 0's rows, then block 1's, canonical order
    eig_im: torch.Tensor
    summary: torch.Tensor                   # [blocks][FD_NMO][n] float64 (FD_MO_*)
    iterations: torch.Tensor                # [n] int32: QR sweeps of the slower block
    status: torch.Tensor                    # [n] int32: 0, FD_MO_NOT_CONVERGED or FD_MO_BAD_INPUT (every word of the lane is then NaN)
    sizes: tuple = (L.FD_SV_NLON, L.FD_SV_NLAT)      # eigenvalues per block: (7, 6) servo loops, (5, 5) filter, (N,) square

    def _rows(self, block: int) -> slice:
        if not 0 <= block < len(self.sizes):
            raise ValueError(f"block must be in 0 .. {len(self.sizes) - 1}, got {block}")
        at = sum(self.sizes[:block])
        return slice(at, at + self.sizes[block])

    def re(self, block: int) -> torch.Tensor:
        return self.eig_re[self._rows(block)]

    def im(self, block: int) -> torch.Tensor:
        return self.eig_im[self._rows(block)]

    @property
    def lon(self):
        """(re, im) [N_lon][n] each: views of the longitudinal block."""
        return self.re(0), self.im(0)

    @property
    def lat(self):
        """(re, im) [N_lat][n] each: views of the lateral block."""
        return self.re(1), self.im(1)

    def eig(self, block: int) -> torch.Tensor:
        """[N_block][n] complex128."""
        return torch.complex(self.re(block), self.im(block))

    def natural_frequency(self, block: int) -> torch.Tensor:
        """[N_block][n]: |lambda| (rad/s for a continuous-time matrix)."""
        re, im = self.re(block), self.im(block)
        return torch.sqrt(re * re + im * im)

    def damping_ratio(self, block: int) -> torch.Tensor:
        """[N_block][n]: -Re / |lambda|, 0 for an eigenvalue at 0 (1 = real and stable, -1 = real and unstable)."""
        wn = self.natural_frequency(block)
        return torch.where(wn == 0.0, torch.zeros_like(wn), -self.re(block) / wn)

    def time_constant(self, block: int) -> torch.Tensor:
        """[N_block][n]: -1 / Re (s; negative for an unstable pole), inf where Re = 0."""
        re = self.re(block)
        return torch.where(re == 0.0, torch.full_like(re, float("inf")), -1.0 / re)

    def time_to_double(self, block: int) -> torch.Tensor:
        """[N_block][n]: ln 2 / Re where Re > 0, else inf."""
        re = self.re(block)
        return torch.where(re > 0.0, math.log(2.0) / re, torch.where(re == re, torch.full_like(re, float("inf")), re))

    def to_s_plane(self, block: int, dt: float) -> torch.Tensor:
        """[N_block][n] complex128: ln z / dt, the continuous-time poles a discrete matrix sampled at dt stands for (principal
        branch: frequencies up to the Nyquist rate pi / dt)."""
        if not dt > 0.0:
            raise ValueError(f"to_s_plane: dt > 0, got {dt}")
        return torch.log(self.eig(block)) / float(dt)

    def abscissa(self) -> torch.Tensor:
        """[blocks][n]: max Re (< 0: the continuous-time block is stable)."""
        return self.summary[:, L.FD_MO_ABSCISSA]

    def spectral_radius(self) -> torch.Tensor:
        """[blocks][n]: max |lambda| (< 1: the discrete-time block is Schur)."""
        return self.summary[:, L.FD_MO_RADIUS]

    def min_damping(self) -> torch.Tensor:
        """[blocks][n]: the smallest damping ratio of the block."""
        return self.summary[:, L.FD_MO_MIN_ZETA]


describe_status = ServoModes.describe_status                 # 'ok' or the name of the status


def empty(n: int, device, sizes=(L.FD_SV_NLON, L.FD_SV_NLAT)) -> ServoModes:
    """An unwritten report to pass as `out=`."""
    rows = sum(sizes)
    return ServoModes(torch.empty((rows, n), dtype=torch.float64, device=device), torch.empty((rows, n), dtype=torch.float64, device=device),
                      torch.empty((len(sizes), L.FD_NMO, n), dtype=torch.float64, device=device), torch.empty(n, dtype=torch.int32, device=device),
                      torch.empty(n, dtype=torch.int32, device=device), tuple(sizes))


def _inputs(n: int, named):
    """Shapes, dtypes, one device: everything that can be told without a device, in that order; then that the device is a GPU."""
    if n < 1:
        raise ValueError("expected at least one aircraft")
    dev = named[0][1].device
    for name, t, shape in named:
        if tuple(t.shape) != shape or t.dtype != torch.float64:
            raise ValueError(f"{name}: expected float64 {list(shape)}, got {t.dtype} {list(t.shape)}")
        if t.device != dev:
            raise ValueError(f"{name}: expected a tensor on {dev}, got one on {t.device}")
    return dev


def _output(out: Optional[ServoModes], n: int, dev, sizes) -> ServoModes:
    if out is not None:
        rows = sum(sizes)
        if tuple(out.sizes) != tuple(sizes):
            raise ValueError(f"out: a report of blocks {tuple(out.sizes)} cannot take blocks {tuple(sizes)}")
        for name, t, dtype, shape in (("eig_re", out.eig_re, torch.float64, (rows, n)), ("eig_im", out.eig_im, torch.float64, (rows, n)),
                                      ("summary", out.summary, torch.float64, (len(sizes), L.FD_NMO, n)),
                                      ("iterations", out.iterations, torch.int32, (n,)), ("status", out.status, torch.int32, (n,))):
            if t.dtype != dtype or t.device != dev or tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError(f"out.{name}: expected a contiguous {dtype} tensor {list(shape)} on {dev}, got {t.dtype} {list(t.shape)} on {t.device}")
    if dev.type != "cuda":                                       # the kernel would take a host pointer for a device pointer
        raise ValueError(f"the inputs must be on the GPU, got tensors on {dev}")
    return empty(n, dev, sizes) if out is None else out


def _outs(out: ServoModes):
    return (_lib.ptr(out.eig_re), _lib.ptr(out.eig_im), _lib.ptr(out.summary), _lib.ptr(out.iterations), _lib.ptr(out.status), _lib.current_stream())


def flight_modes_into(A: torch.Tensor, B: torch.Tensor, x0: torch.Tensor, K: torch.Tensor, out: Optional[ServoModes] = None) -> ServoModes:
    """One launch of fdyn_servo_flight_modes on device tensors: A [12][12][n], B [12][4][n], x0 [12][n], K [26][n], all float64; the
    poles of the continuous augmented closed loops.  With `out` given nothing is allocated (the form to capture in a graph)."""
    n = int(A.shape[-1])
    dev = _inputs(n, (("A", A, (L.FD_NX, L.FD_NX, n)), ("B", B, (L.FD_NX, L.FD_NU, n)), ("x0", x0, (L.FD_NX, n)), ("K", K, (L.FD_NSVK, n))))
    out = _output(out, n, dev, (L.FD_SV_NLON, L.FD_SV_NLAT))
    rc = _lib.load().fdyn_servo_flight_modes(_lib.ptr(A), _lib.ptr(B), _lib.ptr(x0), _lib.ptr(K), n, *_outs(out))
    _lib.check(rc, "fdyn_servo_flight_modes")
    return out


def sampled_modes_into(K: torch.Tensor, F: torch.Tensor, x0: torch.Tensor, dt: float, out: Optional[ServoModes] = None) -> ServoModes:
    """One launch of fdyn_servo_sampled_modes: K [26][n], F [120][n] designed at this dt, x0 [12][n]; the poles of the loop as
    `step_servo` flies it in its linear region.  spectral_radius() < 1: stable."""
    n = int(K.shape[-1])
    dev = _inputs(n, (("K", K, (L.FD_NSVK, n)), ("F", F, (L.FD_NSKF, n)), ("x0", x0, (L.FD_NX, n))))
    out = _output(out, n, dev, (L.FD_SV_NLON, L.FD_SV_NLAT))
    rc = _lib.load().fdyn_servo_sampled_modes(_lib.ptr(K), _lib.ptr(F), _lib.ptr(x0), float(dt), n, *_outs(out))
    _lib.check(rc, "fdyn_servo_sampled_modes")
    return out


def filter_modes_into(F: torch.Tensor, out: Optional[ServoModes] = None) -> ServoModes:
    """One launch of fdyn_servo_filter_modes: F [120][n]; the poles of (I - L) Phi, five per block."""
    n = int(F.shape[-1])
    dev = _inputs(n, (("F", F, (L.FD_NSKF, n)),))
    out = _output(out, n, dev, (L.FD_SK_NB, L.FD_SK_NB))
    rc = _lib.load().fdyn_servo_filter_modes(_lib.ptr(F), n, *_outs(out))
    _lib.check(rc, "fdyn_servo_filter_modes")
    return out


def square_modes_into(M: torch.Tensor, out: Optional[ServoModes] = None) -> ServoModes:
    """One launch of fdyn_square_modes: M [N][N][n] float64, one row-major N x N per aircraft taken as it is, 2 <= N <= 7; a report of
    one block."""
    if M.dim() != 3 or M.shape[0] != M.shape[1] or not L.FD_SMO_MIN_N <= int(M.shape[0]) <= L.FD_SMO_MAX_N:
        raise ValueError(f"M: expected [N][N][n] with {L.FD_SMO_MIN_N} <= N <= {L.FD_SMO_MAX_N}, got {tuple(M.shape)}")
    N, n = int(M.shape[0]), int(M.shape[-1])
    dev = _inputs(n, (("M", M, (N, N, n)),))
    if out is None:
        M = M.contiguous()
    out = _output(out, n, dev, (N,))
    rc = _lib.load().fdyn_square_modes(_lib.ptr(M), N, n, *_outs(out))
    _lib.check(rc, "fdyn_square_modes")
    return out


def sampled_poles(design, kalman, x0: Optional[torch.Tensor] = None, out: Optional[ServoModes] = None) -> ServoModes:
    """The poles of the loop `servo.step_into` flies with this ServoDesign at the ServoKalmanDesign's dt (the filter design supplies
    Phi and Gamma).  x0 [12][n]: the trim (None: the servo design's own)."""
    if design.n != kalman.n:
        raise ValueError(f"the servo design has {design.n} aircraft, the servo Kalman design {kalman.n}")
    x0 = design.x0 if x0 is None else x0
    if x0 is None:
        raise ValueError("sampled_poles: the servo design carries no trim; give x0 [12][n]")
    from .servo import check_step
    check_step(design, kalman.dt, "sampled_poles")
    return sampled_modes_into(design.K, kalman.F, x0, float(kalman.dt), out)

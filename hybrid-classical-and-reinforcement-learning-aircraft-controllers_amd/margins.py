"""Loop margins for whole fleets: how much robustness the LQR and LQG loops have AS THEY ARE FLOWN -- sampled at dt, through the
estimator -- trim -> linearise -> design (gain and filter) -> MARGINS -> fly.

The LQR certificate covers the continuous-time loop, the Kalman certificate the filter alone.  `fdyn_loop_margins`
(csrc/margin_kernels.hip) evaluates, per aircraft and per block, the return difference I + L_i(z) at the plant input on a grid of
points z = exp(j omega dt) and reports alpha = min sigma_min(I + L_i): independent gain changes of both control channels inside
[1 / (1 + alpha), 1 / (1 - alpha)], or phase changes up to 2 asin(alpha / 2), keep the sampled linear loop stable.

    fleet.trim(20.0); fleet.design_lqr(); fleet.design_kalman(dt=0.02)
    m = fleet.loop_margins()                     # feedback="estimate" | "measurement" | "truth"
    m.alpha_s.min(dim=0)                         # [n]: the worse block of each aircraft
    m.gain_margin_db(), m.phase_margin_deg()     # [2][n] each (low, high) / degrees

Nothing here synchronises with the device except `count_not_ok` and `describe_status` on a tensor element.
"""
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _lib, layout as L
from .lqg import FEEDBACK
from .trim import StatusResult

STATUS_BITS = ((L.FD_MRG_NOT_STABLE, "nominal loop not certified stable"), (L.FD_MRG_SINGULAR, "a pole on a grid point"),
               (L.FD_MRG_BAD_INPUT, "invalid gain or filter"))
MAX_OMEGA = 256
OMEGA_LOW = 1e-2                                                 # rad/s: where the default grid starts


def default_grid(dt: float, n: int = 64) -> np.ndarray:
    """[n] float64: omega logarithmic from 1e-2 rad/s to the Nyquist rate pi / dt (`unit_circle` stores that point as z = -1)."""
    if not (dt > 0.0) or not 2 <= int(n) <= MAX_OMEGA:
        raise ValueError(f"default_grid: dt > 0 and 2 <= n <= {MAX_OMEGA}, got dt = {dt}, n = {n}")
    w = np.geomspace(OMEGA_LOW, math.pi / dt, int(n))
    w[-1] = math.pi / dt
    return w


def unit_circle(omega, dt: float):
    """(zre, zim) [n] float64: z = exp(j omega dt) for omega strictly increasing in (0, pi / dt]; a point at the Nyquist rate is
    stored exactly as (-1, 0).  The kernel sees only these."""
    w = np.asarray(omega, np.float64)
    if w.ndim != 1 or not 1 <= w.size <= MAX_OMEGA:
        raise ValueError(f"omega: expected 1 to {MAX_OMEGA} grid points in one dimension, got shape {w.shape}")
    if not np.isfinite(w).all() or not (w > 0.0).all() or not (np.diff(w) > 0.0).all():
        raise ValueError("omega must be finite, > 0 and strictly increasing")
    if not (dt > 0.0) or w[-1] > math.pi / dt:
        raise ValueError(f"omega must not exceed the Nyquist rate pi / dt = {math.pi / dt if dt > 0.0 else float('nan'):.6g} rad/s")
    nyquist = w >= math.pi / dt
    return np.where(nyquist, -1.0, np.cos(w * dt)), np.where(nyquist, 0.0, np.sin(w * dt))


@dataclass
class LoopMargins(StatusResult):
    STATUS_BITS = STATUS_BITS

    alpha_s: torch.Tensor                   # [2][n] float64: min over the grid of sigma_min(I + L_i), longitudinal | lateral
    idx_s: torch.Tensor                     # [2][n] int32: the first grid index attaining it (-1: no margin to report)
    alpha_t: torch.Tensor                   # [2][n] float64: min of 1 / sigma_max(T), the complementary-sensitivity disk
    idx_t: torch.Tensor                     # [2][n] int32
    status: torch.Tensor                    # [n] int32: FD_MRG_* bits, 0 = the disk guarantee holds
    curve: Optional[torch.Tensor] = None    # [2][n_omega][n] float64: sigma_min(I + L_i) at every grid point
    omega: Optional[torch.Tensor] = None    # [n_omega] float64 on the device (None: the caller gave z only)
    dt: float = 0.0
    feedback: int = L.FD_LQG_ESTIMATE

    def _omega_at(self, idx: torch.Tensor) -> torch.Tensor:
        if self.omega is None:
            raise ValueError("this report carries no omega grid (margins_into was given z only)")
        w = self.omega[idx.clamp(min=0).long()]
        return torch.where(idx >= 0, w, torch.full_like(w, float("nan")))

    @property
    def omega_s(self) -> torch.Tensor:
        """[2][n]: the frequency (rad/s) at which alpha_s is attained (NaN: no margin to report)."""
        return self._omega_at(self.idx_s)

    @property
    def omega_t(self) -> torch.Tensor:
        return self._omega_at(self.idx_t)

    def gain_margin(self):
        """(low, high) [2][n] each: every pair of channel gains inside [low, high] = [1 / (1 + alpha_s), 1 / (1 - alpha_s)] keeps
        the loop stable (high = +inf where alpha_s >= 1)."""
        a = self.alpha_s
        high = torch.where(a < 1.0, 1.0 / (1.0 - a).clamp(min=1e-300), torch.full_like(a, float("inf")))
        return 1.0 / (1.0 + a), torch.where(a == a, high, a)

    def gain_margin_db(self):
        """(low, high) in dB: 20 log10 of `gain_margin`."""
        low, high = self.gain_margin()
        return 20.0 * torch.log10(low), 20.0 * torch.log10(high)

    def phase_margin_deg(self) -> torch.Tensor:
        """[2][n]: independent phase changes of both channels up to 2 asin(alpha_s / 2) keep the loop stable (180 where alpha_s >= 2)."""
        a = self.alpha_s
        return torch.where(a == a, torch.rad2deg(2.0 * torch.asin((0.5 * a).clamp(max=1.0))), a)


describe_status = LoopMargins.describe_status                # 'ok' or the names of the FD_MRG_* bits set in one status word


def margins_into(K: torch.Tensor, F: torch.Tensor, zre: torch.Tensor, zim: torch.Tensor, feedback="estimate",
                 out: Optional[LoopMargins] = None, curve: bool = False) -> LoopMargins:
    """One launch of fdyn_loop_margins on device tensors: K [16][n], F [80][n], zre / zim [n_omega], all float64; with `out` given
    nothing is allocated (the form to capture in a graph; its `curve` is filled when it has one)."""
    n, dev = int(K.shape[-1]), K.device
    if tuple(K.shape) != (L.FD_NLQK, n) or tuple(F.shape) != (L.FD_NKF, n):
        raise ValueError(f"expected K [{L.FD_NLQK}][n] and F [{L.FD_NKF}][n], got {tuple(K.shape)} and {tuple(F.shape)}")
    if zre.dim() != 1 or zre.shape != zim.shape or not 1 <= int(zre.shape[0]) <= MAX_OMEGA:
        raise ValueError(f"zre, zim: expected two vectors of 1 to {MAX_OMEGA} grid points, got {tuple(zre.shape)} and {tuple(zim.shape)}")
    if any(t.dtype != torch.float64 for t in (K, F, zre, zim)):
        raise ValueError("K, F, zre and zim must be float64")
    if any(t.device != dev for t in (F, zre, zim)):
        raise ValueError("K, F, zre and zim must be on one device")
    fb = FEEDBACK.get(feedback, -1) if isinstance(feedback, str) else int(feedback)
    if fb not in FEEDBACK.values():
        raise ValueError(f"feedback must be one of {tuple(FEEDBACK)}")
    n_omega = int(zre.shape[0])
    if out is None:
        two = lambda dtype: torch.empty((2, n), dtype=dtype, device=dev)
        out = LoopMargins(two(torch.float64), two(torch.int32), two(torch.float64), two(torch.int32), torch.empty(n, dtype=torch.int32, device=dev),
                          torch.empty((2, n_omega, n), dtype=torch.float64, device=dev) if curve else None)
    else:
        if out.n != n or (out.curve is not None and tuple(out.curve.shape) != (2, n_omega, n)):
            raise ValueError(f"out: a report of {out.n} aircraft" + ("" if out.curve is None else f" with curve {tuple(out.curve.shape)}") +
                             f" cannot take {n} aircraft on {n_omega} grid points")
        if curve and out.curve is None:
            raise ValueError("out: curve=True needs a report that has a curve [2][n_omega][n]")
        words = [("alpha_s", out.alpha_s, torch.float64, (2, n)), ("idx_s", out.idx_s, torch.int32, (2, n)), ("alpha_t", out.alpha_t, torch.float64, (2, n)),
                 ("idx_t", out.idx_t, torch.int32, (2, n)), ("status", out.status, torch.int32, (n,))]
        if out.curve is not None:
            words.append(("curve", out.curve, torch.float64, (2, n_omega, n)))
        for name, t, dtype, shape in words:
            if t.dtype != dtype or t.device != dev or tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError(f"out.{name}: expected a contiguous {dtype} tensor {list(shape)} on {dev}, got {t.dtype} {list(t.shape)} on {t.device}")
    rc = _lib.load().fdyn_loop_margins(_lib.ptr(K), _lib.ptr(F), fb, _lib.ptr(zre), _lib.ptr(zim), n_omega, n, _lib.ptr(out.alpha_s),
                                       _lib.ptr(out.idx_s), _lib.ptr(out.alpha_t), _lib.ptr(out.idx_t), _lib.ptr(out.curve), _lib.ptr(out.status),
                                       _lib.current_stream())
    _lib.check(rc, "fdyn_loop_margins")
    out.feedback = fb
    return out


def loop_margins(lqr_design, kalman_design, feedback="estimate", omega=None, curve: bool = False) -> LoopMargins:
    """The margins of the loop `lqg.step_into` flies with these two designs, at the filter's dt.  omega: None (`default_grid`) or
    the frequencies in rad/s, strictly increasing in (0, pi / dt].  Under truth or measurement feedback this is the sampled LQR
    loop: the filter design then only supplies Phi and Gamma."""
    if lqr_design.n != kalman_design.n:
        raise ValueError(f"the LQR design has {lqr_design.n} aircraft, the Kalman design {kalman_design.n}")
    dt = float(kalman_design.dt)
    w = default_grid(dt) if omega is None else np.asarray(omega.detach().cpu() if isinstance(omega, torch.Tensor) else omega, np.float64)
    zre, zim = unit_circle(w, dt)
    dev = lqr_design.K.device
    out = margins_into(lqr_design.K, kalman_design.F, torch.as_tensor(zre, device=dev), torch.as_tensor(zim, device=dev), feedback, None, curve)
    out.omega, out.dt = torch.as_tensor(w, device=dev), dt
    return out

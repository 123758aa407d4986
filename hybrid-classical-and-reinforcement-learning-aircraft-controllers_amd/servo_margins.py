"""Loop margins of the LQ servo for whole fleets: how much robustness the servo loop has AS IT IS FLOWN -- the gain through a
zero-order hold at dt, the integrators advanced by forward Euler, and under estimate feedback through the servo's Kalman filter --
trim -> linearise -> design (gain and filter) -> MARGINS -> fly.

`fdyn_servo_loop_margins` (csrc/servo_margin_kernels.hip, include/fdyn_servo_margins.h) evaluates, per aircraft and per block, the
return difference I + L_i(z) at the plant input of the linear region of `step_servo` / `step_servo_lqg` on a grid of points
z = exp(j omega dt) and reports alpha = min sigma_min(I + L_i), read exactly as `hcrl_amd.margins` reads the regulators': independent
gain changes of both control channels inside [1 / (1 + alpha), 1 / (1 - alpha)], or phase changes up to 2 asin(alpha / 2), keep the
sampled linear loop stable.  The report is `margins.LoopMargins`; the grid is `margins.default_grid` / `margins.unit_circle`.

    fleet.trim(20.0); fleet.design_servo(); fleet.design_servo_kalman(dt=0.02)
    m = fleet.servo_loop_margins()               # feedback="estimate" | "measurement" | "truth"
    m.alpha_s.min(dim=0)                         # [n]: the worse block of each aircraft
    m.gain_margin_db(), m.phase_margin_deg()     # [2][n] each (low, high) / degrees

Nothing here synchronises with the device.
"""
from typing import Optional

import numpy as np
import torch

from . import _lib, layout as L
from .lqg import FEEDBACK
from .margins import MAX_OMEGA, LoopMargins, default_grid, unit_circle
from .servo import check_step


def servo_margins_into(K: torch.Tensor, F: torch.Tensor, x0: torch.Tensor, dt: float, zre: torch.Tensor, zim: torch.Tensor,
                       feedback="estimate", out: Optional[LoopMargins] = None, curve: bool = False) -> LoopMargins:
    """One launch of fdyn_servo_loop_margins on device tensors: K [26][n], F [120][n], x0 [12][n], zre / zim [n_omega], all float64;
    with `out` given nothing is allocated (the form to capture in a graph; its `curve` is filled when it has one)."""
    n, dev = int(K.shape[-1]), K.device
    if tuple(K.shape) != (L.FD_NSVK, n) or tuple(F.shape) != (L.FD_NSKF, n) or tuple(x0.shape) != (L.FD_NX, n):
        raise ValueError(f"expected K [{L.FD_NSVK}][n], F [{L.FD_NSKF}][n] and x0 [{L.FD_NX}][n], got {tuple(K.shape)}, {tuple(F.shape)} and {tuple(x0.shape)}")
    if n < 1:
        raise ValueError("expected at least one aircraft")
    if zre.dim() != 1 or zre.shape != zim.shape or not 1 <= int(zre.shape[0]) <= MAX_OMEGA:
        raise ValueError(f"zre, zim: expected two vectors of 1 to {MAX_OMEGA} grid points, got {tuple(zre.shape)} and {tuple(zim.shape)}")
    if any(t.dtype != torch.float64 for t in (K, F, x0, zre, zim)):
        raise ValueError("K, F, x0, zre and zim must be float64")
    if any(t.device != dev for t in (F, x0, zre, zim)):
        raise ValueError("K, F, x0, zre and zim must be on one device")
    fb = FEEDBACK.get(feedback, -1) if isinstance(feedback, str) else int(feedback)
    if fb not in FEEDBACK.values():
        raise ValueError(f"feedback must be one of {tuple(FEEDBACK)}")
    n_omega = int(zre.shape[0])
    if out is not None:
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
    if dev.type != "cuda":                                       # the last check: everything above can be told without a device
        raise ValueError(f"K, F, x0, zre and zim must be on the GPU, got tensors on {dev}")
    if out is None:
        two = lambda dtype: torch.empty((2, n), dtype=dtype, device=dev)
        out = LoopMargins(two(torch.float64), two(torch.int32), two(torch.float64), two(torch.int32), torch.empty(n, dtype=torch.int32, device=dev),
                          torch.empty((2, n_omega, n), dtype=torch.float64, device=dev) if curve else None)
    rc = _lib.load().fdyn_servo_loop_margins(_lib.ptr(K), _lib.ptr(F), _lib.ptr(x0), float(dt), fb, _lib.ptr(zre), _lib.ptr(zim), n_omega, n,
                                             _lib.ptr(out.alpha_s), _lib.ptr(out.idx_s), _lib.ptr(out.alpha_t), _lib.ptr(out.idx_t),
                                             _lib.ptr(out.curve), _lib.ptr(out.status), _lib.current_stream())
    _lib.check(rc, "fdyn_servo_loop_margins")
    out.feedback, out.dt = fb, float(dt)
    return out


def servo_loop_margins(servo_design, servo_kalman_design, x0: Optional[torch.Tensor] = None, feedback="estimate", omega=None,
                       curve: bool = False) -> LoopMargins:
    """The margins of the loop `servo_lqg.lqg_step_into` flies with these two designs, at the filter's dt.  x0 [12][n]: the trim (None:
    the servo design's own).  omega: None (`default_grid`) or the frequencies in rad/s, strictly increasing in (0, pi / dt].  Under
    truth or measurement feedback this is the sampled servo of `servo.step_into`: the filter design then only supplies Phi and
    Gamma."""
    if servo_design.n != servo_kalman_design.n:
        raise ValueError(f"the servo design has {servo_design.n} aircraft, the servo Kalman design {servo_kalman_design.n}")
    x0 = servo_design.x0 if x0 is None else x0
    if x0 is None:
        raise ValueError("servo_loop_margins: the servo design carries no trim; give x0 [12][n]")
    dt = float(servo_kalman_design.dt)
    check_step(servo_design, dt, "servo_loop_margins")
    w = default_grid(dt) if omega is None else np.asarray(omega.detach().cpu() if isinstance(omega, torch.Tensor) else omega, np.float64)
    zre, zim = unit_circle(w, dt)
    dev = servo_design.K.device
    out = servo_margins_into(servo_design.K, servo_kalman_design.F, x0, dt, torch.as_tensor(zre, device=dev), torch.as_tensor(zim, device=dev),
                             feedback, None, curve)
    out.omega = torch.as_tensor(w, device=dev)
    return out

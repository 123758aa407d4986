"""Predicted performance of the LQ servo for whole fleets: what the designed loop will hold on its sensors -- trim -> linearise ->
gain -> filter -> margins -> modes -> PREDICTED RMS ERRORS AND CHATTER -- without flying it, one lane per aircraft.

`fdyn_servo_loop_margins` says how robust the loop is and `fdyn_servo_*_modes` how fast; the two entry points of
include/fdyn_servo_covariance.h (csrc/servo_covariance_kernels.hip) say how many metres of altitude error it will hold, how good
the estimate will be and how much the surfaces will chatter: the steady-state covariance of the linear loop the margins and the
modes already describe, three small Stein equations per block by Smith doubling.

    fleet.trim(20.0); servo = fleet.design_servo(); fleet.design_servo_kalman(dt=0.01)
    c = fleet.servo_covariance()                 # feedback="estimate" | "measurement" | "truth"
    c.rms_tracking()                             # [3][n]: airspeed (m/s), altitude (m), heading (rad)
    c.chatter()                                  # [4][n]: variance of u_k - u_{k-1}, what `servo_lqg.chatter` adds per step
    c.headroom(servo.u0)                         # [4][n]: distance to the nearer control limit in predicted sigma

A sweep of 65 536 weight or noise candidates is ranked by predicted altitude RMS or chatter in one launch; flights only confirm
the winners.  The loop is taken as linear at the trim: the prediction does not hold where a control reaches its limit (`headroom`
says where), and wraps and error clips are ignored.  Nothing here synchronises with the device except `count_not_ok` and
`describe_status` on a tensor element.
"""
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _lib, layout as L
from . import trim as T
from .lqg import FEEDBACK

STATUS_BITS = ((L.FD_SCV_NOT_CONVERGED, "not converged"), (L.FD_SCV_UNSTABLE, "loop or filter not certified stable"),
               (L.FD_SCV_BAD_INPUT, "invalid gain, filter, noise or dt"))
# set_controls' limits in FD_U_* order: surfaces to [-1, 1], throttle to [0, 1]
CONTROL_LOW, CONTROL_HIGH = (-1.0, -1.0, -1.0, 0.0), (1.0, 1.0, 1.0, 1.0)


@dataclass
class ServoCovariance(T.StatusResult):
    STATUS_BITS = STATUS_BITS
    FAILURE = "have no predicted covariance"

    report: torch.Tensor                    # [FD_NSCV][n] float64: variances (FD_SCV_VAR_*)
    cov: Optional[torch.Tensor]             # [FD_NSCC][n] float64 (FD_SCC_*), or None when not asked for
    residual: torch.Tensor                  # [n] float64: worst relative residual of the equations solved (NaN: nothing solved)
    iterations: torch.Tensor                # [n] int32: doublings of the slowest solve
    status: torch.Tensor                    # [n] int32: FD_SCV_* bits; every word of a lane with a non-zero status is NaN
    feedback: int = L.FD_LQG_ESTIMATE
    dt: float = 0.0

    def _rows(self, at: int, count: int) -> torch.Tensor:
        return self.report[at:at + count]

    def rms_state(self) -> torch.Tensor:
        """[10][n]: RMS of the state's deviation from the trim, (u, w, q, theta, z | v, p, r, phi, psi)."""
        return torch.sqrt(self._rows(L.FD_SCV_VAR_X, L.FD_NSKX))

    def rms_estimate_error(self) -> torch.Tensor:
        """[10][n]: RMS of xhat - d in the same order."""
        return torch.sqrt(self._rows(L.FD_SCV_VAR_EST, L.FD_NSKX))

    def rms_tracking(self) -> torch.Tensor:
        """[3][n]: RMS airspeed (m/s), altitude (m) and heading (rad) error of the true state."""
        return torch.sqrt(self._rows(L.FD_SCV_VAR_ERR, 3))

    def rms_integrators(self) -> torch.Tensor:
        """[3][n]: RMS of i_V, i_h, i_psi."""
        return torch.sqrt(self._rows(L.FD_SCV_VAR_INTEG, 3))

    def rms_control(self) -> torch.Tensor:
        """[4][n]: RMS of the controls about the trim's, FD_U_* order (elevator, aileron, rudder, throttle)."""
        return torch.sqrt(self._rows(L.FD_SCV_VAR_U, L.FD_NU))

    def chatter(self) -> torch.Tensor:
        """[4][n]: variance of u_k - u_{k-1}, FD_U_* order: what `ServoLqgState.chatter` adds per step."""
        return self._rows(L.FD_SCV_VAR_DU, L.FD_NU)

    def expected_accumulators(self, n_steps: int):
        """(err_est [10][n], chatter [4][n]): what a flight of n_steps steps in the steady state would add to
        `ServoLqgState.err_est` and `.chatter`."""
        return self._rows(L.FD_SCV_VAR_EST, L.FD_NSKX) * float(n_steps), self.chatter() * float(n_steps)

    def headroom(self, u0: torch.Tensor) -> torch.Tensor:
        """[4][n]: the distance from the trim controls u0 [4][n] to the nearer `set_controls` limit, in predicted control sigma
        (inf for a control that does not move).  Below about 3 the prediction is not to be trusted: the loop clips and is no
        longer the linear one.  Flown / predicted on the CPU restatement (default sigma, 16 noise rows, 10 s discarded, 30 s
        accumulated):

            condition, feedback                 saturated steps  throttle headroom  chatter           true-error mean squares (V, h, psi)
            rc_plane 20 m/s dt 0.01, estimate   0                8.6                0.989 .. 1.007    1.011, 1.008, 1.066
            cessna 25 m/s dt 0.02, estimate     0                17.0               0.979 .. 1.001    0.971, 1.064, 1.089
            cessna 25 m/s dt 0.02, measurement  0                4.9                0.982 .. 0.998    0.992, 1.061, 1.080
            rc_plane 15 m/s dt 0.02, estimate   43               3.1                0.979 .. 1.006    0.959, 1.081, 1.076
            rc_plane 20 m/s dt 0.01, measurem.  1719             1.9                throttle 0.943    h 1.37
            rc_plane 15 m/s dt 0.02, measurem.  9576             0.7                throttle 0.548    h 15.9
        """
        if tuple(u0.shape) != (L.FD_NU, self.n):
            raise ValueError(f"u0: expected [{L.FD_NU}][{self.n}], got {list(u0.shape)}")
        u0 = u0.to(torch.float64)
        lo = torch.tensor(CONTROL_LOW, dtype=torch.float64, device=u0.device)[:, None]
        hi = torch.tensor(CONTROL_HIGH, dtype=torch.float64, device=u0.device)[:, None]
        return torch.minimum(u0 - lo, hi - u0) / self.rms_control()

    def matrices(self, block: int):
        """(Se [5][5][n], Sxe [NA][5][n], Sx [NA][NA][n]) of block 0 (longitudinal, NA = 7) or 1 (lateral, NA = 6): views of cov."""
        if self.cov is None:
            raise ValueError("the report was computed without cov")
        if block not in (0, 1):
            raise ValueError(f"block must be 0 or 1, got {block}")
        na, nb = (L.FD_SV_NLAT if block else L.FD_SV_NLON), L.FD_SK_NB
        e, xe, x = ((L.FD_SCC_E_LAT, L.FD_SCC_XE_LAT, L.FD_SCC_X_LAT) if block else (L.FD_SCC_E_LON, L.FD_SCC_XE_LON, L.FD_SCC_X_LON))
        return (self.cov[e:e + nb * nb].view(nb, nb, self.n), self.cov[xe:xe + na * nb].view(na, nb, self.n),
                self.cov[x:x + na * na].view(na, na, self.n))


describe_status = ServoCovariance.describe_status                 # 'ok' or the names of the status bits


def empty(n: int, device, cov: bool = True) -> ServoCovariance:
    """An unwritten report to pass as `out=`."""
    f64 = dict(dtype=torch.float64, device=device)
    return ServoCovariance(torch.empty((L.FD_NSCV, n), **f64), torch.empty((L.FD_NSCC, n), **f64) if cov else None, torch.empty(n, **f64),
                           torch.empty(n, dtype=torch.int32, device=device), torch.empty(n, dtype=torch.int32, device=device))


def _feedback(feedback) -> int:
    fb = FEEDBACK.get(feedback, -1) if isinstance(feedback, str) else int(feedback)
    if fb not in FEEDBACK.values():
        raise ValueError(f"feedback must be one of {tuple(FEEDBACK)}")
    return fb


def _noise_rows(name: str, t, n: int, dev):
    """None, [10] or [10][n] -> (contiguous float64 tensor on dev or None, per_lane)."""
    if t is None:
        return None, 0
    if not isinstance(t, torch.Tensor):
        t = torch.as_tensor(np.asarray(t, dtype=np.float64), device=dev)
    if t.dtype != torch.float64 or tuple(t.shape) not in ((L.FD_NSKX,), (L.FD_NSKX, n)):
        raise ValueError(f"{name}: expected float64 [{L.FD_NSKX}] or [{L.FD_NSKX}][{n}], got {t.dtype} {list(t.shape)}")
    if t.device != dev:
        raise ValueError(f"{name}: expected a tensor on {dev}, got one on {t.device}")
    return t.contiguous(), int(t.dim() == 2)


def servo_covariance_into(K: torch.Tensor, F: torch.Tensor, x0: torch.Tensor, dt: float, sigma, w_rate=None, feedback="estimate",
                          out: Optional[ServoCovariance] = None, cov: bool = True) -> ServoCovariance:
    """One launch of fdyn_servo_covariance on device tensors: K [26][n], F [120][n] designed at this dt, x0 [12][n], all float64;
    sigma [10] or [10][n] the measurement noise the loop applies; w_rate None (no process noise, what the flights have), [10] or
    [10][n] in state units per sqrt(s).  With `out` given nothing is allocated (the form to capture in a graph); cov=False (or an
    `out` without cov) skips the 200 covariance rows."""
    fb = _feedback(feedback)
    n = int(K.shape[-1])
    if n < 1:
        raise ValueError("expected at least one aircraft")
    dev = K.device
    for name, t, shape in (("K", K, (L.FD_NSVK, n)), ("F", F, (L.FD_NSKF, n)), ("x0", x0, (L.FD_NX, n))):
        if tuple(t.shape) != shape or t.dtype != torch.float64:
            raise ValueError(f"{name}: expected float64 {list(shape)}, got {t.dtype} {list(t.shape)}")
        if t.device != dev:
            raise ValueError(f"{name}: expected a tensor on {dev}, got one on {t.device}")
    sigma, sigma_per_lane = _noise_rows("sigma", sigma, n, dev)
    if sigma is None:
        raise ValueError("sigma: the measurement noise is required")
    w_rate, w_per_lane = _noise_rows("w_rate", w_rate, n, dev)
    if out is not None:
        for name, t, dtype, shape in (("report", out.report, torch.float64, (L.FD_NSCV, n)), ("cov", out.cov, torch.float64, (L.FD_NSCC, n)),
                                      ("residual", out.residual, torch.float64, (n,)), ("iterations", out.iterations, torch.int32, (n,)),
                                      ("status", out.status, torch.int32, (n,))):
            if name == "cov" and t is None:
                continue
            if t.dtype != dtype or t.device != dev or tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError(f"out.{name}: expected a contiguous {dtype} tensor {list(shape)} on {dev}, got {t.dtype} {list(t.shape)} on {t.device}")
    if dev.type != "cuda":                                       # the kernel would take a host pointer for a device pointer
        raise ValueError(f"the inputs must be on the GPU, got tensors on {dev}")
    if out is None:
        out = empty(n, dev, cov)
    rc = _lib.load().fdyn_servo_covariance(_lib.ptr(K.contiguous()), _lib.ptr(F.contiguous()), _lib.ptr(x0.contiguous()), float(dt), _lib.ptr(sigma),
                                           sigma_per_lane, _lib.ptr(w_rate), w_per_lane, fb, n, _lib.ptr(out.report), _lib.ptr(out.cov),
                                           _lib.ptr(out.residual), _lib.ptr(out.iterations), _lib.ptr(out.status), _lib.current_stream())
    _lib.check(rc, "fdyn_servo_covariance")
    out.feedback, out.dt = fb, float(dt)
    return out


def servo_covariance(servo_design, kalman_design, x0: Optional[torch.Tensor] = None, dt: Optional[float] = None, sigma=None,
                     process_rates=None, feedback="estimate", out: Optional[ServoCovariance] = None) -> ServoCovariance:
    """The predicted covariances of the loop `servo_lqg.lqg_step_into` flies with this ServoDesign and ServoKalmanDesign.  x0: the
    trim (None: the servo design's own); dt: None = the filter's (any other dt is refused: Phi and Gamma were discretised at the
    filter's); sigma: None = `kalman_design.sigma`, the measurement noise `lqg_step_into` applies with this design (a design
    without one is refused: give sigma); process_rates: None = no process noise acts, as in every flight of `step_servo_lqg`."""
    if servo_design.n != kalman_design.n:
        raise ValueError(f"the servo design has {servo_design.n} aircraft, the servo Kalman design {kalman_design.n}")
    x0 = servo_design.x0 if x0 is None else x0
    if x0 is None:
        raise ValueError("servo_covariance: the servo design carries no trim; give x0 [12][n]")
    if dt is not None and float(dt) != float(kalman_design.dt):
        raise ValueError(f"servo_covariance: the filter was designed at dt {kalman_design.dt}, got dt {dt}")
    from .servo import check_step
    check_step(servo_design, kalman_design.dt, "servo_covariance")
    if sigma is None:
        sigma = getattr(kalman_design, "sigma", None)
    if sigma is None:
        raise ValueError("servo_covariance: the Kalman design carries no measurement noise (sigma); give sigma [10] or [10][n]")
    return servo_covariance_into(servo_design.K, kalman_design.F, x0, float(kalman_design.dt), sigma, process_rates, feedback, out)


@dataclass
class SteinSolution(T.StatusResult):
    STATUS_BITS = STATUS_BITS
    FAILURE = "have no solution"

    X: torch.Tensor                         # [N][M][n] float64; NaN in every word of a lane with a non-zero status
    residual: torch.Tensor                  # [n] float64
    iterations: torch.Tensor                # [n] int32
    status: torch.Tensor                    # [n] int32: 0, FD_SCV_NOT_CONVERGED or FD_SCV_BAD_INPUT


def stein_solve(A: torch.Tensor, B: torch.Tensor, Q: torch.Tensor, out: Optional[SteinSolution] = None) -> SteinSolution:
    """One launch of fdyn_stein_solve: X = A X B^T + Q per aircraft, A [N][N][n], B [M][M][n], Q [N][M][n] float64, 1 <= N, M <= 7.
    No stability test first: an unstable pair answers FD_SCV_NOT_CONVERGED."""
    if A.dim() != 3 or B.dim() != 3 or Q.dim() != 3 or A.shape[0] != A.shape[1] or B.shape[0] != B.shape[1]:
        raise ValueError(f"expected A [N][N][n], B [M][M][n], Q [N][M][n], got {tuple(A.shape)}, {tuple(B.shape)}, {tuple(Q.shape)}")
    N, M, n = int(A.shape[0]), int(B.shape[0]), int(A.shape[-1])
    if not (L.FD_SCV_MIN_N <= N <= L.FD_SCV_MAX_N and L.FD_SCV_MIN_N <= M <= L.FD_SCV_MAX_N):
        raise ValueError(f"N and M must be in {L.FD_SCV_MIN_N} .. {L.FD_SCV_MAX_N}, got {N} and {M}")
    if n < 1:
        raise ValueError("expected at least one aircraft")
    dev = A.device
    for name, t, shape in (("A", A, (N, N, n)), ("B", B, (M, M, n)), ("Q", Q, (N, M, n))):
        if tuple(t.shape) != shape or t.dtype != torch.float64:
            raise ValueError(f"{name}: expected float64 {list(shape)}, got {t.dtype} {list(t.shape)}")
        if t.device != dev:
            raise ValueError(f"{name}: expected a tensor on {dev}, got one on {t.device}")
    if out is not None:
        for name, t, dtype, shape in (("X", out.X, torch.float64, (N, M, n)), ("residual", out.residual, torch.float64, (n,)),
                                      ("iterations", out.iterations, torch.int32, (n,)), ("status", out.status, torch.int32, (n,))):
            if t.dtype != dtype or t.device != dev or tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError(f"out.{name}: expected a contiguous {dtype} tensor {list(shape)} on {dev}, got {t.dtype} {list(t.shape)} on {t.device}")
    if dev.type != "cuda":
        raise ValueError(f"the inputs must be on the GPU, got tensors on {dev}")
    if out is None:
        out = SteinSolution(torch.empty((N, M, n), dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.float64, device=dev),
                            torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev))
    rc = _lib.load().fdyn_stein_solve(_lib.ptr(A.contiguous()), _lib.ptr(B.contiguous()), _lib.ptr(Q.contiguous()), N, M, n, _lib.ptr(out.X),
                                      _lib.ptr(out.residual), _lib.ptr(out.iterations), _lib.ptr(out.status), _lib.current_stream())
    _lib.check(rc, "fdyn_stein_solve")
    return out

"""Gain-scheduled LQR for whole fleets: trim -> linearise -> DESIGN -> fly.

The reference derives its PID structure from "linearised rate dynamics near trim" (docs/control_hierarchy_design.tex:282) and
never does the derivation; `hcrl_amd.trim` gives every aircraft its equilibrium and its own A, B.  `fdyn_lqr_design`
(csrc/lqr_kernels.hip) turns those into a state-feedback gain per aircraft -- two 4 x 4 Riccati equations in fp64, one lane per
aircraft, one launch for the fleet -- and `fdyn_lqr_step_*` flies u = u0 - K (x - x0) over the fleets' own integrator.

    fleet = BatchedSixDOF(65536, "mixed", types=("rc_plane", "cessna"), type_index=idx)
    fleet.trim(20.0)
    design = fleet.design_lqr()                  # LqrDesign: K [16][n], status 0 = a certified stabilising gain
    fleet.step_lqr(design, n_steps=100, dt=0.01)

Nothing here synchronises with the device except `describe_status` on a tensor element, `count_not_ok` and the `strict` check,
which read results back on purpose.
"""
from dataclasses import dataclass, fields
from typing import Optional

import numpy as np
import torch

from . import _lib, layout as L
from . import trim as T

STATUS_BITS = ((L.FD_LQR_NOT_CONVERGED, "not converged"), (L.FD_LQR_NO_CERTIFICATE, "no stability certificate"),
               (L.FD_LQR_BAD_INPUT, "invalid model or weights"))


@dataclass
class LqrWeights(T.LaneTable):
    """Bryson's rule: the largest acceptable excursion of each regulated word and of each control; the penalty is 1 / max^2.
    Scalars, or length-n arrays for a sweep of weight sets in one launch (`rows`)."""
    u: object = 2.0            # m/s
    w: object = 2.0            # m/s
    q: object = 0.5            # rad/s
    theta: object = 0.1        # rad
    v: object = 2.0            # m/s
    p: object = 1.0            # rad/s
    r: object = 0.5            # rad/s
    phi: object = 0.2          # rad
    elevator: object = 0.3     # normalised controls, as set_controls takes them
    throttle: object = 0.3
    aileron: object = 0.3
    rudder: object = 0.3

    ENTRY = "LQR maximum"

    def maxima(self):
        """The twelve maxima in FD_LQW_* order."""
        return tuple(getattr(self, f.name) for f in fields(self))

    _entries = maxima

    @staticmethod
    def _values(m: np.ndarray) -> np.ndarray:
        """The penalties `vector` [FD_NLQW] and `rows` [FD_NLQW][n] return: 1 / max^2."""
        with np.errstate(all="ignore"):
            return 1.0 / (m * m)


assert len(fields(LqrWeights)) == L.FD_NLQW


def weights_tensor(weights, n: int, device) -> torch.Tensor:
    """None (the defaults), an LqrWeights, or penalties as an array / tensor [FD_NLQW] or [FD_NLQW][n] -> float64 on the device."""
    if weights is None:
        weights = LqrWeights()
    if isinstance(weights, LqrWeights):
        return torch.as_tensor(weights.rows(n) if weights.per_lane else weights.vector(), device=device)
    return T.table_tensor(weights, n, device, "weights", L.FD_NLQW)


@dataclass
class LqrDesign(T.StatusResult):
    STATUS_BITS = STATUS_BITS
    FAILURE = "have no certified stabilising gain"

    K: torch.Tensor                         # [16][n] float64: K_lon 2 x 4 row-major, then K_lat 2 x 4 (FD_LQK_*)
    residual: torch.Tensor                  # [n] float64: relative Riccati residual of the worse block (NaN: invalid input)
    iterations: torch.Tensor                # [n] int32: doubling steps of the slower block
    status: torch.Tensor                    # [n] int32: FD_LQR_* bits, 0 = a certified stabilising gain
    x0: Optional[torch.Tensor] = None       # [12][n] float64: the point the gains regulate to
    u0: Optional[torch.Tensor] = None       # [4][n]  float64

    def gain_matrix(self) -> torch.Tensor:
        """[4][12][n]: the feedback matrix on the full state (u = u0 - K (x - x0)), zeros outside the two blocks."""
        K = torch.zeros((L.FD_NU, L.FD_NX, self.n), dtype=self.K.dtype, device=self.K.device)
        for base, ctl, states in ((L.FD_LQK_LON, T.LONGITUDINAL_CONTROLS, T.LONGITUDINAL_STATES),
                                  (L.FD_LQK_LAT, T.LATERAL_CONTROLS, T.LATERAL_STATES)):
            for j, c in enumerate(ctl):
                for k, s in enumerate(states):
                    K[c, s] = self.K[base + 4 * j + k]
        return K

    def closed_loop(self, A: torch.Tensor, B: torch.Tensor) -> torch.Tensor:
        """A - B K [12][12][n] on the device."""
        return A - torch.einsum("ikn,kjn->ijn", B, self.gain_matrix())

    def modes(self, A: torch.Tensor, B: torch.Tensor):
        """FleetModes of a - b K per block (one launch of fdyn_flight_modes): the closed-loop poles of the model A, B under these
        gains."""
        from . import modes as MO
        return MO.modes_into(A, B, self.K)


describe_status = LqrDesign.describe_status                  # 'ok' or the names of the FD_LQR_* bits set in one status word


def lqr_into(A: torch.Tensor, B: torch.Tensor, weights: torch.Tensor, out: Optional[LqrDesign] = None) -> LqrDesign:
    """One launch of fdyn_lqr_design on device tensors: A [12][12][n], B [12][4][n], weights [12] or [12][n], all float64; with
    `out` given nothing is allocated (the form to capture in a graph)."""
    n, dev = T.check_model(A, B, weights, "weights", L.FD_NLQW), A.device
    if out is None:
        out = LqrDesign(torch.empty((L.FD_NLQK, n), dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.float64, device=dev),
                        torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev))
    rc = _lib.load().fdyn_lqr_design(_lib.ptr(A), _lib.ptr(B), _lib.ptr(weights), int(weights.dim() == 2), n, _lib.ptr(out.K),
                                     _lib.ptr(out.residual), _lib.ptr(out.iterations), _lib.ptr(out.status), _lib.current_stream())
    _lib.check(rc, "fdyn_lqr_design")
    return out


def design_lqr(trim_result, params: torch.Tensor, type_index=None, scales=None, weights=None) -> LqrDesign:
    """Linearise every aircraft at its trim (fdyn_linearize at x0, u0), then design.  params [n_types][FD_NP] on the device;
    type_index [n] or None; scales as `trim.scale_rows` takes them; weights as `weights_tensor` takes them."""
    A, B = T.linearize_at_trim(trim_result, params, type_index, scales)
    out = lqr_into(A, B, weights_tensor(weights, trim_result.n, A.device))
    out.x0, out.u0 = trim_result.x0, trim_result.u0
    return out


def sampled_poles(design: LqrDesign, kalman):
    """FleetModes of Phi - Gamma Kb per block: the poles of the state-feedback loop as fdyn_lqr_step_* flies it at the step
    `kalman` (a KalmanDesign) was discretised at, composed on the device; spectral_radius() < 1 = Schur."""
    from . import modes as MO
    if design.n != kalman.n:
        raise ValueError(f"the LQR design has {design.n} aircraft, the Kalman design {kalman.n}")
    Kb = torch.stack([design.K[base:base + 8].reshape(2, 4, design.n) for base in (L.FD_LQK_LON, L.FD_LQK_LAT)])
    return MO.block_modes_into(kalman.phi() - torch.einsum("bikn,bkjn->bijn", kalman.gamma(), Kb))


def require_ok(design: LqrDesign, what: str = "design_lqr"):
    """ValueError naming how many lanes have no certified gain, and why for the first of them."""
    design.require_ok(what)


def step_into(precision: str, x: torch.Tensor, design: LqrDesign, params: torch.Tensor, type_index: Optional[torch.Tensor],
              dt: float, n_steps: int, surf_out: Optional[torch.Tensor] = None, sat_steps: Optional[torch.Tensor] = None):
    """One launch of fdyn_lqr_step_<precision>: x [12][n] in the precision's storage type, advanced in place."""
    if design.x0 is None or design.u0 is None:
        raise ValueError("the design carries no trim point (x0, u0)")
    n = int(x.shape[1])
    if x.dtype != _lib.state_dtype(precision) or design.n != n:
        raise ValueError(f"x must be [12][{design.n}] {_lib.state_dtype(precision)}")
    rc = getattr(_lib.load(), f"fdyn_lqr_step_{precision}")(
        _lib.ptr(x), _lib.ptr(design.x0), _lib.ptr(design.u0), _lib.ptr(design.K), _lib.ptr(type_index), _lib.ptr(params),
        int(params.shape[0]), n, float(dt), int(n_steps), _lib.ptr(surf_out), _lib.ptr(sat_steps), _lib.current_stream())
    _lib.check(rc, "fdyn_lqr_step")

"""Steady flight for whole fleets: which state and which controls hold each aircraft in equilibrium, and the linear model there.

The reference states the trim condition (docs/6dof_mathematical_formulation.tex:1380-1410: x_dot = 0, "set controls to
estimated trim values") and derives its PID structure from "linearised rate dynamics near trim"
(docs/control_hierarchy_design.tex:282); it codes neither.  `fdyn_trim` and `fdyn_linearize` (csrc/trim_kernels.hip) do both
on the device, one lane per aircraft, in fp64 over the same equations of motion the fleets integrate.

    res = trim_fleet(65536, airspeed=20.0, climb_angle=np.radians(3), types=("rc_plane", "cessna"), type_index=idx)
    res.ok            # [n] bool: a flyable equilibrium (status == 0)
    fleet.trim(20.0)  # BatchedSixDOF / BatchedCascade / hybrid fleets: solve, then start the fleet there
    A, B = fleet.linearize()

Nothing here synchronises with the device except `TrimResult.surfaces`, `describe_status` and the `strict` check of
`BatchedSixDOF.trim`, which read results back on purpose.
"""
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, layout as L
from .flight_types import ControlSurfaces
from .params import param_table

STATUS_BITS = ((L.FD_TRIM_NOT_CONVERGED, "not converged"), (L.FD_TRIM_CONTROL_RANGE, "control out of range"),
               (L.FD_TRIM_ALPHA_LIMIT, "angle of attack at its limit"), (L.FD_TRIM_PITCH_LIMIT, "pitch at its limit"),
               (L.FD_TRIM_BAD_SPEC, "invalid flight condition"))
# rows / columns of the two classical sub-systems inside A [12][12] and B [12][4]
LONGITUDINAL_STATES = (L.FD_X_U, L.FD_X_W, L.FD_X_Q, L.FD_X_PITCH)
LONGITUDINAL_CONTROLS = (L.FD_U_ELEVATOR, L.FD_U_THROTTLE)
LATERAL_STATES = (L.FD_X_V, L.FD_X_P, L.FD_X_R, L.FD_X_ROLL)
LATERAL_CONTROLS = (L.FD_U_AILERON, L.FD_U_RUDDER)


def status_names(bits, status: int) -> str:
    """'ok' or the comma-joined names of the (bit, name) pairs of `bits` that are set in one status word."""
    names = [name for bit, name in bits if int(status) & bit]
    return ", ".join(names) if names else "ok"


class StatusResult:
    """What TrimResult, LqrDesign, KalmanDesign, LoopMargins and FleetModes share: the reading of their `status` [n] int32.  A subclass names
    its module's STATUS_BITS and, where it has a strict check, what its failed lanes lack (FAILURE)."""
    STATUS_BITS = ()
    FAILURE = "have a non-zero status"

    @property
    def n(self) -> int:
        return int(self.status.shape[0])

    @property
    def ok(self) -> torch.Tensor:
        return self.status == 0

    def count_not_ok(self) -> int:
        return int((self.status != 0).sum())

    @classmethod
    def describe_status(cls, status: int) -> str:
        """'ok' or the names of the module's status bits set in one status word."""
        return status_names(cls.STATUS_BITS, status)

    def require_ok(self, what: str):
        """ValueError naming how many lanes have a non-zero status, and why for the first of them."""
        bad = self.count_not_ok()
        if bad:
            first = int(torch.nonzero(self.status != 0)[0])
            raise ValueError(f"{what}: {bad} of {self.n} aircraft {self.FAILURE} "
                             f"(first: aircraft {first}: {self.describe_status(int(self.status[first]))})")


def broadcast_rows(n: int, values: Sequence, what: str = "value") -> np.ndarray:
    """Scalars or length-n arrays -> float64 [len(values)][n]; anything else is a ValueError naming the offender."""
    out = np.empty((len(values), int(n)), dtype=np.float64)
    for k, v in enumerate(values):
        a = np.asarray(v.detach().cpu() if isinstance(v, torch.Tensor) else v, dtype=np.float64)
        if a.ndim > 1 or (a.ndim == 1 and a.shape[0] not in (1, n)):
            raise ValueError(f"{what} {k}: expected a scalar or {n} values, got shape {a.shape}")
        out[k] = a
    return out


def flight_condition(n: int, airspeed, climb_angle=0.0, turn_rate=0.0, altitude=100.0, heading=0.0) -> np.ndarray:
    """spec [FD_NTS][n] float64 in FD_TS_* order."""
    return broadcast_rows(n, (airspeed, climb_angle, turn_rate, altitude, heading), "flight condition word")


def scale_rows(n: int, scales, device) -> Optional[torch.Tensor]:
    """None, five scalars / length-n arrays (mass, Ixx, Iyy, Izz, air density), or an array / tensor [FD_NSC][n]
    -> float64 [FD_NSC][n] on the device (None stays None: every multiplier 1)."""
    if scales is None:
        return None
    if isinstance(scales, torch.Tensor):
        if tuple(scales.shape) != (L.FD_NSC, n):
            raise ValueError(f"scales: expected [{L.FD_NSC}][{n}], got {tuple(scales.shape)}")
        return scales.to(device=device, dtype=torch.float64).contiguous()
    if len(scales) != L.FD_NSC:
        raise ValueError(f"scales: expected {L.FD_NSC} rows (mass, Ixx, Iyy, Izz, air density), got {len(scales)}")
    return torch.as_tensor(broadcast_rows(n, tuple(scales), "scale row"), device=device)


class LaneTable:
    """What LqrWeights and KalmanNoise share: a design table whose `_entries()` are scalars, or length-n arrays for a sweep of
    tables in one launch (`rows`); `_values` maps the entries to what the kernel reads."""
    ENTRY = "entry"                                   # what broadcast_rows calls an offending entry

    @staticmethod
    def _values(entries: np.ndarray) -> np.ndarray:
        return entries

    @property
    def per_lane(self) -> bool:
        return any(np.ndim(v.detach().cpu() if isinstance(v, torch.Tensor) else v) > 0 for v in self._entries())

    def vector(self) -> np.ndarray:
        """[len(entries)] float64 (every entry a scalar)."""
        return self._values(np.array([float(np.asarray(v).reshape(())) for v in self._entries()], dtype=np.float64))

    def rows(self, n: int) -> np.ndarray:
        """[len(entries)][n] float64: scalars broadcast, length-n arrays taken per aircraft."""
        return self._values(broadcast_rows(n, self._entries(), self.ENTRY))


def check_table(table: torch.Tensor, n: int, name: str, rows: int):
    if tuple(table.shape) not in ((rows,), (rows, n)):
        raise ValueError(f"{name}: expected [{rows}] or [{rows}][{n}], got {tuple(table.shape)}")


def table_tensor(table, n: int, device, name: str, rows: int) -> torch.Tensor:
    """An array / tensor [rows] or [rows][n] -> contiguous float64 on the device; `name` is the caller's word for it."""
    w = table if isinstance(table, torch.Tensor) else torch.as_tensor(np.asarray(table, np.float64))
    check_table(w, n, name, rows)
    return w.to(device=device, dtype=torch.float64).contiguous()


def check_model(A: torch.Tensor, B: torch.Tensor, table: torch.Tensor, name: str, rows: int) -> int:
    """n of a linear model A [12][12][n], B [12][4][n] and its design table [rows] or [rows][n], all float64."""
    n = int(A.shape[-1])
    if tuple(A.shape) != (L.FD_NX, L.FD_NX, n) or tuple(B.shape) != (L.FD_NX, L.FD_NU, n):
        raise ValueError(f"expected A [12][12][n] and B [12][4][n], got {tuple(A.shape)} and {tuple(B.shape)}")
    check_table(table, n, name, rows)
    if A.dtype != torch.float64 or B.dtype != torch.float64 or table.dtype != torch.float64:
        raise ValueError(f"A, B and {name} must be float64")
    return n


@dataclass
class TrimResult(StatusResult):
    STATUS_BITS = STATUS_BITS
    FAILURE = "have no flyable equilibrium at the requested condition"

    x0: torch.Tensor            # [12][n] float64: the equilibrium state (FD_X_* rows)
    u0: torch.Tensor            # [4][n]  float64: elevator, aileron, rudder, throttle as set_controls takes them, NOT clipped
    residual: torch.Tensor      # [n] float64: max |F| at the returned point
    iterations: torch.Tensor    # [n] int32
    status: torch.Tensor        # [n] int32: FD_TRIM_* bits

    @property
    def alpha(self) -> torch.Tensor:
        """Angle of attack [n] (rad): the lateral velocity of a trim is zero, so atan2(w, u)."""
        return torch.atan2(self.x0[L.FD_X_W], self.x0[L.FD_X_U])

    @property
    def bank(self) -> torch.Tensor:
        return self.x0[L.FD_X_ROLL]

    def surfaces(self, i: int = 0) -> ControlSurfaces:
        e, a, r, t = self.u0[:, i].cpu().tolist()
        return ControlSurfaces(elevator=e, aileron=a, rudder=r, throttle=t)


describe_status = TrimResult.describe_status                 # 'ok' or the names of the FD_TRIM_* bits set in one status word


def _type_tensor(n, type_index, device):
    if type_index is None:
        return None
    if isinstance(type_index, torch.Tensor):
        t = type_index.to(device=device, dtype=torch.uint8).contiguous()
    else:
        t = torch.as_tensor(np.ascontiguousarray(np.asarray(type_index, np.uint8)), device=device)
    if tuple(t.shape) != (n,):
        raise ValueError(f"type_index: expected {n} entries, got shape {tuple(t.shape)}")
    return t


def trim_into(spec: torch.Tensor, params: torch.Tensor, type_index: Optional[torch.Tensor], scales: Optional[torch.Tensor],
              out: Optional[TrimResult] = None) -> TrimResult:
    """One launch of fdyn_trim on device tensors; with `out` given nothing is allocated (the form to capture in a graph)."""
    n, dev = int(spec.shape[1]), spec.device
    if out is None:
        out = TrimResult(torch.empty((L.FD_NX, n), dtype=torch.float64, device=dev),
                         torch.empty((L.FD_NU, n), dtype=torch.float64, device=dev),
                         torch.empty(n, dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
                         torch.empty(n, dtype=torch.int32, device=dev))
    rc = _lib.load().fdyn_trim(_lib.ptr(spec), _lib.ptr(type_index), _lib.ptr(scales), _lib.ptr(params), int(params.shape[0]), n,
                               _lib.ptr(out.x0), _lib.ptr(out.u0), _lib.ptr(out.residual), _lib.ptr(out.iterations),
                               _lib.ptr(out.status), _lib.current_stream())
    _lib.check(rc, "fdyn_trim")
    return out


def linearize_into(x: torch.Tensor, u: torch.Tensor, params: torch.Tensor, type_index: Optional[torch.Tensor],
                   scales: Optional[torch.Tensor], out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
    """One launch of fdyn_linearize: x [12][n], u [4][n], both float64 or both float32 -> A [12][12][n], B [12][4][n]."""
    if x.dtype != u.dtype or x.dtype not in (torch.float32, torch.float64):
        raise ValueError("x and u must both be float64 or both float32")
    n, dev = int(x.shape[1]), x.device
    if out is None:
        out = (torch.empty((L.FD_NX, L.FD_NX, n), dtype=torch.float64, device=dev),
               torch.empty((L.FD_NX, L.FD_NU, n), dtype=torch.float64, device=dev))
    rc = _lib.load().fdyn_linearize(_lib.ptr(x), _lib.ptr(u), int(x.dtype == torch.float32), _lib.ptr(type_index), _lib.ptr(scales),
                                    _lib.ptr(params), int(params.shape[0]), n, _lib.ptr(out[0]), _lib.ptr(out[1]),
                                    _lib.current_stream())
    _lib.check(rc, "fdyn_linearize")
    return out


def linearize_at_trim(trim_result: TrimResult, params: torch.Tensor, type_index=None, scales=None):
    """(A, B) of every aircraft at its trim (fdyn_linearize at x0, u0): what design_lqr and design_kalman design on.  params
    [n_types][FD_NP] on the device; type_index [n] or None; scales as `scale_rows` takes them."""
    n, dev = trim_result.n, trim_result.x0.device
    return linearize_into(trim_result.x0, trim_result.u0, params, _type_tensor(n, type_index, dev), scale_rows(n, scales, dev))


def trim_fleet(n: int, airspeed, climb_angle=0.0, turn_rate=0.0, altitude=100.0, heading=0.0, types: Sequence = ("rc_plane",),
               type_index=None, scales=None, device=None) -> TrimResult:
    """Trim n aircraft: scalars or length-n arrays per flight-condition word, `types` the airframes and `type_index` [n] which
    of them each aircraft is (None: the first), `scales` per-aircraft multipliers on mass, Ixx, Iyy, Izz, air density."""
    n = int(n)
    spec_host = flight_condition(n, airspeed, climb_angle, turn_rate, altitude, heading)
    device = device or _lib.require_gpu()
    params = torch.as_tensor(param_table(types), device=device).contiguous()
    return trim_into(torch.as_tensor(spec_host, device=device), params, _type_tensor(n, type_index, device),
                     scale_rows(n, scales, device))


def _block(M, rows, cols):
    return M[list(rows)][:, list(cols)]


def longitudinal_block(A, B):
    """(u, w, q, theta | elevator, throttle) sub-system of A [12][12][...] and B [12][4][...] -> ([4][4][...], [4][2][...])."""
    return _block(A, LONGITUDINAL_STATES, LONGITUDINAL_STATES), _block(B, LONGITUDINAL_STATES, LONGITUDINAL_CONTROLS)


def lateral_block(A, B):
    """(v, p, r, phi | aileron, rudder) sub-system -> ([4][4][...], [4][2][...])."""
    return _block(A, LATERAL_STATES, LATERAL_STATES), _block(B, LATERAL_STATES, LATERAL_CONTROLS)


def require_ok(result: TrimResult, what: str = "trim"):
    """ValueError naming how many lanes are not a flyable equilibrium, and why for the first of them."""
    result.require_ok(what)

"""Domain randomisation of the rate env: wind, gusts, per-env mass, inertia and air density.

The ranges follow the reference's design (design_docs/06_RL_AGENT_TRAINING.md "Domain Randomization", `DomainRandomizer`);
the kernels draw from them at every reset (`fdyn_rate_env_{reset,step}_dr_*`, include/fdyn.h).  Each key is a `[lo, hi]`
pair or a scalar (a fixed value):

  wind_speed            m/s, steady wind magnitude                    wind_direction   rad, NED heading the air moves toward
  wind_vertical         m/s, positive down                           turbulence_intensity  gust sigma / reset airspeed
  gust_length           m, length scale L of the gust process        mass, inertia_xx/yy/zz, air_density  multipliers

`redraw: false` keeps whatever the rows hold across resets (fixed-condition evaluation: write `env.dr` yourself).
"""
from dataclasses import dataclass, fields
from typing import Optional, Tuple

import numpy as np

from . import layout as L

Range = Tuple[float, float]

# key -> (dr_consts lo slot, kind): kind picks the validation rule
_KEYS = {
    "wind_speed": (L.FD_DC_WIND_SPEED_LO, "nonneg"),
    "wind_direction": (L.FD_DC_WIND_DIR_LO, "any"),
    "wind_vertical": (L.FD_DC_WIND_VERT_LO, "any"),
    "turbulence_intensity": (L.FD_DC_TURB_LO, "nonneg"),
    "gust_length": (L.FD_DC_GUST_L_LO, "positive"),
    "mass": (L.FD_DC_MASS_LO, "positive"),
    "inertia_xx": (L.FD_DC_IXX_LO, "positive"),
    "inertia_yy": (L.FD_DC_IYY_LO, "positive"),
    "inertia_zz": (L.FD_DC_IZZ_LO, "positive"),
    "air_density": (L.FD_DC_RHO_LO, "positive"),
}


def _pair(key, v) -> Range:
    if np.isscalar(v):
        lo = hi = float(v)
    else:
        v = list(v)
        if len(v) != 2:
            raise ValueError(f"domain_randomization.{key}: expected a scalar or a [lo, hi] pair, got {v!r}")
        lo, hi = float(v[0]), float(v[1])
    if not (np.isfinite(lo) and np.isfinite(hi)):
        raise ValueError(f"domain_randomization.{key}: non-finite bound")
    if lo > hi:
        raise ValueError(f"domain_randomization.{key}: lo {lo} > hi {hi}")
    kind = _KEYS[key][1]
    if kind == "nonneg" and lo < 0:
        raise ValueError(f"domain_randomization.{key}: must be >= 0, got {lo}")
    if kind == "positive" and lo <= 0:
        raise ValueError(f"domain_randomization.{key}: must be > 0, got {lo}")
    return lo, hi


@dataclass
class Disturbances:
    """Ranges of the per-episode draws.  The defaults are neutral: still air, no gusts, every multiplier 1."""
    wind_speed: Range = (0.0, 0.0)
    wind_direction: Range = (0.0, 0.0)
    wind_vertical: Range = (0.0, 0.0)
    turbulence_intensity: Range = (0.0, 0.0)
    gust_length: Range = (100.0, 100.0)
    mass: Range = (1.0, 1.0)
    inertia_xx: Range = (1.0, 1.0)
    inertia_yy: Range = (1.0, 1.0)
    inertia_zz: Range = (1.0, 1.0)
    air_density: Range = (1.0, 1.0)
    redraw: bool = True
    enabled: bool = True

    def __post_init__(self):
        for k in _KEYS:
            setattr(self, k, _pair(k, getattr(self, k)))

    @classmethod
    def from_config(cls, cfg: Optional[dict]) -> "Disturbances":
        """From a `domain_randomization:` mapping (unknown keys raise; missing keys stay neutral)."""
        cfg = dict(cfg or {})
        known = {f.name for f in fields(cls)}
        bad = set(cfg) - known
        if bad:
            raise ValueError(f"domain_randomization: unknown key(s) {sorted(bad)}")
        kw = {k: (bool(v) if k in ("redraw", "enabled") else _pair(k, v)) for k, v in cfg.items()}
        return cls(**kw)

    @classmethod
    def design_doc(cls) -> "Disturbances":
        """The ranges of design_docs/06_RL_AGENT_TRAINING.md (DomainRandomizer), gust length 100 m."""
        return cls(wind_speed=(0.0, 5.0), wind_direction=(0.0, 2 * np.pi), turbulence_intensity=(0.0, 0.3),
                   mass=(0.9, 1.1), inertia_xx=(0.8, 1.2), inertia_yy=(0.8, 1.2), inertia_zz=(0.8, 1.2),
                   air_density=(0.95, 1.05))

    def block(self) -> np.ndarray:
        """The fp64 dr_consts [FD_NDC] block (include/fdyn_layout.h, FD_DC_*)."""
        b = np.zeros(L.FD_NDC, np.float64)
        for k, (slot, _) in _KEYS.items():
            b[slot], b[slot + 1] = getattr(self, k)
        b[L.FD_DC_REDRAW] = 1.0 if self.redraw else 0.0
        return b

    def to_config(self) -> dict:
        d = {k: list(getattr(self, k)) for k in _KEYS}
        d["redraw"], d["enabled"] = self.redraw, self.enabled
        return d


def neutral_rows(n: int) -> np.ndarray:
    """dr [FD_NDR][n] of still air and unit multipliers (what a fresh env holds before its first reset)."""
    r = np.zeros((L.FD_NDR, n), np.float64)
    r[L.FD_DR_MASS_S:L.FD_DR_RHO_S + 1] = 1.0
    return r


def as_disturbances(d) -> Optional["Disturbances"]:
    """None / Disturbances / config mapping -> Disturbances or None (a mapping with `enabled: false` is None)."""
    if d is None:
        return None
    if not isinstance(d, Disturbances):
        d = Disturbances.from_config(d)
    return d if d.enabled else None

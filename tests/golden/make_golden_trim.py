#!/usr/bin/env python3
"""Steady-flight fixtures, from the reference's own equations of motion: the Newton iteration and the central differences of
include/fdyn.h (fdyn_trim, fdyn_linearize), run in NumPy (tests/trim_numpy.py) over the reference's
`Simplified6DOF._dynamics` -- which takes its controls as an argument, so they are passed unclipped.

Runs only in the build container (needs /root/reference and `make -C oracle ref`); about a minute.
Writes tests/golden/trim_reference.npz.  DATA only (inputs + expected outputs):
  feasible grid   {rc_plane, cessna} x V {15, 20, 25, 30} x gamma {0, 3, 5 deg} x turn rate {0, 0.1, -0.1, 0.3} x mass scale
                  {0.8, 1, 1.2} = 288 aircraft: type, spec, scales, z, x0, u0, residual, iters, status, and A, B at the trim
  infeasible set  the 8 conditions of tests/trim_numpy.py::infeasible_set on both airframes: the same words, A and B only
                  where the iteration converged (NaN elsewhere)
tests/test_trim_oracle.py repeats the computation over the CPU oracle and compares; tests/test_gpu_trim.py uses both.
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = os.environ.get("REFERENCE_ROOT", "/root/reference")


def main():
    sys.dont_write_bytecode = True
    sys.path.insert(0, os.path.join(REPO, "oracle", "_ref"))
    sys.path.insert(0, REF)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import trim_numpy as tn
    from controllers.types import ControlSurfaces
    from simulation import AircraftParams, Simplified6DOF, SimulationAircraftBackend

    def airframe(name, scales):
        base = SimulationAircraftBackend({"aircraft_type": name})._get_aircraft_params(name)
        kw = dict(vars(base))
        for field, s in zip(("mass", "inertia_xx", "inertia_yy", "inertia_zz", "air_density"), scales):
            kw[field] = kw[field] * s
        sim = Simplified6DOF(AircraftParams(**kw))
        f = lambda x, u: sim._dynamics(np.asarray(x, np.float64), ControlSurfaces(elevator=u[0], aileron=u[1], rudder=u[2], throttle=u[3]))  # noqa: E731
        return f, sim.params.gravity, sim._max_alpha_rad, sim._max_pitch_rad

    def solve(ty, spec, scales):
        n = len(ty)
        out = dict(z=np.zeros((n, 7)), x0=np.zeros((n, 12)), u0=np.zeros((n, 4)), residual=np.zeros(n), iters=np.zeros(n, np.int32),
                   status=np.zeros(n, np.int32), A=np.full((n, 12, 12), np.nan), B=np.full((n, 12, 4), np.nan))
        for i in range(n):
            f, g, max_alpha, max_pitch = airframe(tn.TYPES[ty[i]], scales[i])
            r = tn.trim(f, spec[i], g, max_alpha, max_pitch)
            for k in ("z", "x0", "u0", "residual", "iters", "status"):
                out[k][i] = r[k]
            if not r["status"] & (tn.NOT_CONVERGED | tn.BAD_SPEC):
                out["A"][i], out["B"][i] = tn.linearize(f, r["x0"], r["u0"])
        return out

    ty, spec, scales = tn.feasible_grid()
    feas = solve(ty, spec, scales)
    assert np.all(feas["status"] == 0), np.flatnonzero(feas["status"])
    print(f"feasible grid: {len(ty)} aircraft, iterations {feas['iters'].min()}..{feas['iters'].max()}, "
          f"worst residual {feas['residual'].max():.2e}")
    ity, ispec, want = tn.infeasible_set()
    inf = solve(ity, ispec, np.ones((len(ity), 5)))
    for i, (must_set, must_clear) in enumerate(want):
        s = int(inf["status"][i])
        print(f"  infeasible {i:2d} {tn.TYPES[ity[i]]:8s} V = {ispec[i, 0]:5.1f} gamma = {np.degrees(ispec[i, 1]):4.1f}: status {s:2d}, "
              f"iters {inf['iters'][i]:2d}, alpha {inf['z'][i, 0]: .3f}, throttle {inf['z'][i, 6]: .3f}")
        assert s & must_set == must_set and not s & must_clear, (i, s, must_set, must_clear)
    data = {"type": ty, "spec": spec, "scales": scales, **feas}
    data.update({"inf_type": ity, "inf_spec": ispec, **{"inf_" + k: v for k, v in inf.items()}})
    path = os.path.join(REPO, "tests", "golden", "trim_reference.npz")
    np.savez_compressed(path, **data)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()

"""The LQ servo on the CPU: the NumPy restatement (tests/servo_numpy.py) of fdyn_servo_design against an independent solution of
the same Riccati equations, and of the control law flown over the CPU oracle's RK4 to commands.

Gates (none derived from what the restatement returns):
  design   X against the stable invariant subspace of the Hamiltonian (numpy.linalg.eig): 1e-9 relative; every X positive
           definite (numpy.linalg.eigvalsh), residual <= 1e-10; every block within 12 doublings
  flight   the four probe conditions, +4 m/s, +30 m and +60 deg commanded at t = 1 s: at 40 s |e_V| <= 1e-3 m/s, |e_h| <= 1e-3 m,
           |e_psi| <= 1e-4 rad; |roll| <= 1.3 rad and |pitch| <= 0.9 rad throughout
"""
import os

import numpy as np
import pytest

import servo_numpy as sn
from conftest import GOLDEN


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "trim_reference.npz"))


def _hamiltonian_solution(a, b, q, r):
    """X = U2 U1^-1 from the eigenvectors of the stable eigenvalues of [[a, -G], [-Q, -a^T]]: shares no code with the doubling."""
    n = len(a)
    G = b @ np.diag(1.0 / r) @ b.T
    H = np.block([[a, -G], [-np.diag(q), -a.T]])
    lam, V = np.linalg.eig(H)
    stable = np.argsort(lam.real)[:n]
    assert lam.real[stable].max() < 0.0 < np.sort(lam.real)[n]
    X = np.real(V[n:, stable] @ np.linalg.inv(V[:n, stable]))
    return 0.5 * (X + X.T)


def test_design_agrees_with_the_hamiltonian_solution_on_all_golden_aircraft(golden):
    ref = sn.golden_designs(golden)
    assert len(ref["status"]) == 288 and not ref["status"].any(), np.flatnonzero(ref["status"])
    assert ref["iters"].max() <= 12 and ref["residual"].max() <= 1e-10, (ref["iters"].max(), ref["residual"].max())
    weights = sn.block_weights(sn.default_weights())
    worst, turning = 0.0, 0
    for i in range(288):
        turning += int(golden["spec"][i][2] != 0.0)
        for (a, b), (q, r), X in zip(sn.augmented_blocks(golden["A"][i], golden["B"][i], golden["x0"][i]), weights, ref["X"][i]):
            assert np.linalg.eigvalsh(X).min() > 0.0, i
            Xh = _hamiltonian_solution(a, b, q, r)
            worst = max(worst, float(np.abs(X - Xh).max() / np.abs(Xh).max()))
            assert np.linalg.eigvals(a - b @ np.diag(1.0 / r) @ b.T @ X).real.max() < 0.0, i
    print(f"576 blocks ({turning} turning trims): worst |X - X_hamiltonian| / max|X| = {worst:.3e}; residual <= {ref['residual'].max():.3e}; "
          f"doublings {ref['iters'].min()}..{ref['iters'].max()}")
    assert turning == 216
    assert worst <= 1e-9


def test_bad_input_is_refused():
    g = np.load(os.path.join(GOLDEN, "trim_reference.npz"))
    A, B, x0, w = g["A"][5], g["B"][5], g["x0"][5], sn.default_weights()
    good = sn.design(A, B, x0, w)
    assert good["status"] == 0 and good["K"].any()
    nan_a, zero_w, still = A.copy(), w.copy(), x0.copy()
    nan_a[3, 2] = np.nan                                   # d udot / d z: read by the longitudinal block only
    zero_w[12] = 0.0
    still[[3, 5]] = 0.0
    for bad in (sn.design(nan_a, B, x0, w), sn.design(A, B, x0, zero_w), sn.design(A, B, still, w)):
        assert bad["status"] == sn.BAD_INPUT and not bad["K"].any() and np.isnan(bad["residual"]) and bad["iters"] == 0
    unread = A.copy()
    unread[0, 0] = np.nan                                  # the north row is in neither block
    assert np.array_equal(sn.design(unread, B, x0, w)["K"], good["K"])


def test_probe_flights_reach_their_commands():
    rows = sn.probe_flights()
    for (name, V, dt, climb), r in zip(sn.PROBE, rows):
        print(f"{name} V {V} dt {dt} climb {climb}: errors at 40 s {np.abs(r['err'])}, max |roll| {r['roll']:.3f}, max |pitch| {r['pitch']:.3f}, "
              f"saturated {r['sat']} of {r['steps']} steps")
    for r in rows:
        assert r["status"] == 0
        e = np.abs(r["err"])
        assert e[0] <= sn.GATE_V and e[1] <= sn.GATE_H and e[2] <= sn.GATE_PSI, e
        assert r["roll"] <= sn.GATE_ROLL and r["pitch"] <= sn.GATE_PITCH, (r["roll"], r["pitch"])
    # the climbing trim flew a moving altitude reference for its first second; every flight saw the clip and the frozen integrators
    assert rows[3]["ref_end"][3] == 0.0 and rows[3]["spec"][1] > 0.0
    assert all(r["sat"] > 0 for r in rows)

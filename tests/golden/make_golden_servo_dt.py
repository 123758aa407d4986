"""Writes tests/golden/servo_dt_reference.npz: the sampled-data servo design at dt 0.01 and 0.02 on the 288 linearisations of
tests/golden/trim_reference.npz with the default weights.  Per dt:
  K, residual, iters, status       the restatement's (tests/servo_dt_numpy.py)
  K_scipy                          an INDEPENDENT answer: Phi, Gamma from scipy.linalg.expm of [[a, b], [0, 0]] dt, the same sampled
                                   model and weights, X from scipy.linalg.solve_discrete_are, K = (R_d + B_d^T X B_d)^-1 B_d^T X A_d by
                                   numpy.linalg.solve.  Recorded here so that no test needs scipy at run time.

    python tests/golden/make_golden_servo_dt.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]

import servo_dt_numpy as sd              # noqa: E402
import servo_lqg_numpy as sl             # noqa: E402
import servo_numpy as sn                 # noqa: E402


def scipy_gain(A, B, x0, weights, dt):
    """K [26] of one aircraft by scipy alone."""
    from scipy.linalg import expm, solve_discrete_are
    out = []
    for (a, b), ci, (q, r) in zip(sl.blocks(A, B), sd.integrator_rows(x0), sn.block_weights(weights)):
        M = np.zeros((7, 7))
        M[:5, :5], M[:5, 5:] = a * dt, b * dt
        E = expm(M)
        N = 5 + len(ci)
        Ad, Bd = np.zeros((N, N)), np.zeros((N, 2))
        Ad[:5, :5], Ad[5:, :5], Ad[5:, 5:], Bd[:5] = E[:5, :5], dt * ci, np.eye(N - 5), E[:5, 5:]
        Q, R = np.diag(q * dt), np.diag(r * dt)
        X = solve_discrete_are(Ad, Bd, Q, R)
        out.append(np.linalg.solve(R + Bd.T @ X @ Bd, Bd.T @ X @ Ad).reshape(-1))
    return np.concatenate(out)


if __name__ == "__main__":
    g = np.load(os.path.join(HERE, "trim_reference.npz"))
    w = sn.default_weights()
    out = dict(dts=np.array(sd.DTS))
    for dt in sd.DTS:
        tag = f"dt{dt:g}".replace(".", "p")
        d = sd.design_many(g["A"], g["B"], g["x0"], w, dt)
        ks = np.array([scipy_gain(g["A"][i], g["B"][i], g["x0"][i], w, dt) for i in range(len(g["A"]))])
        out.update({f"{tag}_K": d["K"], f"{tag}_residual": d["residual"], f"{tag}_iters": d["iters"], f"{tag}_status": d["status"],
                    f"{tag}_K_scipy": ks})
        dev = np.abs(d["K"] - ks) / np.maximum(1.0, np.abs(ks))
        print(f"dt {dt}: status {np.unique(d['status'])}, iters {d['iters'].min()}..{d['iters'].max()}, residual <= {d['residual'].max():.2e}, "
              f"|K - K_scipy| / max(1, |K_scipy|) <= {dev.max():.2e}")
    np.savez(os.path.join(HERE, "servo_dt_reference.npz"), **out)

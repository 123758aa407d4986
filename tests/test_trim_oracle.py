"""Steady-flight solver, CPU side: the NumPy restatement of fdyn_trim / fdyn_linearize (tests/trim_numpy.py) over the CPU
oracle's dynamics against the same algorithm over the reference's own `Simplified6DOF._dynamics`
(tests/golden/trim_reference.npz, written by tests/golden/make_golden_trim.py) -- this ties the on-box reference of
tests/test_gpu_trim.py to the reference project -- and the host logic of hcrl_amd.trim that needs no device.

Gates: z within 1e-9 (two implementations of one function find the same root up to libm rounding amplified by the inverse
Jacobian), status equal, A and B within 1e-6 max(1, |value|) (rounding of one derivative, a few 1e-14, over a step of 2e-5).
"""
import os
import time

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import trim_numpy as tn
from hcrl_amd import layout as L
from hcrl_amd import trim as T
from hcrl_amd import validation as V
from hcrl_amd.flight_types import ControlSurfaces


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "trim_reference.npz"))


@pytest.fixture(scope="module")
def ref():
    t0 = time.perf_counter()
    r = tn.oracle_reference()
    print(f"NumPy Newton + linearisation over the oracle, 288 + 16 aircraft: {time.perf_counter() - t0:.2f} s")
    return r


def test_status_bits_mirror_the_header():
    assert (tn.NOT_CONVERGED, tn.CONTROL_RANGE, tn.ALPHA_LIMIT, tn.PITCH_LIMIT, tn.BAD_SPEC) == (
        L.FD_TRIM_NOT_CONVERGED, L.FD_TRIM_CONTROL_RANGE, L.FD_TRIM_ALPHA_LIMIT, L.FD_TRIM_PITCH_LIMIT, L.FD_TRIM_BAD_SPEC) == (1, 2, 4, 8, 16)
    assert (L.FD_NTS, L.FD_NSC) == (5, 5)
    assert (L.FD_TS_AIRSPEED, L.FD_TS_CLIMB_ANGLE, L.FD_TS_TURN_RATE, L.FD_TS_ALTITUDE, L.FD_TS_HEADING) == (0, 1, 2, 3, 4)


def test_golden_inputs_are_the_grids(golden):
    ty, spec, scales = tn.feasible_grid()
    assert len(ty) == 288
    assert np.array_equal(golden["type"], ty) and np.array_equal(golden["spec"], spec) and np.array_equal(golden["scales"], scales)
    ity, ispec, _ = tn.infeasible_set()
    assert np.array_equal(golden["inf_type"], ity) and np.array_equal(golden["inf_spec"], ispec, equal_nan=True)


def test_feasible_grid_matches_the_reference(golden, ref):
    r = ref["feasible"]
    assert np.array_equal(r["status"], golden["status"]) and not r["status"].any()
    assert r["residual"].max() <= 1e-10 and r["iters"].max() <= 5
    assert np.abs(r["iters"] - golden["iters"]).max() <= 1
    for k in ("z", "x0", "u0"):
        worst = np.abs(r[k] - golden[k]).max()
        print(f"feasible {k}: worst |oracle - reference| = {worst:.3e}")
        assert worst <= 1e-9, (k, worst)
    for k in ("A", "B"):
        err = np.abs(r[k] - golden[k]) / np.maximum(1.0, np.abs(golden[k]))
        print(f"feasible {k}: worst deviation {err.max():.3e}")
        assert err.max() <= 1e-6, (k, err.max())


def test_infeasible_set_matches_the_reference_and_the_table(golden, ref):
    r = ref["infeasible"]
    assert np.array_equal(r["status"], golden["inf_status"])
    for i, (must_set, must_clear) in enumerate(r["want"]):
        s = int(r["status"][i])
        assert s & must_set == must_set and not s & must_clear, (i, s)
    conv = (r["status"] & (tn.NOT_CONVERGED | tn.BAD_SPEC)) == 0
    assert conv.sum() == 8                                                    # the bit-1 / bit-2 lanes and the cessna at 9 m/s
    assert np.abs(r["z"][conv] - golden["inf_z"][conv]).max() <= 1e-9
    for k in ("A", "B"):
        err = np.abs(r[k][conv] - golden["inf_" + k][conv]) / np.maximum(1.0, np.abs(golden["inf_" + k][conv]))
        assert err.max() <= 1e-6, (k, err.max())
    assert np.isnan(golden["inf_A"][~conv]).all()
    # the figures the issue quotes: throttle -0.08 at V = 25 descending, 1.23 / 1.54 at V = 40, alpha 0.60 at V = 9 (rc_plane)
    assert abs(r["z"][0, 6] + 0.08) < 0.005 and abs(r["z"][1, 6] - 1.23) < 0.005 and abs(r["z"][9, 6] - 1.54) < 0.005
    assert abs(r["z"][2, 0] - 0.60) < 0.005


def test_solve7_matches_numpy_and_flags_a_zero_column():
    rs = np.random.RandomState(7)
    a, b = rs.normal(size=(7, 7)), rs.normal(size=7)
    dz, ok = tn.solve7(a, b)
    assert ok and np.abs(dz - np.linalg.solve(a, b)).max() < 1e-12
    a[:, 6] = 0.0
    assert not tn.solve7(a, b)[1]
    a[:, 6] = np.nan
    assert not tn.solve7(a, b)[1]


# ---- hcrl_amd.trim without a device ------------------------------------------------------------------------------------------
def test_flight_condition_broadcasts_scalars_and_arrays():
    spec = T.flight_condition(3, 20.0, climb_angle=[0.0, 0.1, 0.2], turn_rate=np.float32(0.5), heading=torch.tensor([1.0, 2.0, 3.0]))
    assert spec.shape == (L.FD_NTS, 3) and spec.dtype == np.float64
    assert np.array_equal(spec[L.FD_TS_AIRSPEED], [20.0] * 3) and np.array_equal(spec[L.FD_TS_CLIMB_ANGLE], [0.0, 0.1, 0.2])
    assert np.array_equal(spec[L.FD_TS_TURN_RATE], [0.5] * 3) and np.array_equal(spec[L.FD_TS_ALTITUDE], [100.0] * 3)
    assert np.array_equal(spec[L.FD_TS_HEADING], [1.0, 2.0, 3.0])
    assert np.array_equal(T.flight_condition(2, [15.0])[0], [15.0, 15.0])                 # length 1 broadcasts like a scalar
    with pytest.raises(ValueError, match="word 1"):
        T.flight_condition(3, 20.0, climb_angle=[0.0, 0.1])
    with pytest.raises(ValueError):
        T.flight_condition(3, np.zeros((3, 1)))


def test_scale_rows_forms():
    cpu = torch.device("cpu")
    assert T.scale_rows(4, None, cpu) is None
    s = T.scale_rows(4, (1.2, 0.9, [1.0, 1.1, 1.2, 1.3], 1.05, 0.95), cpu)
    assert s.shape == (L.FD_NSC, 4) and s.dtype == torch.float64 and s.is_contiguous()
    assert s[L.FD_SC_MASS].tolist() == [1.2] * 4 and s[L.FD_SC_IYY].tolist() == [1.0, 1.1, 1.2, 1.3] and s[L.FD_SC_RHO].tolist() == [0.95] * 4
    t = torch.ones((L.FD_NSC, 4), dtype=torch.float32)
    assert T.scale_rows(4, t, cpu).dtype == torch.float64
    with pytest.raises(ValueError):
        T.scale_rows(4, (1.0, 1.0, 1.0), cpu)
    with pytest.raises(ValueError):
        T.scale_rows(4, torch.ones((4, L.FD_NSC)), cpu)


def _result(status):
    n = len(status)
    x0 = torch.zeros((L.FD_NX, n), dtype=torch.float64)
    x0[L.FD_X_U], x0[L.FD_X_W], x0[L.FD_X_ROLL] = 20.0 * np.cos(0.1), 20.0 * np.sin(0.1), 0.25
    u0 = torch.tensor([[0.1] * n, [-0.2] * n, [0.3] * n, [0.7] * n], dtype=torch.float64)
    return T.TrimResult(x0, u0, torch.zeros(n, dtype=torch.float64), torch.full((n,), 4, dtype=torch.int32),
                        torch.tensor(status, dtype=torch.int32))


def test_trim_result_views_and_status_decoding():
    res = _result([0, 2, 0, 5, 16])
    assert res.n == 5 and res.ok.tolist() == [True, False, True, False, False] and res.count_not_ok() == 3
    assert torch.allclose(res.alpha, torch.full((5,), 0.1, dtype=torch.float64), atol=1e-15)
    assert res.bank.tolist() == [0.25] * 5
    assert res.surfaces(1) == ControlSurfaces(elevator=0.1, aileron=-0.2, rudder=0.3, throttle=0.7)
    assert T.describe_status(0) == "ok"
    assert T.describe_status(5) == "not converged, angle of attack at its limit"
    assert T.describe_status(2 | 8 | 16) == "control out of range, pitch at its limit, invalid flight condition"


def test_strict_check_names_the_count_and_the_first_reason():
    T.require_ok(_result([0, 0, 0]))                                          # nothing to report
    with pytest.raises(ValueError, match=r"3 of 5 aircraft.*first: aircraft 1: control out of range"):
        T.require_ok(_result([0, 2, 0, 5, 16]), "BatchedSixDOF.trim")


def test_sub_system_blocks_pick_the_classical_states():
    A = np.arange(144.0).reshape(12, 12)
    B = np.arange(48.0).reshape(12, 4)
    Al, Bl = T.longitudinal_block(A, B)
    assert Al.shape == (4, 4) and Bl.shape == (4, 2)
    rows = [L.FD_X_U, L.FD_X_W, L.FD_X_Q, L.FD_X_PITCH]
    assert np.array_equal(Al, A[np.ix_(rows, rows)]) and np.array_equal(Bl, B[np.ix_(rows, [L.FD_U_ELEVATOR, L.FD_U_THROTTLE])])
    Ad, Bd = T.lateral_block(torch.as_tensor(A).unsqueeze(-1).repeat(1, 1, 3), torch.as_tensor(B).unsqueeze(-1).repeat(1, 1, 3))
    rows = [L.FD_X_V, L.FD_X_P, L.FD_X_R, L.FD_X_ROLL]
    assert tuple(Ad.shape) == (4, 4, 3) and tuple(Bd.shape) == (4, 2, 3)
    assert np.array_equal(Ad[:, :, 2].numpy(), A[np.ix_(rows, rows)]) and np.array_equal(Bd[:, :, 0].numpy(), B[np.ix_(rows, [L.FD_U_AILERON, L.FD_U_RUDDER])])


def test_longitudinal_block_of_the_reference_trim_has_the_two_classical_modes(golden):
    """What the linear model is for: at V = 20 level (rc_plane, nominal mass) the longitudinal block splits into a fast,
    well-damped complex pair (short period) and a slow, barely damped one (phugoid)."""
    ty, spec, scales = tn.feasible_grid()
    i = int(np.flatnonzero((ty == 0) & (spec[:, 0] == 20.0) & (spec[:, 1] == 0.0) & (spec[:, 2] == 0.0) & (scales[:, 0] == 1.0))[0])
    Al, _ = T.longitudinal_block(golden["A"][i], golden["B"][i])
    ev = sorted(np.linalg.eigvals(Al), key=abs)
    slow, fast = ev[0], ev[-1]
    assert abs(slow.imag) > 0 and abs(fast.imag) > 0, ev
    assert fast.real < -1.0 and abs(fast) > 3 * abs(slow) and abs(slow.real) < 0.1, ev


def test_trimmed_scenario_constants():
    s = V.TrimmedFlightScenario({"airspeed": 25.0, "climb_deg": 3.0, "turn_rate": 0.1})
    assert (s.duration, s.dt, s.num_steps) == (30.0, 0.01, 3000)
    assert (s.airspeed, s.climb_deg, s.turn_rate, s.altitude) == (25.0, 3.0, 0.1, 100.0)
    assert s.get_name() == "Trimmed Flight" and "25 m/s" in s.get_description()
    assert s._condition()["climb_angle"] == pytest.approx(np.radians(3.0))
    level = V.LevelFlightScenario().get_expected_metrics()
    assert s.get_expected_metrics() == dict(level, min_correlation=None)      # constant channels have no correlation to score
    lf = V.LevelFlightScenario()                                              # untouched by the new scenario
    assert (lf.trim_elevator, lf.trim_throttle) == (0.0, 0.5)

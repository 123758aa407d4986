"""The host layer of the scheduled servo (hcrl_amd.servo_sched) on host tensors: node airspeeds are checked before anything is
launched, the pack puts every word where include/fdyn_servo_sched.h says, `interpolated` is step 0b of the restatement, and a
schedule together with a wind is refused.  No device."""
import numpy as np
import pytest
import torch

import servo_numpy as sn
import servo_sched_numpy as ssn
from hcrl_amd import layout as L
from hcrl_amd import servo as SV
from hcrl_amd import servo_sched as SS


def test_node_airspeeds_are_checked_on_the_host():
    a = SS.node_airspeeds((15.0, 20.0, 25.0, 30.0), 3)
    assert a.shape == (4, 3) and a.flags.c_contiguous and a[:, 1].tolist() == [15.0, 20.0, 25.0, 30.0]
    per_lane = np.array([[15.0, 18.0], [20.0, 19.0], [25.0, 30.0]])
    assert np.array_equal(SS.node_airspeeds(per_lane, 2), per_lane) and np.array_equal(SS.node_airspeeds(torch.as_tensor(per_lane), 2), per_lane)
    assert SS.node_airspeeds([20.0], 2).shape == (1, 2)
    for bad in ((15.0, 15.0), (20.0, 15.0), (15.0, np.nan), (15.0, np.inf), np.array([[15.0, 18.0], [20.0, 17.0]])):
        with pytest.raises(ValueError, match="strictly increasing"):
            SS.node_airspeeds(bad, 2)
    with pytest.raises(ValueError, match="1 to 8 nodes"):
        SS.node_airspeeds(np.arange(9.0) + 10.0, 2)
    with pytest.raises(ValueError, match="1 to 8 nodes"):
        SS.node_airspeeds([], 2)
    with pytest.raises(ValueError, match="expected M values"):
        SS.node_airspeeds(np.ones((2, 3)), 2)
    assert SS.sched_on("airspeed") == L.FD_SCHED_ON_AIRSPEED and SS.sched_on("command") == L.FD_SCHED_ON_COMMAND
    with pytest.raises(ValueError, match="on must be one of"):
        SS.sched_on("estimate")


def _lanes(M, n, rows, seed):
    return torch.as_tensor(np.random.RandomState(seed).standard_normal((rows, M * n)))


def test_pack_interpolation_and_status():
    M, n = 3, 4
    V = torch.as_tensor(np.array([[15.0] * n, [20.0, 21.0, 22.0, 23.0], [30.0] * n]))
    x0, u0, K = _lanes(M, n, L.FD_NX, 0), _lanes(M, n, L.FD_NU, 1), _lanes(M, n, L.FD_NSVK, 2)
    table = SS.pack(V, x0, u0, K)
    assert tuple(table.shape) == (M, L.FD_NSS, n) and table.is_contiguous() and table.dtype == torch.float64
    for k in range(M):
        for i in range(n):
            want = ssn.node(float(V[k, i]), x0[:, k * n + i].numpy(), u0[:, k * n + i].numpy(), K[:, k * n + i].numpy())
            assert np.array_equal(table[k, :, i].numpy(), want), (k, i)
    status = torch.zeros((M, n), dtype=torch.int32)
    status[1, 2] = L.FD_SV_NO_CERTIFICATE
    s = SS.ServoSchedule(table, V, status)
    assert (s.n, s.n_nodes) == (n, M) and s.ok.tolist() == [True, True, False, True] and s.count_not_ok() == 1
    with pytest.raises(ValueError, match=r"1 of 4 aircraft have a node without.*aircraft 2, node 1: no stability certificate"):
        s.require_ok()
    with pytest.raises(ValueError, match="no flight condition"):
        s.frozen_point_modes()
    pos = torch.as_tensor(np.array([0.0, 0.5, 1.25, 2.0]))
    got = s.interpolated(pos).numpy()
    for i in range(n):
        tb = table[:, :, i].numpy()
        sigma = tb[int(pos[i]), 0] + (pos[i].item() - int(pos[i])) * (tb[min(int(pos[i]) + 1, M - 1), 0] - tb[int(pos[i]), 0])
        want, p = ssn.lookup(tb, sigma)
        assert abs(p - pos[i].item()) <= 1e-15 and np.abs(got[:, i] - want).max() <= 1e-14 * np.abs(want).max(), i


def test_a_design_is_a_one_node_schedule():
    n = 3
    x0 = _lanes(1, n, L.FD_NX, 3)
    d = SV.ServoDesign(_lanes(1, n, L.FD_NSVK, 4), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.int32),
                       torch.tensor([0, L.FD_SV_BAD_INPUT, 0], dtype=torch.int32), x0, _lanes(1, n, L.FD_NU, 5))
    s = SS.ServoSchedule.from_design(d)
    assert s.n_nodes == 1 and s.ok.tolist() == [True, False, True]
    assert torch.equal(s.table[0, L.FD_SS_K:], d.K) and torch.equal(s.table[0, L.FD_SS_U0:L.FD_SS_K], d.u0)
    assert torch.equal(s.table[0, L.FD_SS_X0:L.FD_SS_U0], x0[list(ssn.X0_WORDS)])
    with pytest.raises(ValueError, match="no trim point"):
        SS.ServoSchedule.from_design(SV.ServoDesign(d.K, d.residual, d.iterations, d.status))


def test_schedule_and_wind_exclude_each_other():
    n = 2
    s = SS.ServoSchedule(torch.zeros((1, L.FD_NSS, n), dtype=torch.float64), torch.ones((1, n), dtype=torch.float64), torch.zeros((1, n), dtype=torch.int32))
    wind = SV.ServoWind.steady(n, "cpu", 5.0, 0.3)
    x = torch.zeros((L.FD_NX, n), dtype=torch.float64)
    st = SV.ServoState.at_trim(x)
    with pytest.raises(NotImplementedError, match="still air"):
        SV.step_into("f64", x, None, st, torch.zeros((1, L.FD_NP), dtype=torch.float64), None, 0.01, 1, wind=wind, schedule=s)
    mission = SV.ServoMission.start(np.array([[0.0, 0.0, 100.0, 20.0]]), n, "cpu")
    with pytest.raises(NotImplementedError, match="still air"):
        SV.mission_into("f64", x, None, st, mission, torch.zeros((1, L.FD_NP), dtype=torch.float64), None, 0.01, 1, wind=wind, schedule=s)
    with pytest.raises(ValueError, match="on must be one of"):
        SS.sched_step_into("f64", x, s, st, torch.zeros((1, L.FD_NP), dtype=torch.float64), None, 0.01, 1, on="measured")
    assert sn.NSVK == L.FD_NSVK

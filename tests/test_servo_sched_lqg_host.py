"""The host layer of the scheduled servo on noisy sensors (hcrl_amd.servo_sched_lqg) on host tensors: the filter table is packed by
reshape, `interpolated` is step 3 of the restatement, the state starts at position -1, and a missing filter schedule, one made at
another dt or for another schedule, and a schedule that cannot be linearised are refused before anything is launched.  No device."""
import numpy as np
import pytest
import torch

import servo_sched_numpy as ssn
from hcrl_amd import layout as L
from hcrl_amd import servo as SV
from hcrl_amd import servo_sched as SS
from hcrl_amd import servo_sched_lqg as SQ


def _schedule(M, n, seed=0):
    rs = np.random.RandomState(seed)
    table = torch.as_tensor(rs.standard_normal((M, L.FD_NSS, n)))
    V = torch.as_tensor(np.sort(rs.uniform(10.0, 30.0, (M, n)), axis=0))
    table[:, L.FD_SS_V] = V
    return SS.ServoSchedule(table, V, torch.zeros((M, n), dtype=torch.int32))


def _kalman(M, n, dt=0.01, seed=1):
    F = torch.as_tensor(np.random.RandomState(seed).standard_normal((L.FD_NSKF, M * n)))
    return F, SQ.ServoKalmanSchedule(SQ.pack_f(F, M), torch.zeros((M, n), dtype=torch.int32), dt, torch.ones(L.FD_NSKN, dtype=torch.float64),
                                     torch.ones(L.FD_NSKX, dtype=torch.float64))


def test_pack_status_and_interpolation():
    M, n = 3, 4
    F, k = _kalman(M, n)
    assert tuple(k.table_f.shape) == (M, L.FD_NSKF, n) and k.table_f.is_contiguous() and (k.n, k.n_nodes) == (n, M)
    for node in range(M):
        for i in range(n):
            assert torch.equal(k.table_f[node, :, i], F[:, node * n + i]), (node, i)
    assert k.ok.all() and k.count_not_ok() == 0
    k.require_ok()
    k.status[2, 1] = L.FD_KF_NO_CERTIFICATE
    assert k.ok.tolist() == [True, False, True, True]
    with pytest.raises(ValueError, match=r"1 of 4 aircraft have a node without a certified stable filter.*aircraft 1, node 2: no stability certificate"):
        k.require_ok()
    pos = torch.as_tensor(np.array([0.0, 0.5, 1.25, 2.0]))
    got = k.interpolated(pos).numpy()
    for i in range(n):
        tb = np.concatenate([np.arange(M, dtype=np.float64)[:, None], k.table_f[:, :, i].numpy()], axis=1)    # node "airspeeds" 0, 1, 2
        want, p = ssn.lookup(tb, pos[i].item())
        assert p == pos[i].item() and np.abs(got[:, i] - want[1:]).max() <= 1e-14 * np.abs(want[1:]).max(), i
    with pytest.raises(ValueError, match="no flight condition"):
        k.frozen_point_report()


def test_the_state_starts_without_an_operating_point():
    st = SQ.ServoSchedLqgState.zeros(5, "cpu", seed=3)
    assert tuple(st.sched_state.shape) == (2, 5) and st.sched_state.dtype == torch.float64 and st.sched_state.is_contiguous()
    assert (st.sched_state[1] == -1.0).all() and st.seed == 3 and tuple(st.xhat.shape) == (L.FD_NSKX, 5)
    st.sched_state[1] = 1.5
    st.xhat += 1.0
    st.reset(seed=4)
    assert (st.sched_state[1] == -1.0).all() and not st.xhat.any() and st.seed == 4
    x0 = torch.arange(24.0, dtype=torch.float64).reshape(12, 2)
    assert torch.equal(SQ.origin_of(x0), torch.stack([x0[L.FD_X_D], x0[L.FD_X_YAW]]))


def test_a_missing_filter_schedule_or_a_wrong_dt_is_a_value_error():
    M, n = 2, 3
    s, (_, k) = _schedule(M, n), _kalman(M, n, dt=0.01)
    x = torch.zeros((L.FD_NX, n), dtype=torch.float64)
    servo, est, origin = SV.ServoState.at_trim(x), SQ.ServoSchedLqgState.zeros(n, "cpu"), SQ.origin_of(x)
    params = torch.zeros((1, L.FD_NP), dtype=torch.float64)
    with pytest.raises(ValueError, match="no filter schedule"):
        SQ.sched_lqg_step_into("f64", x, s, None, origin, servo, est, params, None, 0.01, 1)
    with pytest.raises(ValueError, match=r"designed at dt = 0\.01, the flight asks for dt = 0\.02"):
        SQ.sched_lqg_step_into("f64", x, s, k, origin, servo, est, params, None, 0.02, 1)
    with pytest.raises(ValueError, match="beside the schedule's table"):
        SQ.sched_lqg_step_into("f64", x, s, _kalman(M + 1, n)[1], origin, servo, est, params, None, 0.01, 1)
    with pytest.raises(ValueError, match="origin must be"):
        SQ.sched_lqg_step_into("f64", x, s, k, origin[:1], servo, est, params, None, 0.01, 1)
    with pytest.raises(ValueError, match="on must be one of"):
        SQ.sched_lqg_step_into("f64", x, s, k, origin, servo, est, params, None, 0.01, 1, on="estimate")
    with pytest.raises(KeyError):
        SQ.sched_lqg_step_into("f64", x, s, k, origin, servo, est, params, None, 0.01, 1, feedback="airspeed")
    with pytest.raises(ValueError, match=r"z must be contiguous float64 \[1\]\[10\]\[3\]"):
        SQ.sched_lqg_step_into("f64", x, s, k, origin, servo, est, params, None, 0.01, 1, z=torch.zeros((2, 10, n), dtype=torch.float64))
    with pytest.raises(ValueError, match="no node trims"):
        SQ.design_servo_kalman_schedule(s, 0.01)
    # the fleet's own refusals come before any launch too
    from hcrl_amd.fleet import BatchedSixDOF
    fleet = object.__new__(BatchedSixDOF)
    fleet.servo, fleet._trim, fleet._servo_kalman_schedule = servo, (type("R", (), dict(x0=x))(), None), None
    with pytest.raises(ValueError, match="has no filter schedule"):
        fleet.step_servo_lqg(1, schedule=s)
    fleet._servo_kalman_schedule = _kalman(M, n)[1]                       # made for another schedule
    with pytest.raises(ValueError, match="has no filter schedule"):
        fleet.step_servo_lqg(1, schedule=s)

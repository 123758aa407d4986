"""hcrl_amd.validation without a GPU: the interface it shares with the reference's validation suite -- metric keys, the printed
summary, the scenarios' constants and thresholds (tests/golden/validation_reference.json, written by
tests/golden/make_golden_validation.py from the reference's own modules) -- and the loud failure without a device."""
import json
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, REPO
from hcrl_amd import _lib, layout as L
from hcrl_amd import validation as V


@pytest.fixture(scope="module")
def ref():
    with open(os.path.join(GOLDEN, "validation_reference.json")) as f:
        return json.load(f)


def test_metric_keys_follow_the_reference_and_the_header(ref):
    assert list(V.METRIC_KEYS) == ref["METRIC_KEYS"] and list(V.CHANNELS) == ref["channels"]
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "fdyn_layout.h")).read(), flags=re.S)
    names = re.findall(r"\bFD_TM_(\w+)", src)
    assert [n.lower() for n in names] == ref["METRIC_KEYS"]                      # declaration order = dictionary order
    assert [getattr(L, "FD_TM_" + n) for n in names] == list(range(35)) and L.FD_NTM == 35 and L.FD_NTC == 14
    assert [getattr(L, "FD_TC_" + c.upper()) for c in ref["channels"]] == list(range(14))
    assert L.FD_NTA == L.FD_TA_CORR + L.FD_TA_NCORR * L.FD_TA_CORR_WORDS and L.FD_TA_MAX == L.FD_TA_POS3D_MAX + 1


def test_summary_text_matches_the_reference(ref):
    z = np.load(os.path.join(GOLDEN, "validation_pairs.npz"))
    for pair, text in ref["summary_text"].items():
        assert V.format_metrics_summary(dict(zip(V.METRIC_KEYS, z["metrics"][int(pair)].tolist()))) == text
    nan_block = V.format_metrics_summary(dict(zip(V.METRIC_KEYS, z["metrics"][0].tolist())))
    assert "Overall Correlation:   nan" in nan_block


def test_scenarios_keep_the_reference_constants(ref):
    class Bare(V.ValidationScenario):
        get_name = get_description = get_initial_conditions = get_control_function = lambda self: None

    want = ref["scenarios"]["ValidationScenario"]
    s = Bare()
    assert (s.duration, s.dt, s.get_expected_metrics()) == (want["duration"], want["dt"], want["expected_metrics"])
    assert Bare({"duration": 2.5, "dt": 0.02}).num_steps == 125
    want = ref["scenarios"]["LevelFlightScenario"]
    s = V.LevelFlightScenario()
    assert (s.get_name(), s.get_description()) == (want["name"], want["description"])
    assert (s.duration, s.dt, s.trim_elevator, s.trim_throttle) == (want["duration"], want["dt"], want["trim_elevator"],
                                                                    want["trim_throttle"])
    assert s.get_expected_metrics() == want["expected_metrics"] and s.num_steps == 3000
    ic, c = s.get_initial_conditions(), s.get_control_function()(1.5)
    assert np.array_equal(ic.to_vector(), [0, 0, -100, 20, 0, 0, 0, 0, 0, 0, 0, 0]) and (ic.airspeed, ic.altitude) == (20.0, 100.0)
    assert (c.elevator, c.aileron, c.rudder, c.throttle) == (0.0, 0.0, 0.0, 0.5)
    assert repr(V.LevelFlightScenario({"duration": 5})) == "Level Flight (duration=5s, dt=0.01s)"


def test_batched_channel_metrics_match_numpy():
    import torch
    rs = np.random.RandomState(3)
    a = np.cumsum(rs.normal(size=(40, 5)), axis=0)
    b = a + 0.1 * rs.normal(size=(40, 5))
    a[:, 4] = 2.0                                                                # a constant column
    ta, tb = torch.as_tensor(a), torch.as_tensor(b)
    assert np.allclose(V.compute_rmse(ta, tb).numpy(), np.sqrt(np.mean((a - b) ** 2, axis=0)), rtol=1e-13)
    assert np.allclose(V.compute_max_error(ta, tb).numpy(), np.abs(a - b).max(axis=0), rtol=0, atol=0)
    r = V.compute_correlation(ta, tb).numpy()
    assert np.allclose(r[:4], [np.corrcoef(a[:, j], b[:, j])[0, 1] for j in range(4)], rtol=0, atol=1e-13) and np.isnan(r[4])
    assert not V.compute_correlation(ta[:1], tb[:1]).numpy().any()
    nr = V.compute_nrmse(ta, tb).numpy()
    assert np.allclose(nr[:4], (np.sqrt(np.mean((a - b) ** 2, axis=0)) / np.ptp(a, axis=0) * 100)[:4], rtol=1e-13) and nr[4] == 0.0


def test_no_gpu_means_loud_failure():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    traj = {c: np.zeros(4) for c in V.CHANNELS}
    with pytest.raises(_lib.FdynError):
        V.compare_trajectories(traj, traj)
    with pytest.raises(_lib.FdynError):
        V.TrajectoryComparison(4)
    with pytest.raises(_lib.FdynError):
        V.run_validation(V.LevelFlightScenario({"duration": 1}), "f64", "mixed", 4, out=lambda *a: None)

"""fdyn_traj_compare and hcrl_amd.validation on the device, against the reference's own compare_trajectories.

tests/golden/validation_pairs.npz (tests/golden/make_golden_validation.py) holds ten pairs of 500-step trajectories flown by the
reference's SimulationAircraftBackend and the 35 metrics its compare_trajectories (pandas + scipy) returns for each, for the
fp64 data and for the data rounded to fp32.  The gate is the project's own for summation-order differences
(tests/test_gpu_eval.py): |got - want| <= 1e-12 max(|want|, 1), with the NaN pattern identical.
"""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from hcrl_amd import _lib, layout as L
from hcrl_amd import validation as V

pytestmark = pytest.mark.gpu

GATE = 1e-12
T, PAIRS = 500, 10
_ATT = [V.CHANNELS.index(c) for c in ("roll", "pitch", "yaw", "p", "q", "r")]
_STATE = [V.CHANNELS.index(c) for c in V._STATE_COLUMNS]
_CORR = [j for j, k in enumerate(V.METRIC_KEYS) if k.endswith("correlation")]


def _load_pairs():
    """-> a, b [10][500][14] float64 in V.CHANNELS order, metrics, metrics_rounded [10][35]."""
    z = np.load(os.path.join(GOLDEN, "validation_pairs.npz"))
    ab = np.ascontiguousarray(z["byte_planes"].T).reshape(-1).view(np.float64).reshape(tuple(z["shape"]))   # [side][pair][13][T]
    stored = [str(c) for c in z["channels"]]
    full = np.zeros(ab.shape[:2] + (L.FD_NTC, ab.shape[3]))
    for j, c in enumerate(V.CHANNELS):
        full[:, :, j] = -ab[:, :, stored.index("down")] if c == "altitude" else ab[:, :, stored.index(c)]
    full = full.transpose(0, 1, 3, 2)
    return full[0], full[1], z["metrics"], z["metrics_rounded"]


def _device_block(traj, dtype=torch.float64):
    """traj [P][T][14] -> x [T][12][P], derived [T][FD_ND][P] on the device."""
    t = torch.as_tensor(np.ascontiguousarray(traj.transpose(1, 2, 0)), device="cuda")          # [T][14][P]
    d = torch.zeros((t.shape[0], L.FD_ND, t.shape[2]), dtype=torch.float64, device="cuda")
    d[:, L.FD_D_AIRSPEED], d[:, L.FD_D_ALTITUDE] = t[:, V.CHANNELS.index("airspeed")], t[:, V.CHANNELS.index("altitude")]
    return t[:, _STATE].to(dtype).contiguous(), d.to(dtype).contiguous()


SENTINEL = -12345.678


def _buffers(n, pad=0):
    acc = torch.zeros(L.FD_NTA * n + pad, dtype=torch.float64, device="cuda")
    out = torch.full((L.FD_NTM * n + pad,), SENTINEL, dtype=torch.float64, device="cuda")
    acc[L.FD_NTA * n:] = SENTINEL
    return acc, out


def _call(xa, da, xb, db, steps, n, acc, out):
    f32 = lambda t: int(t is not None and t.dtype == torch.float32)      # noqa: E731
    rc = _lib.load().fdyn_traj_compare(_lib.ptr(xa), f32(xa), _lib.ptr(da), _lib.ptr(xb), f32(xb), _lib.ptr(db), steps, n,
                                       _lib.ptr(acc), _lib.ptr(out), _lib.current_stream())
    _lib.check(rc, "fdyn_traj_compare")


def _compare(xa, da, xb, db, chunks=None, pad=0):
    """Feed [T][..][n] blocks in `chunks` (default: one launch); -> acc [FD_NTA][n], out [FD_NTM][n], the two padded buffers."""
    steps, n = xa.shape[0], xa.shape[2]
    acc, out = _buffers(n, pad)
    t0 = 0
    for c in chunks or [steps]:
        sl = slice(t0, t0 + c)
        _call(xa[sl], None if da is None else da[sl], xb[sl], None if db is None else db[sl], c, n, acc, None)
        t0 += c
    assert t0 == steps
    _call(None, None, None, None, 0, n, acc, out)
    torch.cuda.synchronize()
    return (acc[:L.FD_NTA * n].reshape(L.FD_NTA, n).cpu().numpy(), out[:L.FD_NTM * n].reshape(L.FD_NTM, n).cpu().numpy(),
            acc.cpu().numpy(), out.cpu().numpy())


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _assert_gate(got, want, gate=GATE, what=""):
    """got, want [..][35] (metrics last): same NaN pattern, |got - want| <= gate max(|want|, 1)."""
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN pattern differs"
    err = np.abs(got - want) / np.maximum(np.abs(want), 1.0)
    worst = np.nanmax(err)
    j = np.unravel_index(np.nanargmax(err), err.shape)
    print(f"{what}: worst deviation {worst:.3e} at {j} ({V.METRIC_KEYS[j[-1]]})")
    assert worst <= gate, (what, worst, j, V.METRIC_KEYS[j[-1]])


@pytest.fixture(scope="module")
def pairs():
    a, b, m, mr = _load_pairs()
    return {"a": a, "b": b, "metrics": m, "metrics_rounded": mr}


@pytest.fixture(scope="module")
def single(pairs):
    """All ten pairs in ONE launch (n = 10, T = 500, fp64): what the other tests compare against bit for bit."""
    xa, da = _device_block(pairs["a"])
    xb, db = _device_block(pairs["b"])
    acc, out, _, _ = _compare(xa, da, xb, db)
    return {"xa": xa, "da": da, "xb": xb, "db": db, "acc": acc, "out": out}


def test_reference_parity(pairs, single):
    """1. The ten reference pairs: NaN pattern identical, every metric within 1e-12 max(|want|, 1) of compare_trajectories;
    the drop-in compare_trajectories on dicts of arrays gives the very same numbers pair by pair."""
    assert np.isnan(pairs["metrics"][0]).sum() == 8 and not np.isnan(pairs["metrics"][2:]).any()
    _assert_gate(single["out"].T, pairs["metrics"], what="single launch")
    for p in range(PAIRS):
        cols = lambda t: {c: t[:, j] for j, c in enumerate(V.CHANNELS)}      # noqa: E731
        m = V.compare_trajectories(cols(pairs["a"][p]), cols(pairs["b"][p]))
        assert list(m) == list(V.METRIC_KEYS) and all(type(v) is float for v in m.values())
        assert np.array_equal(_bits(np.array(list(m.values()))), _bits(single["out"][:, p])), p
    short = V.compare_trajectories({c: pairs["a"][3][:, j] for j, c in enumerate(V.CHANNELS)},
                                   {c: pairs["b"][3][:123, j] for j, c in enumerate(V.CHANNELS)})     # cut to the shorter
    assert short["position_3d_max_error"] <= single["out"][L.FD_TM_POSITION_3D_MAX_ERROR, 3] and short["position_3d_rmse"] > 0


def test_chunking_is_bit_identical(single):
    """2. Chunks of 1, 7, 64 and the rest, and TrajectoryComparison(chunk=16) fed one step at a time (31 full rings and a partial
    one): acc and out bit-identical to the single launch -- the carried unwrap state, the pivots and the constant flags."""
    acc, out, _, _ = _compare(single["xa"], single["da"], single["xb"], single["db"], chunks=[1, 7, 64, T - 72])
    assert np.array_equal(_bits(acc), _bits(single["acc"])) and np.array_equal(_bits(out), _bits(single["out"]))
    acc, out, _, _ = _compare(single["xa"], single["da"], single["xb"], single["db"], chunks=[1] * 3 + [T - 3])
    assert np.array_equal(_bits(acc), _bits(single["acc"])) and np.array_equal(_bits(out), _bits(single["out"]))
    cmp_ = V.TrajectoryComparison(PAIRS, chunk=16)
    for t in range(T):
        cmp_.update(single["xa"][t], single["xb"][t], single["da"][t], single["db"][t])
    m = cmp_.metrics().cpu().numpy()
    assert np.array_equal(_bits(m), _bits(single["out"])) and np.array_equal(_bits(cmp_.acc.cpu().numpy()), _bits(single["acc"]))
    assert cmp_.as_dict(4) == dict(zip(V.METRIC_KEYS, single["out"][:, 4].tolist()))
    cmp_.reset()                                                  # a fresh comparison: no step at all gives zeros
    assert not cmp_.metrics().cpu().numpy().any()
    cmp_.update(single["xa"][:1], single["xb"][:1], single["da"][:1], single["db"][:1])              # one step: k < 2 -> r = 0
    one = cmp_.metrics().cpu().numpy()
    assert not one[_CORR].any() and not np.isnan(one).any()


@pytest.mark.parametrize("a_f32,b_f32", [(True, False), (True, True)])
def test_storage_types(pairs, a_f32, b_f32):
    """3. fp32 storage on one or both sides: the data rounded to fp32 (a side passed as fp64 holds the rounded values widened
    again), against the reference's metrics of the rounded trajectories, same gate."""
    rounded = lambda t: t.astype(np.float32).astype(np.float64)             # noqa: E731
    xa, da = _device_block(rounded(pairs["a"]), torch.float32 if a_f32 else torch.float64)
    xb, db = _device_block(rounded(pairs["b"]), torch.float32 if b_f32 else torch.float64)
    _, out, _, _ = _compare(xa, da, xb, db, chunks=[137, T - 137])
    _assert_gate(out.T, pairs["metrics_rounded"], what=f"a_f32={a_f32} b_f32={b_f32}")


@pytest.mark.parametrize("n", [1, 63, 65, 257])
def test_batch_edges(pairs, single, n):
    """4. Partial waves and more than one workgroup (64 lanes each): the ten pairs tiled over n lanes; every lane bit-equal to
    its pair's column of the single launch, and the 64 sentinel words behind acc and out untouched."""
    lane = np.arange(n) % PAIRS
    xa, da = _device_block(pairs["a"][lane])
    xb, db = _device_block(pairs["b"][lane])
    acc, out, acc_raw, out_raw = _compare(xa, da, xb, db, pad=64)
    assert np.array_equal(_bits(acc), _bits(single["acc"][:, lane])) and np.array_equal(_bits(out), _bits(single["out"][:, lane]))
    assert (acc_raw[L.FD_NTA * n:] == SENTINEL).all() and (out_raw[L.FD_NTM * n:] == SENTINEL).all()


def test_derived_rows_in_kernel(single):
    """5. da = db = NULL (airspeed and altitude derived in the kernel) against passing fdyn_derived_f64's rows: bit-equal, the
    kernel calls the device function fdyn_derived_f64 is made of.  Also the argument errors."""
    lib = _lib.load()

    def derived(x):                                               # x [T][12][n] -> [T][FD_ND][n] in one launch
        steps, _, n = x.shape
        flat = x.permute(1, 0, 2).reshape(L.FD_NX, steps * n).contiguous()
        d = torch.empty((L.FD_ND, steps * n), dtype=torch.float64, device="cuda")
        _lib.check(lib.fdyn_derived_f64(_lib.ptr(flat), steps * n, _lib.ptr(d), _lib.current_stream()))
        return d.reshape(L.FD_ND, steps, n).permute(1, 0, 2).contiguous()
    xa, xb = single["xa"], single["xb"]
    acc0, out0, _, _ = _compare(xa, None, xb, None)
    acc1, out1, _, _ = _compare(xa, derived(xa), xb, derived(xb))
    assert np.array_equal(_bits(acc0), _bits(acc1)) and np.array_equal(_bits(out0), _bits(out1))
    _assert_gate(out0.T, single["out"].T, what="derived in kernel vs the reference's airspeed column")
    acc, out = _buffers(PAIRS)
    args = (_lib.ptr(xa), 0, None, _lib.ptr(xb), 0, None)
    assert lib.fdyn_traj_compare(*args, -1, PAIRS, _lib.ptr(acc), None, None) == _lib.FDYN_ERR_BAD_SIZE
    assert lib.fdyn_traj_compare(*args, 1, -1, _lib.ptr(acc), None, None) == _lib.FDYN_ERR_BAD_SIZE
    assert lib.fdyn_traj_compare(*args, 1, PAIRS, None, None, None) == _lib.FDYN_ERR_NULL
    assert lib.fdyn_traj_compare(None, 0, None, _lib.ptr(xb), 0, None, 1, PAIRS, _lib.ptr(acc), None, None) == _lib.FDYN_ERR_NULL
    assert lib.fdyn_traj_compare(*args, 1, 0, None, None, None) == _lib.FDYN_OK


# |metric - fixture| / max(|fixture|, 1) of pair 0 when the CPU oracle (fp64, the reference's arithmetic in C) flies the level
# flight and NumPy reduces it, measured in the build container: see test_level_flight_fleets_end_to_end
ORACLE_DEVIATION = 5.551115123125783e-16          # 2.5 ulp of 1: the oracle reproduces the reference's flight to rounding
END_TO_END_GATE = 100 * ORACLE_DEVIATION


def _numpy_metrics(a, b):
    """a, b [T][14][n] in V.CHANNELS order (radians) -> [35][n]: the reference's formulas in vectorised NumPy (np.degrees,
    np.unwrap(period=360), RMSE, max error, and np.corrcoef's r = sum(am bm) / sqrt(sum(am^2) sum(bm^2)) about the means)."""
    a, b = a.copy(), b.copy()
    a[:, _ATT], b[:, _ATT] = np.degrees(a[:, _ATT]), np.degrees(b[:, _ATT])
    yaw = V.CHANNELS.index("yaw")
    a[:, yaw], b[:, yaw] = np.unwrap(a[:, yaw], period=360, axis=0), np.unwrap(b[:, yaw], period=360, axis=0)
    e = a - b
    rmse, mx = np.sqrt(np.mean(e ** 2, axis=0)), np.abs(e).max(axis=0)
    pos = np.sqrt(e[:, 0] ** 2 + e[:, 1] ** 2 + e[:, 2] ** 2)
    am, bm = a - a.mean(axis=0), b - b.mean(axis=0)
    with np.errstate(all="ignore"):
        r = np.clip((am * bm).sum(axis=0) / np.sqrt((am ** 2).sum(axis=0) * (bm ** 2).sum(axis=0)), -1.0, 1.0)
    r[(a == a[:1]).all(axis=0) | (b == b[:1]).all(axis=0)] = np.nan
    ch = {c: j for j, c in enumerate(V.CHANNELS)}
    m = {}
    for k in V.METRIC_KEYS:
        kind, _, rest = k.partition("_")
        if k == "position_3d_rmse":
            m[k] = np.sqrt(np.mean(pos ** 2, axis=0))
        elif k == "position_3d_max_error":
            m[k] = pos.max(axis=0)
        elif kind in ("position", "velocity", "attitude", "rate", "altitude", "airspeed"):
            c = ch[kind] if kind in ("altitude", "airspeed") else ch[rest.split("_")[0]]
            m[k] = r[c] if "correlation" in k else (mx[c] if "max_error" in k else rmse[c])
    m["mean_position_correlation"] = np.mean([m[f"position_{c}_correlation"] for c in ("north", "east", "down")], axis=0)
    m["mean_attitude_correlation"] = np.mean([m[f"attitude_{c}_correlation"] for c in ("roll", "pitch", "yaw")], axis=0)
    m["overall_correlation"] = np.mean([m["mean_position_correlation"], m["mean_attitude_correlation"]], axis=0)
    return np.stack([m[k] for k in V.METRIC_KEYS])


def oracle_level_flight_deviation(orc, pairs):
    """The figure END_TO_END_GATE is derived from (CPU only): the oracle flies LevelFlightScenario(duration 5) for rc_plane and
    cessna with the backend's sub-stepping, NumPy reduces the pair, and the result is compared with fixture pair 0."""
    from hcrl_amd.params import aircraft_params_for
    sc = V.LevelFlightScenario({"duration": 5})
    u = orc.clip_controls(sc.get_control_function()(0.0).to_array())
    sides = []
    for kind in ("rc_plane", "cessna"):
        P, x = aircraft_params_for(kind).to_block(), sc.get_initial_conditions().to_vector().astype(np.float64)
        rows = np.zeros((sc.num_steps, L.FD_NTC, 1))
        for k in range(sc.num_steps):
            orc.backend_step(P, x, u, sc.dt, sc.DT_PHYSICS)
            d = orc.derived(x)
            rows[k, _STATE, 0] = x
            rows[k, V.CHANNELS.index("airspeed"), 0], rows[k, V.CHANNELS.index("altitude"), 0] = d[0], d[1]
        sides.append(rows)
    got, want = _numpy_metrics(*sides)[:, 0], pairs["metrics"][0]
    assert np.array_equal(np.isnan(got), np.isnan(want))
    return float(np.nanmax(np.abs(got - want) / np.maximum(np.abs(want), 1.0)))


def test_level_flight_fleets_end_to_end(pairs):
    """6. LevelFlightScenario(duration 5).run_fleets on two f64 BatchedSixDOF fleets, rc_plane against cessna, n = 64: every
    aircraft against the reference's own simulation AND metrics (fixture pair 0).  Gate: 100 x the deviation of the same
    metrics when the CPU oracle flies the scenario and NumPy reduces it (oracle_level_flight_deviation, measured in the build
    container: 5.55e-16, so the gate is 5.55e-14; the device's fleets measured 6.8e-15), which leaves room for the GPU's libm and contraction at the scale the f64 parity
    tests accept."""
    from hcrl_amd.fleet import BatchedSixDOF
    n = 64
    cmp_ = V.LevelFlightScenario({"duration": 5}).run_fleets(BatchedSixDOF(n, "f64", types=("rc_plane",)),
                                                             BatchedSixDOF(n, "f64", types=("cessna",)))
    got = cmp_.metrics().cpu().numpy()
    assert float(cmp_.acc[L.FD_TA_COUNT].min()) == float(cmp_.acc[L.FD_TA_COUNT].max()) == T
    assert np.array_equal(_bits(got), _bits(np.repeat(got[:, :1], n, axis=1)))                # identical aircraft, identical lanes
    _assert_gate(got.T, np.tile(pairs["metrics"][0], (n, 1)), gate=END_TO_END_GATE, what="level flight, fleets")


def test_many_workgroups_f64_against_mixed():
    """7. f64 against mixed fleets from the cfg-2 envelope draw, n = 4096 (64 workgroups), 200 steps, update_fleets after every
    step; the states (and fdyn_derived_f64's airspeed / altitude rows, which the kernel reproduces bit for bit -- test 5) are
    recorded as well and reduced with NumPy.  Correlations sit at 1 - eps here, so their gate is 1e-10 absolute; everything
    else 1e-12 relative to the value itself.  Aircraft with a channel of variance < 1e-20 are left out of the correlation
    comparison only (at most 1 %)."""
    from hcrl_amd.fleet import BatchedSixDOF
    from test_gpu_parity_scale import _cfg2_inputs
    n, steps, dt = 4096, 200, 0.01
    x0, u = _cfg2_inputs(n, seed=20261004)
    fleets = [BatchedSixDOF(n, "f64"), BatchedSixDOF(n, "mixed")]
    cmp_ = V.TrajectoryComparison(n, chunk=1)                     # the fleets' own x buffers, read in place
    rec = torch.zeros((2, steps, L.FD_NTC, n), dtype=torch.float64, device="cuda")
    for f in fleets:
        f.reset(x0)
        f.set_controls(u)
    for t in range(steps):
        for s, f in enumerate(fleets):
            f.step(dt, 0.001)
            d = f.derived()
            rec[s, t, _STATE] = f.x
            rec[s, t, V.CHANNELS.index("airspeed")], rec[s, t, V.CHANNELS.index("altitude")] = d[L.FD_D_AIRSPEED], d[L.FD_D_ALTITUDE]
        cmp_.update_fleets(*fleets)
    got = cmp_.metrics().cpu().numpy()
    host = rec.cpu().numpy()
    want = _numpy_metrics(host[0], host[1])
    assert np.array_equal(np.isnan(got), np.isnan(want)) and not np.isnan(want[[j for j in range(L.FD_NTM) if j not in _CORR]]).any()
    rest = [j for j in range(L.FD_NTM) if j not in _CORR]
    rel = np.abs(got[rest] - want[rest]) / np.abs(np.where(want[rest] == 0, 1.0, want[rest]))
    print(f"worst relative deviation outside the correlations: {rel.max():.3e}; largest 3-D RMSE {want[L.FD_TM_POSITION_3D_RMSE].max():.3e} m")
    assert rel.max() <= 1e-12, (rel.max(), V.METRIC_KEYS[rest[int(np.argmax(rel.max(axis=1)))]])
    deg = host.copy()
    deg[:, :, _ATT] = np.degrees(deg[:, :, _ATT])
    flat = (deg.var(axis=1) < 1e-20).any(axis=(0, 1))                                      # [n]: some channel barely moves
    assert flat.mean() <= 0.01, flat.sum()
    err = np.abs(got[_CORR] - want[_CORR])[:, ~flat]
    print(f"worst correlation deviation: {np.nanmax(err):.3e} over {(~flat).sum()} aircraft")
    assert np.nanmax(err) <= 1e-10

"""fdyn_servo_flight_modes, fdyn_servo_sampled_modes, fdyn_servo_filter_modes, fdyn_square_modes and hcrl_amd.servo_modes on the device.

Reference on the box: the NumPy restatement (tests/servo_modes_numpy.py) on the servo matrices of the 288 linearisations of
tests/golden/trim_reference.npz under the restatements' default servo and servo-Kalman designs, computed once per session.

Gates (none derived from what the kernel returns):
  grid          the three servo entries on the 288 linearisations at dt 0.02 (the sampled loop at 0.01 as well): every word of eig_re,
                eig_im, summary, iters and status BIT-IDENTICAL to the restatement (fp64 on both sides, one rounding per operation in
                the same order; + - * / and sqrt only)
  square        fdyn_square_modes at every N = 2 .. 7 on degenerate_cases and shift_cases: bit-identical; the capped case status 1, the
                NaN / inf lanes status 2 and all-NaN words
  shapes        n = 1, 63, 65, 257 with sentinel pads behind every output; summary = iters = NULL leaves the rest bit-equal; a lane's
                result does not depend on its position or on its wave-mates (lanes permuted: the check that a diverged wave's window
                logic is per lane)
  consistency   fdyn_square_modes at N = 7 / 6 / 5 on the matrices torch composes against the fused entries' spectra: the trace gate of
                tests/test_servo_modes_oracle.py on both (the operation order differs: not bit-identical), and its Bauer-Fike gate
                between the two spectra; at N = 4 on the two blocks fdyn_block_modes takes, against fdyn_block_modes within the
                Bauer-Fike gate -- DIFFERENT algorithms (that one sweeps the whole 4 x 4 and copies the 3 x 3 a deflation leaves, this one
                shrinks a window), so bits are not asked for
  bad lanes     a NaN in K, in F, in A inside a block, V0 = 0, interleaved among good lanes: the good lanes bit-identical to a launch
                without them, the bad ones all NaN with status 2; a NaN of A OUTSIDE the blocks is not read
  graph         replay bit-equal to eager for all four entries; refused calls write nothing
  fleet         BatchedSixDOF.trim -> design_servo -> design_servo_kalman -> servo_modes(loop=...) for the ten aircraft of
                lqr_numpy.oracle_flights: on the fleet's own words bit-identical to the restatement and inside the oracle test's two
                gates against LAPACK; against the NumPy chain over the CPU oracle within 1e-9 kappa_2(V) |M|_2 (Bauer-Fike for a
                matrix perturbation of 1e-9 |M|_2, the tolerance tests/test_gpu_servo_margins.py holds the same two chains to); the
                report's helpers against their NumPy definitions at rtol 1e-14
"""
import faulthandler
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import lqr_numpy as ln
import modes_numpy as mo
import servo_lqg_numpy as sl
import servo_modes_numpy as smn
import servo_numpy as sn
import trim_numpy as tn
from hcrl_amd import _lib, layout as L
from hcrl_amd import modes as MO
from hcrl_amd import servo_modes as SMO
from hcrl_amd import trim as T
from hcrl_amd.fleet import BatchedSixDOF

pytestmark = pytest.mark.gpu

SENTINEL = -12345.678
ISENT = -1234567
PAD = 96
DEV = "cuda"
KEYS = ("re", "im", "summary", "iters", "status")
TIME_LIMIT_S = 120
C, EPS = 100.0, 2.0 ** -52                                       # tests/test_servo_modes_oracle.py


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(TIME_LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _soa(a):
    """host [n][...] -> device [...][n]"""
    return torch.as_tensor(np.ascontiguousarray(np.moveaxis(np.asarray(a, np.float64), 0, -1)), device=DEV)


def _padded(rows, n, dtype=torch.float64, fill=SENTINEL):
    return torch.full((rows * n + PAD,), fill, dtype=dtype, device=DEV)


def _call(name, pre, n, sizes, summary=True, iters=True, expect_rc=0, drop=None):
    """One launch of entry point `name`: pre = its arguments before n (device tensors, scalars), sizes = eigenvalues per block ->
    dict shaped as servo_modes_numpy.blocks_modes shapes it; every output buffer has a sentinel pad behind it, asserted untouched.
    drop: the index in `pre`, or the name of an output, to pass as NULL."""
    rows, nb, m = sum(sizes), len(sizes), max(n, 1)
    re, im, sm = _padded(rows, m), _padded(rows, m), _padded(nb * L.FD_NMO, m)
    it, st = _padded(1, m, torch.int32, ISENT), _padded(1, m, torch.int32, ISENT)
    args = [(_lib.ptr(a) if isinstance(a, torch.Tensor) else a) for a in pre]
    outs = dict(re=_lib.ptr(re), im=_lib.ptr(im), sm=_lib.ptr(sm) if summary else None, it=_lib.ptr(it) if iters else None, st=_lib.ptr(st))
    if isinstance(drop, int):
        args[drop] = None
    elif drop:
        outs[drop] = None
    rc = getattr(_lib.load(), name)(*args, n, outs["re"], outs["im"], outs["sm"], outs["it"], outs["st"], _lib.current_stream())
    torch.cuda.synchronize()
    assert rc == expect_rc, (name, rc)
    if rc:
        for buf, sent in ((re, SENTINEL), (im, SENTINEL), (sm, SENTINEL), (it, ISENT), (st, ISENT)):
            assert bool((buf == sent).all()), "a refused launch wrote something"
        return None
    for buf, r, sent in ((re, rows, SENTINEL), (im, rows, SENTINEL), (sm, nb * L.FD_NMO if summary else 0, SENTINEL), (it, 1 if iters else 0, ISENT),
                         (st, 1, ISENT)):
        assert bool((buf[r * n:] == sent).all()), "wrote behind an output buffer (or into one it was not given)"
    return dict(re=re[:rows * n].reshape(rows, n).T.cpu().numpy(), im=im[:rows * n].reshape(rows, n).T.cpu().numpy(),
                summary=sm[:nb * L.FD_NMO * n].reshape(nb, L.FD_NMO, n).permute(2, 0, 1).cpu().numpy() if summary else None,
                iters=it[:n].cpu().numpy() if iters else None, status=st[:n].cpu().numpy())


def _flight(A, B, x0, K, **kw):
    return _call("fdyn_servo_flight_modes", [_soa(A), _soa(B), _soa(x0), _soa(K)], len(A), (7, 6), **kw)


def _sampled(K, F, x0, dt, **kw):
    return _call("fdyn_servo_sampled_modes", [_soa(K), _soa(F), _soa(x0), float(dt)], len(K), (7, 6), **kw)


def _filter(F, **kw):
    return _call("fdyn_servo_filter_modes", [_soa(F)], len(F), (5, 5), **kw)


def _square(M, **kw):
    M = np.asarray(M, np.float64)
    N = M.shape[1]
    return _call("fdyn_square_modes", [_soa(M.reshape(len(M), N * N)), N], len(M), (N,), **kw)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same(a, b, keys=KEYS):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in keys)


def _take(r, idx, keys=KEYS):
    return {k: r[k][idx] for k in keys}


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "trim_reference.npz"))


@pytest.fixture(scope="module")
def loops(golden):
    return smn.golden_loops(golden)


@pytest.fixture(scope="module")
def want(golden):
    return smn.golden_reports(golden)


@pytest.fixture(scope="module")
def AB(golden):
    return np.asarray(golden["A"], np.float64), np.asarray(golden["B"], np.float64)


# ---- the kernels against the restatement ------------------------------------------------------------------------------------------
def test_flight_modes_grid_is_bit_identical_to_the_restatement(AB, loops, want):
    got = _flight(*AB, loops["x0"], loops["K"])
    assert not got["status"].any() and got["iters"].max() >= 10
    assert _same(got, want["continuous"]), [k for k in KEYS if not np.array_equal(_bits(got[k]), _bits(want["continuous"][k]))]
    ok = loops["status"] == 0
    assert (got["summary"][ok][:, :, mo.ABSCISSA] < 0.0).all()


@pytest.mark.parametrize("dt", smn.DTS)
def test_sampled_modes_grid_is_bit_identical_to_the_restatement(loops, want, dt):
    got = _sampled(loops["K"], loops["F"][dt], loops["x0"], dt)
    assert not got["status"].any()
    assert _same(got, want["sampled"][dt]), [k for k in KEYS if not np.array_equal(_bits(got[k]), _bits(want["sampled"][dt][k]))]
    assert (got["summary"][:, :, mo.RADIUS] < 1.0).all()


@pytest.mark.parametrize("dt", smn.DTS)
def test_filter_modes_grid_is_bit_identical_to_the_restatement(loops, want, dt):
    got = _filter(loops["F"][dt])
    assert not got["status"].any()
    assert _same(got, want["filter"][dt]), [k for k in KEYS if not np.array_equal(_bits(got[k]), _bits(want["filter"][dt][k]))]
    assert (got["summary"][:, :, mo.RADIUS] < 1.0).all()


@pytest.mark.parametrize("N", range(smn.MIN_N, smn.MAX_N + 1))
def test_square_modes_on_the_degenerate_and_shift_cases(N):
    cases = smn.degenerate_cases(N) + [(name, m) for name, m, _, _ in smn.shift_cases(N)]
    ref = smn.square_modes([m for _, m in cases])
    got = _square([m for _, m in cases])
    for i, (name, m) in enumerate(cases):
        assert _same(_take(got, [i]), _take(ref, [i])), (N, name, _take(got, [i]), _take(ref, [i]))
        if not np.isfinite(m).all():
            assert got["status"][i] == smn.BAD_INPUT and np.isnan(got["re"][i]).all() and np.isnan(got["im"][i]).all() and np.isnan(got["summary"][i]).all()
        elif name.endswith("to the cap"):
            assert got["status"][i] == smn.NOT_CONVERGED and np.isnan(got["re"][i]).all() and np.isnan(got["summary"][i]).all() and got["iters"][i] >= 30
        else:
            assert got["status"][i] == 0, (N, name)
    assert (got["status"] == smn.BAD_INPUT).sum() == 3 and (got["status"] == smn.NOT_CONVERGED).sum() == (1 if N > 2 else 0)


# ---- shapes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 63, 65, 257))
def test_shapes_pads_and_optional_outputs(AB, loops, want, n):
    idx = (np.arange(n) * 7 + 3) % 288
    dt = 0.02
    runs = (("continuous", lambda **kw: _flight(AB[0][idx], AB[1][idx], loops["x0"][idx], loops["K"][idx], **kw), want["continuous"]),
            ("sampled", lambda **kw: _sampled(loops["K"][idx], loops["F"][dt][idx], loops["x0"][idx], dt, **kw), want["sampled"][dt]),
            ("filter", lambda **kw: _filter(loops["F"][dt][idx], **kw), want["filter"][dt]),
            ("square", lambda **kw: _square([loops["continuous"][i][0] for i in idx], **kw), None))
    for name, run, ref in runs:
        full = run()
        if ref is not None:
            assert _same(full, _take(ref, idx)), (name, n)
        else:
            assert np.array_equal(_bits(full["re"]), _bits(want["continuous"]["re"][idx, :7])), n           # the same 7 x 7 through the other door
        bare = run(summary=False, iters=False)
        assert _same(bare, full, ("re", "im", "status")) and bare["summary"] is None and bare["iters"] is None, (name, n)


def test_a_lane_does_not_depend_on_its_position_or_its_wave_mates(loops, want):
    """7 x 7 matrices that deflate at different sweeps and in different orders, some refused, some capped, side by side in one wave:
    permuted, reversed and alone they give the same words."""
    cases = [m for _, m in smn.degenerate_cases(7)] + [m for _, m, _, _ in smn.shift_cases(7)] + [loops["continuous"][i][0] for i in range(0, 288, 3)]
    cases += [loops["sampled"][0.02][i][0] for i in range(1, 288, 5)]
    base = _square(cases)
    assert len(cases) > 128 and set(base["status"]) == {0, 1, 2} and len(set(base["iters"])) >= 8
    rs = np.random.RandomState(7)
    for perm in (rs.permutation(len(cases)), np.arange(len(cases))[::-1], rs.permutation(len(cases))[:70]):
        assert _same(_square([cases[i] for i in perm]), _take(base, perm))
    for i in (0, 17, len(cases) - 1):
        assert _same(_square([cases[i]]), _take(base, [i]))
    # the servo entries: both blocks of a lane, wave-mates swapped
    perm = rs.permutation(288)
    got = _sampled(loops["K"][perm], loops["F"][0.02][perm], loops["x0"][perm], 0.02)
    assert _same(got, _take(want["sampled"][0.02], perm))


# ---- consistency -------------------------------------------------------------------------------------------------------------------
def _gate_pair(a, b, M):
    """Two spectra of (nearly) one matrix M -> (trace ratio of a, trace ratio of b, Bauer-Fike ratio between them or None)."""
    _, bf, nrm = smn.bauer_fike(M)
    tr = lambda lam: abs(lam.sum() - np.trace(M)) / (len(M) * EPS * nrm)
    return tr(a), tr(b), (None if bf / nrm > 1e8 else smn.assignment_gap(a, b) / (EPS * bf))


def test_square_modes_on_torch_composed_matrices_agree_with_the_fused_entries(golden, AB, loops, want):
    from hcrl_amd import servo as SV, servo_lqg as SL
    dt, n = 0.02, 288
    zi, zd = torch.zeros(n, dtype=torch.int32, device=DEV), torch.zeros(n, dtype=torch.float64, device=DEV)
    design = SV.ServoDesign(_soa(loops["K"]), zd, zi, zi.clone(), _soa(loops["x0"]))
    kalman = SL.ServoKalmanDesign(_soa(loops["F"][dt]), zd, zi, zi.clone(), dt)
    A, B = _soa(AB[0]), _soa(AB[1])
    composed = {"continuous": design.closed_loop(A, B)}
    eye = torch.eye(5, dtype=torch.float64, device=DEV)[None, :, :, None]
    filt = torch.einsum("bikn,bkjn->bijn", eye - kalman.gain(), kalman.phi())
    composed["filter"] = (filt[0], filt[1])
    fused = {"continuous": want["continuous"], "filter": want["filter"][dt]}
    worst = [0.0, 0.0]
    for loop, mats in composed.items():
        at = 0
        for M in mats:
            N = int(M.shape[0])
            sq = SMO.square_modes_into(M)
            torch.cuda.synchronize()
            assert bool(sq.ok.all()) and sq.sizes == (N,)
            lam_sq = (sq.eig_re + 1j * sq.eig_im).T.cpu().numpy()
            Mh = M.permute(2, 0, 1).cpu().numpy()
            for i in range(n):
                lam_f = fused[loop]["re"][i, at:at + N] + 1j * fused[loop]["im"][i, at:at + N]
                ta, tb, bf = _gate_pair(lam_sq[i], lam_f, Mh[i])
                assert ta <= C and tb <= C and (bf is None or bf <= C), (loop, N, i, ta, tb, bf)
                worst = [max(worst[0], ta, tb), max(worst[1], bf or 0.0)]
            at += N
    print(f"square against fused on torch-composed matrices: trace ratio {worst[0]:.3g}, Bauer-Fike ratio {worst[1]:.3g} (gate {C:g})")


def test_square_modes_at_4_agree_with_block_modes(golden):
    """Two algorithms on one matrix: Bauer-Fike, not bits."""
    blocks = mo.golden_blocks(golden)["closed"]                  # [288][2][4][4]
    old = MO.block_modes_into(torch.as_tensor(np.ascontiguousarray(blocks.transpose(1, 2, 3, 0)), device=DEV))
    torch.cuda.synchronize()
    assert bool(old.ok.all())
    worst, left = 0.0, 0
    for b in range(2):
        new = _square(blocks[:, b])
        assert not new["status"].any()
        lam_old = (old.eig_re[4 * b:4 * b + 4] + 1j * old.eig_im[4 * b:4 * b + 4]).T.cpu().numpy()
        for i in range(len(blocks)):
            _, _, bf = _gate_pair(new["re"][i] + 1j * new["im"][i], lam_old[i], blocks[i, b])
            if bf is None:
                left += 1
                continue
            assert bf <= C, (b, i, bf)
            worst = max(worst, bf)
    print(f"N = 4 against fdyn_block_modes: Bauer-Fike ratio {worst:.3g}, {left} blocks left out (kappa > 1e8)")
    assert left <= 0.02 * 2 * len(blocks)


# ---- bad lanes ---------------------------------------------------------------------------------------------------------------------
def test_bad_lanes_do_not_disturb_their_neighbours(AB, loops, want):
    n, dt = 130, 0.02
    idx = np.arange(n)
    A, B, x0, K, F = AB[0][idx].copy(), AB[1][idx].copy(), loops["x0"][idx].copy(), loops["K"][idx].copy(), loops["F"][dt][idx].copy()
    bad_k, bad_f, bad_a, bad_v, unread = 5, 66, 64, 129, 70
    K[bad_k, 20] = np.nan
    F[bad_f, 55] = np.nan                                        # a word of Gamma_lon
    A[bad_a, sn.LON_STATES[1], sn.LON_STATES[2]] = np.nan
    x0[bad_v, sn.X_U] = x0[bad_v, sn.X_W] = 0.0
    A[unread, 0, 1] = A[unread, sn.LON_STATES[0], sn.LAT_STATES[0]] = np.nan                   # outside the two blocks
    x0[unread, [0, 1, 2, 4, 6, 7, 8, 9, 10, 11]] = np.nan                                      # not u, w
    for name, got, ref, bad in (("continuous", _flight(A, B, x0, K), want["continuous"], {bad_k, bad_a, bad_v}),
                                ("sampled", _sampled(K, F, x0, dt), want["sampled"][dt], {bad_k, bad_f, bad_v}),
                                ("filter", _filter(F), want["filter"][dt], set())):
        good = np.array([i for i in idx if i not in bad])
        assert _same(_take(got, good), _take(ref, good)), name
        assert unread in good
        for i in bad:
            assert got["status"][i] == smn.BAD_INPUT and got["iters"][i] == 0, (name, i)
            assert np.isnan(got["re"][i]).all() and np.isnan(got["im"][i]).all() and np.isnan(got["summary"][i]).all(), (name, i)
    F[3, L.FD_SKF_L_LAT + 7] = np.inf
    got = _filter(F)
    assert got["status"][3] == smn.BAD_INPUT and np.isnan(got["re"][3]).all() and got["status"][bad_f] == 0          # Gamma is not read
    assert _sampled(K[:1], F[:1], x0[:1], 0.0)["status"][0] == smn.BAD_INPUT and _sampled(K[:1], F[:1], x0[:1], 1.5)["status"][0] == smn.BAD_INPUT


# ---- graph and refusals -----------------------------------------------------------------------------------------------------------
def test_graph_replay_is_bit_equal_to_eager(AB, loops):
    dt, n = 0.02, 288
    A, B, x0, K, F = _soa(AB[0]), _soa(AB[1]), _soa(loops["x0"]), _soa(loops["K"]), _soa(loops["F"][dt])
    M = _soa(np.array([lane[0] for lane in loops["sampled"][dt]]))
    entries = ((lambda out=None: SMO.flight_modes_into(A, B, x0, K, out), (7, 6)), (lambda out=None: SMO.sampled_modes_into(K, F, x0, dt, out), (7, 6)),
               (lambda out=None: SMO.filter_modes_into(F, out), (5, 5)), (lambda out=None: SMO.square_modes_into(M, out), (7,)))
    for run, sizes in entries:
        eager = run()
        out = SMO.empty(n, A.device, sizes)
        for t in (out.eig_re, out.eig_im, out.summary):
            t.fill_(SENTINEL)
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            run(out)
        gr.replay()
        torch.cuda.synchronize()
        assert bool(eager.ok.all())
        for a, b in ((eager.eig_re, out.eig_re), (eager.eig_im, out.eig_im), (eager.summary, out.summary)):
            assert np.array_equal(_bits(a.cpu().numpy()), _bits(b.cpu().numpy()))
        assert torch.equal(eager.iterations, out.iterations) and torch.equal(eager.status, out.status)


def test_refused_calls_write_nothing(AB, loops):
    dt = 0.02
    A, B, x0, K, F = _soa(AB[0][:4]), _soa(AB[1][:4]), _soa(loops["x0"][:4]), _soa(loops["K"][:4]), _soa(loops["F"][dt][:4])
    M = _soa(np.zeros((4, 49)))
    calls = (("fdyn_servo_flight_modes", [A, B, x0, K], (7, 6)), ("fdyn_servo_sampled_modes", [K, F, x0, dt], (7, 6)),
             ("fdyn_servo_filter_modes", [F], (5, 5)), ("fdyn_square_modes", [M, 7], (7,)))
    for name, pre, sizes in calls:
        for n in (0, -1):
            assert _call(name, pre, n, sizes, expect_rc=_lib.FDYN_ERR_BAD_SIZE) is None
        for drop in [k for k, a in enumerate(pre) if isinstance(a, torch.Tensor)] + ["re", "im", "st"]:
            assert _call(name, pre, 4, sizes, expect_rc=_lib.FDYN_ERR_NULL, drop=drop) is None
    for N in (1, 8):
        assert _call("fdyn_square_modes", [M, N], 4, (7,), expect_rc=_lib.FDYN_ERR_BAD_SIZE) is None


# ---- the fleet ---------------------------------------------------------------------------------------------------------------------
def test_fleet_chain_against_numpy_over_the_oracle():
    base = sn.compare_flights()
    n = len(base["type"])
    fleet = BatchedSixDOF(n, "f64", types=tn.TYPES, type_index=base["type"])
    with pytest.raises(ValueError, match="no certified stabilising servo gain"):
        fleet.servo_modes()
    fleet.trim(base["spec"][:, 0], base["spec"][:, 1], base["spec"][:, 2], ln.ALTITUDE, ln.HEADING)
    servo = fleet.design_servo()
    with pytest.raises(ValueError, match="no certified stable servo filter"):
        fleet.servo_modes("sampled")
    res, scales = fleet._trim
    A, B = T.linearize_at_trim(res, fleet.params, fleet.type_index, scales)
    host = lambda t: np.ascontiguousarray(np.moveaxis(t.cpu().numpy(), -1, 0))
    Ah, Bh, Kh, xh = host(A), host(B), host(servo.K), host(servo.x0)
    for dt in smn.DTS:
        kal = fleet.design_servo_kalman(dt)
        Fh = host(kal.F)
        F_ref = sl.design_many(base["A"], base["B"], dt, sl.default_noise())["F"]
        chains = {"continuous": (smn.servo_flight_modes(Ah, Bh, xh, Kh), [smn.continuous_blocks(Ah[i], Bh[i], xh[i], Kh[i]) for i in range(n)],
                                 [smn.continuous_blocks(base["A"][i], base["B"][i], base["x0"][i], base["K"][i]) for i in range(n)]),
                  "sampled": (smn.servo_sampled_modes(Kh, Fh, xh, dt), [smn.sampled_blocks(Kh[i], Fh[i], xh[i], dt) for i in range(n)],
                              [smn.sampled_blocks(base["K"][i], F_ref[i], base["x0"][i], dt) for i in range(n)]),
                  "filter": (smn.servo_filter_modes(Fh), [smn.filter_blocks(Fh[i]) for i in range(n)], [smn.filter_blocks(F_ref[i]) for i in range(n)])}
        for loop, (own, own_mats, ref_mats) in chains.items():
            m = fleet.servo_modes(loop)
            torch.cuda.synchronize()
            assert bool(m.ok.all()) and m.sizes == ((5, 5) if loop == "filter" else (7, 6))
            got = dict(re=m.eig_re.T.cpu().numpy(), im=m.eig_im.T.cpu().numpy(), summary=m.summary.permute(2, 0, 1).cpu().numpy(),
                       iters=m.iterations.cpu().numpy(), status=m.status.cpu().numpy())
            assert _same(got, own), (loop, dt)
            worst = [0.0, 0.0, 0.0]
            for i in range(n):
                for b in range(2):
                    lam = m.eig(b)[:, i].cpu().numpy()
                    ref, bf, nrm = smn.bauer_fike(own_mats[i][b])
                    N = len(lam)
                    r_bf, r_tr = smn.assignment_gap(lam, ref) / (EPS * bf), abs(lam.sum() - np.trace(own_mats[i][b])) / (N * EPS * nrm)
                    ref2, bf2, _ = smn.bauer_fike(ref_mats[i][b])
                    r_chain = smn.assignment_gap(lam, ref2) / (1e-9 * bf2)
                    assert r_bf <= C and r_tr <= C and r_chain <= 1.0, (loop, dt, i, b, r_bf, r_tr, r_chain)
                    worst = [max(worst[0], r_bf), max(worst[1], r_tr), max(worst[2], r_chain)]
            print(f"{loop} dt {dt}: Bauer-Fike ratio {worst[0]:.3g}, trace ratio {worst[1]:.3g} (gate {C:g}); against the NumPy chain over the oracle "
                  f"{worst[2]:.3g} of 1e-9 kappa |M|")
            if loop == "continuous":
                assert bool((m.abscissa() < 0.0).all())
            else:
                assert bool((m.spectral_radius() < 1.0).all())
            # the helpers against their NumPy definitions
            for b in range(2):
                re, im = m.re(b).cpu().numpy(), m.im(b).cpu().numpy()
                wn = np.sqrt(re * re + im * im)
                np.testing.assert_allclose(m.natural_frequency(b).cpu().numpy(), wn, rtol=1e-14, atol=0.0)
                np.testing.assert_allclose(m.damping_ratio(b).cpu().numpy(), np.where(wn == 0.0, 0.0, -re / np.where(wn == 0.0, 1.0, wn)), rtol=1e-14, atol=0.0)
                with np.errstate(all="ignore"):
                    np.testing.assert_allclose(m.time_constant(b).cpu().numpy(), np.where(re == 0.0, np.inf, -1.0 / re), rtol=1e-14, atol=0.0)
                    np.testing.assert_allclose(m.time_to_double(b).cpu().numpy(), np.where(re > 0.0, np.log(2.0) / re, np.inf), rtol=1e-14, atol=0.0)
                if loop != "continuous" and not ((im == 0.0) & (re <= 0.0)).any():     # off the branch cut, where the two logs may differ by a sign of pi
                    np.testing.assert_allclose(m.to_s_plane(b, dt).cpu().numpy(), np.log(re + 1j * im) / dt, rtol=1e-14, atol=1e-14 / dt)
            assert torch.equal(m.lon[0], m.eig_re[:m.sizes[0]]) and torch.equal(m.lat[1], m.eig_im[m.sizes[0]:])
            assert torch.equal(m.min_damping(), m.summary[:, L.FD_MO_MIN_ZETA])
    same = SMO.sampled_poles(servo, fleet._servo_kalman)
    assert torch.equal(same.eig_re, fleet.servo_modes("sampled").eig_re)

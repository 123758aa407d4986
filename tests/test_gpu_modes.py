"""fdyn_flight_modes, fdyn_block_modes and hcrl_amd.modes on the device.

Reference on the box: the NumPy restatement (tests/modes_numpy.py) on the 288 linearisations of tests/golden/trim_reference.npz, open
loop and under the LQR restatement's default design, computed once per session.

Gates (none derived from what the kernel returns):
  grid          every word of eig_re, eig_im, summary, iters and status BIT-IDENTICAL to the restatement, open and closed loop (fp64
                on both sides, one rounding per operation in the same order; + - * / and sqrt only, as the margin kernel)
  shapes        n = 1, 63, 65, 257 with sentinel pads behind every output; summary = iters = NULL leaves the rest bit-equal; lane
                position is irrelevant
  K = NULL      equals K = 0 to the bit;  fdyn_block_modes on the blocks torch cuts out (and closes) equals fdyn_flight_modes
  bad lanes     NaN in A, in K, an infinity in A and in B interleaved among good lanes: the good lanes bit-identical to a launch
                without them, the bad ones all NaN with status 2; a NaN of A OUTSIDE the two blocks is not read
  graph         replay bit-equal to eager
  shifts        modes_numpy.shift_cases and the tie-rule matrices through fdyn_block_modes: bit-identical, the capped one status 1
  refusals      NULL required pointers and n = 0 give the return codes and write nothing
  fleet         BatchedSixDOF.trim -> design_lqr -> modes on the device against trim -> linearise -> design -> eigvals in NumPy
                over the CPU oracle (the ten aircraft of lqr_numpy.oracle_flights) within 1e-10 |m|_inf, the gate of
                tests/test_modes_oracle.py; KalmanDesign.filter_poles() and lqr.sampled_poles() inside the unit circle wherever the
                designs' status is 0
"""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import lqr_numpy as ln
import modes_numpy as mo
import trim_numpy as tn
from hcrl_amd import _lib, layout as L
from hcrl_amd import lqr as Q
from hcrl_amd import modes as MO
from hcrl_amd.fleet import BatchedSixDOF

pytestmark = pytest.mark.gpu

SENTINEL = -12345.678
ISENT = -1234567
PAD = 96
DEV = "cuda"
KEYS = ("re", "im", "summary", "iters", "status")


def _dev(a):
    return torch.as_tensor(np.array(a, order="C"), device=DEV)


def _padded(rows, n, dtype=torch.float64, fill=SENTINEL):
    return torch.full((rows * n + PAD,), fill, dtype=dtype, device=DEV)


def _collect(rc, expect_rc, n, re, im, sm, it, st, summary, iters):
    torch.cuda.synchronize()
    assert rc == expect_rc, rc
    if rc:
        for buf, sent in ((re, SENTINEL), (im, SENTINEL), (sm, SENTINEL), (it, ISENT), (st, ISENT)):
            assert bool((buf == sent).all()), "a refused launch wrote something"
        return None
    for buf, rows, sent in ((re, 8, SENTINEL), (im, 8, SENTINEL), (sm, 12 if summary else 0, SENTINEL), (it, 1 if iters else 0, ISENT),
                            (st, 1, ISENT)):
        assert bool((buf[rows * n:] == sent).all()), "wrote behind an output buffer (or into one it was not given)"
    lanes = lambda t, k: t[:2 * k * n].reshape(2, k, n).permute(2, 0, 1).cpu().numpy()
    return dict(re=lanes(re, 4), im=lanes(im, 4), summary=lanes(sm, L.FD_NMO) if summary else None,
                iters=it[:n].cpu().numpy() if iters else None, status=st[:n].cpu().numpy())


def _outputs(n):
    return _padded(8, n), _padded(8, n), _padded(12, n), _padded(1, n, torch.int32, ISENT), _padded(1, n, torch.int32, ISENT)


def _flight(A, B, K=None, summary=True, iters=True, n=None, expect_rc=0, drop=None):
    """A [n][12][12], B [n][12][4], K [n][16] or None (host, lane-major) -> dict of host arrays shaped as modes_numpy shapes them;
    every output buffer has a sentinel pad behind it, asserted untouched.  drop: the name of a required pointer to pass as NULL."""
    n = len(A) if n is None else n
    A_d, B_d = _dev(np.asarray(A).transpose(1, 2, 0)), _dev(np.asarray(B).transpose(1, 2, 0))
    K_d = None if K is None else _dev(np.asarray(K).T)
    re, im, sm, it, st = _outputs(max(n, 1))
    ptrs = dict(A=_lib.ptr(A_d), re=_lib.ptr(re), im=_lib.ptr(im), st=_lib.ptr(st))
    if drop:
        ptrs[drop] = None
    rc = _lib.load().fdyn_flight_modes(ptrs["A"], _lib.ptr(B_d), _lib.ptr(K_d), n, ptrs["re"], ptrs["im"], _lib.ptr(sm) if summary else None,
                                       _lib.ptr(it) if iters else None, ptrs["st"], _lib.current_stream())
    return _collect(rc, expect_rc, n, re, im, sm, it, st, summary, iters)


def _block(M, summary=True, iters=True, n=None, expect_rc=0, drop=None):
    """M [n][2][4][4] (host) or a device tensor [2][16][n]."""
    M_d = M if isinstance(M, torch.Tensor) else _dev(np.asarray(M).reshape(len(M), 32).T)
    n = int(M_d.shape[-1]) if n is None else n
    re, im, sm, it, st = _outputs(max(n, 1))
    ptrs = dict(M=_lib.ptr(M_d), re=_lib.ptr(re), im=_lib.ptr(im), st=_lib.ptr(st))
    if drop:
        ptrs[drop] = None
    rc = _lib.load().fdyn_block_modes(ptrs["M"], n, ptrs["re"], ptrs["im"], _lib.ptr(sm) if summary else None, _lib.ptr(it) if iters else None,
                                      ptrs["st"], _lib.current_stream())
    return _collect(rc, expect_rc, n, re, im, sm, it, st, summary, iters)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same(a, b, keys=KEYS):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in keys)


def _take(r, idx):
    return {k: r[k][idx] for k in KEYS}


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "trim_reference.npz"))


@pytest.fixture(scope="module")
def blocks(golden):
    return mo.golden_blocks(golden)


@pytest.fixture(scope="module")
def want(blocks):
    return {"open": mo.block_modes(blocks["open"]), "closed": mo.block_modes(blocks["closed"])}


@pytest.fixture(scope="module")
def grid_closed(golden, blocks):
    """The 288 aircraft under the default LQR in ONE launch: what the shape tests compare with."""
    return _flight(golden["A"], golden["B"], blocks["K"])


# ---- the kernel against the restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loop", ["open", "closed"])
def test_grid_is_bit_identical_to_the_restatement(golden, blocks, want, loop):
    got, ref = _flight(golden["A"], golden["B"], blocks["K"] if loop == "closed" else None), want[loop]
    assert got["status"].shape == (288,) and not got["status"].any(), np.flatnonzero(got["status"])
    for k in ("re", "im", "summary"):
        diff = _bits(got[k]) != _bits(ref[k])
        ulp = np.abs(_bits(got[k]).astype(np.int64) - _bits(ref[k]).astype(np.int64)).max()
        print(f"{loop} loop: {k}: {int(diff.sum())} of {diff.size} words differ from the restatement's, worst {int(ulp)} ulp")
    print(f"{loop} loop: at most {int(got['iters'].max())} sweeps; abscissa lon {got['summary'][:, 0, 0].min():.4f}..{got['summary'][:, 0, 0].max():.4f}, "
          f"lat {got['summary'][:, 1, 0].min():.4f}..{got['summary'][:, 1, 0].max():.4f}; unstable poles {int(got['summary'][:, :, 4].sum())}")
    assert _same(got, ref)


@pytest.mark.parametrize("n", [1, 63, 65, 257])
def test_shapes_lane_position_and_optional_outputs(n, grid_closed, golden, blocks):
    idx = (np.arange(n) * 7 + 3) % 288
    A, B, K = golden["A"][idx], golden["B"][idx], blocks["K"][idx]
    got = _flight(A, B, K)
    assert _same(got, _take(grid_closed, idx)), "a lane's result depends on where it sits in the launch"
    bare = _flight(A, B, K, summary=False, iters=False)
    assert bare["summary"] is None and bare["iters"] is None and _same(bare, got, ("re", "im", "status"))
    bare = _block(blocks["closed"][idx], summary=False, iters=False)
    assert _same(bare, got, ("re", "im", "status"))


def test_no_gain_is_a_zero_gain_to_the_bit(golden):
    A = golden["A"].copy()
    lon, lat = np.ix_(ln.LON_STATES, ln.LON_STATES), np.ix_(ln.LAT_STATES, ln.LAT_STATES)
    A[5][lon] = np.where(np.triu(np.ones((4, 4), dtype=bool)), A[5][lon], -0.0)      # -0 words inside a block, whatever sign b K = 0 takes
    A[6][lat] = np.where(np.eye(4, dtype=bool), A[6][lat], -0.0)
    none = _flight(A, golden["B"])
    assert _same(none, _flight(A, golden["B"], np.zeros((288, 16))))
    assert _same(none, _flight(A, golden["B"], -np.zeros((288, 16))))
    assert not none["status"].any()


def test_block_modes_on_blocks_cut_by_torch_equals_flight_modes(golden, blocks, want):
    A, B, K = _dev(golden["A"].transpose(1, 2, 0)), _dev(golden["B"].transpose(1, 2, 0)), _dev(blocks["K"].T)
    cut = []
    for base, states, ctl in ((L.FD_LQK_LON, ln.LON_STATES, ln.LON_CONTROLS), (L.FD_LQK_LAT, ln.LAT_STATES, ln.LAT_CONTROLS)):
        a = A[list(states)][:, list(states)]
        b = B[list(states)][:, list(ctl)]
        kb = K[base:base + 8].reshape(2, 4, 288)
        cut.append((a, a - (b[:, 0:1] * kb[0:1] + b[:, 1:2] * kb[1:2])))                   # one rounding per torch operation
    for k, loop in enumerate(("open", "closed")):
        M = torch.stack([cut[0][k], cut[1][k]]).reshape(2, 16, 288).contiguous()
        got = _block(M)
        assert _same(got, want[loop]), loop
        assert _same(got, _flight(golden["A"], golden["B"], blocks["K"] if k else None)), loop
    assert _same(_block(blocks["closed"]), want["closed"])


def test_bad_lanes_and_their_neighbours(golden, blocks):
    keep = np.arange(0, 288, 4)                                          # 72 good aircraft, both airframes
    lon, lat = ln.LON_STATES, ln.LAT_STATES

    def spoil(kind, a, b, k):
        if kind == 0: a[lon[1], lon[2]] = np.nan                         # NaN in the longitudinal block of A
        if kind == 1: a[lat[3], lat[0]] = np.inf                         # an infinity in the lateral block of A
        if kind == 2: k[11] = np.nan                                     # NaN in the lateral gains
        if kind == 3: b[lon[0], ln.LON_CONTROLS[1]] = -np.inf            # an infinity in the longitudinal block of B
        if kind == 4: a[0, 0] = a[lon[0], lat[0]] = a[2, 8] = np.nan; b[1, 0] = np.nan      # outside the blocks: not read
    A, B, K, kind = [], [], [], []
    for j, i in enumerate(keep):
        A.append(golden["A"][i]); B.append(golden["B"][i]); K.append(blocks["K"][i]); kind.append(-1)
        if j % 3 == 2:
            c = (j // 3) % 5
            a, b, k = golden["A"][i].copy(), golden["B"][i].copy(), blocks["K"][i].copy()
            spoil(c, a, b, k)
            A.append(a); B.append(b); K.append(k); kind.append(c)
    A, B, K, kind = np.array(A), np.array(B), np.array(K), np.array(kind)
    assert all((kind == c).sum() >= 2 for c in range(5))
    mixed = _flight(A, B, K)
    alone = _flight(golden["A"][keep], golden["B"][keep], blocks["K"][keep])
    assert not alone["status"].any()
    assert _same(_take(mixed, kind < 0), alone), "a good lane changed because of its neighbour"
    assert _same(mixed, mo.flight_modes(A, B, K))
    dead = (kind >= 0) & (kind <= 3)
    assert (mixed["status"][dead] == mo.BAD_INPUT).all() and (mixed["iters"][dead] == 0).all() and not mixed["status"][~dead].any()
    assert np.isnan(mixed["re"][dead]).all() and np.isnan(mixed["im"][dead]).all() and np.isnan(mixed["summary"][dead]).all()
    assert np.isfinite(mixed["re"][~dead]).all() and np.isfinite(mixed["summary"][~dead]).all()
    # open loop the gains and B are not read: only the two kinds that spoil A are bad
    open_ = _flight(A, B)
    assert _same(open_, mo.flight_modes(A, B)) and ((open_["status"] == mo.BAD_INPUT) == ((kind == 0) | (kind == 1))).all()
    # the same lanes through fdyn_block_modes
    M = mo.closed_blocks(A, B, K)
    assert _same(_block(M), mo.block_modes(M))


def test_exceptional_shifts_sweep_cap_and_tie_rule_on_the_device():
    """modes_numpy.shift_cases (both stages past sweeps 10 and 20; one matrix to the cap: status 1, all NaN) and the matrices whose
    poles share a real part, each beside an ordinary block and among ordinary lanes: bit-identical to the restatement."""
    plain = dict(mo.degenerate_cases())["already Hessenberg"]
    mats = [m for _, m, _, _, _ in mo.shift_cases()] + [m for name, m in mo.degenerate_cases() if "vertical line" in name]
    M = np.array([[plain, plain]] + [pair for m in mats for pair in ([m, plain], [plain, m], [plain, plain])])
    got, ref = _block(M), mo.block_modes(M)
    assert _same(got, ref)
    assert sorted(set(got["status"].tolist())) == [0, mo.NOT_CONVERGED] and (got["status"] == mo.NOT_CONVERGED).sum() == 2
    assert got["iters"].max() == 30 and np.isnan(got["re"][got["status"] != 0]).all() and np.isfinite(got["re"][got["status"] == 0]).all()


def test_graph_replay_equals_eager(golden, blocks):
    A, B, K = _dev(golden["A"].transpose(1, 2, 0)), _dev(golden["B"].transpose(1, 2, 0)), _dev(blocks["K"].T)
    M = _dev(blocks["closed"].reshape(288, 32).T).reshape(2, 4, 4, 288)
    eager, eager_b = MO.modes_into(A, B, K), MO.block_modes_into(M)
    out, out_b = MO.modes_into(A, B), MO.modes_into(A, B)                 # other values, then overwritten by the replay
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                            # warm-up outside the capture
        MO.modes_into(A, B, None, out)
        MO.block_modes_into(M, out_b)
    torch.cuda.current_stream().wait_stream(s)
    assert not torch.equal(out.eig_re, eager.eig_re)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        MO.modes_into(A, B, K, out)
        MO.block_modes_into(M, out_b)
    gr.replay()
    torch.cuda.synchronize()
    for e, o in ((eager, out), (eager_b, out_b), (eager, eager_b)):
        for a, b in ((e.eig_re, o.eig_re), (e.eig_im, o.eig_im), (e.summary, o.summary)):
            assert np.array_equal(_bits(a.cpu().numpy()), _bits(b.cpu().numpy()))
        assert torch.equal(e.iterations, o.iterations) and torch.equal(e.status, o.status)


def test_refused_calls_write_nothing(golden, blocks):
    A, B, K = golden["A"][:5], golden["B"][:5], blocks["K"][:5]
    assert _flight(A, B, K, n=0, expect_rc=_lib.FDYN_ERR_BAD_SIZE) is None
    assert _flight(A, B, K, n=-1, expect_rc=_lib.FDYN_ERR_BAD_SIZE) is None
    assert _block(blocks["closed"][:5], n=0, expect_rc=_lib.FDYN_ERR_BAD_SIZE) is None
    for drop in ("A", "re", "im", "st"):
        assert _flight(A, B, K, expect_rc=_lib.FDYN_ERR_NULL, drop=drop) is None
    for drop in ("M", "re", "im", "st"):
        assert _block(blocks["closed"][:5], expect_rc=_lib.FDYN_ERR_NULL, drop=drop) is None
    with pytest.raises(ValueError, match=r"A \[12\]\[12\]\[n\]"):
        MO.modes_into(_dev(np.zeros((12, 11, 5))), _dev(np.zeros((12, 4, 5))))
    with pytest.raises(ValueError, match="K"):
        MO.modes_into(_dev(np.zeros((12, 12, 5))), _dev(np.zeros((12, 4, 5))), _dev(np.zeros((16, 4))))
    with pytest.raises(ValueError, match=r"\[2\]\[4\]\[4\]\[n\]"):
        MO.block_modes_into(_dev(np.zeros((2, 16, 5))))


# ---- the fleet -----------------------------------------------------------------------------------------------------------------
def test_fleet_chain_against_numpy_over_the_oracle():
    """trim -> design_lqr -> modes on the device against trim -> linearise -> design -> eigvals in NumPy over the CPU oracle (the
    ten aircraft of lqr_numpy.oracle_flights), under the 1e-10 |m|_inf gate; then the sampled loop and the filter."""
    base = ln.oracle_flights()["all"]
    n = len(base["type"])
    fleet = BatchedSixDOF(n, "f64", types=tn.TYPES, type_index=base["type"])
    with pytest.raises(ValueError, match="no trim"):
        fleet.modes()
    fleet.trim(base["spec"][:, 0], base["spec"][:, 1], base["spec"][:, 2], ln.ALTITUDE, ln.HEADING)
    design = fleet.design_lqr()
    for name, m, Mref in (("open", fleet.modes(), mo.closed_blocks(base["A"], base["B"])),
                          ("closed", fleet.modes(design), mo.closed_blocks(base["A"], base["B"], base["K"]))):
        assert isinstance(m, MO.FleetModes) and bool(m.ok.all()) and m.n == n and tuple(m.eig.shape) == (2, 4, n) and m.eig.dtype == torch.complex128
        eig, worst = m.eig.permute(2, 0, 1).cpu().numpy(), 0.0
        for i in range(n):
            for b in range(2):
                worst = max(worst, mo.match_gap(eig[i, b], np.linalg.eigvals(Mref[i, b])) / mo.norm_inf(Mref[i, b]))
        print(f"{name} loop: fleet chain against NumPy over the oracle: worst eigenvalue gap {worst:.3e} |m|; abscissa "
              f"{float(m.abscissa().min()):.4f}..{float(m.abscissa().max()):.4f}, min damping {float(m.min_damping().min()):.4f}")
        assert worst <= 1e-10
        # the derived views against the same formulas in NumPy on the values read back
        re, im = eig.real.transpose(1, 2, 0), eig.imag.transpose(1, 2, 0)
        wn = np.hypot(re, im)
        assert np.allclose(m.natural_frequency().cpu().numpy(), wn, rtol=1e-14, atol=0.0)
        assert np.allclose(m.damping_ratio().cpu().numpy(), -re / wn, rtol=1e-14, atol=1e-300)
        with np.errstate(divide="ignore"):
            assert np.allclose(m.time_constant().cpu().numpy(), -1.0 / re, rtol=1e-14) and np.allclose(
                m.time_to_double().cpu().numpy(), np.where(re > 0.0, np.log(2.0) / np.where(re > 0.0, re, 1.0), np.inf), rtol=1e-14)
        assert torch.equal(m.abscissa(), m.re[:, 0])
        assert torch.allclose(m.min_damping(), m.damping_ratio().min(dim=1).values, rtol=1e-14, atol=0.0)
        assert torch.allclose(m.spectral_radius(), m.natural_frequency().max(dim=1).values, rtol=1e-14, atol=0.0)
    assert bool((fleet.modes(design).abscissa() < 0.0).all())
    A, B = fleet.linearize()
    assert _same_report(design.modes(A, B), fleet.modes(design))
    for dt in mo.DTS:
        kal = fleet.design_kalman(dt)
        poles, sampled = kal.filter_poles(), Q.sampled_poles(design, kal)
        assert bool(poles.ok.all()) and bool(sampled.ok.all())
        assert bool((poles.spectral_radius()[:, kal.ok] < 1.0).all()) and bool((sampled.spectral_radius()[:, design.ok & kal.ok] < 1.0).all())
        # Phi = exp(a dt), so ln z / dt of Phi's eigenvalues are the open-loop poles.  An error e in z becomes e / (|z| dt): with
        # eps cond(V) |Phi| about 2.2e-16 x 226 x 1.3 in z, |z| >= 0.3 and dt = 0.01 that is 2e-11; the gate leaves three orders
        back = MO.block_modes_into(kal.phi()).to_s_plane(dt).permute(2, 0, 1).cpu().numpy()
        cont = fleet.modes().eig.permute(2, 0, 1).cpu().numpy()
        gap = max(mo.match_gap(back[i, b], cont[i, b]) / max(1.0, np.abs(cont[i, b]).max()) for i in range(n) for b in range(2))
        z = sampled.eig.permute(2, 0, 1).cpu().numpy()
        assert np.allclose(sampled.to_s_plane(dt).permute(2, 0, 1).cpu().numpy(), np.log(z) / dt, rtol=1e-12, atol=1e-12)
        print(f"dt {dt}: filter radius {float(poles.spectral_radius().max()):.6f}, sampled-loop radius {float(sampled.spectral_radius().max()):.6f}, "
              f"ln z / dt of Phi against the open-loop poles {gap:.3e}")
        assert gap <= 2e-8
    with pytest.raises(ValueError, match="dt > 0"):
        poles.to_s_plane(0.0)


def _same_report(a, b):
    return all(np.array_equal(_bits(x.cpu().numpy()), _bits(y.cpu().numpy())) for x, y in
               ((a.eig_re, b.eig_re), (a.eig_im, b.eig_im), (a.summary, b.summary), (a.iterations, b.iterations), (a.status, b.status)))

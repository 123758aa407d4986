"""The hand-written MFMA kernels of a rollout step -- csrc/lstm_mfma.hip (tiled cell and its BPTT-forward form),
csrc/lstm_mfma64.hip (one wave per SIMD, single and pair), csrc/policy_trunk.hip, csrc/policy_fe64.hip -- each through its C entry
point against the float64 reference of tests/mfma_ref.py, element-wise within the bounds derived there from the operands, or,
for the multi-layer kernels with dense random weights, under the two statistical caps stated there.  The multi-layer kernels are
also probed one layer at a time: every other layer is a pass-through whose output is known.

tests/test_mfma_ref_host.py shows on the CPU that an fp32 emulation of these kernels passes the same comparisons on the same
cases and that seeded defects fail them.  Every output buffer holds a sentinel before the launch; references are cached per
case (on the CPU up to 4096 rows; larger cases compute theirs in float64 on the device and check its first 256 rows against the
CPU's).  Every test prints the largest |error| / bound it saw (pytest -s).

Largest |error| / bound on an MI355X (a reported figure, not a threshold; 1 is the bound):
                                        c'       h' fp32   h' bf16   activations
  tiled cell, small shapes              0.0016   0.0014    0.85      --
  tiled cell, 20 000 / 40 000 rows      0.0012   0.0007    0.72      --
  one wave per SIMD, single             0.0013   --        0.73      --
  one wave per SIMD, pair               0.0014   --        0.72      --
  train form                            0.0016   --        0.84      0.96
  trunks: layer-1 probes 0.93, layer-2 probes 0.96; dense: 0 elements outside the hard cap, at most 5.2e-5 of them outside the
          soft one
  features: embedding probes 0.78, layer-1 probes 0.75, layer-2 probes 0.79, projection probe 0.92; dense: 0 outside the hard
            cap, 3.1e-5 (B = 256) and 8.1e-5 (B = 768) of the elements outside the soft one
(The bf16 figures sit near 1 by construction: the bound of a stored bf16 value is its own rounding, 2^-8 |ref|, plus twice the
fp32 bound, and a rounding error does come close to 2^-8 |ref|.  The fp32 outputs use a thousandth of their bound.)
"""
import functools

import pytest
import torch

import mfma_ref as M
from mfma_ref import BF, SENT
from hcrl_amd import _lib

gpu = pytest.mark.gpu
CPU_REF_MAX = 4096


def _ids(cases):
    return ["kx%d-kh%d-H%d-B%d-%s" % c for c in cases]


@functools.lru_cache(maxsize=None)
def _small_ref(args):
    return M.ref_cell64(M.cell_case(*args))


def _reference(d, args=None):
    """(case, reference) on the device the comparison runs on: the CPU up to CPU_REF_MAX rows, else float64 on the GPU, its
    first 256 rows checked against the CPU reference."""
    if d.B <= CPU_REF_MAX:
        return d, (_small_ref(args) if args is not None else M.ref_cell64(d))
    dd = M.case_to(d, "cuda")
    r, r0 = M.ref_cell64(dd), M.ref_cell64(d, rows=slice(0, 256))
    for name in ("c", "h", "tol_c", "tol_h32"):
        a, b = getattr(r, name)[:256].cpu(), getattr(r0, name)
        assert float(((a - b).abs() / b.abs().clamp(min=1.0)).max()) < 1e-11, name
    return dd, r


def _launch_cell(d, with_h32=False, train=False, with_next=True, alias=False, pair=None):
    """One launch from the stored operands of `d` (and of `pair`, the critic's, for the paired entry) -> dict of outputs."""
    lib, st, B, H = _lib.load(), _lib.current_stream(), d.B, d.H
    outs = []
    cases = [d] if pair is None else [d, pair]
    x, keep = d.x.cuda(), (None if d.keep is None else d.keep.cuda())
    ops = []
    for q in cases:
        o = dict(W=q.W.cuda(), bias=q.bias.cuda(), h_prev=None if q.h is None else q.h.cuda(), c_prev=None if q.c is None else q.c.cuda())
        o["h"] = o["h_prev"] if alias else torch.full((B, H), SENT, dtype=BF, device="cuda")
        o["c"] = (o["c_prev"] if alias else torch.full((B, H), SENT, device="cuda")) if q.kh else None
        ops.append(o)
    o = ops[0]
    if pair is not None:
        args = [_lib.ptr(t) for p in ops for t in (p["h_prev"], p["c_prev"], p["W"], p["bias"], p["h"], p["c"])]
        rc = lib.fdyn_lstm_cell_mfma_pair(_lib.ptr(x), d.kx, _lib.ptr(keep), d.kh, B, H, *args, st)
    elif train:
        ng, K2 = (4 if d.kh else 3), d.kx + H + 8
        o["act"] = torch.full((B, ng * H), SENT, dtype=BF, device="cuda")
        o["nxt"] = torch.full((B, K2), SENT, dtype=BF, device="cuda") if with_next else None
        kn = d.keep_next.cuda() if with_next else None
        rc = lib.fdyn_lstm_cell_mfma_train(_lib.ptr(x), d.kx, _lib.ptr(o["h_prev"]), d.kh, _lib.ptr(o["c_prev"]), _lib.ptr(keep),
                                           _lib.ptr(o["W"]), _lib.ptr(o["bias"]), _lib.ptr(o["h"]), _lib.ptr(o["c"]), _lib.ptr(o["act"]),
                                           (o["nxt"].data_ptr() + 2 * d.kx) if with_next else None, K2 if with_next else 0,
                                           _lib.ptr(kn), B, H, st)
    else:
        o["h32"] = torch.full((B, H), SENT, device="cuda") if with_h32 else None
        rc = lib.fdyn_lstm_cell_mfma(_lib.ptr(x), d.kx, _lib.ptr(o["h_prev"]), d.kh, _lib.ptr(o["c_prev"]), _lib.ptr(keep), _lib.ptr(o["W"]),
                                     _lib.ptr(o["bias"]), _lib.ptr(o["h"]), _lib.ptr(o["c"]), _lib.ptr(o["h32"]), B, H, st)
    assert rc == 0, rc
    torch.cuda.synchronize()
    for p in ops:
        outs.append({k: p.get(k) for k in ("c", "h", "h32", "act", "nxt")})
    return outs if pair is not None else outs[0]


def _compare(tag, d, out, args=None):
    dd, r = _reference(d, args)
    dev = r.c.device
    got = {k: (None if v is None else v.to(dev)) for k, v in out.items() if k != "nxt"}
    if out.get("nxt") is not None:
        nxt = out["nxt"].to(dev)
        got["hn"] = nxt[:, d.kx:d.kx + d.H]
        assert bool((nxt[:, :d.kx] == SENT).all()) and bool((nxt[:, d.kx + d.H:] == SENT).all()), "written outside its columns"
    res = M.check_cell(dd, r, got)
    print("MEASURE", tag, {k: round(v, 4) for k, v in res.items()})
    assert max(res.values()) <= 1.0, res
    return res


# ---- 3.1 the tiled cell ---------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("with_h32", [True, False], ids=["h32", "noh32"])
@pytest.mark.parametrize("kx,kh,H,B,keep", M.CELL_SHAPES, ids=_ids(M.CELL_SHAPES))
def test_tiled_cell_matches_fp64_within_the_derived_bound(kx, kh, H, B, keep, with_h32):
    """fdyn_lstm_cell_mfma below 32 768 rows: all four (kx, kh), ragged and full tiles (generic and software-pipelined path, both in
    one launch at B = 777), H = 32 / 96 / 256, saturated gates (biases +-30, +-100), |c_prev| up to 50, keep masks mixed (first row
    0, last 1, a whole tile 0) / all ones / all zeros / NULL, stale 1e30 state in restarted rows."""
    args = (kx, kh, H, B, keep)
    d = M.cell_case(*args)
    _compare(f"tiled {args} h32={with_h32}", d, _launch_cell(d, with_h32), args)


@gpu
@pytest.mark.parametrize("kx,kh,H,B,keep", M.CELL_TILED_LARGE, ids=_ids(M.CELL_TILED_LARGE))
def test_tiled_cell_at_intermediate_splits(kx, kh, H, B, keep):
    """An fp32 copy of h' keeps 20 000 and 40 000 rows in the tiled kernel, which then splits a row's hidden slices over 4 and 2
    workgroups on a 256-CU device."""
    d = M.cell_case(kx, kh, H, B, keep)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    print("MEASURE split", B, M.cell_split(B, H, cus), "CUs", cus)
    _compare(f"tiled large B={B}", d, _launch_cell(d, True))


@gpu
def test_tiled_cell_cases_cover_every_split_of_this_device():
    """split in {1, 2, 4, 8} by the launcher's rule from this device's CU count.  Which values some batch size can reach at all is
    found by scanning the batch size; a reachable value the cases above do not produce is a failure, one that no batch size
    reaches on this device a skip."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    got = {M.cell_split(B, H, cus) for _, _, H, B, _ in M.CELL_SHAPES + list(M.CELL_TILED_LARGE)}
    reach = M.reachable_splits(cus)
    uncovered = {s: b for s, b in reach.items() if s not in got}
    assert not uncovered, f"with {cus} CUs these splits are reachable (split: batch) but not run: {uncovered}"
    unreachable = {1, 2, 4, 8} - set(reach)
    if unreachable:
        pytest.skip(f"with {cus} CUs no batch size gives split {sorted(unreachable)}")


# ---- 3.2 one wave per SIMD ------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("keep", M.KEEP_MODES)
def test_one_wave_per_simd_cell_matches_fp64(keep):
    """B = 32 768 without an fp32 copy of h': the one-wave-per-SIMD kernel.  The mixed mask (keep = 0 on a whole 256-row workgroup,
    a whole 64-row wave and a whole 32-row tile besides the random rows) runs with the state ALIASED, which only that kernel
    accepts; its result is compared with fp64 of the state as it was before the call."""
    d = M.w64_case(keep)
    assert _lib.load().fdyn_lstm_cell_mfma_inplace_ok(128, 256, 256, d.B) == 1
    _compare(f"w64 {keep}", d, _launch_cell(d, alias=(keep == "mixed")))


@gpu
def test_one_wave_per_simd_pair_matches_fp64_per_cell():
    """fdyn_lstm_cell_mfma_pair at 32 768 rows with distinct actor and critic operands (same x and keep), each against its own
    reference and bound."""
    d0, d1 = M.pair_cases()
    assert _lib.load().fdyn_lstm_cell_mfma_inplace_ok(128, 256, 256, d0.B) == 1       # the paired kernel serves this shape (not two tiled launches)
    outs = _launch_cell(d0, pair=d1)
    assert not torch.equal(outs[0]["h"], outs[1]["h"])
    _compare("pair actor", d0, outs[0])
    _compare("pair critic", d1, outs[1])


# ---- 3.3 the train form ---------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("with_next", [True, False], ids=["next", "nonext"])
@pytest.mark.parametrize("kx,kh,H,B,keep", M.TRAIN_SHAPES, ids=_ids(M.TRAIN_SHAPES))
def test_train_cell_matches_fp64_within_the_derived_bound(kx, kh, H, B, keep, with_next):
    """fdyn_lstm_cell_mfma_train, (128, 128) included: c', h' and the stored activations (4-gate layout, (i, g, o) for kh = 0) within
    their bounds, h_next equal to h' keep_next and nothing written outside its columns; h_next == NULL."""
    args = (kx, kh, H, B, keep)
    d = M.cell_case(*args)
    res = _compare(f"train {args} next={with_next}", d, _launch_cell(d, train=True, with_next=with_next), args)
    assert ("hn" in res) == with_next and "act" in res


# ---- 3.4 the trunks -------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _trunk_ref(B, mode):
    return M.ref_trunk64(M.trunk_case(B, mode))


@gpu
@pytest.mark.parametrize("mode", M.TRUNK_MODES)
@pytest.mark.parametrize("B", [1, 33, 300])
def test_policy_trunks_layer_by_layer_and_dense(B, mode):
    """fdyn_policy_trunks.  l1a / l1b: layer 2 is a 0/1 selection (b2 = 0), so lat[j] = relu(mid[sel(j)]) and layer 1 is checked
    element-wise against its derived bound; l2a / l2b: layer 1 selects columns of h (b1 = 0), mid is exact and layer 2 is checked
    element-wise; dense: both random, fp64 with the same rounding point under the statistical caps."""
    d, lib = M.trunk_case(B, mode), _lib.load()
    dev = [t.cuda().contiguous() for t in (d.h[0], d.h[1], d.W1, d.b1, M.pack_w2p(d.W2), d.b2)]
    lat = [torch.full((B, 64), SENT, dtype=BF, device="cuda") for _ in range(2)]
    assert lib.fdyn_policy_trunks(*(t.data_ptr() for t in dev), lat[0].data_ptr(), lat[1].data_ptr(), B, _lib.current_stream()) == 0
    torch.cuda.synchronize()
    res = M.check_trunk(d, _trunk_ref(B, mode), [t.cpu() for t in lat])
    print("MEASURE trunk", B, mode, res)
    for t, v in res.items():
        if mode == "dense":
            assert v[0] == 0 and v[1] <= M.CAP_FRAC, (t, v)
        else:
            assert v <= 1.0, (t, v)


# ---- 3.5 the features -----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _fe_ref(B, mode):
    d = M.fe_case(B, mode)
    r = M.ref_fe64(d)
    return (r.feats, None) if mode == "dense" else M.fe_probe_ref(d, r)


@gpu
@pytest.mark.parametrize("mode", M.FE_MODES)
@pytest.mark.parametrize("B", [256, 768])
def test_policy_features_layer_by_layer_and_dense(B, mode):
    """fdyn_policy_features on the snapshot prepare_inference() builds from the model's weights.  Probe modes (mfma_ref.fe_case):
    one layer dense random, every other layer a pass-through whose output is known -- the embedding, each LSTM layer (two
    selections x two signs behind the projection's ReLU cover all 256 units) and the projection, element-wise against the derived
    bound carried through the pass-throughs behind the layer.  dense: all four layers random, fp64 with the same rounding points
    under the statistical caps."""
    from hcrl_amd.policy import RateLSTMPolicy
    d, lib = M.fe_case(B, mode), _lib.load()
    p = RateLSTMPolicy(compute_dtype=BF)
    fe = p.features_extractor
    with torch.no_grad():
        fe.embedding[0].weight.copy_(d.w_emb); fe.embedding[0].bias.copy_(d.b_emb)
        fe.lstm.weight_ih_l0.copy_(d.w1); fe.lstm.bias_ih_l0.copy_(d.b1); fe.lstm.bias_hh_l0.zero_()
        fe.lstm.weight_ih_l1.copy_(d.w2); fe.lstm.bias_ih_l1.copy_(d.b2); fe.lstm.bias_hh_l1.zero_()
        fe.output_proj[0].weight.copy_(d.w_p); fe.output_proj[0].bias.copy_(d.b_p)
    p = p.cuda()
    p.prepare_inference()
    inf = p._inf
    img, bias = M.fe_pack(d)
    assert torch.equal(inf.fe_img.cpu().view(torch.int16), img.view(torch.int16)) and torch.equal(inf.fe_bias.cpu(), bias)
    obs = d.obs.cuda().contiguous()
    feats = torch.full((B, 128), SENT, dtype=BF, device="cuda")
    _lib.check(lib.fdyn_policy_features(obs.data_ptr(), inf.fe_img.data_ptr(), inf.fe_bias.data_ptr(), feats.data_ptr(), B,
                                        _lib.current_stream()), "policy_features")
    torch.cuda.synchronize()
    ref, tol = _fe_ref(B, mode)
    if mode == "dense":
        hard, soft = M.caps(feats.cpu(), ref)
        print("MEASURE fe dense", B, hard, f"{soft:.2e}")
        assert hard == 0 and soft <= M.CAP_FRAC, (hard, soft)
    else:
        v = M.ratio(feats.cpu(), ref, tol)
        print("MEASURE fe probe", B, mode, round(v, 4))
        assert v <= 1.0, v

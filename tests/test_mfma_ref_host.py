"""tests/mfma_ref.py checked on the CPU: the fp32 emulation of the MFMA policy kernels passes every comparison that
tests/test_gpu_mfma_kernels.py applies to the kernels, on the same cached cases, and seeded defects fail them.  So the bounds
and the statistical caps are known to hold for a correct fp32 implementation, and to bite, before anything runs on a GPU.

One listed defect cannot fail and is pinned as such: a log2 e truncated to 1.4427 changes an exponent by 3.4e-6 of its size,
a sigmoid by at most 3.4e-6 sup |x sigmoid'(x)| = 7.6e-7, c' by that times (|keep c_prev| + 2) -- below the allowance
A max(1, |c'|), A = 2e-5, whatever the data (test_truncated_log2e_stays_below_the_activation_allowance).
"""
import pytest
import torch

import mfma_ref as M
from mfma_ref import F64


def _print(*a):
    print("MEASURE", *a)


# ---- the module's own footing --------------------------------------------------------------------------------------------

def test_kernel_side_constants_match_the_host_packing():
    from hcrl_amd import policy
    assert tuple(policy._KPERM16) == M.KORDER16
    assert tuple(policy.FE_GATE_SCALE) == M.GATE_SCALE


def test_fp64_cell_reference_equals_nn_lstm_cell():
    d = M.cell_case(128, 128, 128, 33, "ones")
    cell = torch.nn.LSTMCell(128, 128).to(F64)
    with torch.no_grad():
        cell.weight_ih.copy_(d.W[:, :128].to(F64)); cell.weight_hh.copy_(d.W[:, 128:].to(F64))
        cell.bias_ih.copy_(d.bias.to(F64)); cell.bias_hh.zero_()
        h, c = cell(d.x.to(F64), (d.h.to(F64), d.c.to(F64)))
    r = M.ref_cell64(d)
    assert float((r.h - h).abs().max()) < 1e-12 and float(((r.c - c).abs() / c.abs().clamp(min=1)).max()) < 1e-12


def test_activation_forms_alone_are_far_inside_the_allowance():
    """The exp2 / rcp forms in float32 against fp64: the figures quoted in mfma_ref's header."""
    s, t, tc = M.measure_activation_forms()
    _print(f"activation forms alone: sigmoid {s:.2e} tanh {t:.2e} tanh(c) {tc:.2e}  A = {M.A_ACT:.0e}")
    # twice the figures measured here (8.9e-8, 1.8e-7, 1.8e-7), and with them far inside A
    assert s <= 2 * 8.9e-8 and t <= 2 * 1.8e-7 and tc <= 2 * 1.8e-7 and 2 * 1.8e-7 < M.A_ACT


def test_truncated_log2e_stays_below_the_activation_allowance():
    """Not detectable at A = 2e-5 by any data: the emulation with log2 e = 1.4427 stays inside every bound, and moves c' of a
    case with |c_prev| up to 50 by less than A max(1, |c'|)."""
    d = M.cell_case(128, 256, 256, 777)
    r = M.ref_cell64(d)
    good, bad = M.emu_cell(d), M.emu_cell(d, "log2e")
    assert max(M.check_cell(d, r, bad).values()) <= 1.0
    move = (bad["c"].double() - good["c"].double()).abs() / r.c.abs().clamp(min=1.0)
    _print(f"log2e truncated: c' moves by {float(move.max()):.2e} max(1, |c'|)")
    assert 0.0 < float(move.max()) < M.A_ACT


# ---- the cells ---------------------------------------------------------------------------------------------------------------

def _ids(cases):
    return ["kx%d-kh%d-H%d-B%d-%s" % c for c in cases]


@pytest.mark.parametrize("kx,kh,H,B,keep", M.CELL_SHAPES + M.TRAIN_SHAPES, ids=_ids(M.CELL_SHAPES + M.TRAIN_SHAPES))
def test_emulated_cell_is_inside_every_bound(kx, kh, H, B, keep):
    d = M.cell_case(kx, kh, H, B, keep)
    res = M.check_cell(d, M.ref_cell64(d), M.emu_cell(d))
    _print("emu cell", kx, kh, H, B, keep, {k: round(v, 4) for k, v in res.items()})
    assert max(res.values()) <= 1.0, res


@pytest.mark.parametrize("which", ["tiled-20000", "tiled-40000", "w64-mixed", "w64-ones", "w64-zeros", "w64-null", "pair-0", "pair-1"])
def test_emulated_cell_is_inside_every_bound_large(which):
    """The large cases of the device tests, on a spot sample of rows."""
    kind, arg = which.split("-")
    d = (M.cell_case(128, 256, 256, int(arg), "mixed") if kind == "tiled" else
         M.w64_case(arg) if kind == "w64" else M.pair_cases()[int(arg)])
    d = M.case_rows(d, M.spot_rows(d.B))
    res = M.check_cell(d, M.ref_cell64(d), M.emu_cell(d))
    assert max(res.values()) <= 1.0, res


def test_cell_cases_hold_the_edges_they_are_meant_to():
    d = M.w64_case("mixed")
    assert float(d.keep[512:768].sum()) == 0 and float(d.keep[1088:1152].sum()) == 0 and d.keep[0] == 0 and d.keep[-1] == 1
    live = d.keep != 0
    assert float(d.c[live].abs().max()) > 40 and float(d.c[live].abs().max()) <= 50 and float(d.c[~live].abs().min()) > 0.9 * M.BIG
    assert sorted({abs(v) for _, _, v in M.SAT_BIASES}) == [30.0, 100.0]
    d = M.cell_case(128, 256, 256, 777)
    assert float(d.keep[32:64].sum()) == 0 and bool(torch.isfinite(M.ref_cell64(d).h).all())


# (defect, case, outputs at least one of which must leave its bound)
_CELL_DEFECT_CASES = [
    ("bias_bf16", (128, 256, 256, 777, "mixed"), ("c", "h32", "act")),
    ("bias_bf16", (256, 0, 256, 33, "mixed"), ("h32", "act")),
    ("drop_last_k", (128, 256, 256, 777, "mixed"), ("c",)),
    ("drop_last_k", (128, 128, 96, 160, "mixed"), ("c",)),
    ("drop_last_k", (128, 0, 256, 31, "mixed"), ("h",)),
    ("swap_rows", (128, 256, 256, 33, "mixed"), ("c",)),
    ("swap_rows", (256, 0, 32, 160, "mixed"), ("h",)),
    ("keep_last_row", (128, 256, 256, 33, "zeros"), ("c",)),
    ("keep_last_row", (128, 128, 256, 33, "zeros"), ("h",)),
    ("c_prev_bf16", (128, 256, 256, 128, "ones"), ("c",)),
    ("c_prev_bf16", (128, 128, 256, 1, "mixed"), ("c",)),         # B = 1: the one row is kept (last row 1)
]


@pytest.mark.parametrize("defect,case,outputs", _CELL_DEFECT_CASES, ids=[f"{d}-{'-'.join(map(str, c))}" for d, c, _ in _CELL_DEFECT_CASES])
def test_seeded_cell_defect_fails_its_comparison(defect, case, outputs):
    d = M.cell_case(*case)
    r = M.ref_cell64(d)
    res = M.check_cell(d, r, M.emu_cell(d, defect))
    _print("defect", defect, case, {k: round(v, 3) for k, v in res.items()})
    assert all(res[o] > 1.0 for o in outputs), res


def test_seeded_cell_defects_fail_the_train_outputs():
    """The stored activations and the packed next-step rows see the defects too."""
    d = M.cell_case(128, 256, 96, 33)
    r = M.ref_cell64(d)
    for defect in ("bias_bf16", "drop_last_k", "swap_rows"):
        assert M.check_cell(d, r, M.emu_cell(d, defect))["act"] > 1.0, defect
    out = M.emu_cell(d)
    out["hn"] = out["h"].clone()                                # keep_next ignored
    assert M.check_cell(d, r, out)["hn"] == float("inf")


def test_split_rule_covers_every_split_at_256_cus():
    assert set(M.reachable_splits(256)) == {1, 2, 4, 8} and set(M.reachable_splits(2)) == {1, 2, 4}
    got = {M.cell_split(B, H, 256) for _, _, H, B, _ in M.CELL_SHAPES + list(M.CELL_TILED_LARGE)}
    assert got == {1, 2, 4, 8}, got
    assert M.cell_split(20000, 256, 256) == 4 and M.cell_split(40000, 256, 256) == 2 and M.cell_split(160, 96, 256) == 1


# ---- the trunks -------------------------------------------------------------------------------------------------------------

TRUNK_B = (1, 33, 300)


@pytest.mark.parametrize("mode", M.TRUNK_MODES)
@pytest.mark.parametrize("B", TRUNK_B)
def test_emulated_trunks_are_inside_every_bound(B, mode):
    d = M.trunk_case(B, mode)
    res = M.check_trunk(d, M.ref_trunk64(d), M.emu_trunk(d, M.pack_w2p(d.W2)))
    _print("emu trunk", B, mode, res)
    for t, v in res.items():
        if mode == "dense":
            # the reference-alone figures of the caps: measured 0 and 0 in every case; one element is the figure's resolution
            assert v[0] == 0 and v[1] * B * 64 <= 1 and v[1] <= M.CAP_FRAC, (t, v)
        else:
            assert v <= 1.0, (t, v)


def _trunk_fails(d, lats):
    res = M.check_trunk(d, M.ref_trunk64(d), lats)
    if d.mode == "dense":
        return all(not (v[0] == 0 and v[1] <= M.CAP_FRAC) for v in res.values())
    return all(v > 1.0 for v in res.values())


@pytest.mark.parametrize("B", [33, 300])
def test_seeded_trunk_defects_fail(B):
    for mode, defect in (("dense", "no_kperm"), ("l2a", "no_kperm"), ("l2b", "no_kperm"), ("l1a", "bias_bf16"), ("l2b", "bias_bf16"),
                         ("l1a", "drop_last_k"), ("l1b", "drop_last_k"), ("dense", "drop_last_k")):
        d = M.trunk_case(B, mode)
        W2p = d.W2.clone() if defect == "no_kperm" else M.pack_w2p(d.W2)
        assert _trunk_fails(d, M.emu_trunk(d, W2p, None if defect == "no_kperm" else defect)), (mode, defect)


def test_one_bf16_step_in_the_trunk_intermediate_is_caught_by_the_layer1_probe():
    """One element of layer 1's output off by one bf16 step: found by the layer-1 probe (element-wise, derived bound)."""
    d = M.trunk_case(300, "l1a")
    refs, W2p = M.ref_trunk64(d), M.pack_w2p(d.W2)
    ref, tol = refs[0]
    mid = M.emu_trunk(d, W2p)[0].float()                        # = layer 1's output at the selected units
    up = M.bf16_step(mid, True)
    score = torch.where(mid > 0, (up.double() - ref).abs() / tol, torch.zeros_like(tol))
    row, j = divmod(int(score.argmax()), 64)
    lats = M.emu_trunk(d, W2p, "mid_step", (row, int(d.sel[j]), True))
    res = M.check_trunk(d, refs, lats)
    _print("trunk mid_step", (row, j), res)
    assert res[0] > 1.0 and int((lats[0].float() != mid).sum()) == 1


# ---- the features extractor ----------------------------------------------------------------------------------------------

FE_B = (256, 768)
FE_SOFT_MEASURED = 1.22e-4             # largest fraction the emulation alone leaves outside the soft cap (B = 768; 0 at 256 and 512)


def test_saturated_pass_through_value_is_away_from_a_rounding_boundary():
    t, margin = M.sat_value_and_margin()
    assert t == 0.76171875 and margin >= 1e-4


@pytest.mark.parametrize("mode", M.FE_PROBES)
@pytest.mark.parametrize("B", FE_B)
def test_emulated_features_probe_is_inside_its_bound(B, mode):
    d = M.fe_case(B, mode)
    r = M.ref_fe64(d)
    out = M.emu_fe64(d, *M.fe_pack(d))
    # what stands in front of the layer under test is known exactly: the emulation and the reference agree bit for bit there
    t, _ = M.sat_value_and_margin()
    if d.under in ("l1", "l2", "pr"):
        assert torch.equal(out["a1"].double(), r.a1)
    if d.under in ("l2", "pr"):
        assert torch.equal(out["h1"].double(), r.h1) and set(r.h1.unique().tolist()) == {-t, 0.0, t}
    if d.under == "pr":
        assert torch.equal(out["h2"].double(), r.h2) and set(r.h2.unique().tolist()) == {-t, 0.0, t}
    ref, tol = M.fe_probe_ref(d, r)
    v = M.ratio(out["feats"], ref, tol)
    _print("emu fe probe", B, mode, round(v, 4), "nonzero outputs", float((ref > 0).double().mean()))
    assert v <= 1.0 and float((ref > 0).double().mean()) > 0.2


@pytest.mark.parametrize("B", FE_B + (512,))
def test_emulated_dense_features_are_inside_the_caps(B):
    """Reference-alone figures of the caps: what the fp32 emulation leaves outside them, for the cases the device runs
    (B = 256: 0 and 0, B = 768: 0 and 1.2e-4) and at B = 512 (0 and 0)."""
    d = M.fe_case(B)
    hard, soft = M.caps(M.emu_fe64(d, *M.fe_pack(d))["feats"], M.ref_fe64(d).feats)
    _print("emu fe dense", B, hard, f"{soft:.2e}")
    assert hard == 0 and soft <= 2 * FE_SOFT_MEASURED < M.CAP_FRAC


@pytest.mark.parametrize("gate", [0, 2, 3])
def test_missing_gate_scale_factor_fails_the_dense_and_the_probe_test(gate):
    scale = list(M.GATE_SCALE)
    scale[gate] = 1.0
    d = M.fe_case(256)
    assert not M.caps_ok(M.emu_fe64(d, *M.fe_pack(d, scale))["feats"], M.ref_fe64(d).feats)
    for mode in ("l1a+", "l2b-"):
        d = M.fe_case(256, mode)
        assert M.ratio(M.emu_fe64(d, *M.fe_pack(d, scale))["feats"], *M.fe_probe_ref(d)) > 1.0


@pytest.mark.parametrize("layer,mode", [(1, "l1a+"), (1, "l1b-"), (2, "l2a-"), (2, "l2b+")])
def test_one_bf16_step_inside_fe64_escapes_the_dense_test_and_is_caught_by_the_probe(layer, mode):
    """One element of h1 / h2 off by one bf16 step.  Against random weights the statistical caps cannot see it (one wrong
    element reaches an output scaled by one weight); the probe of that layer does."""
    B = 256
    d = M.fe_case(B, mode)
    img, bias = M.fe_pack(d)
    ref, tol = M.fe_probe_ref(d)
    # every element stepped at once shows where one step is most visible; then that ONE element is stepped
    allup = M.emu_fe64(d, img, bias, (layer, slice(None), slice(None), True))["feats"]
    score = torch.where(ref > 0, (allup.double() - ref).abs() / tol, torch.zeros_like(tol))
    row, j = divmod(int(score.argmax()), 128)
    unit = int(d.sel[j]) if layer == 2 else int(M.SRC2[d.sel[j]])
    clean = M.emu_fe64(d, img, bias)["feats"]
    one = M.emu_fe64(d, img, bias, (layer, row, unit, True))["feats"]
    v = M.ratio(one, ref, tol)
    _print("fe step", layer, mode, (row, unit), round(v, 3))
    assert v > 1.0 and M.ratio(clean, ref, tol) <= 1.0 and 1 <= int((one != clean).sum()) <= 2
    dd = M.fe_case(B)
    base = M.emu_fe64(dd, *M.fe_pack(dd))
    unit = int(base[f"h{layer}"][row].abs().argmax())                           # the largest element of the row: the largest step
    dense = M.emu_fe64(dd, *M.fe_pack(dd), (layer, row, unit, True))["feats"]
    assert M.caps_ok(dense, M.ref_fe64(dd).feats)
    assert not torch.equal(dense, base["feats"])                                # the step did reach the output

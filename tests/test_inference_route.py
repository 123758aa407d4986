"""Host side of the fused rollout step (hcrl_amd/inference.py): the weight snapshot, its in-place refresh, the route table and
the policies the kernels do not serve.  No GPU: the library is loaded only for its two host-only entry points."""
import copy

import pytest
import torch

from hcrl_amd import _lib, inference
from hcrl_amd.inference import Knobs, Route
from hcrl_amd.policy import RateLSTMPolicy, _mlp

BF, F32 = torch.bfloat16, torch.float32
KNOB_VARS = ("FDYN_NO_MFMA", "FDYN_NO_FE64", "FDYN_NO_CELL_PAIR", "FDYN_NO_TRUNK", "FDYN_NO_TRUNK_HEADS", "FDYN_INPLACE_STATE")


def _policy(**kw):
    torch.manual_seed(0)
    p = RateLSTMPolicy(compute_dtype=BF, **kw)
    p.prepare_inference()
    return p


def _tensors(x):
    if isinstance(x, torch.Tensor):
        return [x]
    return [] if x is None else [t for y in x for t in _tensors(y)]


def _all_tensors(snap):
    return [t for f in inference.fields(snap) for t in _tensors(getattr(snap, f.name))]


def test_snapshot_of_the_reference_shape_has_every_part():
    s = _policy()._inf
    assert isinstance(s, inference.Snapshot)
    assert s.fe_img.dtype == BF and s.fe_img.numel() * 2 == _lib.load().fdyn_policy_features_image_bytes() == 702464
    assert s.fe_bias.dtype == F32 and s.fe_bias.numel() == 2304
    assert [(w.shape, w.dtype) for w in s.fe_w] == [((1024, 128), BF), ((1024, 256), BF)]
    assert [(b.shape, b.dtype) for b in s.fe_b] == [((1024,), F32)] * 2
    for w, b in ((s.pi_w, s.pi_b), (s.vf_w, s.vf_b)):
        assert (w.shape, w.dtype, b.shape, b.dtype) == ((1024, 384), BF, (1024,), F32)
    layers = {"emb": [(128, 18)], "proj": [(128, 256)], "pi": [(128, 256), (64, 128)], "vf": [(128, 256), (64, 128)],
              "act": [(4, 64)], "val": [(1, 64)]}
    for name, shapes in layers.items():
        got = getattr(s, name)
        got = [got] if isinstance(got, tuple) else got
        assert [(w.shape, w.dtype, b.shape, b.dtype) for w, b in got] == [(sh, BF, (sh[0],), BF) for sh in shapes], name
    assert (s.trunk_w1.shape, s.trunk_w1.dtype, s.trunk_b1.shape, s.trunk_b1.dtype) == ((2, 128, 256), BF, (2, 128), F32)
    assert (s.trunk_w2p.shape, s.trunk_w2p.dtype, s.trunk_b2.shape, s.trunk_b2.dtype) == ((2, 64, 128), BF, (2, 64), F32)
    assert all(t.is_contiguous() for t in _all_tensors(s))


def test_snapshot_is_no_part_of_the_module():
    p = _policy()
    fresh = RateLSTMPolicy(compute_dtype=BF)
    assert p.state_dict().keys() == fresh.state_dict().keys()
    assert not any(m is p._inf for m in p.modules()) and len(list(p.buffers())) == len(list(fresh.buffers()))


def test_refresh_is_in_place_and_equals_a_fresh_build():
    p = _policy()
    before = [t.data_ptr() for t in _all_tensors(p._inf)]
    with torch.no_grad():
        for prm in p.parameters():
            prm.add_(0.05 * torch.randn_like(prm))
    p.prepare_inference()
    assert [t.data_ptr() for t in _all_tensors(p._inf)] == before
    q = copy.deepcopy(p)
    q._inf = None
    q.prepare_inference()
    mine, fresh = _all_tensors(p._inf), _all_tensors(q._inf)
    assert len(mine) == len(fresh) == 30       # 4 LSTM-layer + 4 cell + 16 Linear + 2 image + 4 trunk tensors
    assert all(a.data_ptr() != b.data_ptr() and torch.equal(a, b) for a, b in zip(mine, fresh))


def test_refresh_refuses_a_replaced_layer():
    p = _policy()
    p.action_net = torch.nn.Linear(64, 6)                  # another width: the heads kernels no longer serve the policy
    with pytest.raises(ValueError):
        p.prepare_inference()
    p = _policy()
    kept = p._inf.pi[0][0].clone()
    p.pi_net = _mlp([256, 96, 64])                         # still served (GEMM trunks), but not the layout of the snapshot
    with pytest.raises(ValueError):
        p.prepare_inference()
    assert torch.equal(p._inf.pi[0][0], kept)              # nothing was broadcast into the old tensors
    other = copy.deepcopy(p._inf)
    other.fe_bias = other.fe_bias.double()                 # same shape, another dtype
    with pytest.raises(ValueError):
        p._inf.refresh(other)


# what today's conditions give, written out: features by the flags handed in at a batch the one-kernel features extractor serves
# (B % 256 == 0 and B >= 32768; every other batch runs layer by layer), then cells and heads, per knob set
FE64 = {None: "policy_features", torch.uint8: "policy_features_flags", torch.bool: "policy_features"}
LAYERWISE = {None: "layerwise", torch.uint8: "layerwise", torch.bool: "layerwise"}
EXPECTED = {
    (): (FE64, "lstm_cell_mfma_pair", "policy_trunks_heads"),
    ("FDYN_NO_MFMA",): (FE64, "lstm_cell_mfma_pair", "policy_trunks_heads"),            # decides _fused_ok, not the route
    ("FDYN_INPLACE_STATE",): (FE64, "lstm_cell_mfma_pair", "policy_trunks_heads"),      # decides recurrent_inplace_ok
    ("FDYN_NO_FE64",): (LAYERWISE, "lstm_cell_mfma_pair", "policy_trunks_heads"),
    ("FDYN_NO_CELL_PAIR",): (FE64, "lstm_cell_mfma", "policy_trunks_heads"),
    ("FDYN_NO_TRUNK",): (FE64, "lstm_cell_mfma_pair", "gemm+policy_heads"),
    ("FDYN_NO_TRUNK_HEADS",): (FE64, "lstm_cell_mfma_pair", "policy_trunks+policy_heads"),
    ("FDYN_NO_TRUNK", "FDYN_NO_TRUNK_HEADS"): (FE64, "lstm_cell_mfma_pair", "gemm+policy_heads"),
    KNOB_VARS[1:5]: (LAYERWISE, "lstm_cell_mfma", "gemm+policy_heads"),
}
FE64_BATCH = {300: False, 512: False, 32768: True, 32768 + 64: False, 65536: True}


@pytest.mark.parametrize("on", list(EXPECTED), ids=lambda on: "+".join(on) or "default")
def test_route_table(on, monkeypatch):
    snap = _policy()._inf
    for name in KNOB_VARS:
        monkeypatch.delenv(name, raising=False)
    for name in on:
        monkeypatch.setenv(name, "0" if name == "FDYN_INPLACE_STATE" else "1")
    k = inference.knobs()
    assert [inference.knob(name) for name in KNOB_VARS] == [name in on for name in KNOB_VARS]
    assert k == Knobs(*(name in on for name in KNOB_VARS[1:5]))
    features, cells, heads = EXPECTED[on]
    for B, fe64 in FE64_BATCH.items():
        for flags in (None, torch.uint8, torch.bool):
            got = inference.route(snap, B, flags == torch.uint8, k)
            assert got == Route((features if fe64 else LAYERWISE)[flags], cells, heads), (B, flags)


def test_route_without_the_optional_parts():
    """A policy the cells and heads serve, whose features extractor and trunks do not have the reference's shape."""
    s = _policy(lstm_hidden_size=128, net_arch_pi=(96, 64))._inf
    assert s is not None and s.fe_img is None and s.fe_bias is None and s.trunk_w1 is None and s.trunk_b2 is None
    for B in FE64_BATCH:
        assert inference.route(s, B, True, Knobs()) == Route("layerwise", "lstm_cell_mfma_pair", "gemm+policy_heads")


def test_inplace_state_follows_the_library_and_the_knobs(monkeypatch):
    for name in KNOB_VARS:
        monkeypatch.delenv(name, raising=False)
    lib, p = _lib.load(), _policy()
    for B, want in zip(FE64_BATCH, (False, False, True, False, True)):
        assert inference.inplace_ok(B) == bool(lib.fdyn_lstm_cell_mfma_inplace_ok(128, 256, 256, B)) == want
        assert not p.recurrent_inplace_ok(B, "cpu")
    monkeypatch.setenv("FDYN_INPLACE_STATE", "1")
    assert inference.inplace_ok(65536)
    monkeypatch.setenv("FDYN_INPLACE_STATE", "0")
    assert not inference.inplace_ok(65536)
    monkeypatch.delenv("FDYN_INPLACE_STATE")
    monkeypatch.setenv("FDYN_NO_MFMA", "1")
    assert not inference.inplace_ok(65536)


@pytest.mark.parametrize("kw", [dict(policy_lstm_hidden=128), dict(net_arch_pi=(128, 32)), dict(use_lstm=False)], ids=str)
def test_policies_the_kernels_do_not_serve_keep_the_plain_path(kw):
    p = _policy(**kw)
    assert p._inf is None and not inference.served(p)
    assert not p._fused_ok(torch.zeros(4, 18)) and not p.recurrent_inplace_ok(65536, "cuda")
    with torch.no_grad():
        a, v, lp, _ = p.step(torch.zeros(4, 18), p.initial_state(4), torch.zeros(4), deterministic=True)
    assert a.shape == (4, 4) and v.shape == (4,) and lp.shape == (4,)
    with torch.no_grad():
        assert not _policy()._fused_ok(torch.zeros(4, 18))          # a served policy, a CPU tensor

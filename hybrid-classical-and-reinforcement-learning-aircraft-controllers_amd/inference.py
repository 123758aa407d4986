"""Fused rollout step of `RateLSTMPolicy`: everything between "weights changed" and "actions, value, log-prob, new state".

  Snapshot    the weights as the kernels read them (bf16 matrices, fp32 biases, the packed images of csrc/policy_fe64.hip and
              csrc/policy_trunk.hip), built by `snapshot()` -- which is also where it is decided, once, whether the kernels can
              serve the policy at all -- and refreshed in place (a captured rollout graph holds the pointers);
  knob()      the six environment switches, read at call time; knobs() the four of them that choose between entry points;
  route()     which entry points a step launches, from the snapshot, the batch and the knobs: host logic only;
  step()      the route looked up, then three launch stages: features -> the two recurrent cells -> trunks, heads and sampling.

Weight-side shapes and dtypes are checked when the snapshot is built or refreshed; the operands of a call (observations, states,
masks, flag buffers) before every launch, because the kernels trust their sizes.  policy.py keeps the network, the plain and
the training paths, and thin methods that delegate here.
"""
import os
from dataclasses import dataclass, fields
from typing import List, NamedTuple, Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from .fused import episode_flags
from .layout import FD_ACT_DIM as ACT_DIM, FD_OBS_DIM as OBS_DIM

HIDDEN, FEATURES = 256, 128        # the recurrent cells the MFMA kernels serve: [128 | 256] -> 4 x 256 (include/fdyn.h)
LATENT = 64                        # trunk output width fdyn_policy_heads / fdyn_policy_trunks_heads read
FE64_MIN_BATCH = 128 * 256         # csrc/policy_fe64.hip takes whole 256-row workgroups; smaller batches run layer by layer

# k order inside every block of 16 of a layer whose input arrives as the previous layer's MFMA output tile (csrc/policy_fe64.hip)
_KPERM16 = (0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15)
_KPERM_CACHE = {}


def _kperm(K, device):
    """Column order of a K-wide weight matrix whose input arrives as MFMA output fragments; one device tensor per (K, device),
    built once (prepare_inference runs before every rollout: a torch.tensor(list, device=cuda) there is a synchronous H2D copy)."""
    key = (int(K), str(device))
    if key not in _KPERM_CACHE:
        _KPERM_CACHE[key] = torch.tensor([16 * (k // 16) + _KPERM16[k % 16] for k in range(K)], device=device)
    return _KPERM_CACHE[key]


FE_GATE_SCALE = (-1.4426950408889634, 1.0, -2.0 * 1.4426950408889634, -1.4426950408889634)     # gates i, f (unused), g, o


def pack_fe_weights(w_emb, w1, w2, w_proj):
    """The features extractor's four weight matrices as the byte image csrc/policy_fe64.hip streams through LDS.

    Chunks in the order the kernel uses them -- embedding [128 rows, K 18 -> 32]; per 32-unit slice of LSTM layer 1 and 2 the
    rows of gates (i, g) [64 rows] then of gate o [32 rows] (gate f multiplies the zero cell state and is not needed); per
    32-feature slice of the projection [32 rows] -- each row K bf16 followed by 16 bytes of padding, each chunk padded to a
    multiple of 1 KB.  Layers 1, 2 and the projection read their input straight out of the previous layer's MFMA output
    registers, which fixes the order of k inside every block of 16 (_KPERM16)."""
    bf = torch.bfloat16
    H = w1.shape[0] // 4

    def perm(K):
        return _kperm(K, w1.device)

    def chunk(rows):                      # rows [R, K] -> bytes of the padded LDS image, a whole number of 1 KB pieces
        R = rows.shape[0]
        img = torch.cat([rows.to(bf), torch.zeros(R, 8, dtype=bf, device=rows.device)], 1).reshape(-1)
        pad = (-img.numel()) % 512
        return torch.cat([img, torch.zeros(pad, dtype=bf, device=rows.device)])

    parts = [chunk(F.pad(w_emb.detach().float(), (0, 32 - w_emb.shape[1])))]
    # rows of the LSTM layers pre-scaled (in fp32, before the one rounding to bf16) by the factor their gate's exponent takes:
    # sigmoid(z) = 1 / (1 + 2^(-z log2 e)) for i and o, tanh(z) = (1 - 2^(-2 z log2 e)) / (1 + ...) for g -- the kernel's
    # accumulators (which start from the equally scaled biases) then ARE the exponents: FE_GATE_SCALE
    gate_scale = torch.tensor(FE_GATE_SCALE, dtype=torch.float32, device=w1.device).repeat_interleave(H)[:, None]
    for w in (w1, w2):
        wp = (w.detach().float() * gate_scale)[:, perm(w.shape[1])]
        for s in range(H // 32):
            parts.append(chunk(torch.cat([wp[32 * s:32 * s + 32], wp[2 * H + 32 * s:2 * H + 32 * s + 32]], 0)))
            parts.append(chunk(wp[3 * H + 32 * s:3 * H + 32 * s + 32]))
    wq = w_proj.detach().float()[:, perm(w_proj.shape[1])]
    for s in range(w_proj.shape[0] // 32):
        parts.append(chunk(wq[32 * s:32 * s + 32]))
    return torch.cat(parts).contiguous()


# ---- the weight snapshot ---------------------------------------------------------------------------------------------------
Layer = Tuple[torch.Tensor, torch.Tensor]          # (weight bf16 [out, in], bias bf16 [out]) of a Linear that a ReLU follows


@dataclass
class Snapshot:
    fe_w: List[torch.Tensor]          # zero-state LSTM layers of the features extractor: W_ih bf16 [4H, in]
    fe_b: List[torch.Tensor]          #   b_ih + b_hh fp32 [4H]
    pi_w: torch.Tensor                # actor cell: [W_ih | W_hh] bf16 [1024, 128 + 256]
    pi_b: torch.Tensor                #   b_ih + b_hh fp32 [1024]
    vf_w: torch.Tensor                # critic cell, the same
    vf_b: torch.Tensor
    # the small Linear layers, pre-cast once per rollout: under autocast every call re-casts weight and bias
    # (17 tiny cast launches = 75 us of a 65 536-env policy step, rocprofv3)
    emb: List[Layer]
    proj: List[Layer]
    pi: List[Layer]
    vf: List[Layer]
    act: Layer                        # action_net [4, 64]
    val: Layer                        # value_net [1, 64]
    # the whole features extractor as one kernel (csrc/policy_fe64.hip): None unless it has the reference's shape
    fe_img: Optional[torch.Tensor] = None         # pack_fe_weights
    fe_bias: Optional[torch.Tensor] = None        # fp32 [128 + 1024 + 1024 + 128]
    # the two trunks as one kernel (csrc/policy_trunk.hip): None unless both are [256 -> 128 -> 64]
    trunk_w1: Optional[torch.Tensor] = None       # bf16 [2, 128, 256] (actor, critic)
    trunk_b1: Optional[torch.Tensor] = None       # fp32 [2, 128]
    trunk_w2p: Optional[torch.Tensor] = None      # bf16 [2, 64, 128], columns in _kperm order
    trunk_b2: Optional[torch.Tensor] = None       # fp32 [2, 64]

    def check(self):
        """What the kernels trust about the weights, asserted where they are made instead of before every launch."""
        bf, f32 = torch.bfloat16, torch.float32

        def cell(w, b, k_in):
            return (w.is_contiguous() and w.dtype == bf and b.dtype == f32 and b.numel() == w.shape[0] and w.shape[0] % 128 == 0
                    and (k_in is None or w.shape == (4 * HIDDEN, k_in)))
        assert all(cell(w, b, None) for w, b in zip(self.fe_w, self.fe_b)), "lstm_cell_mfma operand shapes"
        assert cell(self.pi_w, self.pi_b, FEATURES + HIDDEN) and cell(self.vf_w, self.vf_b, FEATURES + HIDDEN), "lstm_cell_mfma operand shapes"
        assert self.act[0].shape == (ACT_DIM, LATENT) and self.val[0].shape == (1, LATENT), "policy_heads operand shapes"
        if self.fe_img is not None:
            assert self.fe_bias.numel() == 128 + 1024 + 1024 + 128 and (
                not self.fe_img.is_cuda or self.fe_img.numel() * 2 == _lib.load().fdyn_policy_features_image_bytes()), \
                "policy_features operand shapes"
        if self.trunk_w1 is not None:
            assert self.trunk_w1.shape == (2, 128, HIDDEN) and self.trunk_w2p.shape == (2, LATENT, 128), "policy_trunks operand shapes"

    def refresh(self, new: "Snapshot"):
        """Take the values of `new` IN PLACE: a captured rollout graph holds these pointers."""
        pairs = [p for f in fields(self) for p in _tensor_pairs(getattr(self, f.name), getattr(new, f.name), f.name)]
        for dst, src in pairs:            # every pair was checked before the first one is written
            dst.copy_(src)


def _tensor_pairs(dst, src, name):
    """(old, new) of every tensor of a snapshot field; ValueError unless the two sides have the same layout."""
    if isinstance(dst, torch.Tensor) and isinstance(src, torch.Tensor):
        if dst.shape != src.shape or dst.dtype != src.dtype or dst.device != src.device:     # copy_ would broadcast, cast or move
            raise ValueError(f"inference snapshot: {name} was {tuple(dst.shape)} {dst.dtype} on {dst.device}, the policy now gives "
                             f"{tuple(src.shape)} {src.dtype} on {src.device}; a snapshot is refreshed in place, never reshaped")
        return [(dst, src)]
    if isinstance(dst, (list, tuple)) and isinstance(src, (list, tuple)) and len(dst) == len(src):
        return [p for i, (d, s) in enumerate(zip(dst, src)) for p in _tensor_pairs(d, s, f"{name}[{i}]")]
    if dst is None and src is None:
        return []
    raise ValueError(f"inference snapshot: {name} no longer has the layout it was built with")


def _linears(seq):
    return [m for m in seq if isinstance(m, nn.Linear)]


def served(policy) -> bool:
    """True if the fused kernels can run this policy: decided from the weight shapes alone, once per snapshot."""
    if not policy.use_lstm or policy.hidden != HIDDEN:
        return False
    fe = policy.features_extractor
    fe_w = [getattr(fe.lstm, f"weight_ih_l{k}") for k in range(fe.lstm.num_layers)]
    return (all(w.shape[1] in (128, 256) and w.shape[0] % 128 == 0 for w in fe_w)
            and policy.lstm_actor.weight_ih_l0.shape == (4 * HIDDEN, FEATURES) and policy.lstm_critic.weight_ih_l0.shape == (4 * HIDDEN, FEATURES)
            and policy.action_net.weight.shape == (ACT_DIM, LATENT) and policy.value_net.weight.shape == (1, LATENT))


def snapshot(policy) -> Optional[Snapshot]:
    """The weights of `policy` as bf16 [4H, in+H] / fp32 bias tensors for the fused rollout path, or None where `served` says no."""
    if not served(policy):
        return None
    fe, bf = policy.features_extractor, torch.bfloat16

    def cat(l, k):
        return torch.cat([getattr(l, f"weight_ih_l{k}"), getattr(l, f"weight_hh_l{k}")], 1).detach().to(bf).contiguous()

    def bias(l, k):
        return (getattr(l, f"bias_ih_l{k}") + getattr(l, f"bias_hh_l{k}")).detach().float().contiguous()

    def lin(seq):
        return [(m.weight.detach().to(bf).contiguous(), m.bias.detach().to(bf).contiguous()) for m in _linears(seq)]
    snap = Snapshot(
        fe_w=[getattr(fe.lstm, f"weight_ih_l{k}").detach().to(bf).contiguous() for k in range(fe.lstm.num_layers)],
        fe_b=[bias(fe.lstm, k) for k in range(fe.lstm.num_layers)],
        pi_w=cat(policy.lstm_actor, 0), pi_b=bias(policy.lstm_actor, 0), vf_w=cat(policy.lstm_critic, 0), vf_b=bias(policy.lstm_critic, 0),
        emb=lin(fe.embedding), proj=lin(fe.output_proj), pi=lin(policy.pi_net), vf=lin(policy.vf_net),
        act=lin([policy.action_net])[0], val=lin([policy.value_net])[0])
    emb_l, proj_l = _linears(fe.embedding), _linears(fe.output_proj)
    if (fe.lstm.num_layers == 2 and len(emb_l) == 1 and len(proj_l) == 1 and emb_l[0].weight.shape == (128, OBS_DIM)
            and fe.lstm.weight_ih_l0.shape == (1024, 128) and fe.lstm.weight_ih_l1.shape == (1024, 256)
            and proj_l[0].weight.shape == (128, 256)):
        snap.fe_img = pack_fe_weights(emb_l[0].weight, fe.lstm.weight_ih_l0, fe.lstm.weight_ih_l1, proj_l[0].weight)
        snap.fe_bias = torch.cat([emb_l[0].bias.detach().float(), bias(fe.lstm, 0), bias(fe.lstm, 1),
                                  proj_l[0].bias.detach().float()]).contiguous()
    pi_l, vf_l = _linears(policy.pi_net), _linears(policy.vf_net)
    if len(pi_l) == 2 and len(vf_l) == 2 and all(l[0].weight.shape == (128, 256) and l[1].weight.shape == (64, 128) for l in (pi_l, vf_l)):
        perm = _kperm(128, pi_l[0].weight.device)
        snap.trunk_w1 = torch.stack([pi_l[0].weight.detach(), vf_l[0].weight.detach()]).to(bf).contiguous()
        snap.trunk_b1 = torch.stack([pi_l[0].bias.detach(), vf_l[0].bias.detach()]).float().contiguous()
        snap.trunk_w2p = torch.stack([pi_l[1].weight.detach()[:, perm], vf_l[1].weight.detach()[:, perm]]).to(bf).contiguous()
        snap.trunk_b2 = torch.stack([pi_l[1].bias.detach(), vf_l[1].bias.detach()]).float().contiguous()
    snap.check()
    return snap


def prepare(old: Optional[Snapshot], policy) -> Optional[Snapshot]:
    """The snapshot `policy` holds after its weights changed: a new one the first time, the old one refreshed in place after that."""
    new = snapshot(policy)
    if old is None:
        return new
    if new is None:
        raise ValueError("inference snapshot: the policy's layers changed to shapes the fused path does not serve; "
                         "a snapshot is refreshed in place, never reshaped")
    old.refresh(new)
    return old


# ---- knobs and route -------------------------------------------------------------------------------------------------------
def knob(name: str) -> bool:
    """True if the environment switch `name` is thrown (DESIGN.md has the table of the six).  Read at call time: tests and A/B
    scripts flip them between two calls -- and one variable at a time: a read costs 2 us, a rollout step has no time for spares."""
    value = os.environ.get(name)
    return value == "0" if name == "FDYN_INPLACE_STATE" else bool(value)      # the one switch that is thrown by "0"


class Knobs(NamedTuple):
    """The four switches that choose between entry points; True = the named kernel or form is OFF.  (FDYN_NO_MFMA, the fused path
    as a whole, is read by RateLSTMPolicy._fused_ok; FDYN_INPLACE_STATE=0 by inplace_ok.)"""
    no_fe64: bool = False             # FDYN_NO_FE64: features layer by layer instead of csrc/policy_fe64.hip
    no_cell_pair: bool = False        # FDYN_NO_CELL_PAIR: actor and critic cell as two launches
    no_trunk: bool = False            # FDYN_NO_TRUNK: trunks as hipBLASLt GEMMs instead of csrc/policy_trunk.hip
    no_trunk_heads: bool = False      # FDYN_NO_TRUNK_HEADS: trunks and heads as two launches


def knobs() -> Knobs:
    return Knobs(knob("FDYN_NO_FE64"), knob("FDYN_NO_CELL_PAIR"), knob("FDYN_NO_TRUNK"), knob("FDYN_NO_TRUNK_HEADS"))


class Route(NamedTuple):
    """The entry points of one fused step, by the names they have in include/fdyn.h (without the fdyn_ prefix)."""
    features: str     # policy_features_flags | policy_features | layerwise
    cells: str        # lstm_cell_mfma_pair | lstm_cell_mfma
    heads: str        # policy_trunks_heads | policy_trunks+policy_heads | gemm+policy_heads


def route(snap: Snapshot, B: int, uint8_flags: bool, k: Knobs) -> Route:
    """uint8_flags: the caller handed in the previous env step's done flags, both as uint8 (what the features kernel can read)."""
    if snap.fe_img is not None and B % 256 == 0 and B >= FE64_MIN_BATCH and not k.no_fe64:
        features = "policy_features_flags" if uint8_flags else "policy_features"
    else:
        features = "layerwise"
    if snap.trunk_w1 is None or k.no_trunk:
        heads = "gemm+policy_heads"
    else:
        heads = "policy_trunks+policy_heads" if k.no_trunk_heads else "policy_trunks_heads"
    return Route(features, "lstm_cell_mfma" if k.no_cell_pair else "lstm_cell_mfma_pair", heads)


def inplace_ok(batch: int) -> bool:
    """The device-independent part of RateLSTMPolicy.recurrent_inplace_ok, for a policy the fused path serves."""
    return (not knob("FDYN_INPLACE_STATE") and not knob("FDYN_NO_MFMA")
            and bool(_lib.load().fdyn_lstm_cell_mfma_inplace_ok(FEATURES, HIDDEN, HIDDEN, int(batch))))


# ---- the three launch stages -----------------------------------------------------------------------------------------------
def mlp_bf16(x, layers: List[Layer]):
    for w, b in layers:
        x = torch._addmm_activation(b, x, w.t())        # relu(x W^T + b): bias + ReLU in the GEMM epilogue (hipBLASLt)
    return x


def _check_flags(flags, B):
    term, trunc, es, kp, _ctr = flags
    assert term.shape == (B,) and trunc.shape == (B,) and es.shape == (B,) and kp.shape == (B,) and es.dtype == torch.float32 \
        and kp.dtype == torch.float32 and all(t.is_contiguous() for t in (term, trunc, es, kp)), "policy_features_flags operands"


def _features(snap, kind, obs, flags):
    """obs [B, 18] -> feats bf16 [B, 128].  flags = (terminated, truncated, episode_start, keep, counter) or None: the glue between
    the previous env step and this step, done by the features kernel for its rows where the route says so, else by
    fused.episode_flags in a launch of its own, before anything reads keep."""
    lib, st, B, bf = _lib.load(), _lib.current_stream(), obs.shape[0], torch.bfloat16
    if flags is not None and kind != "policy_features_flags":
        episode_flags(*flags)
    if kind == "layerwise":
        x = mlp_bf16(obs.to(bf), snap.emb)
        for w, b in zip(snap.fe_w, snap.fe_b):                       # zero-state layers: no h/c input at all
            assert x.is_contiguous() and x.dtype == bf and x.shape == (B, w.shape[1]), "lstm_cell_mfma operand shapes"
            h = torch.empty((B, w.shape[0] // 4), dtype=bf, device=obs.device)
            _lib.check(lib.fdyn_lstm_cell_mfma(x.data_ptr(), x.shape[1], None, 0, None, None, w.data_ptr(), b.data_ptr(),
                                               h.data_ptr(), None, None, B, w.shape[0] // 4, st), "lstm_cell_mfma")
            x = h
        return mlp_bf16(x, snap.proj)
    # one kernel from the observation to the features: activations stay in registers between the four layers
    o32 = obs.float().contiguous()
    assert o32.shape == (B, OBS_DIM), "policy_features operand shapes"
    feats = torch.empty((B, FEATURES), dtype=bf, device=obs.device)
    if kind == "policy_features_flags":
        _check_flags(flags, B)
        term, trunc, es, kp, ctr = flags
        _lib.check(lib.fdyn_policy_features_flags(o32.data_ptr(), snap.fe_img.data_ptr(), snap.fe_bias.data_ptr(), feats.data_ptr(),
                                                  term.data_ptr(), trunc.data_ptr(), es.data_ptr(), kp.data_ptr(), _lib.ptr(ctr), B, st),
                   "policy_features_flags")
    else:
        _lib.check(lib.fdyn_policy_features(o32.data_ptr(), snap.fe_img.data_ptr(), snap.fe_bias.data_ptr(), feats.data_ptr(), B, st),
                   "policy_features")
    return feats


def _cell_operands(lib, feats, h_prev, c_prev, h_out, c_out, keep):
    """One cell's state as the kernel reads it (h bf16, c fp32) and the buffers it writes: the caller's where they fit -- the
    kernel then writes the new state straight into the ping-pong pair, or in place where its shape allows -- else fresh ones."""
    B, H, bf = feats.shape[0], HIDDEN, torch.bfloat16
    hp, cp = h_prev.to(bf).contiguous(), c_prev.float().contiguous()
    assert feats.is_contiguous() and feats.dtype == bf and feats.shape == (B, FEATURES) and hp.shape == (B, H) and cp.shape == (B, H) \
        and keep.shape == (B,), "lstm_cell_mfma operand shapes"
    ok = h_out is not None and h_out.dtype == bf and h_out.shape == (B, H) and h_out.is_contiguous() and c_out.dtype == torch.float32 \
        and c_out.shape == (B, H) and c_out.is_contiguous() \
        and ((h_out.data_ptr() != hp.data_ptr() and c_out.data_ptr() != cp.data_ptr()) or lib.fdyn_lstm_cell_mfma_inplace_ok(FEATURES, H, H, B))
    h = h_out if ok else torch.empty((B, H), dtype=bf, device=feats.device)
    c = c_out if ok else torch.empty((B, H), dtype=torch.float32, device=feats.device)
    return hp, cp, h, c


def _cells(snap, kind, feats, states, keep, out_states):
    """The actor and the critic cell on the same features -> [pi_h, pi_c, vf_h, vf_c] of the new state."""
    lib, st, B, H = _lib.load(), _lib.current_stream(), feats.shape[0], HIDDEN
    outs = (None, None, None, None) if out_states is None else tuple(out_states)
    cells = []
    for w, b, i in ((snap.pi_w, snap.pi_b, 0), (snap.vf_w, snap.vf_b, 2)):
        hp, cp, h, c = _cell_operands(lib, feats, states[i], states[i + 1], outs[i], outs[i + 1], keep)
        cells.append((hp, cp, w, b, h, c))
    if kind == "lstm_cell_mfma":                          # A/B knob: the two launches of rounds 1-2
        for hp, cp, w, b, h, c in cells:
            _lib.check(lib.fdyn_lstm_cell_mfma(feats.data_ptr(), FEATURES, hp.data_ptr(), H, cp.data_ptr(), keep.data_ptr(),
                                               w.data_ptr(), b.data_ptr(), h.data_ptr(), c.data_ptr(), None, B, H, st), "lstm_cell_mfma")
    else:       # one launch (fdyn_lstm_cell_mfma_pair falls back to two where the paired kernel does not apply)
        _lib.check(lib.fdyn_lstm_cell_mfma_pair(feats.data_ptr(), FEATURES, keep.data_ptr(), H, B, H,
                                                *[t.data_ptr() for cell in cells for t in cell], st), "lstm_cell_mfma_pair")
    return [t for cell in cells for t in cell[4:]]


def _heads(snap, kind, h_pi, h_vf, log_std, noise_seed, noise_step, deterministic):
    """The two trunks, the 64 -> 4 and 64 -> 1 output layers and the sampling -> (actions [B, 4], value [B], logp [B]), fp32.
    In-kernel Philox keyed by a per-policy seed, the env index and a step counter that lives on the device, so a captured graph
    draws fresh noise on every replay."""
    lib, st, B, bf, dev = _lib.load(), _lib.current_stream(), h_pi.shape[0], torch.bfloat16, h_pi.device
    lat = None                                            # policy_trunks_heads: the trunk outputs never leave the registers
    if kind == "gemm+policy_heads":
        lat = mlp_bf16(h_pi, snap.pi), mlp_bf16(h_vf, snap.vf)
    else:
        assert h_pi.dtype == bf and h_vf.dtype == bf and h_pi.is_contiguous() and h_vf.is_contiguous() \
            and h_pi.shape == (B, HIDDEN) and h_vf.shape == (B, HIDDEN), "policy_trunks operand shapes"
        trunks = [h_pi.data_ptr(), h_vf.data_ptr(), snap.trunk_w1.data_ptr(), snap.trunk_b1.data_ptr(), snap.trunk_w2p.data_ptr(),
                  snap.trunk_b2.data_ptr()]
        if kind == "policy_trunks+policy_heads":
            lat = torch.empty((B, LATENT), dtype=bf, device=dev), torch.empty((B, LATENT), dtype=bf, device=dev)
            _lib.check(lib.fdyn_policy_trunks(*trunks, lat[0].data_ptr(), lat[1].data_ptr(), B, st), "policy_trunks")
    actions = torch.empty((B, ACT_DIM), dtype=torch.float32, device=dev)
    logp = torch.empty(B, dtype=torch.float32, device=dev)
    value = torch.empty(B, dtype=torch.float32, device=dev)
    tail = [snap.act[0].data_ptr(), snap.act[1].data_ptr(), snap.val[0].data_ptr(), snap.val[1].data_ptr(),
            log_std.detach().float().contiguous().data_ptr(), noise_seed, noise_step.data_ptr(), int(deterministic),
            actions.data_ptr(), logp.data_ptr(), value.data_ptr(), B, st]
    if lat is None:
        _lib.check(lib.fdyn_policy_trunks_heads(*trunks, *tail), "policy_trunks_heads")
    else:
        assert all(t.shape == (B, LATENT) and t.dtype == bf and t.is_contiguous() for t in lat), "policy_heads operand shapes"
        _lib.check(lib.fdyn_policy_heads(lat[0].data_ptr(), lat[1].data_ptr(), *tail), "policy_heads")
    return actions, value, logp


def step(snap: Snapshot, noise, obs, states, episode_start, deterministic, out_states, keep, bump_noise, done_flags):
    """RateLSTMPolicy.step on the explicit bf16 path (no autocast): pre-cast Linear weights, one MFMA kernel per LSTM cell.
    noise = (log_std, seed, device step counter); the rest as RateLSTMPolicy.step -> actions, value, logp, [pi_h, pi_c, vf_h, vf_c]."""
    log_std, noise_seed, noise_step = noise
    if keep is None:
        assert done_flags is None, "done_flags needs the caller's keep buffer"
        keep = (1.0 - episode_start.float()).contiguous()        # the mask is applied inside the kernel
    flags = None
    if done_flags is not None:
        flags = (done_flags[0], done_flags[1], episode_start, keep, noise_step)
    elif bump_noise:
        noise_step.add_(1)
    uint8_flags = flags is not None and flags[0].dtype == torch.uint8 and flags[1].dtype == torch.uint8
    r = route(snap, obs.shape[0], uint8_flags, knobs())
    feats = _features(snap, r.features, obs, flags)
    new = _cells(snap, r.cells, feats, states, keep, out_states)
    return (*_heads(snap, r.heads, new[0], new[2], log_std, noise_seed, noise_step, deterministic), new)

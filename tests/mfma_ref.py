"""References, error bounds and an fp32 emulation of the hand-written MFMA policy kernels (csrc/lstm_mfma.hip, lstm_mfma64.hip,
policy_trunk.hip, policy_fe64.hip).  Plain torch on whatever device the operands live on; nothing here needs a GPU.
tests/test_mfma_ref_host.py runs the emulation through every comparison below (and shows that seeded defects fail them);
tests/test_gpu_mfma_kernels.py runs the kernels through the same comparisons.

Conventions (those of test_gpu_policy_kernels.py): a reference starts from the values the kernel reads (bf16 operands rounded
first, then widened); data are random and asymmetric, biases non-zero; the cases are cached and never modified.

Tolerances.  u = 2^-23 is twice the fp32 unit roundoff (the rounding mode of the MFMA accumulation is not documented); a K-term
dot product plus bias, summed in any order, scaled and fed to an exponent FMA, is within

    tg = (K + 3) u (|a| @ |W|^T + |b|)                                                    (gate pre-activation, per element)

of the exact value.  Through sigmoid' <= 1/4, tanh' <= 1, sigmoid <= 1:

    tol_c   = tg_i / 4 + tg_g + |keep c_prev| tg_f / 4 + A max(1, |c_ref|)
    tol_h32 = tg_o / 4 + tol_c + A
    bf16 outputs        2^-8 |ref| + 2 tol          (_step_tol's convention: one rounding of a value within tol)
    stored activations  2^-8 |ref| + 2 (tg / 4 + A)   (tg instead of tg / 4 for the g gate)

A = 2e-5 is TOL_FWD32 of test_gpu_policy_kernels.py: the project's figure for the exp2 / rcp activation forms.  The forms
alone, written in float32 with correctly rounded exp2 and division, are within 8.9e-8 (sigmoid) and 1.8e-7 (tanh) of fp64
(measure_activation_forms, asserted in the host test): A leaves two orders of magnitude for the hardware's 1-ulp exp2 and rcp.

Linear layers (trunks, embedding, projection) have no activation form: their bound is (K + 3) u (|a| @ |W|^T + |b|), doubled and
joined by 2^-8 |ref| behind the bf16 rounding of the output.

Statistical caps (multi-layer kernels end to end, against fp64 with the same rounding points): no element further than
4 2^-8 |ref| + 1e-3, at most 1 % of the elements further than 2^-8 |ref| + 4e-5.  What the fp32 emulation alone leaves outside
them is asserted in the host test for the very cases the device runs.
"""
import functools
import types

import torch

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
U = 2.0 ** -23
A_ACT = 2e-5                           # TOL_FWD32 of test_gpu_policy_kernels.py
BF_HALF = 2.0 ** -8                    # largest relative error of one rounding to bf16
CAP_HARD = (4 * BF_HALF, 1e-3)         # no element outside rel |ref| + abs
CAP_SOFT = (BF_HALF, 4e-5)             # at most CAP_FRAC of the elements outside
CAP_FRAC = 0.01
SENT = 768.0                           # exact in bf16, far outside every value these kernels produce
L2E = 1.4426950408889634
L2E32 = float(torch.tensor(L2E, dtype=F32))
GATE_SCALE = (-L2E, 1.0, -2.0 * L2E, -L2E)         # what policy.FE_GATE_SCALE has to be: exponent factors of gates i, f, g, o
# k order inside every block of 16 of a layer that reads the previous layer's 32x32 MFMA output tile: position j = 8 hf + p of
# k-step hq holds tile register e = 8 hq + p of lane half hf, which is feature (e & 3) + 8 (e >> 2) + 4 hf of the slice
KORDER16 = tuple(((p & 3) + 8 * (p >> 2) + 4 * hf) for hf in range(2) for p in range(8))


def bf(t):
    return t.to(BF).to(t.dtype)


def _f32(v, like):
    return torch.as_tensor(v, dtype=F32, device=like.device)


def fma(a, b, c):
    """fp32 fused multiply-add: the product of two floats is exact in fp64, the sum is rounded once more on the way back."""
    ref = next(t for t in (a, b, c) if isinstance(t, torch.Tensor))
    a, b, c = (t if isinstance(t, torch.Tensor) else _f32(t, ref) for t in (a, b, c))
    return (a.double() * b.double() + c.double()).float()


def rcp(x):
    return 1.0 / x


def korder(K, device="cpu"):
    return torch.tensor([16 * (k // 16) + KORDER16[k % 16] for k in range(K)], device=device)


def ratio(out, ref, tol):
    """max |out - ref| / tol; inf where an output is not finite."""
    out = out.detach().to(F64)
    if not bool(torch.isfinite(out).all()):
        return float("inf")
    return float(((out - ref).abs() / tol).max())


def caps(out, ref):
    """(elements outside the hard cap, fraction outside the soft cap)."""
    d = (out.detach().to(F64) - ref).abs()
    if not bool(torch.isfinite(d).all()):
        return int(d.numel()), 1.0
    hard = int((d > CAP_HARD[0] * ref.abs() + CAP_HARD[1]).sum())
    soft = float((d > CAP_SOFT[0] * ref.abs() + CAP_SOFT[1]).double().mean())
    return hard, soft


def caps_ok(out, ref):
    hard, soft = caps(out, ref)
    return hard == 0 and soft <= CAP_FRAC


# ---- the activation forms alone -------------------------------------------------------------------------------------------

def sigmoid_form(acc, b, l2e=L2E32):
    """sigmoid(acc + b) as the cells compute it: rcp(1 + exp2(fma(acc, -log2 e, -b log2 e)))."""
    return rcp(1.0 + torch.exp2(fma(acc, -l2e, b * _f32(-l2e, b))))


def tanh_form(acc, b, l2e=L2E32):
    """tanh(acc + b): fma(-2, rcp(exp2(fma(acc, 2 log2 e, 2 b log2 e)) + 1), 1)."""
    return fma(-2.0, rcp(torch.exp2(fma(acc, 2.0 * l2e, b * _f32(2.0 * l2e, b))) + 1.0), 1.0)


def tanh_plain(c):
    """tanh(c) of the cell state: 1 - 2 rcp(exp2(2 c log2 e) + 1)."""
    return fma(-2.0, rcp(torch.exp2((2.0 * c) * _f32(L2E32, c)) + 1.0), 1.0)


def measure_activation_forms():
    """Largest |form - fp64| over a grid of (acc, bias) in float32: (sigmoid, tanh, tanh of the state)."""
    g = torch.Generator().manual_seed(3)
    acc = (torch.rand(400000, generator=g) * 40 - 20).float()
    b = (torch.randn(400000, generator=g) * 0.5).float()
    x = acc.double() + b.double()
    c = (torch.rand(400000, generator=g) * 120 - 60).float()
    return (float((sigmoid_form(acc, b).double() - torch.sigmoid(x)).abs().max()),
            float((tanh_form(acc, b).double() - torch.tanh(x)).abs().max()),
            float((tanh_plain(c).double() - torch.tanh(c.double())).abs().max()))


# ---- the recurrent cell -----------------------------------------------------------------------------------------------------

KEEP_MODES = ("mixed", "ones", "zeros", "null")
# (gate, hidden unit, bias): saturated gates; negative units count from the end (the last slice)
SAT_BIASES = ((0, 1, 30.0), (1, 5, -30.0), (2, 9, 100.0), (3, 13, -100.0), (0, 17, -100.0), (2, 21, -30.0), (1, 25, 100.0),
              (3, 29, 30.0), (0, -2, 100.0), (2, -6, -100.0), (3, -10, -30.0), (1, -12, 30.0))
BIG = 1.0e30                           # what a restarted row's stale state holds (finite: 0 * inf is NaN in any reference)


def _keep_vector(B, mode, g, block_zero):
    if mode == "null":
        return None
    if mode == "ones":
        return torch.ones(B)
    if mode == "zeros":
        return torch.zeros(B)
    k = (torch.rand(B, generator=g) > 0.25).float()
    if B >= 64:
        k[32:64] = 0.0                                          # one whole 32-row tile
    for lo, n in block_zero:                                    # whole workgroups / waves of the one-wave-per-SIMD kernel
        k[lo:lo + n] = 0.0
    k[0], k[-1] = 0.0, 1.0
    return k


@functools.lru_cache(maxsize=None)
def cell_case(kx, kh, H, B, keep="mixed", seed=0, block_zero=()):
    """Stored operands of one cell step on the CPU.  kh = 0: zero-state layer (no h, c, keep)."""
    g = torch.Generator().manual_seed(100003 * seed + 1009 * kx + 13 * kh + 7 * H + B)
    r = lambda *s: torch.randn(*s, generator=g)                                 # noqa: E731
    d = types.SimpleNamespace(kx=kx, kh=kh, H=H, B=B, K=kx + kh, keep_mode=keep)
    d.x = (r(B, kx) * 0.7 + 0.1).to(BF)
    d.W = (r(4 * H, kx + kh) * 0.08 + 0.01).to(BF)
    d.bias = r(4 * H) * 0.3 + 0.1
    for gate, unit, val in SAT_BIASES:
        d.bias[gate * H + unit % H] = val
    d.keep_next = (torch.rand(B, generator=g) > 0.3).float()
    d.keep_next[0], d.keep_next[-1] = 1.0, 0.0
    d.h = d.c = d.keep = None
    if kh:
        d.h = (r(B, kh) * 0.5 - 0.05).to(BF)
        d.c = r(B, H)
        d.c[2::11] = (torch.rand(d.c[2::11].shape, generator=g) * 2 - 1) * 50.0
        d.keep = _keep_vector(B, keep, g, block_zero)
        if d.keep is not None:                                                  # restarted rows hold stale, large state
            dead = d.keep == 0
            sign = torch.where(torch.rand(B, generator=g) > 0.5, 1.0, -1.0)[:, None]
            d.h = torch.where(dead[:, None], (sign * BIG).to(BF), d.h)
            d.c = torch.where(dead[:, None], -sign * BIG, d.c)
    return d


def case_to(d, device):
    out = types.SimpleNamespace(**vars(d))
    for k, v in vars(d).items():
        if isinstance(v, torch.Tensor):
            setattr(out, k, v.to(device))
    return out


def _masked_operand(d, dtype):
    x = d.x.to(dtype)
    if not d.kh:
        return x
    h = d.h.to(dtype)
    if d.keep is not None:
        h = torch.where(d.keep[:, None] != 0, h, torch.zeros_like(h))           # keep is 0 or 1: a select, as the kernels do
    return torch.cat([x, h], 1)


def case_rows(d, rows):
    """The same case restricted to some of its rows (an index tensor or a slice)."""
    out = types.SimpleNamespace(**{k: (v[rows] if isinstance(v, torch.Tensor) and v.shape[:1] == (d.B,) else v) for k, v in vars(d).items()})
    out.B = out.x.shape[0]
    return out


def ref_cell64(d, rows=None):
    """fp64 of one cell step from the stored operands (optionally of some rows): c, h, act (4-gate layout, or (i, g, o)
    for kh = 0), hn = h keep_next, and the bounds tol_c, tol_h32, tol_h, tol_act of this module's header."""
    if rows is not None:
        d = case_rows(d, rows)
    a, W, b = _masked_operand(d, F64), d.W.to(F64), d.bias.to(F64)
    gates = a @ W.t() + b
    tg = (d.K + 3) * U * (a.abs() @ W.abs().t() + b.abs())
    i, f, g, o = gates.chunk(4, 1)
    tgi, tgf, tgg, tgo = tg.chunk(4, 1)
    si, sf, tg_, so = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
    r = types.SimpleNamespace()
    r.c = si * tg_
    tol_c = tgi / 4 + tgg
    if d.kh:
        kc = d.c.to(F64) * (1.0 if d.keep is None else d.keep.to(F64)[:, None])
        r.c = r.c + sf * kc
        tol_c = tol_c + kc.abs() * tgf / 4
    r.tol_c = tol_c + A_ACT * r.c.abs().clamp(min=1.0)
    r.h = so * torch.tanh(r.c)
    r.tol_h32 = tgo / 4 + r.tol_c + A_ACT
    r.tol_h = BF_HALF * r.h.abs() + 2 * r.tol_h32
    acts = [(si, tgi / 4), (sf, tgf / 4), (tg_, tgg), (so, tgo / 4)]
    if not d.kh:
        del acts[1]
    r.act = torch.cat([a_ for a_, _ in acts], 1)
    r.tol_act = torch.cat([BF_HALF * a_.abs() + 2 * (t_ + A_ACT) for a_, t_ in acts], 1)
    r.hn = r.h * d.keep_next.to(F64)[:, None]
    return r


CELL_DEFECTS = ("bias_bf16", "drop_last_k", "swap_rows", "keep_last_row", "log2e", "c_prev_bf16")


def emu_cell(d, defect=None):
    """The cell in float32 with the kernels' rounding points and activation forms: c (fp32), h (bf16), h32, act (bf16),
    hn (bf16).  `defect`: one of CELL_DEFECTS."""
    assert defect is None or defect in CELL_DEFECTS
    H, l2e = d.H, (float(torch.tensor(1.4427, dtype=F32)) if defect == "log2e" else L2E32)
    bias = bf(d.bias) if defect == "bias_bf16" else d.bias
    if defect == "keep_last_row" and d.keep is not None:
        d = types.SimpleNamespace(**vars(d))
        d.keep = d.keep.clone()
        d.keep[-1] = 1.0
    a, W = _masked_operand(d, F32), d.W.float()
    if defect == "drop_last_k":
        a = a.clone()
        a[:, -1] = 0.0
    if defect == "swap_rows":
        W = W.clone()
        W[[3, 2 * H + 7]] = W[[2 * H + 7, 3]]
    i, f, g, o = (a @ W.t()).chunk(4, 1)
    bi, bf_, bg, bo = bias.chunk(4)
    si, tg_, so = sigmoid_form(i, bi, l2e), tanh_form(g, bg, l2e), sigmoid_form(o, bo, l2e)
    c = si * tg_
    acts = [si, tg_, so]
    if d.kh:
        sf = sigmoid_form(f, bf_, l2e)
        cp = bf(d.c) if defect == "c_prev_bf16" else d.c
        kc = cp if d.keep is None else d.keep[:, None] * cp
        c = fma(sf, kc, c)
        acts.insert(1, sf)
    hv = so * tanh_plain(c)
    return dict(c=c, h=hv.to(BF), h32=hv, act=torch.cat(acts, 1).to(BF), hn=(hv * d.keep_next[:, None]).to(BF))


def check_cell(d, r, out, rows=None):
    """{name: max |out - ref| / bound} of the outputs present in `out` (c, h, h32, act, hn).  hn is compared with
    h keep_next as VALUES (a restarted row may hold -0)."""
    sel = (lambda t: t) if rows is None else (lambda t: t[rows])
    res = {}
    for name, ref, tol in (("c", r.c, r.tol_c), ("h", r.h, r.tol_h), ("h32", r.h, r.tol_h32), ("act", r.act, r.tol_act)):
        if out.get(name) is not None and not (name == "c" and not d.kh):
            res[name] = ratio(sel(out[name]), ref, tol)
    if out.get("hn") is not None:
        kn = sel(d.keep_next.to(out["hn"].device))
        res["hn"] = 0.0 if torch.equal(sel(out["hn"]).float(), sel(out["h"]).float() * kn[:, None]) else float("inf")
    return res


def reachable_splits(cus, H=256):
    """{split: smallest batch that gives it} over every batch size up to the first that needs no split at hidden width H."""
    out = {}
    for blocks in range(1, 2 * cus + 2):
        out.setdefault(cell_split(128 * blocks, H, cus), 128 * blocks)
    return out


def cell_split(B, H, cus):
    """launch()'s rule in csrc/lstm_mfma.hip: workgroups that share one 128-row block."""
    row_blocks, split = (B + 127) // 128, 1
    while split < H // 32 and row_blocks * split < 2 * cus:
        split *= 2
    while (H // 32) % split:
        split //= 2
    return split


# what the device tests run (kx, kh, H, B, keep mode); the host test runs the emulation through the same cases
PAIRS = ((128, 256), (128, 0), (256, 0), (128, 128))
CELL_SHAPES = ([(kx, kh, 256, B, "mixed") for kx, kh in PAIRS for B in (1, 31, 33, 128, 777)] +
               [(kx, kh, H, 160, "mixed") for kx, kh in PAIRS for H in (32, 96, 256)] +
               [(kx, kh, 256, 33, k) for kx, kh in ((128, 256), (128, 128)) for k in ("ones", "zeros", "null")] +
               [(128, 256, 256, 128, k) for k in ("ones", "zeros", "null")])
CELL_TILED_LARGE = ((128, 256, 256, 20000, "mixed"), (128, 256, 256, 40000, "mixed"))
TRAIN_SHAPES = [(kx, kh, H, B, "mixed") for kx, kh in PAIRS for B in (33, 777) for H in (96, 256)]
W64_B = 32768                                                   # smallest batch the public entry gives to the one-wave-per-SIMD kernel
W64_BLOCK_ZERO = ((512, 256), (1024 + 64, 64))                  # keep = 0 on a whole 256-row workgroup and on a whole 64-row wave
W64_CASES = tuple((128, 256, 256, W64_B, k) for k in KEEP_MODES)


def w64_case(keep, seed=0):
    return cell_case(128, 256, 256, W64_B, keep, seed, W64_BLOCK_ZERO if keep == "mixed" else ())


def pair_cases():
    """Actor and critic operands of the paired launch: the same x and keep mask, everything else distinct."""
    d0 = w64_case("mixed", seed=1)
    src = cell_case(128, 256, 256, W64_B, "ones", 2)
    d1 = types.SimpleNamespace(**vars(src))
    d1.x, d1.keep, d1.keep_mode = d0.x, d0.keep, d0.keep_mode
    dead = (d0.keep == 0)[:, None]
    d1.h = torch.where(dead, d0.h, src.h)                       # restarted rows: the stale, large state
    d1.c = torch.where(dead, -d0.c, src.c)
    return d0, d1


def spot_rows(B):
    """Rows a large case is checked on where the whole fp64 reference is not wanted (the host test): the first 512, the rows
    around the zeroed workgroup / wave, the last 256."""
    return torch.cat([torch.arange(0, 768), torch.arange(1024, 1280), torch.arange(B - 256, B)])


# ---- the trunks -----------------------------------------------------------------------------------------------------------

TRUNK_MODES = ("dense", "l1a", "l1b", "l2a", "l2b")


def trunk_sel1(s):
    """Layer-1 probe: lat[j] = relu(mid[sel(j)]); s = 0, 1 cover the 128 units between them."""
    return torch.tensor([2 * ((29 * j + 3) % 64) + s for j in range(64)])


def trunk_sel2(s):
    """Layer-2 probe: mid[n] = relu(h[sel(n)]); s = 0, 1 cover the 256 columns."""
    return torch.tensor([2 * ((37 * n + 11) % 128) + s for n in range(128)])


@functools.lru_cache(maxsize=None)
def trunk_case(B, mode="dense"):
    g = torch.Generator().manual_seed(4000 + B)                 # the same h, W for every mode of a size
    r = lambda *s: torch.randn(*s, generator=g)                                 # noqa: E731
    d = types.SimpleNamespace(B=B, mode=mode)
    d.h = (r(2, B, 256) * 0.6 + 0.05).to(BF)
    d.W1, d.b1 = (r(2, 128, 256) * 0.08).to(BF), r(2, 128) * 0.2 + 0.05
    d.W2, d.b2 = (r(2, 64, 128) * 0.1).to(BF), r(2, 64) * 0.2 + 0.03
    if mode in ("l1a", "l1b"):
        d.sel = trunk_sel1(int(mode == "l1b"))
        d.W2, d.b2 = torch.zeros(2, 64, 128, dtype=BF), torch.zeros(2, 64)
        d.W2[:, torch.arange(64), d.sel] = 1.0
    elif mode in ("l2a", "l2b"):
        d.sel = trunk_sel2(int(mode == "l2b"))
        d.W1, d.b1 = torch.zeros(2, 128, 256, dtype=BF), torch.zeros(2, 128)
        d.W1[:, torch.arange(128), d.sel] = 1.0
    return d


def pack_w2p(W2):
    """The host packing of layer 2 (policy.py keeps the k order)."""
    from hcrl_amd.policy import _KPERM16
    perm = torch.tensor([16 * (k // 16) + _KPERM16[k % 16] for k in range(W2.shape[-1])], device=W2.device)
    return W2[..., perm].contiguous()


def ref_trunk64(d):
    """-> [per trunk] (ref, tol or None): the element-wise reference and bound of the probe modes; for `dense` the fp64 result
    with the kernel's rounding point (mid rounded to bf16) and no element-wise bound."""
    out = []
    for t in range(2):
        h, W1, b1, W2, b2 = (x[t].to(F64) for x in (d.h, d.W1, d.b1, d.W2, d.b2))
        pre1 = h @ W1.t() + b1
        tg1 = (256 + 3) * U * (h.abs() @ W1.abs().t() + b1.abs())
        if d.mode.startswith("l1"):
            ref = torch.relu(pre1)[:, d.sel]
            out.append((ref, BF_HALF * ref.abs() + 2 * tg1[:, d.sel]))
            continue
        mid = bf(torch.relu(pre1))
        ref = torch.relu(mid @ W2.t() + b2)
        tg2 = (128 + 3) * U * (mid.abs() @ W2.abs().t() + b2.abs())
        out.append((ref, BF_HALF * ref.abs() + 2 * tg2 if d.mode.startswith("l2") else None))
    return out


TRUNK_DEFECTS = ("no_kperm", "mid_step", "bias_bf16", "drop_last_k")


def bf16_step(v, up):
    """The neighbouring bf16 value of a bf16-representable float32 tensor (away from / towards zero by one step)."""
    bits = v.to(BF).view(torch.int16).clone()
    return (bits + (1 if up else -1)).view(BF).float()


def emu_trunk(d, W2p, defect=None, at=None):
    """Both trunks in float32 from the PACKED layer-2 image, read in the kernel's k order -> [lat_pi, lat_vf] bf16.
    defect mid_step: element `at` = (row, unit, up) of layer 1's bf16 output moved by one bf16 step."""
    assert defect is None or defect in TRUNK_DEFECTS
    lats, ko = [], korder(128)
    for t in range(2):
        h, W1, b1, b2 = d.h[t].float(), d.W1[t].float(), d.b1[t], d.b2[t]
        if defect == "bias_bf16":
            b1, b2 = bf(b1), bf(b2)
        if defect == "drop_last_k":
            h = h.clone()
            h[:, -1] = 0.0
        mid = bf(torch.relu(h @ W1.t() + b1))
        if defect == "mid_step":
            row, unit, up = at
            mid[row, unit] = bf16_step(mid[row, unit], up)
        lats.append(torch.relu(mid[:, ko] @ W2p[t].float().t() + b2).to(BF))
    return lats


def check_trunk(d, refs, lats):
    """Probe modes: {trunk: ratio}; dense: {trunk: (hard, soft)} of caps()."""
    return {t: (caps(lats[t], ref) if tol is None else ratio(lats[t], ref, tol)) for t, (ref, tol) in enumerate(refs)}


# ---- the features extractor -----------------------------------------------------------------------------------------------

FE_PROBES = ("emba", "embb", "l1a+", "l1a-", "l1b+", "l1b-", "l2a+", "l2a-", "l2b+", "l2b-", "proj")
FE_MODES = ("dense",) + FE_PROBES
PASS_BIAS = 30.0                       # i and o biases of a pass-through LSTM layer: sigmoid(30) = 1 - 1e-13
SAT_W = 64.0                           # g weight of a SATURATED pass-through (in front of the layer under test): inputs are 0 or
SAT_MIN_IN = 0.5                       #   at least 0.5 in size, so tanh(g) is 0 or +-1 and the output one of {-t, 0, +t}
SRC1 = (torch.arange(256) * 5 + 3) % 128           # input a pass-through unit n of layer 1 / layer 2 reads
SRC2 = (torch.arange(256) * 7 + 1) % 256


def _sel256(s):
    return torch.tensor([2 * ((53 * j + 17) % 128) + s for j in range(128)])


def _pass_lstm(K, src, w):
    """A zero-state layer whose unit n is a known monotone function of input src[n]: g = w[n] x, i = o = PASS_BIAS."""
    W, b = torch.zeros(1024, K), torch.zeros(1024)
    W[2 * 256 + torch.arange(256), src] = w
    b[:256], b[3 * 256:] = PASS_BIAS, PASS_BIAS
    return W, b


# the g weight 1 as the image holds it: scaled by the gate's exponent factor, rounded to bf16 (1.0018)
PASS_Q = float(torch.tensor(GATE_SCALE[2], dtype=F32).to(BF).to(F64) / torch.tensor(GATE_SCALE[2], dtype=F32).to(F64))


def pass64(x, q=PASS_Q):
    """fp64 of a pass-through unit with g weight 1: sigmoid(30) tanh(sigmoid(30) tanh(q x)).  Lipschitz constant q."""
    s = torch.sigmoid(torch.tensor(PASS_BIAS, dtype=F64))
    return s * torch.tanh(s * torch.tanh(q * x))


def sat_value_and_margin():
    """t = what a saturated pass-through gives for a positive input, and its distance from the nearest bf16 rounding boundary
    (the kernel's float32 and the reference's float64 must round it to the same bf16 value)."""
    t = pass64(torch.tensor(SAT_W * SAT_MIN_IN, dtype=F64))                    # saturated: the rounded weight changes nothing
    tb = t.to(BF).to(F64)
    half = (bf16_step(tb.float(), True).to(F64) - tb) / 2            # half a step of its binade
    return float(tb), float(half - (t - tb).abs())


@functools.lru_cache(maxsize=None)
def fe_case(B, mode="dense"):
    """Model-side weights (fp32) of the features extractor and an observation batch.  dense: the weight scales of
    test_policy_features_kernel_matches_plain_torch_fp32.  Probe modes: ONE layer dense random (an LSTM layer with saturating
    biases on a few units), every other layer a pass-through whose output is known:
      embedding                 a1[n] = relu(obs[n % 16])                    exact (obs holds bf16 values)
      LSTM layer in front       h[n] = +-t or 0 (saturated: g = +-64 x)      exact, away from a rounding boundary
      LSTM layer behind         h[n] = pass64(input[src(n)])                 monotone, Lipschitz PASS_Q = 1.0018
      projection                feats[j] = relu(+-h2[sel(j)])                exact; a / b select the even / odd units, +/- the sign
    """
    assert mode in FE_MODES
    g = torch.Generator().manual_seed(7000 + B)
    r = lambda *s: torch.randn(*s, generator=g)                                 # noqa: E731
    d = types.SimpleNamespace(B=B, mode=mode)
    w = lambda o, i: r(o, i) * (1.6 / i ** 0.5)                                 # noqa: E731
    d.w_emb, d.b_emb = w(128, 18), r(128) * 0.5
    d.w1, d.b1 = w(1024, 128), r(1024) * 0.5
    d.w2, d.b2 = w(1024, 256), r(1024) * 0.5
    d.w_p, d.b_p = w(128, 256), r(128) * 0.5
    d.obs = r(B, 18) * torch.linspace(0.2, 2.0, 18)
    signs = torch.where(torch.rand(2, 256, generator=g) > 0.5, 1.0, -1.0)
    if mode == "dense":
        return d
    under = mode[:2] if mode != "proj" else "pr"                                # em, l1, l2, pr
    d.under = under
    if under in ("l2", "pr"):                                                   # a saturated layer in front: inputs 0 or >= 0.5
        d.obs = torch.where(d.obs > 0, d.obs.abs() + SAT_MIN_IN, d.obs)
    d.obs = bf(d.obs)
    d.sel = _sel256(int(mode.rstrip("+-").endswith("b")))
    d.sign = -1.0 if mode.endswith("-") else 1.0
    for gate, unit, val in SAT_BIASES:                                          # the LSTM layer under test saturates on a few units
        d.b1[gate * 256 + unit % 256] = val
        d.b2[gate * 256 + unit % 256] = val
    if under != "em":
        d.w_emb, d.b_emb = torch.zeros(128, 18), torch.zeros(128)
        d.w_emb[torch.arange(128), torch.arange(128) % 16] = 1.0
    if under != "l1":
        d.w1, d.b1 = _pass_lstm(128, SRC1, SAT_W * signs[0] if under in ("l2", "pr") else 1.0)
    if under != "l2":
        d.w2, d.b2 = _pass_lstm(256, SRC2, SAT_W * signs[1] if under == "pr" else 1.0)
    if under != "pr":
        d.w_p, d.b_p = torch.zeros(128, 256), torch.zeros(128)
        d.w_p[torch.arange(128), d.sel] = d.sign
    return d


def fe_pack(d, gate_scale=None):
    """(image, bias vector) as prepare_inference() builds them, through policy.pack_fe_weights.  gate_scale: a replacement for
    policy.FE_GATE_SCALE during the packing (a seeded host defect)."""
    from hcrl_amd import inference
    saved = inference.FE_GATE_SCALE
    try:
        if gate_scale is not None:
            inference.FE_GATE_SCALE = tuple(gate_scale)
        img = inference.pack_fe_weights(d.w_emb, d.w1, d.w2, d.w_p)
    finally:
        inference.FE_GATE_SCALE = saved
    return img, torch.cat([d.b_emb, d.b1, d.b2, d.b_p]).float().contiguous()


def _lstm_q64(w):
    """The weights a zero-state layer effectively multiplies by: scaled by the gate's exponent factor in fp32, rounded to bf16
    (the image), and the factor taken out again."""
    gs = torch.tensor(GATE_SCALE, dtype=F32).repeat_interleave(256)[:, None]
    return (w.float() * gs).to(BF).to(F64) / gs.to(F64)


def _zs_layer64(a, w, b):
    """-> h (unrounded) and its fp32 bound tol_h32 (the cell's, without c_prev)."""
    wq, b = _lstm_q64(w), b.to(F64)
    z = a @ wq.t() + b
    tg = (a.shape[1] + 3) * U * (a.abs() @ wq.abs().t() + b.abs())
    i, _, g, o = z.chunk(4, 1)
    ti, _, tg_, to = tg.chunk(4, 1)
    return torch.sigmoid(o) * torch.tanh(torch.sigmoid(i) * torch.tanh(g)), to / 4 + ti / 4 + tg_ + 2 * A_ACT


def ref_fe64(d):
    """fp64 with the kernel's rounding points, from the MODEL's weights (independent of pack_fe_weights): a1, h1, h2 as the
    kernel keeps them (bf16), their unrounded values and fp32 bounds, and feats (unrounded)."""
    r = types.SimpleNamespace()
    x, we, be = bf(d.obs).to(F64), d.w_emb.to(BF).to(F64), d.b_emb.to(F64)
    r.a1_raw = torch.relu(x @ we.t() + be)
    r.tol_a1 = (18 + 3) * U * (x.abs() @ we.abs().t() + be.abs())
    r.a1 = bf(r.a1_raw)
    r.h1_raw, r.tol_h1 = _zs_layer64(r.a1, d.w1, d.b1)
    r.h1 = bf(r.h1_raw)
    r.h2_raw, r.tol_h2 = _zs_layer64(r.h1, d.w2, d.b2)
    r.h2 = bf(r.h2_raw)
    wp, bp = d.w_p.to(BF).to(F64), d.b_p.to(F64)
    r.feats = torch.relu(r.h2 @ wp.t() + bp)
    r.tol_feats = (256 + 3) * U * (r.h2.abs() @ wp.abs().t() + bp.abs())
    return r


def fe_image_chunks(img):
    """The weight image decoded the way csrc/policy_fe64.hip reads it: (W_emb [128, 32], [per LSTM layer] W [1024, K] with the
    rows of gate f left zero, W_proj [128, 256]), columns in IMAGE order."""
    pos = [0]

    def take(rows, K):
        n = rows * (K + 8)
        t = img[pos[0]:pos[0] + n].view(rows, K + 8)[:, :K].float()
        pos[0] += n + (-n) % 512
        return t
    emb = take(128, 32)
    layers = []
    for K in (128, 256):
        W = torch.zeros(1024, K)
        for s in range(8):
            ig = take(64, K)
            W[32 * s:32 * s + 32], W[512 + 32 * s:512 + 32 * s + 32] = ig[:32], ig[32:]
            W[768 + 32 * s:768 + 32 * s + 32] = take(32, K)
        layers.append(W)
    proj = torch.cat([take(32, 256) for _ in range(4)], 0)
    assert pos[0] == img.numel()
    return emb, layers, proj


def emu_fe64(d, img, bias, step_at=None):
    """policy_fe64.hip in float32 from the packed image and the bias vector: same rounding points, accumulators that start from
    the scaled biases, the fused forms (1 - y) / ((1 + y)(1 + x)) with the +-40 clamp on the g exponent.
    step_at = (layer, rows, units, up): elements of h1 (layer 1) or h2 (2) moved by one bf16 step (index tensors or slices).
    -> dict a1, h1, h2 (float32 holding bf16 values), feats (bf16)."""
    emb, layers, proj = fe_image_chunks(img)
    b_e, b_1, b_2, b_p = bias[:128], bias[128:1152], bias[1152:2176], bias[2176:]
    cg = _f32(-2.0, bias) * _f32(L2E32, bias)
    inv_cg = 1.0 / cg
    x = torch.zeros(d.B, 32)
    x[:, :18] = bf(d.obs.float())
    out = {}
    a = out["a1"] = bf(torch.relu(x @ emb.t() + b_e))
    sc = torch.tensor([-L2E32, 0.0, -2.0 * L2E32, -L2E32]).repeat_interleave(256)
    for n, (W, b) in enumerate(zip(layers, (b_1, b_2)), 1):
        acc = (b * sc) + a[:, korder(a.shape[1])] @ W.t()                       # the image's columns are in the kernel's k order
        ai, _, ag, ao = acc.chunk(4, 1)
        xi, y = torch.exp2(ai), torch.exp2(ag.clamp(-40.0, 40.0))
        z = fma(y, inv_cg, inv_cg)
        z = rcp(fma(z, xi, z))
        ig = fma(-y, z, z)                                                      # CG sigmoid(i) tanh(g)
        xo, y = torch.exp2(ao), torch.exp2(ig)
        z = 1.0 + y
        z = rcp(fma(z, xo, z))
        a = bf(fma(-y, z, z))
        if step_at is not None and step_at[0] == n:
            _, rows, units, up = step_at
            a[rows, units] = bf16_step(a[rows, units], up)
        out[f"h{n}"] = a
    out["feats"] = torch.relu(a[:, korder(256)] @ proj.t() + b_p).to(BF)
    return out


def _through_pass(tol_in, raw):
    """Bound behind a pass-through layer (Lipschitz PASS_Q, its own forms within 2 A_ACT) and the bf16 rounding of its output."""
    return (1 + BF_HALF) * (PASS_Q * tol_in + 2 * A_ACT) + BF_HALF * raw.abs()


def fe_probe_ref(d, r=None):
    """(ref, tol) of a probe mode's feats: the layer under test's reference and derived bound, carried through the known
    pass-throughs behind it -- the reference UNROUNDED up to the output, the bound widened by each pass-through's Lipschitz
    constant (PASS_Q) and one bf16 rounding."""
    r = ref_fe64(d) if r is None else r
    stored = lambda raw, tol: BF_HALF * raw.abs() + 2 * tol                     # noqa: E731  a bf16 value computed within tol
    if d.under == "pr":
        return r.feats, stored(r.feats, r.tol_feats)
    if d.under == "l2":
        return torch.relu(d.sign * r.h2_raw[:, d.sel]), stored(r.h2_raw, r.tol_h2)[:, d.sel]
    if d.under == "l1":
        h2 = pass64(r.h1_raw[:, SRC2])
        return torch.relu(d.sign * h2[:, d.sel]), _through_pass(stored(r.h1_raw, r.tol_h1)[:, SRC2], h2)[:, d.sel]
    h1 = pass64(r.a1_raw[:, SRC1])
    t1 = _through_pass(stored(r.a1_raw, r.tol_a1)[:, SRC1], h1)
    h2 = pass64(h1[:, SRC2])
    return torch.relu(h2[:, d.sel]), _through_pass(t1[:, SRC2], h2)[:, d.sel]

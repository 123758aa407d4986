"""The kernels of csrc/policy_kernels.hip (and the heads of csrc/policy_trunk.hip) that every PPO update runs through, each
against a plain float64 reference of the same operation written in this file: the BPTT point-wise kernels one step at a time
through the C ABI, the bias partial sums and their reduction, fused.lstm_sequence as a node against an fp64 recurrence, the
output heads, the PPO loss and GAE at edge sizes.

Conventions: every reference starts from the values the kernel reads (bf16 operands are rounded first, then widened); data
are random and asymmetric, biases non-zero; output buffers hold a sentinel before each launch, so an element a kernel does
not write fails its comparison.  The references are built on the CPU and cached per shape; the tests never modify them.

All tests but one need the GPU and carry the `gpu` mark one by one (not a module-wide `pytestmark`):
test_fp64_recurrence_equals_nn_lstm checks this file's own recurrence against torch.nn.LSTM and runs without a device.
"""
import functools
import math
import types

import pytest
import torch
import torch.nn.functional as F

from hcrl_amd import _lib, fused

gpu = pytest.mark.gpu

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
SENT = 768.0                        # sentinel: exact in bf16, far outside every value these kernels produce
TOL_FWD32, TOL_GRAD32 = 2e-5, 8e-5  # test_fused_lstm_cell_matches_plain_torch_fp32's single-cell figures (fp32: tol, 4 * tol)
KX = 24                             # columns in front of the recurrent block of a packed next-step input row
DTYPES = [pytest.param(F32, id="fp32"), pytest.param(BF, id="bf16")]


def _wide(t):
    return t.detach().cpu().to(F64)


def _step_tol(ref, tol32, lowp):
    """Element-wise single-step tolerance.  fp32 output: tol32 * max(1, max|ref|).  bf16 output: 2^-8 |ref| + twice that --
    one bf16 rounding of a value that is itself within the fp32 tolerance."""
    t = tol32 * max(1.0, float(ref.abs().max()))
    return 2.0 ** -8 * ref.abs() + 2.0 * t if lowp else torch.full_like(ref, t)


def _close(name, out, ref, tol32, lowp):
    out, ref = _wide(out), ref.detach().to(F64)
    assert out.shape == ref.shape, (name, out.shape, ref.shape)
    assert bool(torch.isfinite(out).all()), name
    over = (out - ref).abs() - _step_tol(ref, tol32, lowp)
    k = int(over.argmax())
    assert float(over.max()) <= 0.0, (name, "flat index", k, "got", float(out.flatten()[k]), "want", float(ref.flatten()[k]))


def _p(t, offset_elems=0):
    return None if t is None else t.data_ptr() + offset_elems * t.element_size()


# ---- fp64 references of one BPTT step -------------------------------------------------------------------------------------

def ref_gates_to_act(pre, bias, group_rows):
    gates = pre if bias is None else pre + bias[torch.arange(pre.shape[0]) // group_rows]
    i, f, g, o = gates.chunk(4, -1)
    return torch.cat([torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)], -1)


def ref_cell(act, c_prev, keep, keep_next=None, c_stored=None):
    """c = s(f) (keep c_prev) + s(i) tanh(g), h = s(o) tanh(c), h_next = h keep_next, from the ACTIVATED gates.  c_stored: the
    value of c the kernel reads back (fp32) replaces the recomputed one; the gradient still flows through the formula."""
    ai, af, ag, ao = act.chunk(4, -1)
    c = af * (keep[:, None] * c_prev) + ai * ag
    if c_stored is not None:
        c = c + (c_stored - c.detach())
    h = ao * torch.tanh(c)
    return h, c, (None if keep_next is None else h * keep_next[:, None])


def ref_step_bwd(saved, from_pre, bias, group_rows, c_prev, keep, c_new, dh, dh2, dh2_keep, dc_next):
    """dgates, dc_prev by autograd through the forward above, from dh_total = dh + dh2_keep dh2 and dc_next.  `saved` holds the
    stored pre-activations (from_pre) or the stored activations; from the latter, the derivative of each non-linearity is
    taken in terms of its stored output, as any backward pass from saved activations has to."""
    x = saved.clone().requires_grad_()
    cp = c_prev.clone().requires_grad_()
    act = ref_gates_to_act(x, bias, group_rows) if from_pre else x
    h, c, _ = ref_cell(act, cp, keep, None, c_new)
    dht = dh if dh2 is None else dh + dh2_keep[:, None] * dh2
    loss = (h * dht).sum()
    if dc_next is not None:
        loss = loss + (c * dc_next).sum()
    gx, gc = torch.autograd.grad(loss, [x, cp])
    if not from_pre:
        ai, af, ag, ao = saved.chunk(4, -1)
        gx = gx * torch.cat([ai * (1 - ai), af * (1 - af), 1 - ag * ag, ao * (1 - ao)], -1)
    return gx, gc


@functools.lru_cache(maxsize=None)
def _step_case(H, B, dtype):
    """Stored operands (CPU, storage dtype) of one BPTT step and the fp64 forward results from them."""
    g = torch.Generator().manual_seed(1000 * H + B)
    r = lambda *s: torch.randn(*s, generator=g, dtype=F64)                      # noqa: E731
    nbias = 2 if B % 2 == 0 else 1                                              # two bias rows (two cells) where B is even
    d = types.SimpleNamespace(H=H, B=B, dtype=dtype, group_rows=B // nbias)
    d.pre = (r(B, 4 * H) * 1.5).to(dtype)
    d.bias = (r(nbias, 4 * H) * 0.5 + 0.1).to(dtype)
    d.c_prev = r(B, H).to(F32)

    def mask(first):                                                            # ~30 % zeros, row 0 and the last row opposite
        m = (torch.rand(B, generator=g) > 0.3).to(F32)
        m[0], m[-1] = first, 1.0 - first
        return m
    d.keep, d.keep_next, d.dh2_keep = mask(0.0), mask(1.0), mask(0.0)
    d.dh = r(B, H).to(dtype)
    d.dh2buf = r(B, KX + H + 8).to(dtype)                                       # the recurrent gradient sits in columns [KX, KX + H)
    d.dc_next = r(B, H).to(F32)
    d.act64 = ref_gates_to_act(d.pre.to(F64), d.bias.to(F64), d.group_rows)
    d.h64, d.c64, d.hn64 = ref_cell(d.act64, d.c_prev.to(F64), d.keep.to(F64), d.keep_next.to(F64))
    d.act, d.c_new = d.act64.to(dtype), d.c64.to(F32)                           # what a forward pass leaves for the backward
    return d


@functools.lru_cache(maxsize=None)
def _step_bwd_ref(H, B, dtype, from_pre, inner):
    d = _step_case(H, B, dtype)
    w = lambda t: t.to(F64)                                                     # noqa: E731
    return ref_step_bwd(w(d.pre if from_pre else d.act), from_pre, w(d.bias), d.group_rows, w(d.c_prev), w(d.keep), w(d.c_new),
                        w(d.dh), w(d.dh2buf[:, KX:KX + H]) if inner else None, w(d.dh2_keep) if inner else None,
                        w(d.dc_next) if inner else None)


# ---- 1. one step of the sequence kernels through the C ABI -----------------------------------------------------------------

@gpu
@pytest.mark.parametrize("with_act,with_next,with_bias", [(a, n, b) for a in (1, 0) for n in (1, 0) for b in (1, 0)],
                         ids=[f"act{a}-next{n}-bias{b}" for a in (1, 0) for n in (1, 0) for b in (1, 0)])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,B", [(256, 37), (256, 300), (64, 130), (40, 19)])
def test_seq_fwd_step_matches_fp64(H, B, dtype, with_act, with_next, with_bias):
    """fdyn_lstm_seq_fwd with each of act_out, the packed h_next = h keep_next and the per-cell bias rows given or NULL
    (independently: the default BPTT path passes bias without act_out, the last step no h_next): h, c and the optional outputs
    element-wise against fp64; nothing is written outside columns [KX, KX + H) of the next-step rows."""
    d, lib, lowp = _step_case(H, B, dtype), _lib.load(), dtype == BF
    pre, c_prev, keep = d.pre.cuda(), d.c_prev.cuda(), d.keep.cuda()
    h = torch.full((B, H), SENT, dtype=dtype, device="cuda")
    c = torch.full((B, H), SENT, device="cuda")
    act = torch.full((B, 4 * H), SENT, dtype=dtype, device="cuda") if with_act else None
    nxt = torch.full((B, KX + H + 8), SENT, dtype=dtype, device="cuda") if with_next else None
    kn = d.keep_next.cuda() if with_next else None
    bias = d.bias.cuda() if with_bias else None
    rc = lib.fdyn_lstm_seq_fwd(_p(pre), int(lowp), _p(c_prev), _p(keep), _p(h), _p(c), _p(act), _p(nxt, KX) if with_next else None,
                               KX + H + 8, _p(kn), _p(bias), d.group_rows, B, H, _lib.current_stream())
    assert rc == 0
    torch.cuda.synchronize()
    if with_bias:
        act64, (h64, c64, hn64) = d.act64, (d.h64, d.c64, d.hn64)
    else:
        act64 = ref_gates_to_act(d.pre.to(F64), None, 1)
        h64, c64, hn64 = ref_cell(act64, d.c_prev.to(F64), d.keep.to(F64), d.keep_next.to(F64))
    _close("h", h, h64, TOL_FWD32, lowp)
    _close("c", c, c64, TOL_FWD32, False)
    if with_act:
        _close("act", act, act64, TOL_FWD32, lowp)
    if with_next:
        _close("h_next", nxt[:, KX:KX + H], hn64, TOL_FWD32, lowp)
        assert bool((nxt[:, :KX] == SENT).all()) and bool((nxt[:, KX + H:] == SENT).all())


def _run_seq_bwd(entry, d, rpb, inner, inplace):
    lib, H, B, lowp = _lib.load(), d.H, d.B, d.dtype == BF
    from_pre, use_ws = entry.startswith("pre"), entry in ("bsum", "pre_ws")
    saved = (d.pre if from_pre else d.act).cuda().clone()
    dg = saved if inplace else torch.full_like(saved, SENT)
    dcp = torch.full((B, H), SENT, device="cuda")
    c_prev, c_new, keep, dh, bias = d.c_prev.cuda(), d.c_new.cuda(), d.keep.cuda(), d.dh.cuda(), d.bias.cuda()
    dh2buf, k2, dcn = (d.dh2buf.cuda(), d.dh2_keep.cuda(), d.dc_next.cuda()) if inner else (None, None, None)
    nblk = (B + rpb - 1) // rpb if use_ws else 0
    ws = torch.full((nblk, 4 * H), SENT, device="cuda") if use_ws else None
    common = (_p(c_prev), _p(keep), _p(c_new), _p(dh), _p(dh2buf, KX) if inner else None, KX + H + 8 if inner else 0, _p(k2), _p(dcn),
              _p(dg), _p(dcp))
    tail = (B, H, _lib.current_stream())
    if entry == "bwd":
        rc = lib.fdyn_lstm_seq_bwd(_p(saved), int(lowp), *common, *tail)
    elif entry == "bsum":
        rc = lib.fdyn_lstm_seq_bwd_bsum(_p(saved), int(lowp), *common, _p(ws), rpb, *tail)
    else:
        rc = lib.fdyn_lstm_seq_bwd_pre(_p(saved), int(lowp), _p(bias), d.group_rows, *common, _p(ws), rpb if use_ws else 0, *tail)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return dg, dcp, ws


def _check_bias_rows(ws, dgates, rpb):
    """Each block's partial row = the fp64 column sum of the STORED dgates rows of that block, within the fp32 summation bound
    n 2^-23 sum|x| (n rows in the block); a surviving sentinel (a ragged last block not fully written) fails it."""
    ws, dg = _wide(ws), _wide(dgates)
    B = dg.shape[0]
    assert ws.shape[0] == (B + rpb - 1) // rpb
    for b in range(ws.shape[0]):
        rows = dg[b * rpb:min(B, (b + 1) * rpb)]
        bound = rows.shape[0] * 2.0 ** -23 * rows.abs().sum(0)
        over = (ws[b] - rows.sum(0)).abs() - bound
        assert float(over.max()) <= 0.0, ("bias partial row", b, "rows", rows.shape[0], "column", int(over.argmax()))


_BWD_CASES = ([("bwd", H, B, 0) for H, B in ((256, 37), (256, 300), (64, 130), (40, 19))] +
              [("pre", H, B, 0) for H, B in ((256, 37), (256, 300), (64, 130), (40, 19))] +
              [(e, H, B, r) for e in ("bsum", "pre_ws") for H, B, r in ((256, 37, 8), (256, 37, 32), (256, 300, 128), (64, 130, 128))])


@gpu
@pytest.mark.parametrize("inner", [False, True], ids=["last_step", "inner_step"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("entry,H,B,rpb", _BWD_CASES, ids=[f"{e}-H{H}-B{B}-rpb{r}" for e, H, B, r in _BWD_CASES])
def test_seq_bwd_step_matches_fp64(entry, H, B, rpb, dtype, inner):
    """fdyn_lstm_seq_bwd / _bwd_bsum / _bwd_pre (bias_ws NULL and given), last-step form (no dh2 / dh2_keep / dc_next) and
    inner-step form (all three, dh2_stride > H): dgates and dc_prev (= keep * ...) element-wise against fp64 autograd, out of
    place and with dgates aliasing the saved gates (bit-equal), and every block's bias partial row."""
    d, lowp = _step_case(H, B, dtype), dtype == BF
    dg64, dcp64 = _step_bwd_ref(H, B, dtype, entry.startswith("pre"), inner)
    dg, dcp, ws = _run_seq_bwd(entry, d, rpb, inner, inplace=False)
    _close("dgates", dg, dg64, TOL_GRAD32, lowp)
    _close("dc_prev", dcp, dcp64, TOL_GRAD32, False)
    dg2, dcp2, ws2 = _run_seq_bwd(entry, d, rpb, inner, inplace=True)
    assert torch.equal(dg2.view(torch.int16 if lowp else torch.int32), dg.view(torch.int16 if lowp else torch.int32))
    assert torch.equal(dcp2, dcp)
    if ws is not None:
        _check_bias_rows(ws, dg, rpb)
        assert torch.equal(ws2, ws)


@gpu
def test_bias_summing_backward_refuses_shapes_without_one_column_per_lane():
    """_bwd_bsum (and _bwd_pre with bias_ws) need 256 % (H / 8) == 0 and whole passes of 256 lanes per block: H = 40 and
    rows_per_block = 12 at H = 256 come back as FDYN_ERR_BAD_SIZE, nothing is launched."""
    lib, st = _lib.load(), _lib.current_stream()
    for H, B, rpb in ((40, 19, 32), (256, 37, 12), (256, 37, 0)):
        d = _step_case(H, B, F32)
        act, pre, dg = d.act.cuda(), d.pre.cuda(), torch.full((B, 4 * H), SENT, device="cuda")
        dcp, ws = torch.full((B, H), SENT, device="cuda"), torch.full((B, 4 * H), SENT, device="cuda")
        c_prev, c_new, keep, dh, bias = d.c_prev.cuda(), d.c_new.cuda(), d.keep.cuda(), d.dh.cuda(), d.bias.cuda()
        common = (_p(c_prev), _p(keep), _p(c_new), _p(dh), None, 0, None, None, _p(dg), _p(dcp))
        assert lib.fdyn_lstm_seq_bwd_bsum(_p(act), 0, *common, _p(ws), rpb, B, H, st) == _lib.FDYN_ERR_BAD_SIZE
        assert lib.fdyn_lstm_seq_bwd_pre(_p(pre), 0, _p(bias), d.group_rows, *common, _p(ws), rpb, B, H, st) == _lib.FDYN_ERR_BAD_SIZE
        torch.cuda.synchronize()
        assert bool((dg == SENT).all()) and bool((dcp == SENT).all()) and bool((ws == SENT).all())


# ---- the zero-state cell in the three-gate layout ---------------------------------------------------------------------------

def ref_cell0(act):
    ai, ag, ao = act.chunk(3, -1)
    return ao * torch.tanh(ai * ag)


@functools.lru_cache(maxsize=None)
def _cell0_case(H, B, dtype):
    g = torch.Generator().manual_seed(77 * H + B)
    d = types.SimpleNamespace(H=H, B=B, dtype=dtype)
    d.pre = (torch.randn(B, 3 * H, generator=g, dtype=F64) * 1.5 + 0.2).to(dtype)
    d.dh = torch.randn(B, H, generator=g, dtype=F64).to(dtype)
    i, gg, o = d.pre.to(F64).chunk(3, -1)
    d.act64 = torch.cat([torch.sigmoid(i), torch.tanh(gg), torch.sigmoid(o)], -1)
    d.h64 = ref_cell0(d.act64)
    d.act = d.act64.to(dtype)
    a = d.act.to(F64).requires_grad_()                                          # c = i * g is rebuilt from the stored gates
    (ga,) = torch.autograd.grad((ref_cell0(a) * d.dh.to(F64)).sum(), [a])
    ai, ag, ao = a.detach().chunk(3, -1)
    d.dg64 = ga * torch.cat([ai * (1 - ai), 1 - ag * ag, ao * (1 - ao)], -1)
    return d


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,B,rpb", [(256, 37, 32), (256, 300, 128)])
def test_cell0_step_matches_fp64(H, B, rpb, dtype):
    """fdyn_lstm_cell0_fwd / _bwd (three gates, zero state): h and the activated gates, then dgates with and without the bias
    partial rows, each out of place and in place (bit-equal)."""
    d, lib, lowp, st = _cell0_case(H, B, dtype), _lib.load(), dtype == BF, _lib.current_stream()
    bits = torch.int16 if lowp else torch.int32
    outs = []
    for inplace in (False, True):
        gates = d.pre.cuda().clone()
        h = torch.full((B, H), SENT, dtype=dtype, device="cuda")
        act = gates if inplace else torch.full_like(gates, SENT)
        assert lib.fdyn_lstm_cell0_fwd(_p(gates), int(lowp), _p(h), _p(act), B, H, st) == 0
        torch.cuda.synchronize()
        _close("h", h, d.h64, TOL_FWD32, lowp)
        _close("act", act, d.act64, TOL_FWD32, lowp)
        outs.append((h, act))
    assert torch.equal(outs[0][0].view(bits), outs[1][0].view(bits)) and torch.equal(outs[0][1].view(bits), outs[1][1].view(bits))
    h = torch.full((B, H), SENT, dtype=dtype, device="cuda")
    gates = d.pre.cuda()
    assert lib.fdyn_lstm_cell0_fwd(_p(gates), int(lowp), _p(h), None, B, H, st) == 0          # act_out is optional
    torch.cuda.synchronize()
    assert torch.equal(h.view(bits), outs[0][0].view(bits)) and torch.equal(gates, d.pre.cuda())
    dh, first = d.dh.cuda(), None
    for use_ws in (False, True):
        for inplace in (False, True):
            act = d.act.cuda().clone()
            dg = act if inplace else torch.full_like(act, SENT)
            ws = torch.full(((B + rpb - 1) // rpb, 3 * H), SENT, device="cuda") if use_ws else None
            assert lib.fdyn_lstm_cell0_bwd(_p(act), int(lowp), _p(dh), _p(dg), _p(ws), rpb if use_ws else 0, B, H, st) == 0
            torch.cuda.synchronize()
            _close("dgates", dg, d.dg64, TOL_GRAD32, lowp)
            if use_ws:
                _check_bias_rows(ws, dg, rpb)
            first = dg if first is None else first
            assert torch.equal(dg.view(bits), first.view(bits))


# ---- 2. fdyn_colsum_partials --------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("N", [1024, 768, 40])
@pytest.mark.parametrize("nb", [1, 7, 64, 65, 1000])
def test_colsum_partials_matches_fp64(nb, N):
    """The reduction of the bias partial rows (64-row middle stage + final stage) against the fp64 column sum, within the fp32
    summation bound nb 2^-23 sum|x| per column."""
    g = torch.Generator().manual_seed(nb * 4096 + N)
    x = torch.randn(nb, N, generator=g) * 3.0 + 0.5
    part, out = x.cuda(), torch.full((N,), SENT, device="cuda")
    mid = torch.full(((nb + 63) // 64, N), SENT, device="cuda")
    assert _lib.load().fdyn_colsum_partials(_p(part), nb, N, _p(out), _p(mid), _lib.current_stream()) == 0
    torch.cuda.synchronize()
    over = (_wide(out) - x.to(F64).sum(0)).abs() - nb * 2.0 ** -23 * x.to(F64).abs().sum(0)
    assert float(over.max()) <= 0.0, (nb, N, int(over.argmax()))
    assert torch.equal(part, x.cuda())


# ---- 3. fused.lstm_sequence as a node against an fp64 recurrence -------------------------------------------------------------

def ref_sequence(feats, cells, h0, c0, keep):
    """G LSTM cells reading the same feats [T,B,kx] from states h0 / c0 [G,B,H]; keep [T,B] = 0 where an episode starts at that
    step (both states are zeroed before the step).  cells: [(w_ih, w_hh, b_ih, b_hh or None)].  -> h_seq [T,G,B,H],
    c_all [T+1,G,B,H] (c_all[0] = c0).  Works in the dtype of its arguments (float64 in every reference here)."""
    h, c, hs, cs = h0, c0, [], [c0]
    for t in range(feats.shape[0]):
        k = keep[t][None, :, None]
        hm, cm, hn, cn = h * k, c * k, [], []
        for g, (w_ih, w_hh, b_ih, b_hh) in enumerate(cells):
            gates = F.linear(feats[t], w_ih, b_ih) + F.linear(hm[g], w_hh, b_hh)
            i, f, gg, o = gates.chunk(4, -1)
            cg = torch.sigmoid(f) * cm[g] + torch.sigmoid(i) * torch.tanh(gg)
            hn.append(torch.sigmoid(o) * torch.tanh(cg))
            cn.append(cg)
        h, c = torch.stack(hn), torch.stack(cn)
        hs.append(h)
        cs.append(c)
    return torch.stack(hs), torch.stack(cs)


def test_fp64_recurrence_equals_nn_lstm():
    """The reference of this file against torch.nn.LSTM in float64, stepped one step at a time with the state multiplied by
    keep: states and every gradient to 1e-12.  (No GPU needed.)"""
    torch.manual_seed(5)
    T, B, kx, H = 5, 7, 6, 8
    lstm = torch.nn.LSTM(kx, H).to(F64)
    feats = torch.randn(T, B, kx, dtype=F64, requires_grad=True)
    h0, c0 = torch.randn(1, B, H, dtype=F64), torch.randn(1, B, H, dtype=F64)
    keep = (torch.rand(T, B) > 0.3).to(F64)
    keep[:, 0], keep[:, 3] = 1.0, 0.0
    w = torch.randn(T, 1, B, H, dtype=F64)
    wc = torch.randn(T + 1, 1, B, H, dtype=F64)
    h, c, hs, cs = h0, c0, [], [c0]
    for t in range(T):
        k = keep[t][None, :, None]
        _, (h, c) = lstm(feats[t:t + 1], (h * k, c * k))
        hs.append(h)
        cs.append(c)
    ((torch.stack(hs) * w).sum() + (torch.stack(cs) * wc).sum()).backward()
    want = [torch.stack(hs).detach(), torch.stack(cs).detach(), feats.grad.clone()] + [p.grad.clone() for p in lstm.parameters()]
    feats.grad = None
    cell = [p.detach().clone().requires_grad_() for p in (lstm.weight_ih_l0, lstm.weight_hh_l0, lstm.bias_ih_l0, lstm.bias_hh_l0)]
    h_seq, c_all = ref_sequence(feats, [tuple(cell)], h0, c0, keep)
    ((h_seq * w).sum() + (c_all * wc).sum()).backward()
    got = [h_seq.detach(), c_all.detach(), feats.grad] + [p.grad for p in cell]
    for a, b in zip(got, want):
        assert a.shape == b.shape and float((a - b).abs().max()) < 1e-12


SEQ_T, SEQ_B, SEQ_KX, SEQ_H = 5, 72, 128, 256


@functools.lru_cache(maxsize=None)
def _seq_case(G, dtype):
    """Stored operands of the node test (CPU) and the fp64 results from them: {name: tensor}."""
    T, B, kx, H = SEQ_T, SEQ_B, SEQ_KX, SEQ_H
    g = torch.Generator().manual_seed(31 + G)
    r = lambda *s: torch.randn(*s, generator=g)                                  # noqa: E731
    d = types.SimpleNamespace(G=G, dtype=dtype)
    d.feats = (r(T, B, kx) * 0.8).to(dtype)
    d.cells = [(r(4 * H, kx) * 0.08, r(4 * H, H) * 0.06, r(4 * H) * 0.2 + 0.05, r(4 * H) * 0.2 - 0.05) for _ in range(G)]
    d.h0, d.c0 = (r(G, B, H) * 0.5).to(dtype), r(G, B, H) * 0.7
    keep = (torch.rand(T, B, generator=g) > 0.25).to(F32)
    keep[:, 0] = 1.0                                                             # env 0 never restarts
    keep[:, 1], keep[0, 1] = 1.0, 0.0                                            # env 1 restarts at t = 0
    keep[:, 2], keep[T - 1, 2] = 1.0, 0.0                                        # env 2 restarts at t = T - 1
    keep[:, 3] = 0.0                                                             # env 3 restarts at every step
    d.keep = keep
    d.w = r(T, G, B, H).to(dtype)                                                # loss = sum h_seq * w
    feats64 = d.feats.to(F64).requires_grad_()
    leaves = [(wi.to(dtype).to(F64).requires_grad_(), wh.to(dtype).to(F64).requires_grad_(),
               (bi + bh).to(dtype).to(F64).requires_grad_(), None) for wi, wh, bi, bh in d.cells]      # the node adds in fp32, rounds once
    h_seq, c_all = ref_sequence(feats64, leaves, d.h0.to(F64), d.c0.to(F64), keep.to(F64))
    (h_seq * d.w.to(F64)).sum().backward()
    d.ref = {"h_seq": h_seq.detach(), "c_all": c_all.detach(), "dfeats": feats64.grad}
    for k, (wi, wh, b, _) in enumerate(leaves):
        d.ref.update({f"dW_ih{k}": wi.grad, f"dW_hh{k}": wh.grad, f"db_ih{k}": b.grad, f"db_hh{k}": b.grad})
    return d


def _collect(h_seq, c_all, feats, cells):
    out = {"h_seq": _wide(h_seq), "c_all": _wide(c_all), "dfeats": _wide(feats.grad)}
    for k, cell in enumerate(cells):
        out.update({f"d{n}{k}": _wide(p.grad) for n, p in zip(("W_ih", "W_hh", "b_ih", "b_hh"), cell)})
    return out


@functools.lru_cache(maxsize=None)
def _seq_plain(G, dtype):
    """The same recurrence in plain torch on the GPU in the storage dtype, no project kernel: bf16 is rounded where the node
    stores values (the packed input rows, the GEMM's pre-activations, h; the cell state stays fp32, weights and bias are used
    in the storage dtype, their gradients are summed over the steps in fp32)."""
    d = _seq_case(G, dtype)
    feats = d.feats.cuda().requires_grad_()
    cells = [[p.cuda().requires_grad_() for p in cell] for cell in d.cells]
    keep = d.keep.cuda()
    h, c, hs, cs = d.h0.cuda(), d.c0.cuda(), [], [d.c0.cuda()]
    for t in range(SEQ_T):
        hm, cm, hn, cn = h * keep[t][None, :, None].to(dtype), c * keep[t][None, :, None], [], []
        for k, (wi, wh, bi, bh) in enumerate(cells):
            pre = torch.cat([feats[t], hm[k]], 1) @ torch.cat([wi, wh], 1).to(dtype).t()
            gates = pre.float() + (bi + bh).to(dtype).float()
            i, f, gg, o = gates.chunk(4, -1)
            cg = torch.sigmoid(f) * cm[k] + torch.sigmoid(i) * torch.tanh(gg)
            hn.append((torch.sigmoid(o) * torch.tanh(cg)).to(dtype))
            cn.append(cg)
        h, c = torch.stack(hn), torch.stack(cn)
        hs.append(h)
        cs.append(c)
    h_seq, c_all = torch.stack(hs), torch.stack(cs)
    (h_seq.float() * d.w.cuda().float()).sum().backward()
    got = _collect(h_seq, c_all, feats, cells)
    return {n: float((got[n] - d.ref[n]).abs().max()) for n in d.ref}


_SEQ_MODES = [pytest.param(m, dt, id=f"{m}-{n}") for m, dt, n in
              (("pre", F32, "fp32"), ("pre", BF, "bf16"), ("no_pre", F32, "fp32"), ("no_pre", BF, "bf16"), ("mfma_all", BF, "bf16"))]


@gpu
@pytest.mark.parametrize("G", [1, 2])
@pytest.mark.parametrize("mode,dtype", _SEQ_MODES)
def test_lstm_sequence_node_matches_fp64_recurrence(mode, dtype, G, monkeypatch):
    """fused.lstm_sequence (T = 5, B = 72, kx = 128, H = 256; restarts never / at t = 0 / at t = T-1 / at every step) against
    the fp64 recurrence on the same rounded operands, element-wise: h_seq, c_all, dfeats and per cell dW_ih, dW_hh, db_ih,
    db_hh (the two bit-equal).  Modes: the default pre-activation path (fdyn_lstm_seq_bwd_pre), FDYN_NO_PRE=1 (activations
    saved: fdyn_lstm_seq_bwd_bsum for G = 1, fdyn_lstm_seq_bwd for G = 2) and, bf16 only, every forward step through the MFMA
    train cell.

    Bound per element: err <= max(4 e_plain, T x the single-step tolerance of the storage dtype), where e_plain is the largest
    error of the same recurrence in plain torch on the GPU in the storage dtype (_seq_plain).  The factor 4 allows for the fast
    exp / rcp intrinsics and another summation order; the floor keeps a lucky plain run from making the gate impossible.

    Largest err of the node / e_plain over G = 1, 2, measured on an MI355X (every case prints them, pytest -s):
                         h_seq            c_all            dfeats           dW_ih            dW_hh            db
    default  fp32   5.8e-7 / 6.5e-7  1.1e-6 / 1.1e-6  9.1e-7 / 9.2e-7  6.0e-6 / 5.7e-6  4.0e-6 / 4.0e-6  5.2e-6 / 5.8e-6
    default  bf16   3.1e-3 / 3.1e-3  3.2e-3 / 3.2e-3  8.3e-3 / 9.4e-3  3.8e-2 / 5.2e-2  1.4e-2 / 2.3e-2  2.9e-2 / 5.3e-2
    no_pre   fp32   5.8e-7 / 6.5e-7  1.1e-6 / 1.1e-6  9.1e-7 / 9.2e-7  6.0e-6 / 5.7e-6  4.0e-6 / 4.0e-6  5.2e-6 / 5.8e-6
    no_pre   bf16   3.1e-3 / 3.1e-3  3.2e-3 / 3.2e-3  1.1e-2 / 9.4e-3  6.8e-2 / 5.2e-2  2.5e-2 / 2.3e-2  6.4e-2 / 5.3e-2
    mfma_all bf16   2.1e-3 / 3.1e-3  1.0e-3 / 3.2e-3  1.1e-2 / 9.4e-3  5.8e-2 / 5.2e-2  2.2e-2 / 2.3e-2  5.5e-2 / 5.3e-2
    (max |ref|: h 0.87, c 2.9, dfeats 2.0, dW_ih 17, dW_hh 5.2, db 15)
    """
    d = _seq_case(G, dtype)
    e_plain = _seq_plain(G, dtype)
    if mode == "no_pre":
        monkeypatch.setenv("FDYN_NO_PRE", "1")
    else:
        monkeypatch.delenv("FDYN_NO_PRE", raising=False)
    monkeypatch.delenv("FDYN_MFMA_TRAIN", raising=False)
    feats = d.feats.cuda().requires_grad_()
    cells = [[p.cuda().requires_grad_() for p in cell] for cell in d.cells]
    default = fused.MFMA_TRAIN_DEFAULT
    try:
        fused.MFMA_TRAIN_DEFAULT = "all" if mode == "mfma_all" else default
        h_seq, c_all = fused.lstm_sequence(feats, [tuple(c) for c in cells], d.h0.cuda(), d.c0.cuda(), d.keep.cuda())
        (h_seq.float() * d.w.cuda().float()).sum().backward()
        torch.cuda.synchronize()
    finally:
        fused.MFMA_TRAIN_DEFAULT = default
    assert h_seq.dtype == dtype and c_all.dtype == F32 and h_seq.shape == (SEQ_T, G, SEQ_B, SEQ_H)
    got, lowp, failed = _collect(h_seq, c_all, feats, cells), dtype == BF, []
    for n, ref in d.ref.items():
        err = (got[n] - ref).abs()
        floor = SEQ_T * _step_tol(ref, TOL_FWD32 if n in ("h_seq", "c_all") else TOL_GRAD32, lowp)
        print(f"MEASURE seq mode={mode} dtype={'bf16' if lowp else 'fp32'} G={G} {n}: err={float(err.max()):.3e} "
              f"e_plain={e_plain[n]:.3e} max|ref|={float(ref.abs().max()):.3e}")
        if not bool((err <= torch.clamp(floor, min=4.0 * e_plain[n])).all()) or not bool(torch.isfinite(got[n]).all()):
            failed.append((n, float(err.max()), e_plain[n]))
    assert not failed, failed
    for k, cell in enumerate(cells):
        assert torch.equal(cell[2].grad, cell[3].grad), k


# ---- 4. the output heads ----------------------------------------------------------------------------------------------------

LOG_STD = [0.0, -0.5, 0.3, -1.0]
HEAD_SEED, HEAD_STEP = 1234, 5


@functools.lru_cache(maxsize=None)
def _heads_case(B):
    """Head operands with O(1) results: every row of Wa scaled differently, all entries of ba distinct."""
    g = torch.Generator().manual_seed(900 + B)
    r = lambda *s: torch.randn(*s, generator=g)                                  # noqa: E731
    d = types.SimpleNamespace(B=B)
    d.Wa = (r(4, 64) * 0.1 * torch.tensor([0.5, 1.0, 1.7, 2.6])[:, None]).to(BF)
    d.ba = torch.tensor([0.3, -0.7, 1.1, -0.2]).to(BF)
    d.wv, d.bv = (r(64) * 0.2).to(BF), torch.tensor([0.45]).to(BF)
    d.lat = [(r(B, 64) * 0.7 + 0.3).to(BF) for _ in range(2)]                    # heads alone: the two hidden inputs
    # trunks, as test_policy_trunks_kernel_matches_plain_torch_fp32 feeds them
    d.h = [(r(B, 256) * 0.6).to(BF) for _ in range(2)]
    d.W1, d.b1 = (r(2, 128, 256) * 0.08).to(BF), r(2, 128) * 0.2
    d.W2, d.b2 = (r(2, 64, 128) * 0.1).to(BF), r(2, 64) * 0.2
    d.trunk_lat64 = []
    for k in range(2):
        mid = torch.relu(d.h[k].to(F64) @ d.W1[k].to(F64).t() + d.b1[k].to(F64)).to(BF).to(F64)
        d.trunk_lat64.append(torch.relu(mid @ d.W2[k].to(F64).t() + d.b2[k].to(F64)))
    return d


def _heads_ref(d, lat_pi, lat_vf):
    """fp64 means [B,4] / values [B] of the heads and sum|terms| of each output (the 64 products and the bias)."""
    Wa, ba, wv, bv = d.Wa.to(F64), d.ba.to(F64), d.wv.to(F64), d.bv.to(F64)
    mean, value = lat_pi @ Wa.t() + ba, lat_vf @ wv + bv
    return mean, value, lat_pi.abs() @ Wa.abs().t() + ba.abs(), lat_vf.abs() @ wv.abs() + bv.abs()


def _gaussian_head_z(mean64, B):
    """z of fdyn_gaussian_head run on the fp32 reference means with the heads' Philox key, and its logp."""
    mean32, ls = mean64.to(F32).cuda().contiguous(), torch.tensor(LOG_STD, device="cuda")
    step = torch.full((1,), HEAD_STEP, dtype=torch.int32, device="cuda")
    a, lp = torch.full((B, 4), SENT, device="cuda"), torch.full((B,), SENT, device="cuda")
    assert _lib.load().fdyn_gaussian_head(_p(mean32), 0, _p(ls), HEAD_SEED, _p(step), 0, _p(a), _p(lp), B, _lib.current_stream()) == 0
    torch.cuda.synchronize()
    return (_wide(a) - _wide(mean32)) / torch.tensor(LOG_STD, dtype=F64).exp(), _wide(lp)


def _logp_closed_form(z):
    return (-0.5 * z ** 2 - torch.tensor(LOG_STD, dtype=F64) - 0.5 * math.log(2 * math.pi)).sum(1)


@gpu
@pytest.mark.parametrize("B", [257, 300])
def test_policy_heads_match_fp64_dot_products(B):
    """fdyn_policy_heads at visible means.  Deterministic: actions (= means) and value against the fp64 dot products of the
    bf16-rounded operands within the bound of a 64-term fp32 sum, 64 2^-23 sum|terms|.  Sampled: (actions - mean_ref) / std
    equals the same quantity of fdyn_gaussian_head on mean_ref (same Philox key) to 1e-5, logp its closed form to 1e-3."""
    d, lib, st = _heads_case(B), _lib.load(), _lib.current_stream()
    dev = [t.cuda() for t in (d.lat[0], d.lat[1], d.Wa, d.ba, d.wv, d.bv)]
    ls = torch.tensor(LOG_STD, device="cuda")
    step = torch.full((1,), HEAD_STEP, dtype=torch.int32, device="cuda")
    mean64, value64, mabs, vabs = _heads_ref(d, d.lat[0].to(F64), d.lat[1].to(F64))
    assert float(mean64.abs().max()) > 1.0 and float(mean64.std(0).min()) > 0.1               # visible means
    out = {}
    for det in (1, 0):
        a, lp, v = (torch.full(s, SENT, device="cuda") for s in ((B, 4), (B,), (B,)))
        assert lib.fdyn_policy_heads(*(_p(t) for t in dev), _p(ls), HEAD_SEED, _p(step), det, _p(a), _p(lp), _p(v), B, st) == 0
        torch.cuda.synchronize()
        out[det] = (_wide(a), _wide(lp), _wide(v))
        assert float(((out[det][2] - value64).abs() - 64 * 2.0 ** -23 * vabs).max()) <= 0.0
    over = (out[1][0] - mean64).abs() - 64 * 2.0 ** -23 * mabs
    assert float(over.max()) <= 0.0, ("mean", int(over.argmax()))
    z_ref, lp_ref = _gaussian_head_z(mean64, B)
    z = (out[0][0] - mean64) / torch.tensor(LOG_STD, dtype=F64).exp()
    assert float((z - z_ref).abs().max()) < 1e-5 and float(z.std()) > 0.5                     # same noise, really sampled
    assert float((out[0][1] - _logp_closed_form(z)).abs().max()) < 1e-3 and float((out[0][1] - lp_ref).abs().max()) < 1e-3


@gpu
@pytest.mark.parametrize("B", [257, 300])
def test_policy_trunks_heads_match_fp64(B):
    """fdyn_policy_trunks_heads: the heads behind the two trunks, against fp64 on the bf16-rounded operands with the trunk
    output rounded to bf16 as the kernel keeps it.  Bound: the trunk kernel's own tolerance (2e-2 max(1, max|lat|) per element
    of lat) carried through the 64-term sum, plus the fp32 bound of that sum.  Sampled: its noise (sampled - deterministic
    actions, over std) equals fdyn_gaussian_head's for the same key to 1e-5, logp the closed form to 1e-3."""
    from hcrl_amd.policy import _KPERM16
    d, lib, st = _heads_case(B), _lib.load(), _lib.current_stream()
    perm = torch.tensor([16 * (k // 16) + _KPERM16[k % 16] for k in range(128)])
    dev = [t.cuda().contiguous() for t in (d.h[0], d.h[1], d.W1, d.b1, d.W2[:, :, perm], d.b2, d.Wa, d.ba, d.wv, d.bv)]
    ls = torch.tensor(LOG_STD, device="cuda")
    step = torch.full((1,), HEAD_STEP, dtype=torch.int32, device="cuda")
    lat = [t.to(BF).to(F64) for t in d.trunk_lat64]
    mean64, value64, mabs, vabs = _heads_ref(d, lat[0], lat[1])
    assert float(mean64.abs().max()) > 1.0 and float(mean64.std(0).min()) > 0.1
    dl = [2e-2 * max(1.0, float(t.abs().max())) for t in d.trunk_lat64]
    tol_m = dl[0] * d.Wa.to(F64).abs().sum(1)[None, :] + 64 * 2.0 ** -23 * mabs
    tol_v = dl[1] * float(d.wv.to(F64).abs().sum()) + 64 * 2.0 ** -23 * vabs
    out = {}
    for det in (1, 0):
        a, lp, v = (torch.full(s, SENT, device="cuda") for s in ((B, 4), (B,), (B,)))
        assert lib.fdyn_policy_trunks_heads(*(_p(t) for t in dev), _p(ls), HEAD_SEED, _p(step), det, _p(a), _p(lp), _p(v), B, st) == 0
        torch.cuda.synchronize()
        out[det] = (_wide(a), _wide(lp), _wide(v))
        assert float(((out[det][2] - value64).abs() - tol_v).max()) <= 0.0
    over = (out[1][0] - mean64).abs() - tol_m
    assert float(over.max()) <= 0.0, ("mean", int(over.argmax()))
    z_ref, _ = _gaussian_head_z(mean64, B)
    z = (out[0][0] - out[1][0]) / torch.tensor(LOG_STD, dtype=F64).exp()
    assert float((z - z_ref).abs().max()) < 1e-5 and float(z.std()) > 0.5
    assert float((out[0][1] - _logp_closed_form(z_ref)).abs().max()) < 1e-3


# ---- 5. fdyn_ppo_loss and fdyn_gae at edge sizes ---------------------------------------------------------------------------

PPO_CLIP, PPO_VF_COEF, PPO_ENT_COEF = 0.2, 0.5, 0.01


def ref_ppo(mean, values, log_std, actions, old_logp, adv, ret, old_values, normalize_adv, clip_range, clip_range_vf, vf_coef,
            ent_coef):
    """The loss of stable-baselines3's PPO.train for one minibatch of a diagonal-Gaussian policy, restated on float64 tensors.
    -> loss, the library's nine statistics (policy loss, value loss, approx KL, clip fraction, policy + vf_coef value,
    d policy loss / d log_std [4]), dmean, dvalues, dlog_std."""
    mean, values, log_std = (t.detach().clone().requires_grad_() for t in (mean, values, log_std))
    logp = (-((actions - mean) ** 2) / (2 * (2 * log_std).exp()) - log_std - 0.5 * math.log(2 * math.pi)).sum(-1)
    if normalize_adv and adv.numel() > 1:
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    ratio = torch.exp(logp - old_logp)
    pl = -torch.min(adv * ratio, adv * torch.clamp(ratio, 1 - clip_range, 1 + clip_range)).mean()
    vp = values if clip_range_vf is None else old_values + torch.clamp(values - old_values, -clip_range_vf, clip_range_vf)
    vl = F.mse_loss(ret, vp)
    entropy_loss = -(0.5 + 0.5 * math.log(2 * math.pi) + log_std).sum()
    loss = pl + ent_coef * entropy_loss + vf_coef * vl
    (dls_pl,) = torch.autograd.grad(pl, [log_std], retain_graph=True)
    loss.backward()
    with torch.no_grad():
        kl = ((ratio - 1) - (logp - old_logp)).mean()
        cf = ((ratio - 1).abs() > clip_range).to(F64).mean()
        stats = torch.cat([torch.stack([pl, vl, kl, cf, pl + vf_coef * vl]), dls_pl])
    return loss.detach(), stats, mean.grad, values.grad, log_std.grad, ratio.detach()


@functools.lru_cache(maxsize=None)
def _ppo_case(M, mu=0.5, sigma=3.0):
    """fp32 operands of one slice; no sample within 1e-4 of a clip edge (a tie could flip a branch between precisions)."""
    g = torch.Generator().manual_seed(17 + M + int(mu))
    r = lambda *s: torch.randn(*s, generator=g)                                  # noqa: E731
    d = types.SimpleNamespace(M=M)
    d.mean = r(M, 4) * 0.3
    d.act = (d.mean + 0.5 * r(M, 4)).clamp(-1, 1)
    d.log_std = torch.tensor([-0.7, -0.2, 0.1, -1.0])
    d.values, d.ret = r(M), r(M)
    d.adv = r(M) * sigma + mu
    d.old_v = d.values + 0.3 * r(M)
    logp = (-((d.act - d.mean) ** 2) / (2 * (2 * d.log_std).exp()) - d.log_std - 0.5 * math.log(2 * math.pi)).sum(-1)
    d.old_logp = logp + 0.2 * r(M)

    def edge_distance():
        ratio = torch.exp((-((d.act.to(F64) - d.mean.to(F64)) ** 2) / (2 * (2 * d.log_std.to(F64)).exp()) - d.log_std.to(F64)
                           - 0.5 * math.log(2 * math.pi)).sum(-1) - d.old_logp.to(F64))
        return (torch.minimum((ratio - (1 - PPO_CLIP)).abs(), (ratio - (1 + PPO_CLIP)).abs()),
                ((d.values.to(F64) - d.old_v.to(F64)).abs() - 0.2).abs())
    for _ in range(20):                                                          # move the few samples that sit near an edge
        er, ev = edge_distance()
        if float(er.min()) > 1e-3 and float(ev.min()) > 1e-3:
            break
        d.old_logp = torch.where(er <= 1e-3, d.old_logp + 0.01, d.old_logp)
        d.old_v = torch.where(ev <= 1e-3, d.old_v + 0.01, d.old_v)
    er, ev = edge_distance()
    assert float(er.min()) > 1e-4 and float(ev.min()) > 1e-4
    return d


def _ppo_gpu(d, normalize_adv, clip_vf, adv=None):
    m, v, ls = (t.cuda().clone().requires_grad_() for t in (d.mean, d.values, d.log_std))
    args = (d.act.cuda(), d.old_logp.cuda(), (d.adv if adv is None else adv).cuda(), d.ret.cuda(), d.old_v.cuda(), normalize_adv,
            PPO_CLIP, clip_vf, PPO_VF_COEF, PPO_ENT_COEF)
    loss, st4 = fused.ppo_loss(m, v, ls, *args)
    loss.backward()
    with torch.no_grad():
        loss9, st9 = fused._PPOLossFn.apply(m.detach(), v.detach(), ls.detach(), *args)       # all nine statistics
    torch.cuda.synchronize()
    # two launches, whose block sums meet in atomics in another order each: not bit-equal, each goes to the reference
    return _wide(loss), _wide(st9), _wide(m.grad), _wide(v.grad), _wide(ls.grad), _wide(loss9), _wide(st4)


@gpu
@pytest.mark.parametrize("normalize_adv", [True, False])
@pytest.mark.parametrize("clip_vf", [None, 0.2])
@pytest.mark.parametrize("M", [1, 2, 255, 257, 1000, 4099])
def test_ppo_loss_matches_fp64_at_edge_sizes(M, clip_vf, normalize_adv):
    """fused.ppo_loss on CUDA tensors at sub-block and ragged M (the launcher floors M / 256 blocks and strides; at M = 1 SB3
    leaves the advantage un-normalised) against the fp64 restatement of SB3's loss: loss, the nine statistics, dmean, dvalues, dlog_std (rtol 2e-4; atol 2e-6 gradients, 2e-5
    the rest: test_fused_ppo_loss_and_colsum_match_torch's figures)."""
    d = _ppo_case(M)
    w = lambda t: t.to(F64)                                                      # noqa: E731
    ref = ref_ppo(w(d.mean), w(d.values), w(d.log_std), w(d.act), w(d.old_logp), w(d.adv), w(d.ret), w(d.old_v), normalize_adv,
                  PPO_CLIP, clip_vf, PPO_VF_COEF, PPO_ENT_COEF)
    got = _ppo_gpu(d, normalize_adv, clip_vf)
    pairs = list(zip(got[:5], ref[:5], ("loss", "stats", "dmean", "dvalues", "dlog_std")))
    pairs += [(got[5], ref[0], "loss (second launch)"), (got[6], ref[1][:4], "stats (fused.ppo_loss)")]
    for a, b, name in pairs:
        assert torch.allclose(a, b, rtol=2e-4, atol=2e-6 if name.startswith("d") else 2e-5), (name, float((a - b).abs().max()))


@gpu
@pytest.mark.parametrize("mu", [0.0, 10.0, 100.0])
def test_ppo_loss_advantage_offset(mu):
    """Advantage normalisation when |mean| >> std (M = 65 536, adv = mu + randn): dmean and the policy loss against fp64.
    Bound per element: max(4 e_plain, 2e-4 |ref|), e_plain = the largest error of the same fp64 formulas fed with plain two-pass
    fp32 torch (adv - adv.mean()) / (adv.std() + 1e-8).

    The kernels take the moments about the pivot adv[0]; about zero (as they did before), sum a^2 - M mean^2 cancels in fp32 at
    mu = 100 (sum a^2 ~ 6.6e8, one fp32 ulp of it is 64, the wanted M - 1 = 65 535 times the variance sits below it in 10 bits).
    Largest error on an MI355X, moments about zero (the kernels before the pivot; they fail this test at mu = 10 and 100) ->
    about adv[0], and e_plain (every case prints them, pytest -s):
      mu = 0    dmean 4.1e-10 -> 3.7e-10 (e_plain 2.2e-11)   policy loss 9.9e-9 -> 6.1e-8 (e_plain 1.5e-8)
      mu = 10   dmean 2.1e-8  -> 5.2e-10 (e_plain 2.3e-11)   policy loss 4.3e-6 -> 2.0e-7 (e_plain 3.4e-8)
      mu = 100  dmean 2.0e-7  -> 3.8e-10 (e_plain 2.1e-9)    policy loss 7.4e-5 -> 3.8e-8 (e_plain 7.5e-6)
    (max |ref|: dmean 5e-4, policy loss 1.3e-2)"""
    M = 65536
    d = _ppo_case(M, mu=mu, sigma=1.0)
    w = lambda t: t.to(F64)                                                      # noqa: E731
    others = (w(d.mean), w(d.values), w(d.log_std), w(d.act), w(d.old_logp))
    tail = (w(d.ret), w(d.old_v))
    ref = ref_ppo(*others, w(d.adv), *tail, True, PPO_CLIP, None, PPO_VF_COEF, PPO_ENT_COEF)
    a32 = (d.adv - d.adv.mean()) / (d.adv.std() + 1e-8)                          # plain two-pass fp32
    plain = ref_ppo(*others, w(a32), *tail, False, PPO_CLIP, None, PPO_VF_COEF, PPO_ENT_COEF)
    got = _ppo_gpu(d, True, None)
    failed = []
    for name, g_, r_, p_ in (("dmean", got[2], ref[2], plain[2]), ("policy_loss", got[1][0], ref[1][0], plain[1][0])):
        err, e_plain = (g_ - r_).abs(), float((p_ - r_).abs().max())
        print(f"MEASURE offset mu={mu:g} {name}: err={float(err.max()):.3e} e_plain={e_plain:.3e} max|ref|={float(r_.abs().max()):.3e}")
        if not bool((err <= torch.clamp(2e-4 * r_.abs(), min=4.0 * e_plain)).all()):
            failed.append((name, float(err.max()), e_plain))
    assert not failed, failed


def ref_gae(rew, val, starts, last_val, last_done, gamma, lam):
    T = rew.shape[0]
    adv, run = torch.zeros_like(rew), torch.zeros_like(last_val)
    for t in range(T - 1, -1, -1):
        nonterm, next_v = (1.0 - last_done, last_val) if t == T - 1 else (1.0 - starts[t + 1], val[t + 1])
        run = rew[t] + gamma * next_v * nonterm - val[t] + gamma * lam * nonterm * run
        adv[t] = run
    return adv, adv + val


@gpu
@pytest.mark.parametrize("flags", ["random", "starts_ones", "starts_zeros", "last_dones_ones"])
@pytest.mark.parametrize("T,N", [(1, 1), (1, 257), (64, 255), (3, 1000)])
def test_gae_matches_fp64_loop_at_edge_shapes(T, N, flags):
    """compute_gae on CUDA (fdyn_gae) against an fp64 loop: one step, one env, ragged and sub-block N, every env restarting at
    every step / never / all done after the last step.  1e-4 max(1, max|ref|), test_fused_gae_matches_torch_loop's figure."""
    from hcrl_amd.ppo import compute_gae
    g = torch.Generator().manual_seed(T * 10007 + N)
    rew, val = torch.randn(T, N, generator=g) - 0.4, torch.randn(T, N, generator=g) + 0.3
    st = (torch.rand(T, N, generator=g) < 0.1).to(F32)
    lv, ld = torch.randn(N, generator=g), (torch.rand(N, generator=g) < 0.3).to(F32)
    if flags == "starts_ones":
        st = torch.ones(T, N)
    elif flags == "starts_zeros":
        st = torch.zeros(T, N)
    elif flags == "last_dones_ones":
        ld = torch.ones(N)
    a_ref, r_ref = ref_gae(*(t.to(F64) for t in (rew, val, st, lv, ld)), 0.99, 0.95)
    a, r = compute_gae(rew.cuda(), val.cuda(), st.cuda(), lv.cuda(), ld.cuda(), 0.99, 0.95)
    torch.cuda.synchronize()
    assert a.shape == (T, N) and r.shape == (T, N)
    assert float((_wide(a) - a_ref).abs().max()) <= 1e-4 * max(1.0, float(a_ref.abs().max()))
    assert float((_wide(r) - r_ref).abs().max()) <= 1e-4 * max(1.0, float(r_ref.abs().max()))

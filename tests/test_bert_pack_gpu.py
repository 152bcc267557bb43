"""The padding-free bert_large route on the GPU: K30 ``bert_pack_plan``, the
packed embedding LayerNorm and the logit unpack (csrc/kernels/bert_pack.hip),
K12v ``attention_packed`` (csrc/kernels/bert.hip), ``BertLargeQA.forward_packed``
and the served ``bert_large`` with ``TCAMD_BERT_PACKED=1``.

K12v's roundings are K12's (P to bf16 for the PV MFMA under an unrounded l,
the output to bf16), so it is held to K12's derived elementwise bound
``2 * 2^-9 * (A + |ref|) + 1e-6`` and to a rel-L2 below 1e-2 per (row, head,
32-query block), with the helpers of tests/test_bert_kernel_edges_gpu.py.  The
reference is the fp64 softmax of each row over its own keys.

Poisoned neighbours: every query of every row carries ``Q[u] = 4`` along one
shared component ``u`` and every even row's keys 0 there; the odd rows' keys
are ``1000 * u`` and their values 3e4, so a key leaked from a neighbouring row
into an even row scores 500 against valid scores of about 10 (asserted from
the fp64 scores) and is an error thousands of times the bound.  The pad tokens
``[T, t_cap)`` of qkv are NaN, so a read of them shows as NaN; the output is
filled with NaN first, and its pad tokens and the canary rows behind them
must still be NaN afterwards."""

import functools

import numpy as np
import pytest

from tests import bert_pack_cases as cases
from tests.test_bert_kernel_edges_gpu import (D, U_BETA, U_DIM, U_Q, _attn_ref64, _bits, _gen, _k12_bias, _k12_bound,
                                              _report)

torch = pytest.importorskip("torch")

DEV = "cuda"
gpu = pytest.mark.gpu
HEADS = 16
HD = HEADS * D
SCALE = 0.125
CANARY = 0x5A5A5A5A
CANARY_ROWS = 4


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _hip():
    from triton_client_amd.ops import hip

    return hip


# ---------------------------------------------------------------------------
# K30 plan
# ---------------------------------------------------------------------------
def _guarded(n):
    """int32 [n + 8] filled with the canary word; the kernel gets the first n."""
    return torch.full((n + 8,), CANARY, device=DEV, dtype=torch.int32)


def _run_plan(mask_np, t_cap, stride=None):
    hip = _hip()
    rows, s = mask_np.shape
    stride = stride or s
    buf = torch.full((rows, stride), 1, device=DEV, dtype=torch.int32)  # columns past S are valid-looking
    buf[:, :s] = torch.from_numpy(mask_np).to(DEV)
    arrays = [_guarded(rows), _guarded(rows + 1), _guarded(t_cap), _guarded(rows * s)]
    hip.bert_pack_plan(buf.data_ptr(), stride, rows, s, t_cap, *[a.data_ptr() for a in arrays])
    torch.cuda.synchronize()
    sizes = [rows, rows + 1, t_cap, rows * s]
    for a, n, nm in zip(arrays, sizes, ("row_len", "cu", "tok_src", "tok_of")):
        assert (a[n:] == CANARY).all(), "%s: words past the array were written" % nm
    return [a[:n] for a, n in zip(arrays, sizes)]


@gpu
@pytest.mark.parametrize("name,mask,t_cap", cases.plan_cases(), ids=[c[0] for c in cases.plan_cases()])
def test_pack_plan_equals_the_twin(name, mask, t_cap):
    """All four arrays equal the numpy twin on every case (T == t_cap and
    T == t_cap + 1 among them: nothing past t_cap is written, cu keeps the
    true T), canary words behind each array intact; one case also at a row
    stride above S."""
    _need_gpu()
    want = cases.plan_twin(mask, t_cap)
    for stride in (None, mask.shape[1] + 28) if name in ("holes", "s-not-64") else (None,):
        got = _run_plan(mask, t_cap, stride)
        for g, w, nm in zip(got, want, ("row_len", "cu", "tok_src", "tok_of")):
            assert np.array_equal(g.cpu().numpy(), w), "%s (%s, stride %s)" % (nm, name, stride)


def test_pack_plan_refuses_bad_shapes():
    hip = _hip()
    for rows, s, t_cap, stride in [(129, 384, 10, 384), (2, 385, 10, 385), (2, 0, 10, 384), (2, 384, -1, 384),
                                   (2, 384, 10, 383)]:
        with pytest.raises(hip.HipError):
            hip.bert_pack_plan(256, stride, rows, s, t_cap, 256, 256, 256, 256)


# ---------------------------------------------------------------------------
# packed embedding LayerNorm, unpack
# ---------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("H,which", [(1024, "lengths"), (512, "holes"), (1024, "s-not-64")])
def test_packed_embed_is_embed_layernorm_bitwise(H, which):
    """A real token has the bits embed_layernorm gives its (row, position) for
    the wrapped id and the clamped type -- ids negative and far past the
    vocabulary, types negative and past the table among them; a pad token is
    id 0, position 0, type 0, finite; rows past t_cap stay untouched."""
    _need_gpu()
    hip = _hip()
    mask = {c[0]: c[1] for c in cases.plan_cases()}[which]
    rows, s = mask.shape
    n = rows * s
    T = int((mask >= 1).sum())
    t_cap = T + 9
    vocab, ntypes = 50, 3
    g = _gen("embed-packed", H, which)
    word, pos, tok = [(torch.randn(k, H, generator=g)).bfloat16().to(DEV) for k in (vocab, s, ntypes)]
    gamma = (torch.rand(H, generator=g) + 0.5).bfloat16().to(DEV)
    beta = torch.randn(H, generator=g).bfloat16().to(DEV)
    ids = torch.randint(-3 * vocab, 1000 * vocab, (n,), generator=g, dtype=torch.int32)
    tys = torch.randint(-2, ntypes + 3, (n,), generator=g, dtype=torch.int32)
    ids[:4] = torch.tensor([-1, -vocab, vocab, 2 ** 31 - 1], dtype=torch.int32)
    ids, tys = ids.to(DEV), tys.to(DEV)
    _, _, tok_src, _ = cases.plan_twin(mask, t_cap)
    tok_src = torch.from_numpy(tok_src).to(DEV)
    full = torch.empty(n, H, device=DEV, dtype=torch.bfloat16)
    i64, t64 = ids.long().remainder(vocab).contiguous(), tys.long().clamp(0, ntypes - 1).contiguous()
    hip.embed_layernorm(i64.data_ptr(), t64.data_ptr(), word.data_ptr(), pos.data_ptr(), tok.data_ptr(),
                        gamma.data_ptr(), beta.data_ptr(), full.data_ptr(), n, s, H, vocab, ntypes, 1e-12)
    out = torch.full((t_cap + CANARY_ROWS, H), float("nan"), device=DEV, dtype=torch.bfloat16)
    hip.embed_layernorm_packed(ids.data_ptr(), tys.data_ptr(), tok_src.data_ptr(), word.data_ptr(), pos.data_ptr(),
                               tok.data_ptr(), gamma.data_ptr(), beta.data_ptr(), out.data_ptr(), t_cap, n, s, H, vocab,
                               ntypes, 1e-12)
    torch.cuda.synchronize()
    assert torch.isnan(out[t_cap:]).all(), "rows past t_cap were written"
    assert torch.equal(_bits(out[:T]), _bits(full[tok_src[:T].long()])), "real tokens"
    zero = torch.zeros(1, device=DEV, dtype=torch.int64)
    pad = torch.empty(1, H, device=DEV, dtype=torch.bfloat16)
    hip.embed_layernorm(zero.data_ptr(), zero.data_ptr(), word.data_ptr(), pos.data_ptr(), tok.data_ptr(),
                        gamma.data_ptr(), beta.data_ptr(), pad.data_ptr(), 1, s, H, vocab, ntypes, 1e-12)
    torch.cuda.synchronize()
    assert torch.isfinite(out[T:t_cap].float()).all()
    assert torch.equal(_bits(out[T:t_cap]), _bits(pad.expand(t_cap - T, H))), "pad tokens"


@gpu
@pytest.mark.parametrize("which", ["lengths", "holes", "overflow", "empty"])
def test_unpack_is_exact(which):
    """out[r][p] is the packed logit of tok_of[r][p], PAD_LOGIT where it is -1,
    in both planes; canary rows behind both outputs intact."""
    _need_gpu()
    hip = _hip()
    _, mask, t_cap = next(c for c in cases.plan_cases() if c[0] == which)
    rows, s = mask.shape
    _, _, _, tok_of = cases.plan_twin(mask, t_cap)
    g = _gen("unpack", which)
    packed = torch.randn(2, max(t_cap, 1), generator=g).to(DEV)
    tof = torch.from_numpy(tok_of).to(DEV)
    out = torch.full((2, rows + CANARY_ROWS, s), float("nan"), device=DEV)
    hip.unpack_logits(packed[0].data_ptr(), packed[1].data_ptr(), tof.data_ptr(), out[0].data_ptr(), out[1].data_ptr(),
                      rows * s, t_cap)
    torch.cuda.synchronize()
    assert torch.isnan(out[:, rows:]).all(), "rows past the output were written"
    real = (tof >= 0).view(rows, s)
    for k in range(2):
        want = torch.where(real, packed[k][tof.clamp(min=0).long()].view(rows, s),
                           torch.full((), hip.BERT_PAD_LOGIT, device=DEV))
        assert torch.equal(out[k, :rows], want)
    assert (out[:, :rows][:, ~real] == -10000.0).all()


# ---------------------------------------------------------------------------
# K12v
# ---------------------------------------------------------------------------
def _lengths(rows):
    if rows == 12:
        return list(cases.LENGTHS)
    return [cases.LENGTHS[(5 * i + 7) % 12] for i in range(rows)]


@functools.lru_cache(maxsize=None)
def _row_on_device(n, odd, with_bias):
    """One row of ``n`` tokens: (qkv [n][3 * HD] bf16, fp64 ref, A, highest
    valid scaled score, lowest scaled score a key of an odd row would get from
    this row's queries), computed once and never written to afterwards."""
    g = _gen("k12v-row", n, odd)
    qkv = (torch.randn(n, 3, HEADS, D, generator=g) * 1.5).bfloat16()
    qkv[:, 0, :, U_DIM] = U_Q
    qkv[:, 1, :, U_DIM] = 0.0
    if odd:  # the poison: a neighbour's leaked key wins every softmax it enters
        qkv[:, 1] = 0.0
        qkv[:, 1, :, U_DIM] = U_BETA
        qkv[:, 2] = 3e4
    qkv = qkv.reshape(n, 3 * HD).to(DEV)
    bias = _k12_bias(HEADS).to(DEV) if with_bias else None
    ref, a, _, _ = _attn_ref64(qkv, None, HEADS, SCALE, bias)
    q = qkv.view(n, 3, HEADS, D)[:, 0]
    k = qkv.view(n, 3, HEADS, D)[:, 1].double()
    if bias is not None:
        q = (q.float() + bias.view(3, HEADS, D)[0].float()).bfloat16()
    q = q.double()
    hi_valid = (torch.einsum("qhd,khd->hqk", q, k) * SCALE).max().item()
    leak = (q[:, :, U_DIM] * U_BETA * SCALE).min().item()
    return qkv, ref, a, hi_valid, leak


@pytest.fixture(scope="module", autouse=True)
def _drop_shared_rows():
    yield
    _row_on_device.cache_clear()


K12V_CASES = [(1, False, (3, 4)), (5, False, (3, 4)), (5, True, (3, 4)), (7, False, (2, 6)), (12, False, (1, 12)),
              (12, True, (1, 12)), (64, False, (1, 12))]


def test_packed_plan_is_k12s_at_384():
    hip = _hip()
    for rows, _, plan in K12V_CASES:
        assert hip.attention_packed_plan(rows, HEADS) == plan == hip.attention_plan(rows, 384, HEADS)
    assert {hip.attention_packed_plan(r, HEADS) for r in range(1, 129)} == {(3, 4), (2, 6), (1, 12)}
    for bad in [(0, 16), (1, 0)]:
        with pytest.raises(hip.HipError):
            hip.attention_packed_plan(*bad)


@gpu
@pytest.mark.parametrize("rows,with_bias,plan", K12V_CASES,
                         ids=["%d-rows%s-plan%dx%d" % (r, "-bias" if b else "", p[0], p[1]) for r, b, p in K12V_CASES])
def test_k12v_rows_of_every_length_with_poisoned_neighbours(rows, with_bias, plan):
    _need_gpu()
    hip = _hip()
    assert hip.attention_packed_plan(rows, HEADS) == plan
    lens = _lengths(rows)
    parts = [_row_on_device(n, i % 2 == 1, with_bias) if n else None for i, n in enumerate(lens)]
    T = sum(lens)
    t_cap = T + 37
    qkv = torch.full((t_cap, 3 * HD), float("nan"), device=DEV, dtype=torch.bfloat16)
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    for p, t0 in zip(parts, cu):
        if p is not None:
            qkv[t0:t0 + p[0].shape[0]] = p[0]
    # the score precondition: a key leaked from an odd row into an even row beats every valid score by > 200
    for i, p in enumerate(parts):
        if p is not None and i % 2 == 0:
            assert p[4] >= p[3] + 200.0 and p[4] < 2000.0, (i, p[3], p[4])
    row_len = torch.tensor(lens, device=DEV, dtype=torch.int32)
    cu_t = torch.tensor(cu, device=DEV, dtype=torch.int32)
    bias = _k12_bias(HEADS).to(DEV) if with_bias else None
    out = torch.full((t_cap + CANARY_ROWS, HD), float("nan"), device=DEV, dtype=torch.bfloat16)
    hip.attention_packed(qkv.data_ptr(), row_len.data_ptr(), cu_t.data_ptr(), out.data_ptr(), rows, t_cap, HEADS, SCALE,
                         bias=None if bias is None else bias.data_ptr())
    torch.cuda.synchronize()
    assert torch.isnan(out[T:]).all(), "pad tokens or canary rows were written"
    assert torch.isfinite(out[:T].float()).all(), "a token below T is not finite"
    worst_e = worst_r = 0.0
    for i, (p, t0, n) in enumerate(zip(parts, cu, lens)):
        if p is None:
            continue
        _, ref, a, _, _ = p
        got = out[t0:t0 + n].double()
        nb = (n + 31) // 32

        def blk(t):  # [blocks][32][heads][D], zero past the row's end
            z = torch.zeros(nb * 32, HD, device=DEV, dtype=torch.float64)
            z[:n] = t
            return z.view(nb, 32, HEADS, D)

        ratio = blk((got - ref).abs() / _k12_bound(ref, a)).amax((1, 3))
        rel = (blk(got - ref).pow(2).sum((1, 3)) / blk(ref).pow(2).sum((1, 3))).sqrt()
        for name, t, lim in (("elementwise error / bound", ratio, 1.0), ("rel-L2", rel, 1e-2)):
            if (t > lim).any():
                b, h = (t > lim).nonzero()[0].tolist()
                pytest.fail("row %d (len %d, %s) head %d queries %d..%d: %s %.4g > %g" % (
                    i, n, "odd" if i % 2 else "even", h, 32 * b, min(32 * b + 31, n - 1), name, t[b, h].item(), lim))
        worst_e, worst_r = max(worst_e, ratio.max().item()), max(worst_r, rel.max().item())
    _report("K12v %d rows%s plan %s" % (rows, " bias" if with_bias else "", plan), worst_err_over_bound=worst_e,
            worst_block_rel_l2=worst_r)


@gpu
def test_k12v_skips_rows_that_do_not_fit():
    """A row whose tokens would reach past t_cap (a caller's error) is left
    alone: nothing is read or written out of bounds, the other rows are served."""
    _need_gpu()
    hip = _hip()
    p = _row_on_device(65, False, False)
    t_cap = 65
    qkv = p[0].clone()
    row_len = torch.tensor([65, 33], device=DEV, dtype=torch.int32)
    cu = torch.tensor([0, 65, 98], device=DEV, dtype=torch.int32)
    out = torch.full((t_cap + CANARY_ROWS, HD), float("nan"), device=DEV, dtype=torch.bfloat16)
    hip.attention_packed(qkv.data_ptr(), row_len.data_ptr(), cu.data_ptr(), out.data_ptr(), 2, t_cap, HEADS, SCALE)
    torch.cuda.synchronize()
    assert torch.isnan(out[t_cap:]).all() and torch.isfinite(out[:t_cap].float()).all()
    assert ((out[:65].double() - p[1]).abs() <= _k12_bound(p[1], p[2])).all()


# ---------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------
def _rel_l2(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


@gpu
def test_forward_packed_matches_fp32_module_and_padded_forward():
    """bf16, layers=2, the 12 lengths in one batch, ids and types out of range:
    at the valid positions rel-L2 < 5e-2 against the fp32 torch module (the
    bound of test_bert_fused_layers_match_torch_ops) and < 2e-2 against the
    padded bf16 forward (that of test_bert_dense_path_matches_masked_when_no_padding);
    PAD_LOGIT at every other position."""
    _need_gpu()
    from triton_client_amd.models import bert

    m = bert.build(device=DEV, layers=2)
    with torch.no_grad():  # non-zero biases: K12v applies the QKV bias
        for p in m.parameters():
            if p.dim() == 1 and not torch.all(p == 1):
                p.copy_(torch.randn_like(p.float()) * 0.05)
    mask = torch.from_numpy(cases.lengths_mask()).to(DEV)
    rows = mask.shape[0]
    g = _gen("model-packed")
    ids = torch.randint(-50, 2 * bert.VOCAB, (rows, cases.S), generator=g, dtype=torch.int32).to(DEV)
    tt = torch.randint(-1, 4, (rows, cases.S), generator=g, dtype=torch.int32).to(DEV)
    wrapped, clamped = ids.long().remainder(bert.VOCAB), tt.long().clamp(0, 1)
    T = int(mask.sum())
    t_cap = rows * 128
    assert T <= t_cap
    with torch.no_grad():
        got = m.forward_packed(ids, mask, tt, t_cap)
        padded = m(wrapped, mask, clamped)
        ref = bert.build(device=DEV, dtype=torch.float32, layers=2)
        ref.load_state_dict({k: v.float() for k, v in m.state_dict().items()})
        try:
            bert.FUSED = False
            want = ref(wrapped, mask, clamped)
            torch_packed = m.forward_packed(ids, mask, tt, t_cap)  # the torch form of the packed route, in bf16
        finally:
            bert.FUSED = True
    torch.cuda.synchronize()
    valid = mask >= 1
    for k, (g_, p_, w_, tp_) in enumerate(zip(got, padded, want, torch_packed)):
        assert g_.dtype == torch.float32 and g_.shape == (rows, cases.S)
        assert (g_[~valid] == bert.PAD_LOGIT).all() and (tp_[~valid] == bert.PAD_LOGIT).all()
        e32, epad, etorch = _rel_l2(g_[valid], w_[valid]), _rel_l2(g_[valid], p_[valid]), _rel_l2(tp_[valid], w_[valid])
        _report("forward_packed plane %d" % k, vs_fp32=e32, vs_padded=epad, torch_form_vs_fp32=etorch)
        assert e32 < 5e-2 and epad < 2e-2 and etorch < 5e-2, (e32, epad, etorch)


# ---------------------------------------------------------------------------
# served
# ---------------------------------------------------------------------------
NAMES = ("input_ids", "attention_mask", "token_type_ids")


def _small_bert():
    from triton_client_amd.server import gpu_models

    class SmallBert(gpu_models.BertLarge):
        """bert_large with two layers and two row buckets: a few graphs to capture."""

        BUCKETS = (8, 16)

    return SmallBert


@pytest.fixture(scope="module")
def served():
    """{"0" | "1": a loaded two-layer bert_large with TCAMD_BERT_PACKED at that value}."""
    import os

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    cls = _small_bert()
    out = {}
    old = os.environ.get("TCAMD_BERT_PACKED")
    try:
        for knob in ("0", "1"):
            os.environ["TCAMD_BERT_PACKED"] = knob
            out[knob] = cls(layers=2)
            out[knob].load()
    finally:
        if old is None:
            os.environ.pop("TCAMD_BERT_PACKED", None)
        else:
            os.environ["TCAMD_BERT_PACKED"] = old
    yield out
    for m in out.values():
        m.unload()


def _rows(lens, seed):
    """(ids, mask, types) int32 [rows, 384]: a question in segment 0, a context in segment 1."""
    rng = np.random.default_rng(seed)
    n = len(lens)
    ids = rng.integers(1000, 30000, (n, 384)).astype(np.int32)
    mask = cases.prefix_mask(lens)
    tt = np.zeros((n, 384), np.int32)
    for r, ln in enumerate(lens):
        tt[r, min(12, ln):max(ln - 1, 0)] = 1
    return [ids * mask, mask, tt]


def _requests(arrays, split, device=None):
    """bert_large requests of ``split`` rows each; ``device`` = a list that keeps DeviceView inputs alive."""
    from triton_client_amd.server.types import DeviceView, InferRequest, InputTensor

    reqs, first = [], 0
    for n in split:
        ins = []
        for nm, a in zip(NAMES, arrays):
            part = np.ascontiguousarray(a[first:first + n])
            data = part
            if device is not None:
                t = torch.from_numpy(part).to(DEV)
                device.append(t)
                data = DeviceView(t.data_ptr(), part.size * 4, 0)
            ins.append(InputTensor(nm, "INT32", [n, 384], data))
        reqs.append(InferRequest(model_name="bert_large", inputs=ins))
        first += n
    return reqs


def _logits(results):
    """[2][rows][384] from a list of per-request output lists."""
    for r in results:
        assert not isinstance(r, Exception), r
    return np.stack([np.concatenate([np.asarray(r[k].data) for r in results]) for k in range(2)])


def _top2(logits, mask, tt):
    """K27 on [2][rows][384] logits: (spans [rows][2][2], scores [rows][2])."""
    hip = _hip()
    rows = mask.shape[0]
    lg = torch.from_numpy(np.ascontiguousarray(logits)).to(DEV)
    m, t = torch.from_numpy(mask).to(DEV), torch.from_numpy(tt).to(DEV)
    k_row = torch.full((rows,), 2, device=DEV, dtype=torch.int32)
    len_row = torch.full((rows,), 30, device=DEV, dtype=torch.int32)
    spans = torch.zeros(rows, 2, 2, device=DEV, dtype=torch.int32)
    scores = torch.zeros(rows, 2, device=DEV)
    null = torch.zeros(rows, device=DEV)
    hip.qa_spans(lg[0].data_ptr(), lg[1].data_ptr(), 384 * 4, m.data_ptr(), t.data_ptr(), 384 * 4, rows, 384,
                 k_row.data_ptr(), len_row.data_ptr(), 2, spans.data_ptr(), scores.data_ptr(), null.data_ptr())
    torch.cuda.synchronize()
    return spans.cpu().numpy(), scores.cpu().numpy()


SHORT = [100, 37, 128, 64, 90]  # 419 tokens <= 8 * 128


@gpu
def test_served_short_rows_take_a_packed_graph(served):
    """Five short rows: the knob-on model serves them from a packed graph
    (route_counts), its valid logits are within 2e-2 rel-L2 of the knob-off
    model's (two bf16 routes of one model), every other position holds
    PAD_LOGIT, and K27's best span agrees wherever the knob-off best leads its
    runner-up by more than the routes can differ (a span's score is two
    logits, so a gap moves by at most four times the largest logit difference)."""
    arrays = _rows(SHORT, 1)
    on, off = served["1"], served["0"]
    assert on.packed and not off.packed
    assert on.packed_bucket(5, sum(SHORT)) == (8, 128)
    before = dict(on.route_counts), dict(off.route_counts)
    got = _logits(on.execute(_requests(arrays, [2, 3])))
    want = _logits(off.execute(_requests(arrays, [2, 3])))
    assert on.route_counts == {"packed": before[0]["packed"] + 1, "padded": before[0]["padded"]}
    assert off.route_counts == {"packed": 0, "padded": before[1]["padded"] + 1}
    valid = arrays[1] >= 1
    for k in range(2):
        assert (got[k][~valid] == -10000.0).all()
        err = _rel_l2(torch.from_numpy(got[k][valid]), torch.from_numpy(want[k][valid]))
        _report("served packed vs padded plane %d" % k, rel_l2=err)
        assert err < 2e-2, err
    d = float(np.abs(got - want)[:, valid].max())
    s_on, _ = _top2(got, arrays[1], arrays[2])
    s_off, sc_off = _top2(want, arrays[1], arrays[2])
    decided = 0
    for r in range(len(SHORT)):
        if sc_off[r, 0] - sc_off[r, 1] > 4 * d:
            decided += 1
            assert s_on[r, 0].tolist() == s_off[r, 0].tolist(), (r, s_on[r], s_off[r], sc_off[r], d)
    _report("served spans", rows_decided=decided, largest_logit_difference=d)


@gpu
def test_served_full_rows_take_the_padded_graph_bitwise(served):
    """A batch with more than 256 tokens per bucket row fits no packed graph:
    the knob-on model runs the padded graph and answers bit for bit what the
    knob-off model answers."""
    lens = [384, 380, 300, 384, 384, 290, 384, 384]
    arrays = _rows(lens, 2)
    on, off = served["1"], served["0"]
    assert on.packed_bucket(8, sum(lens)) is None
    before = dict(on.route_counts)
    got = _logits(on.execute(_requests(arrays, [8])))
    want = _logits(off.execute(_requests(arrays, [8])))
    assert on.route_counts == {"packed": before["packed"], "padded": before["padded"] + 1}
    assert np.array_equal(got.view(np.int32), want.view(np.int32))


@gpu
def test_served_device_inputs_choose_the_same_bucket(served):
    """The same rows as DeviceViews (what the ensembles hand over) count the
    same tokens on the device: the same packed graph, the same bits."""
    arrays = _rows(SHORT, 1)
    on = served["1"]
    before = dict(on.route_counts)
    host = _logits(on.execute(_requests(arrays, [2, 3])))
    keep = []
    dev = _logits(on.execute(_requests(arrays, [2, 3], device=keep)))
    assert on.route_counts == {"packed": before["packed"] + 2, "padded": before["padded"]}
    assert np.array_equal(host.view(np.int32), dev.view(np.int32))
    # ... and a batch that fits no packed graph, from the device: the padded graph
    full = _rows([384] * 6, 3)
    assert on.packed_bucket(6, 6 * 384) is None
    on.execute(_requests(full, [6], device=keep))
    assert on.route_counts == {"packed": before["packed"] + 2, "padded": before["padded"] + 1}

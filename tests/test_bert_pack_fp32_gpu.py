"""The padding-free route of the fp32-parity ``bert_large_fp32``: K12xv
``attention_f32_packed`` (csrc/kernels/bert.hip), the fp32 packed embedding
LayerNorm (csrc/kernels/bert_pack.hip), ``BertLargeQA.forward_packed`` on the
fp32-parity model and the served ``bert_large_fp32`` with ``TCAMD_BERT_PACKED=1``.

K12xv is K12x's own text over a row geometry, so a valid token must get the
BITS K12x gives it in the same row padded to 384 behind a prefix mask: the
chunk order is the same, a trailing all-masked chunk contributes corr =
exp(0) = 1 and p = exp(-10000 - m) = 0, and the masked keys of the last
partial chunk give 0 whatever finite K / V they hold.  Against fp64 it is
held to K12x's own bound (per-row rel-L2 < 2e-5,
tests/test_bert_kernels_gpu.py::test_attention_f32_matches_fp64).

Poisoned neighbours, as in tests/test_bert_pack_gpu.py: every query carries
``Q[u] = 4`` along one shared component and every clean row's keys 0 there;
a poisoned row's keys are ``1000 * u`` and its values 1e4, so a key leaked
from a neighbour into a clean row scores 500 against valid scores of about 10
and shows as an error far above the bound.  Each row set runs with the odd
rows poisoned and with the even rows poisoned, so that every length is a
clean row once.  The pad tokens ``[T, t_cap)`` of qkv are NaN; the output is
pre-filled with NaN as a canary, which the pad tokens, the rows behind t_cap
and an empty row's (zero-length) span must still hold.

Measured figures: profiles/r23_bert_fp32_packed.md."""

import functools
import os

import numpy as np
import pytest

from tests import bert_pack_cases as cases
from tests import bert_pack_fp32_cases as f32c
from tests.test_bert_accuracy_gpu import FP32_REL
from tests.test_bert_kernel_edges_gpu import D, U_BETA, U_DIM, U_Q, V_POISON, _attn_ref64, _gen, _report

torch = pytest.importorskip("torch")

DEV = "cuda"
gpu = pytest.mark.gpu
HEADS = f32c.HEADS
HD = f32c.HIDDEN
SCALE = 0.125
CANARY_ROWS = 4
K12X_REL = 2e-5   # test_attention_f32_matches_fp64's bound on a row with a valid key
EMBED_REL = 1e-6  # K11p's fp32 bound in test_bert_kernel_edges_gpu.py


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _hip():
    from triton_client_amd.ops import hip

    return hip


# ---------------------------------------------------------------------------
# CPU: the plan, the served model's host side, the routes
# ---------------------------------------------------------------------------
def test_f32_packed_plan_is_k12xs_at_384():
    hip = _hip()
    for rows, want in [(1, 4), (5, 4), (6, 8), (64, 8), (128, 8)]:
        assert hip.attention_f32_packed_plan(rows, HEADS) == want == hip.attention_f32_plan(rows, 384, HEADS)
    for lens, _, waves in f32c.ROW_SETS.values():
        assert hip.attention_f32_packed_plan(len(lens), HEADS) == waves
    for bad in [(0, 16), (1, 0)]:
        with pytest.raises(hip.HipError):
            hip.attention_f32_packed_plan(*bad)


def test_fp32_model_supports_the_packed_route():
    from triton_client_amd.server import gpu_models

    cls = gpu_models.BertLargeFP32
    assert cls.supports_packed is True
    assert max(cls.BUCKETS) == 64 and cls.PACKED_FILL == (128, 256)
    assert cls.packed_bucket(1, 100) == (1, 128)
    assert cls.packed_bucket(1, 129) == (1, 256)
    assert cls.packed_bucket(1, 257) is None
    assert cls.packed_bucket(5, 596) == (8, 128)
    assert cls.packed_bucket(33, 33 * 200) == (40, 256)
    assert cls.packed_bucket(64, 64 * 256) == (64, 256)
    assert cls.packed_bucket(64, 64 * 256 + 1) is None
    assert cls.packed_bucket(65, 65) is None and cls.packed_bucket(0, 0) is None
    for b in cls.BUCKETS:
        for f in cls.PACKED_FILL:
            assert cls.packed_bucket(b, b * f) == (b, f)


def test_every_served_t_cap_is_a_shape_its_x3_route_accepts():
    """The packed forward keys the bf16x3 projections on M = t_cap: no
    (projection, bucket x fill) of the served model falls off its K17 / K18
    route for its shape."""
    from triton_client_amd.models import bert
    from triton_client_amd.server import gpu_models

    cls = gpu_models.BertLargeFP32
    t_caps = sorted({b * f for b in cls.BUCKETS for f in cls.PACKED_FILL})
    assert t_caps[0] == 128 and t_caps[-1] == 64 * 256
    assert bert.packed_x3_route_misses(t_caps) == []


# ---------------------------------------------------------------------------
# K12xv
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _row_f32(n, poisoned):
    """One row of ``n`` tokens: (qkv fp32 [n][3 * HD] on the device, fp64 ref
    [n][HD], highest valid scaled score, lowest scaled score a poisoned row's
    key would get from this row's queries); computed once, never written to."""
    g = _gen("k12xv-row", n, poisoned)
    qkv = torch.randn(n, 3, HEADS, D, generator=g) * 1.5
    qkv[:, 0, :, U_DIM] = U_Q
    qkv[:, 1, :, U_DIM] = 0.0
    if poisoned:
        qkv[:, 1] = 0.0
        qkv[:, 1, :, U_DIM] = U_BETA
        qkv[:, 2] = V_POISON[torch.float32]
    qkv = qkv.reshape(n, 3 * HD).to(DEV)
    ref = _attn_ref64(qkv, None, HEADS, SCALE)[0]
    x = qkv.view(n, 3, HEADS, D).double()
    hi_valid = (torch.einsum("qhd,khd->hqk", x[:, 0], x[:, 1]) * SCALE).max().item()
    leak = (x[:, 0, :, U_DIM] * U_BETA * SCALE).min().item()
    return qkv, ref, hi_valid, leak


@functools.lru_cache(maxsize=None)
def _packed_set(name, flip):
    """(lens, cu, t_cap, parts, qkv [t_cap][3 * HD] with NaN pad tokens) of a row set; row i is poisoned when
    i % 2 != flip."""
    lens, t_cap, _ = f32c.ROW_SETS[name]
    cu = f32c.cu_of(lens)
    parts = [_row_f32(n, i % 2 != flip) if n else None for i, n in enumerate(lens)]
    qkv = torch.full((t_cap, 3 * HD), float("nan"), device=DEV)
    for p, t0 in zip(parts, cu):
        if p is not None:
            qkv[t0:t0 + p[0].shape[0]] = p[0]
    return lens, cu, t_cap, parts, qkv


@pytest.fixture(scope="module", autouse=True)
def _drop_shared_rows():
    yield
    _row_f32.cache_clear()
    _packed_set.cache_clear()


def _run_k12xv(qkv, lens, cu, t_cap, x3=False):
    hip = _hip()
    row_len = torch.tensor(lens, device=DEV, dtype=torch.int32)
    cu_t = torch.tensor(cu, device=DEV, dtype=torch.int32)
    if x3:
        out = torch.full((t_cap + CANARY_ROWS, 3 * HD), float("nan"), device=DEV, dtype=torch.bfloat16)
    else:
        out = torch.full((t_cap + CANARY_ROWS, HD), float("nan"), device=DEV)
    hip.attention_f32_packed(qkv.data_ptr(), row_len.data_ptr(), cu_t.data_ptr(), out.data_ptr(), len(lens), t_cap,
                             HEADS, SCALE, x3=x3)
    torch.cuda.synchronize()
    return out


def _assert_rows_meet_fp64(out, parts, cu, lens, what, skip=()):
    worst = 0.0
    for i, (p, t0, n) in enumerate(zip(parts, cu, lens)):
        if p is None or i in skip:
            continue
        got = out[t0:t0 + n].double()
        assert torch.isfinite(got).all(), "row %d (len %d): not finite" % (i, n)
        err = ((got - p[1]).norm() / p[1].norm()).item()
        worst = max(worst, err)
        assert err < K12X_REL, "row %d (len %d): rel-L2 %.3g" % (i, n, err)
    _report(what, worst_row_rel_l2=worst)


SETS = [(name, flip) for name in f32c.ROW_SETS for flip in (0, 1)]
SET_IDS = ["%s-%s-rows-poisoned" % (n, "even" if f else "odd") for n, f in SETS]


@gpu
@pytest.mark.parametrize("name,flip", SETS, ids=SET_IDS)
def test_k12xv_equals_k12x_bit_for_bit(name, flip):
    """The valid tokens of the packed output, fp32 and bf16x3 operand, are
    torch.equal to K12x's on the rows padded to 384 with finite random pad
    tokens behind a prefix mask; the operand is also bitwise x3_cat of the
    fp32 output."""
    _need_gpu()
    hip = _hip()
    lens, cu, t_cap, parts, qkv = _packed_set(name, flip)
    rows, waves = len(lens), f32c.ROW_SETS[name][2]
    assert hip.attention_f32_packed_plan(rows, HEADS) == waves == hip.attention_f32_plan(rows, 384, HEADS)
    padded = torch.randn(rows, 384, 3 * HD, generator=_gen("k12xv-pad", name)).to(DEV) * 1.5
    for i, (p, n) in enumerate(zip(parts, lens)):
        if p is not None:
            padded[i, :n] = p[0]
    mask = torch.from_numpy(cases.prefix_mask(lens)).to(DEV)
    want = torch.empty(rows * 384, HD, device=DEV)
    want3 = torch.empty(rows * 384, 3 * HD, device=DEV, dtype=torch.bfloat16)
    hip.attention_f32(padded.data_ptr(), mask.data_ptr(), want.data_ptr(), rows, 384, HEADS, SCALE)
    hip.attention_f32(padded.data_ptr(), mask.data_ptr(), want3.data_ptr(), rows, 384, HEADS, SCALE, x3=True)
    got = _run_k12xv(qkv, lens, cu, t_cap)
    got3 = _run_k12xv(qkv, lens, cu, t_cap, x3=True)
    cat3 = torch.empty(t_cap, 3 * HD, device=DEV, dtype=torch.bfloat16)
    hip.x3_cat(got.data_ptr(), cat3.data_ptr(), t_cap, HD)
    torch.cuda.synchronize()
    want, want3 = want.view(rows, 384, HD), want3.view(rows, 384, 3 * HD)
    for i, (t0, n) in enumerate(zip(cu, lens)):
        assert torch.equal(got[t0:t0 + n], want[i, :n]), "fp32 output, row %d (len %d)" % (i, n)
        assert torch.equal(got3[t0:t0 + n], want3[i, :n]), "x3 operand, row %d (len %d)" % (i, n)
        assert torch.equal(got3[t0:t0 + n], cat3[t0:t0 + n]), "x3 operand is not x3_cat, row %d (len %d)" % (i, n)


@gpu
@pytest.mark.parametrize("name,flip", SETS, ids=SET_IDS)
def test_k12xv_against_fp64_with_poisoned_neighbours(name, flip):
    _need_gpu()
    lens, cu, t_cap, parts, qkv = _packed_set(name, flip)
    T = cu[-1]
    # the score precondition: a poisoned row's key leaked into a clean row beats every valid score by > 200
    for i, p in enumerate(parts):
        if p is not None and i % 2 == flip:
            assert p[3] >= p[2] + 200.0 and p[3] < 2000.0, (i, p[2], p[3])
    out = _run_k12xv(qkv, lens, cu, t_cap)
    assert torch.isnan(out[T:]).all(), "pad tokens or canary rows were written"
    assert torch.isfinite(out[:T]).all(), "a token below T is not finite (or an empty row's span is not empty)"
    for i, n in enumerate(lens):  # an empty row's span: nothing between its neighbours' tokens
        assert n > 0 or cu[i] == cu[i + 1]
    _assert_rows_meet_fp64(out, parts, cu, lens, "K12xv %s flip %d" % (name, flip))
    out3 = _run_k12xv(qkv, lens, cu, t_cap, x3=True)
    assert torch.isnan(out3[T:].float()).all(), "x3: pad tokens or canary rows were written"
    assert torch.isfinite(out3[:T].float()).all()


@gpu
def test_k12xv_skips_rows_that_do_not_fit_and_refuses_bad_arguments():
    """cu + len > t_cap (a caller's error): that row alone is left out, nothing
    is read or written out of bounds, the other rows meet the fp64 bound."""
    _need_gpu()
    hip = _hip()
    parts = [_row_f32(65, False), _row_f32(33, False), _row_f32(17, False)]
    # row 1 claims 33 tokens from 65 on, past t_cap = 82; row 2 sits where row 1's first 17 would be
    lens, cu, t_cap = [65, 33, 17], [0, 65, 65], 82
    qkv = torch.full((t_cap, 3 * HD), float("nan"), device=DEV)
    qkv[:65] = parts[0][0]
    qkv[65:82] = parts[2][0]
    out = _run_k12xv(qkv, lens, cu, t_cap)
    assert torch.isnan(out[t_cap:]).all() and torch.isfinite(out[:t_cap]).all()
    _assert_rows_meet_fp64(out, parts, cu, lens, "K12xv row that does not fit", skip=(1,))
    # a row longer than 384 and a negative start are skipped the same way
    only = _run_k12xv(qkv, [385, 17, 17], [0, 65, -1], t_cap)
    assert torch.isnan(only[:65]).all() and torch.isnan(only[82:]).all()
    assert torch.equal(only[65:82], out[65:82])
    # the C entry: no-ops and refusals
    q, o = qkv.data_ptr(), out.data_ptr()
    rl = torch.tensor(lens, device=DEV, dtype=torch.int32)
    cu_t = torch.tensor(cu, device=DEV, dtype=torch.int32)
    hip.attention_f32_packed(q, rl.data_ptr(), cu_t.data_ptr(), o, 0, t_cap, HEADS, SCALE)
    hip.attention_f32_packed(q, rl.data_ptr(), cu_t.data_ptr(), o, 3, 0, HEADS, SCALE)
    torch.cuda.synchronize()
    for args in [(0, rl.data_ptr(), cu_t.data_ptr(), o, 3), (q, 0, cu_t.data_ptr(), o, 3), (q, rl.data_ptr(), 0, o, 3),
                 (q, rl.data_ptr(), cu_t.data_ptr(), 0, 3), (q + 4, rl.data_ptr(), cu_t.data_ptr(), o, 3),
                 (q, rl.data_ptr(), cu_t.data_ptr(), o + 8, 3), (q, rl.data_ptr() + 2, cu_t.data_ptr(), o, 3),
                 (q, rl.data_ptr(), cu_t.data_ptr(), o, 129)]:
        with pytest.raises(hip.HipError):
            hip.attention_f32_packed(*args, t_cap, HEADS, SCALE)
    with pytest.raises(hip.HipError):
        hip.attention_f32_packed(q, rl.data_ptr(), cu_t.data_ptr(), o, 3, t_cap, 0, SCALE)


# ---------------------------------------------------------------------------
# the fp32 packed embedding LayerNorm
# ---------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("which", ["lengths", "holes"])
def test_packed_embed_f32(which):
    """ids and types out of range, tok_src from the twin: a valid token is the
    fp64 LN(word[wrap(id)] + pos[p] + type[clamp(t)]) to K11p's fp32 bound, a
    pad token has the bits of the (0, 0, 0) token, the x3 operand is bitwise
    x3_cat of the fp32 output, nothing past t_cap is written."""
    _need_gpu()
    hip = _hip()
    mask = f32c.lengths_mask_f32() if which == "lengths" else cases.holes_mask()
    rows, s = mask.shape
    n, H = rows * s, HD
    T = int((mask >= 1).sum())
    t_cap = T + 9
    vocab, ntypes, eps = 50, 3, 1e-12
    g = _gen("embed-packed-f32", which)
    word, pos, tok = [torch.randn(k, H, generator=g).to(DEV) for k in (vocab, s, ntypes)]
    gamma = (torch.rand(H, generator=g) + 0.5).to(DEV)
    beta = torch.randn(H, generator=g).to(DEV)
    ids = torch.randint(-3 * vocab, 1000 * vocab, (n,), generator=g, dtype=torch.int32)
    tys = torch.randint(-2, ntypes + 3, (n,), generator=g, dtype=torch.int32)
    edge = torch.from_numpy(np.flatnonzero(mask.reshape(-1) >= 1)[:5])  # ids at the wrap's edges, on valid positions
    ids[edge] = torch.tensor([-1, -vocab, vocab, 2 ** 31 - 1, -2 ** 31], dtype=torch.int32)
    ids, tys = ids.to(DEV), tys.to(DEV)
    tok_src = torch.from_numpy(cases.plan_twin(mask, t_cap)[2]).to(DEV)

    def run(ids_, tys_, src_, cap, n_src, with3=True):
        out = torch.full((cap + CANARY_ROWS, H), float("nan"), device=DEV)
        out3 = torch.full((cap + CANARY_ROWS, 3 * H), float("nan"), device=DEV, dtype=torch.bfloat16)
        hip.embed_layernorm_packed(ids_.data_ptr(), tys_.data_ptr(), src_.data_ptr(), word.data_ptr(), pos.data_ptr(),
                                   tok.data_ptr(), gamma.data_ptr(), beta.data_ptr(), out.data_ptr(), cap, n_src, s, H,
                                   vocab, ntypes, eps, f32=True, out3=out3.data_ptr() if with3 else None)
        torch.cuda.synchronize()
        return out, out3

    out, out3 = run(ids, tys, tok_src, t_cap, n)
    assert torch.isnan(out[t_cap:]).all() and torch.isnan(out3[t_cap:].float()).all(), "rows past t_cap were written"
    assert torch.isfinite(out[:t_cap]).all()
    src = tok_src[:T].long()
    x = (word.double()[ids.long().remainder(vocab)[src]] + pos.double()[src % s]
         + tok.double()[tys.long().clamp(0, ntypes - 1)[src]])
    mu = x.mean(1, keepdim=True)
    ref = (x - mu) / ((x - mu).pow(2).mean(1, keepdim=True) + eps).sqrt() * gamma.double() + beta.double()
    rel = ((out[:T].double() - ref).norm(dim=1) / ref.norm(dim=1)).max().item()
    _report("packed fp32 embed %s" % which, worst_token_rel_l2=rel)
    assert rel < EMBED_REL, rel
    zero = torch.zeros(1, device=DEV, dtype=torch.int32)
    pad, _ = run(zero, zero, zero, 1, 1)  # the real (id 0, position 0, type 0) token
    assert torch.equal(out[T:t_cap], pad[:1].expand(t_cap - T, H)), "pad tokens"
    cat3 = torch.empty(t_cap, 3 * H, device=DEV, dtype=torch.bfloat16)
    hip.x3_cat(out.data_ptr(), cat3.data_ptr(), t_cap, H)
    torch.cuda.synchronize()
    assert torch.equal(out3[:t_cap], cat3), "x3 operand is not x3_cat of the fp32 output"
    alone, untouched = run(ids, tys, tok_src, t_cap, n, with3=False)
    assert torch.equal(alone[:t_cap], out[:t_cap]) and torch.isnan(untouched.float()).all()
    with pytest.raises(ValueError):
        hip.embed_layernorm_packed(256, 256, 256, 256, 256, 256, 256, 256, 256, 4, 4, s, H, vocab, ntypes, eps, out3=256)


# ---------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------
def _row_rel(got, want, valid):
    """Per-row rel-L2 over the row's valid positions (rows without one left out)."""
    errs = []
    for r in range(valid.shape[0]):
        v = valid[r]
        if v.any():
            errs.append(((got[r][v].double() - want[r][v].double()).norm() / want[r][v].double().norm()).item())
    return max(errs)


@gpu
def test_forward_packed_fp32_parity_model():
    """layers=2, the 14 lengths in one batch, ids and types out of range: at
    the valid positions row rel-L2 <= FP32_REL against the fp32 torch module
    (FUSED off) and against the fp32-parity padded forward, PAD_LOGIT
    everywhere else; captured in a graph, the replay gives the eager run's
    bits (so the HIP form has no host sync)."""
    _need_gpu()
    from triton_client_amd.models import bert

    ref = bert.build(device=DEV, dtype=torch.float32, layers=2)
    with torch.no_grad():  # non-zero biases
        for p in ref.parameters():
            if p.dim() == 1 and not torch.all(p == 1):
                p.copy_(torch.randn(p.shape, generator=_gen("bias", tuple(p.shape))).to(DEV) * 0.05)
    m = bert.build(device=DEV, dtype=torch.float32, layers=2)
    m.load_state_dict(ref.state_dict())
    m = bert.prepare_x3(m)
    mask = torch.from_numpy(f32c.lengths_mask_f32()).to(DEV)
    rows = mask.shape[0]
    g = _gen("model-packed-f32")
    ids = torch.randint(-50, 2 * bert.VOCAB, (rows, cases.S), generator=g, dtype=torch.int32).to(DEV)
    tt = torch.randint(-1, 4, (rows, cases.S), generator=g, dtype=torch.int32).to(DEV)
    wrapped, clamped = ids.long().remainder(bert.VOCAB), tt.long().clamp(0, 1)
    t_cap = f32c.ROW_SETS["14-rows"][1]
    assert int(mask.sum()) <= t_cap and bert._packed_f32_ok(m, cases.S) and not bert._packed_f32_ok(ref, cases.S)
    calls = []
    hip = _hip()
    real = hip.attention_f32_packed
    try:
        hip.attention_f32_packed = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
        with torch.no_grad():
            got = m.forward_packed(ids, mask, tt, t_cap)
            padded = m(wrapped, mask, clamped)
    finally:
        hip.attention_f32_packed = real
    assert len(calls) == 2, "the HIP form runs K12xv once per layer"
    with torch.no_grad():
        try:
            bert.FUSED = False
            want = ref(wrapped, mask, clamped)
        finally:
            bert.FUSED = True
    torch.cuda.synchronize()
    valid = mask >= 1
    for k in range(2):
        assert got[k].dtype == torch.float32 and got[k].shape == (rows, cases.S)
        assert (got[k][~valid] == bert.PAD_LOGIT).all()
        assert torch.isfinite(got[k]).all()
        e32, epad = _row_rel(got[k], want[k], valid), _row_rel(got[k], padded[k], valid)
        _report("forward_packed fp32 plane %d" % k, worst_row_vs_fp32_module=e32, worst_row_vs_padded=epad)
        assert e32 <= FP32_REL and epad <= FP32_REL, (e32, epad)
    # no host sync: the whole forward is captured, and the replay repeats the eager bits
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side), torch.no_grad():
        m.forward_packed(ids, mask, tt, t_cap)  # the stream's library workspaces exist before the capture
        with torch.cuda.graph(graph, stream=side):
            cap = m.forward_packed(ids, mask, tt, t_cap)
        graph.replay()
    side.synchronize()
    torch.cuda.synchronize()
    for k in range(2):
        assert torch.equal(cap[k], got[k]), "plane %d: the replay differs from the eager run" % k
    del graph


# ---------------------------------------------------------------------------
# served
# ---------------------------------------------------------------------------
NAMES = ("input_ids", "attention_mask", "token_type_ids")
SHORT = [100, 37, 128, 64, 90]  # 419 tokens <= 8 * 128


@pytest.fixture(scope="module")
def served():
    """{"0" | "1": a loaded two-layer bert_large_fp32 with TCAMD_BERT_PACKED at that value}."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from triton_client_amd.server import gpu_models

    class SmallBertFP32(gpu_models.BertLargeFP32):
        """bert_large_fp32 with two layers and two row buckets: a few graphs to capture."""

        BUCKETS = (8, 16)

    out = {}
    old = os.environ.get("TCAMD_BERT_PACKED")
    try:
        for knob in ("0", "1"):
            os.environ["TCAMD_BERT_PACKED"] = knob
            out[knob] = SmallBertFP32(layers=2)
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


def _serve(model, arrays, split):
    """[2][rows][384] logits of ``arrays`` sent as requests of ``split`` rows each, one execute call."""
    from triton_client_amd.server.types import InferRequest, InputTensor

    reqs, first = [], 0
    for n in split:
        ins = [InputTensor(nm, "INT32", [n, 384], np.ascontiguousarray(a[first:first + n])) for nm, a in zip(NAMES, arrays)]
        reqs.append(InferRequest(model_name="bert_large_fp32", inputs=ins))
        first += n
    results = model.execute(reqs)
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


@gpu
def test_served_fp32_short_rows_take_a_packed_graph(served):
    """Five short rows, one request at a time per model: the knob-1 model
    serves them from a packed graph, its valid logits are within FP32_REL (per
    row) of the knob-0 model's, PAD_LOGIT elsewhere, and K27's best span is the
    same in every row -- each row's leader is ahead of its runner-up by more
    than four times the largest logit difference (a span's score is two
    logits), which is asserted, not assumed."""
    arrays = _rows(SHORT, 1)
    on, off = served["1"], served["0"]
    assert on.packed and not off.packed and on.supports_packed
    assert on.packed_bucket(5, sum(SHORT)) == (8, 128)
    before = dict(on.route_counts), dict(off.route_counts)
    got = _serve(on, arrays, [2, 3])
    want = _serve(off, arrays, [2, 3])
    assert on.route_counts == {"packed": before[0]["packed"] + 1, "padded": before[0]["padded"]}
    assert off.route_counts == {"packed": 0, "padded": before[1]["padded"] + 1}
    valid = arrays[1] >= 1
    for k in range(2):
        assert (got[k][~valid] == -10000.0).all()
        err = _row_rel(torch.from_numpy(got[k]), torch.from_numpy(want[k]), torch.from_numpy(valid))
        _report("served fp32 packed vs padded plane %d" % k, worst_row_rel_l2=err)
        assert err <= FP32_REL, err
    d = float(np.abs(got - want)[:, valid].max())
    s_on, _ = _top2(got, arrays[1], arrays[2])
    s_off, sc_off = _top2(want, arrays[1], arrays[2])
    margins = sc_off[:, 0] - sc_off[:, 1]
    _report("served fp32 spans", largest_logit_difference=d, smallest_margin=float(margins.min()))
    assert (margins > 4 * d).all(), (margins, d)  # no row is left out
    for r in range(len(SHORT)):
        assert s_on[r, 0].tolist() == s_off[r, 0].tolist(), (r, s_on[r], s_off[r], sc_off[r], d)


@gpu
def test_served_fp32_full_rows_take_the_padded_graph_bitwise(served):
    """More than 256 tokens per bucket row fit no packed graph: the knob-1
    model runs the padded graph and answers the knob-0 model's bits."""
    lens = [384, 380, 300, 384, 384, 290, 384, 384]
    arrays = _rows(lens, 2)
    on, off = served["1"], served["0"]
    assert on.packed_bucket(8, sum(lens)) is None
    before = dict(on.route_counts)
    got = _serve(on, arrays, [8])
    want = _serve(off, arrays, [8])
    assert on.route_counts == {"packed": before["packed"], "padded": before["padded"] + 1}
    assert np.array_equal(got.view(np.int32), want.view(np.int32))

"""The BERT kernels of csrc/kernels/bert.hip on every launch plan and mask
edge, against fp64 torch references taken one sequence at a time: K12
attention, K12x fp32-parity attention, x3_cat, K11 / K11p / the embedding
LayerNorm and the QA head.

Every K12 / K12x case asserts, through ``hip.attention_plan`` /
``hip.attention_f32_plan``, the launch plan it exists to cover, so a retune
cannot move it off that path unnoticed.

K12's elementwise bound is derived, not tuned.  The kernel rounds P to bf16
for the PV MFMA while ``l`` sums the unrounded p, and rounds the output to
bf16, so for every output element

    |got - ref| <= 2 * 2^-9 * (A + |ref|) + 1e-6

with A the softmax-weighted mean of |V| for that query and dimension (from the
fp64 reference); the factor 2 covers v_exp_f32 and the fp32 accumulation.
``test_k12_bound_holds_for_fp64_emulation`` (no GPU) checks that an fp64
emulation with exactly those two roundings stays inside the bound on every
sequence the GPU cases use.  The other bounds are those of
test_bert_kernels_gpu.py and test_gemm_gpu.py, applied per block, head or row
instead of per tensor.

Poisoned padding: padded keys carry V rows of 3e4 (1e4 for K12x) and K rows
``beta * u`` along a component ``u`` that every query shares, so a padded
key's scaled score exceeds every valid score by more than 200 (asserted from
the fp64 scores).  The reference is the fp64 softmax over the valid keys
only, taken by index: one leaked key is an error thousands of times the
bound, and a running maximum over unbiased padded scores is NaN.

Outputs are filled with NaN first and carry extra rows that must stay NaN.
The tests print their worst figures (run with ``-s``);
profiles/bert_kernel_edges.md keeps them."""

import functools
import zlib

import pytest

torch = pytest.importorskip("torch")

DEV = "cuda"
gpu = pytest.mark.gpu
CANARY_ROWS = 4  # a 4-wave block's guarded waves past ``rows`` would land here


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _hip():
    from triton_client_amd.ops import hip

    return hip


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _report(what, **figs):
    print("[bert-edges] %s: %s" % (what, " ".join("%s=%.3g" % kv for kv in figs.items())))


# ---------------------------------------------------------------------------
# attention: sequences, masks, the fp64 reference
# ---------------------------------------------------------------------------
D = 64
U_DIM = 63      # the queries' shared component u = e_63 ...
U_Q = 4.0       # ... Q[:, u] = 4 for every query, 0 in every valid key,
U_BETA = 1000.0  # ... K_pad = 1000 u: scaled score 0.125 * 4 * 1000 = 500 for every (query, padded key)
V_POISON = {torch.bfloat16: 3e4, torch.float32: 1e4}


def _pattern(S, i):
    """Mask of sequence ``i`` of a poisoned-padding case (1 = valid), or None
    for an unpadded one; "full" marks the fully masked sequence."""
    m = torch.ones(S, dtype=torch.int32)
    i %= 9
    if i == 0:    # a tail that ends inside a chunk
        m[S - 37:] = 0
    elif i == 1:  # a tail that ends exactly on a chunk boundary: no partial chunk
        m[S - 64:] = 0
    elif i == 2:  # leading padding over the first chunk and part of the second
        m[:64 + 23] = 0
    elif i == 3:  # single holes at both ends of the first chunk boundary and of the sequence
        m[[0, 63, 64, S - 1]] = 0
    elif i == 4:  # only one valid key, in the second chunk
        m[:] = 0
        m[70] = 1
    elif i == 5:  # unpadded
        return None
    elif i == 6:  # fully masked, between two ordinary sequences
        m[:] = 0
    elif i == 7:  # a short tail
        m[S - 5:] = 0
    else:         # only one valid key: the first
        m[:] = 0
        m[0] = 1
    return m


def _tail_mask(S, i):
    """The neighbouring files' masks: tails of different lengths, one hole."""
    m = torch.ones(S, dtype=torch.int32)
    m[S - 7 * (i + 1) * (S // 64):] = 0
    if i == 0:
        m[5] = 0
    return m


def _make_seq(S, heads, i, kind, dtype):
    """Sequence ``i`` of a case: (qkv [S][3 * heads * 64] of ``dtype`` on the
    CPU, int32 mask [S] or None).  It depends on (S, heads, i, kind, dtype)
    alone, so cases that differ in ``seqs`` share sequences and references."""
    g = _gen("qkv", S, heads, i, str(dtype))
    qkv = (torch.randn(S, 3, heads, D, generator=g) * 1.5).to(dtype)
    mask = None
    if kind == "tails":
        mask = _tail_mask(S, i)
    elif kind == "poison":
        mask = _pattern(S, i)
        if mask is not None and mask.any():
            pad = mask == 0
            qkv[:, 0, :, U_DIM] = U_Q
            qkv[:, 1, :, U_DIM] = 0.0
            qkv[pad, 1] = 0.0
            qkv[pad, 1, :, U_DIM] = U_BETA
            qkv[pad, 2] = V_POISON[dtype]
    return qkv.reshape(S, 3 * heads * D), mask


def _attn_ref64(qkv, mask, heads, scale, bias=None, emulate=False):
    """fp64 attention of one sequence.  Keys: the valid ones, taken by index
    (no additive bias); all of them when none is valid (what the additive
    -10000 of the kernels and of torch comes to).  Returns ref [S][heads * 64],
    A = sum_k p |v| in the same shape, and (lowest padded, highest padded,
    highest valid) scaled score, or None without padding.  ``bias``: K12's
    separate projection bias (q + b_q rounded to bf16 as the kernel does, b_k
    dropped, b_v added to the output).  ``emulate``: also the fp64 emulation of
    K12's two roundings (P to bf16 under an unrounded l, the output to bf16)."""
    S = qkv.shape[0]
    x = qkv.view(S, 3, heads, D).permute(1, 2, 0, 3)
    q, k, v = x[0], x[1].double(), x[2].double()
    bv = 0.0
    if bias is not None:
        b = bias.view(3, heads, 1, D)
        q = (q.float() + b[0].float()).to(qkv.dtype)
        bv = b[2].double()
    s = (q.double() @ k.transpose(-1, -2)) * scale  # [heads][S queries][S keys]
    edges = None
    if mask is not None and mask.any() and not mask.all():
        valid = mask.to(s.device) != 0
        idx = valid.nonzero().flatten()
        sp = s[:, :, ~valid]
        edges = (sp.min().item(), sp.max().item(), s[:, :, idx].max().item())
        s, v = s[:, :, idx], v[:, idx]
    m = s.max(-1, keepdim=True).values
    p = torch.exp(s - m)
    l = p.sum(-1, keepdim=True)
    ref = (p @ v) / l + bv
    a = (p @ v.abs()) / l
    flat = lambda t: t.transpose(0, 1).reshape(S, heads * D)  # noqa: E731
    emu = None
    if emulate:
        pb = p.float().bfloat16().double()
        emu = flat(((pb @ v) / l + bv).float().bfloat16().double())
    return flat(ref), flat(a), edges, emu


def _k12_bound(ref, a):
    return 2.0 * 2.0 ** -9 * (a + ref.abs()) + 1e-6


def _assert_poison_scores(edges):
    lo_pad, hi_pad, hi_valid = edges
    assert lo_pad >= hi_valid + 200.0 and hi_pad < 2000.0, edges


# K12 cases: (seqs, S, heads, scale, kind, separate bias, expected (splits, waves))
def _k12(seqs, S, plan, kind="dense", heads=16, scale=0.125, bias=False):
    ident = "%dx%d-%s%s%s%s-plan%dx%d" % (seqs, S, kind, "" if heads == 16 else "-h%d" % heads,
                                          "" if scale == 0.125 else "-scale%g" % scale, "-bias" if bias else "",
                                          plan[0], plan[1])
    return pytest.param(seqs, S, heads, scale, kind, bias, plan, id=ident)


K12_PLANS = [  # (seqs, S) -> plan at 16 heads: every pair the plan can return for S in 64..384
    (2, 64, (1, 2)),
    (3, 128, (2, 2)), (9, 128, (1, 4)),
    (2, 192, (3, 2)), (6, 192, (2, 3)), (9, 192, (1, 6)),
    (2, 256, (2, 4)), (9, 256, (1, 8)),
    (3, 320, (2, 5)), (9, 320, (1, 10)),
    (2, 384, (3, 4)), (7, 384, (2, 6)), (9, 384, (1, 12)),
]
ALL_PAIRS = {(1, 2), (2, 2), (1, 4), (3, 2), (2, 3), (1, 6), (2, 4), (1, 8), (2, 5), (1, 10), (3, 4), (2, 6), (1, 12)}

K12_CASES = [_k12(n, S, plan, kind) for n, S, plan in K12_PLANS for kind in ("dense", "tails")]
K12_CASES += [
    _k12(2, 192, (3, 2), "tails", heads=12),
    _k12(3, 128, (2, 2), "tails", heads=1),
    _k12(2, 128, (2, 2), "tails", scale=0.2),
    _k12(9, 384, (1, 12), "dense", bias=True), _k12(9, 384, (1, 12), "tails", bias=True),
    _k12(3, 320, (2, 5), "dense", bias=True), _k12(3, 320, (2, 5), "tails", bias=True),
    # every mask pattern (one per sequence) on the largest plan, on other multi-chunk lengths, on every split count
    _k12(9, 384, (1, 12), "poison"), _k12(9, 128, (1, 4), "poison"),
    _k12(8, 192, (2, 3), "poison"), _k12(8, 256, (2, 4), "poison"), _k12(5, 384, (3, 4), "poison"),
]

# K12x cases: (seqs, S, kind, expected waves), 16 heads
K12X_CASES = [pytest.param(n, S, kind, w, id="%dx%d-%s-waves%d" % (n, S, kind, w)) for n, S, w in
              [(16, 128, 8), (8, 256, 8), (6, 384, 8), (3, 192, 4), (1, 512, 4)] for kind in ("dense", "tails")]
K12X_CASES += [pytest.param(n, S, "poison", w, id="%dx%d-poison-waves%d" % (n, S, w)) for n, S, w in
               [(8, 256, 8), (9, 384, 8), (5, 192, 4)]]


def test_plan_queries_cover_every_pair():
    """Host only: the plan queries give every case the plan it names; the K12
    cases cover all 13 (splits, waves) pairs of S in 64..384 both unmasked and
    masked, and the poisoned ones every split count and the largest plan; the
    K12x cases cover both wave counts; a sweep over seqs and S finds no pair
    outside the table; bad shapes are refused."""
    hip = _hip()
    seen = {}
    for c in K12_CASES:
        seqs, S, heads, _, kind, _, plan = c.values
        assert hip.attention_plan(seqs, S, heads) == plan, c.id
        if heads == 16:
            seen.setdefault(kind, set()).add(plan)
    assert seen["dense"] == ALL_PAIRS and seen["tails"] == ALL_PAIRS
    assert {(1, 12), (1, 4), (2, 3), (2, 4), (3, 4)} <= seen["poison"]
    swept = {hip.attention_plan(n, S, 16) for n in range(1, 70) for S in range(64, 385, 64)}
    assert swept == ALL_PAIRS
    waves = set()
    for c in K12X_CASES:
        seqs, S, _, w = c.values
        assert hip.attention_f32_plan(seqs, S, 16) == w, c.id
        waves.add(w)
    assert waves == {4, 8}
    for bad in [(0, 64, 16), (1, 100, 16), (1, 448, 16), (1, 64, 0)]:
        with pytest.raises(hip.HipError):
            hip.attention_plan(*bad)
    for bad in [(0, 64, 16), (1, 100, 16), (1, 64, 0)]:
        with pytest.raises(hip.HipError):
            hip.attention_f32_plan(*bad)


def _k12_bias(heads):
    return (torch.randn(3 * heads * D, generator=_gen("bias", heads)) * 0.5).bfloat16()


def test_k12_bound_holds_for_fp64_emulation():
    """No GPU: on every distinct sequence of the K12 cases, an fp64 attention
    that rounds P to bf16 (l unrounded) and the output to bf16 stays inside
    the derived elementwise bound, and the poisoned sequences meet the score
    precondition."""
    done, worst = set(), 0.0
    for c in K12_CASES:
        seqs, S, heads, scale, kind, bias, _ = c.values
        for i in range(seqs):
            key = (S, heads, scale, kind, bias, i)
            if key in done:
                continue
            done.add(key)
            qkv, mask = _make_seq(S, heads, i, kind, torch.bfloat16)
            ref, a, edges, emu = _attn_ref64(qkv, mask, heads, scale, _k12_bias(heads) if bias else None,
                                             emulate=True)
            if kind == "poison" and edges is not None:
                _assert_poison_scores(edges)
            ratio = ((emu - ref).abs() / _k12_bound(ref, a)).max().item()
            assert ratio <= 1.0, (key, ratio)
            worst = max(worst, ratio)
    _report("K12 fp64 emulation", sequences=len(done), worst_err_over_bound=worst)


@functools.lru_cache(maxsize=None)
def _seq_on_device(S, heads, i, kind, dtype, scale, with_bias, forced_full=False):
    """One sequence's inputs and fp64 reference on the device, computed once
    and shared by the cases that use it (never written to afterwards)."""
    qkv, mask = _make_seq(S, heads, i, kind, dtype)
    if forced_full:
        mask = torch.zeros(S, dtype=torch.int32)
    bias = _k12_bias(heads).to(DEV) if with_bias else None
    qkv = qkv.to(DEV)
    ref, a, edges, _ = _attn_ref64(qkv, mask, heads, scale, bias)
    return qkv, mask, ref, a, edges


@pytest.fixture(scope="module", autouse=True)
def _drop_shared_references():
    yield
    _seq_on_device.cache_clear()


def _assemble(seqs, S, heads, kind, dtype, scale, with_bias=False, full_at=None):
    parts = [_seq_on_device(S, heads, i, kind, dtype, scale, with_bias, forced_full=(i == full_at))
             for i in range(seqs)]
    qkv = torch.cat([p[0] for p in parts])
    masks = [p[1] for p in parts]
    mask = None
    if any(m is not None for m in masks):
        mask = torch.stack([torch.ones(S, dtype=torch.int32) if m is None else m for m in masks]).to(DEV)
    if kind == "poison":
        for p in parts:
            if p[4] is not None:
                _assert_poison_scores(p[4])
    return qkv, mask, parts


@gpu
@pytest.mark.parametrize("seqs,S,heads,scale,kind,with_bias,plan", K12_CASES)
def test_k12_every_plan_and_mask_edge(seqs, S, heads, scale, kind, with_bias, plan):
    """K12 against fp64 per (sequence, head, 32-query block): the derived
    elementwise bound and the neighbouring file's rel-L2 < 1e-2."""
    _need_gpu()
    hip = _hip()
    assert hip.attention_plan(seqs, S, heads) == plan
    HD = heads * D
    qkv, mask, parts = _assemble(seqs, S, heads, kind, torch.bfloat16, scale, with_bias)
    assert (mask is not None) == (kind != "dense")
    bias = _k12_bias(heads).to(DEV) if with_bias else None
    out = torch.full((seqs * S + 2, HD), float("nan"), device=DEV, dtype=torch.bfloat16)
    hip.attention(qkv.data_ptr(), None if mask is None else mask.data_ptr(), out.data_ptr(), seqs, S, heads, scale,
                  bias=None if bias is None else bias.data_ptr())
    torch.cuda.synchronize()
    assert torch.isnan(out[seqs * S:]).all(), "rows past the output were written"
    worst_e = worst_r = 0.0
    for i, (_, _, ref, a, _) in enumerate(parts):
        got = out[i * S:(i + 1) * S].double()
        assert torch.isfinite(got).all(), "sequence %d: non-finite output" % i
        blk = lambda t: t.view(S // 32, 32, heads, D)  # noqa: E731
        ratio = blk((got - ref).abs() / _k12_bound(ref, a)).amax((1, 3))  # [block][head]
        rel = (blk(got - ref).pow(2).sum((1, 3)) / blk(ref).pow(2).sum((1, 3))).sqrt()
        for name, t, lim in (("elementwise error / bound", ratio, 1.0), ("rel-L2", rel, 1e-2)):
            if (t > lim).any():
                b, h = (t > lim).nonzero()[0].tolist()
                pytest.fail("sequence %d head %d queries %d..%d: %s %.4g > %g" % (i, h, 32 * b, 32 * b + 31, name,
                                                                                 t[b, h].item(), lim))
        worst_e, worst_r = max(worst_e, ratio.max().item()), max(worst_r, rel.max().item())
    _report("K12 %dx%d h%d %s%s plan %s" % (seqs, S, heads, kind, " bias" if with_bias else "", plan),
            worst_err_over_bound=worst_e, worst_block_rel_l2=worst_r)


def _k12x_check(got, parts, S, heads):
    worst = worst_full = 0.0
    for i, (_, mask, ref, _, _) in enumerate(parts):
        g = got[i * S:(i + 1) * S].double().view(S, heads, D)
        r = ref.view(S, heads, D)
        assert torch.isfinite(g).all(), "sequence %d: non-finite output" % i
        rel = ((g - r).pow(2).sum((0, 2)) / r.pow(2).sum((0, 2))).sqrt()  # per head
        # a fully masked sequence: every fp32 score carries the -10000 offset,
        # which leaves ~10 fewer bits of it (as in the reference's fp32 path)
        full = mask is not None and not mask.any()
        lim = 2e-3 if full else 2e-5
        assert (rel < lim).all(), "sequence %d head %d: rel-L2 %.4g >= %g" % (i, rel.argmax().item(),
                                                                              rel.max().item(), lim)
        if full:
            worst_full = max(worst_full, rel.max().item())
        else:
            worst = max(worst, rel.max().item())
    return worst, worst_full


@gpu
@pytest.mark.parametrize("seqs,S,kind,waves", K12X_CASES)
def test_k12x_both_kernels_and_mask_edges(seqs, S, kind, waves):
    """K12x (4- and 8-wave kernels) against fp64 per (sequence, head): the
    neighbouring file's 2e-5, 2e-3 on a fully masked sequence."""
    _need_gpu()
    hip = _hip()
    heads = 16
    assert hip.attention_f32_plan(seqs, S, heads) == waves
    full_at = 2 if kind == "tails" and seqs > 2 else None
    qkv, mask, parts = _assemble(seqs, S, heads, kind, torch.float32, 0.125, full_at=full_at)
    out = torch.full((seqs * S + 2, heads * D), float("nan"), device=DEV)
    hip.attention_f32(qkv.data_ptr(), None if mask is None else mask.data_ptr(), out.data_ptr(), seqs, S, heads, 0.125)
    torch.cuda.synchronize()
    assert torch.isnan(out[seqs * S:]).all(), "rows past the output were written"
    worst, worst_full = _k12x_check(out, parts, S, heads)
    _report("K12x %dx%d %s waves %d" % (seqs, S, kind, waves), worst_head_rel_l2=worst,
            worst_fully_masked_rel_l2=worst_full)


def _x3_def(x):
    """The bf16x3 operand by its definition: [hi | hi | lo], hi = bf16_rne(x), lo = bf16_rne(x - hi)."""
    hi = x.bfloat16()
    lo = (x - hi.float()).bfloat16()
    return torch.cat([hi, hi, lo], dim=1)


def _bits(t):
    return t.view(torch.int16)


@gpu
@pytest.mark.parametrize("seqs,S,kind", [(16, 128, "tails"), (8, 256, "poison")])
def test_k12x_x3_operand_is_the_definition(seqs, S, kind):
    """The 8-wave K12x kernel's x3 form, bitwise against the torch definition
    of the operand applied to the kernel's own fp32 output."""
    _need_gpu()
    hip = _hip()
    heads = 16
    assert hip.attention_f32_plan(seqs, S, heads) == 8
    qkv, mask, _ = _assemble(seqs, S, heads, kind, torch.float32, 0.125)
    rows = seqs * S
    out = torch.full((rows + 2, heads * D), float("nan"), device=DEV)
    out3 = torch.full((rows + 2, 3 * heads * D), float("nan"), device=DEV, dtype=torch.bfloat16)
    hip.attention_f32(qkv.data_ptr(), mask.data_ptr(), out.data_ptr(), seqs, S, heads, 0.125)
    hip.attention_f32(qkv.data_ptr(), mask.data_ptr(), out3.data_ptr(), seqs, S, heads, 0.125, x3=True)
    torch.cuda.synchronize()
    assert torch.isnan(out[rows:]).all() and torch.isnan(out3[rows:]).all(), "rows past the output were written"
    assert torch.isfinite(out[:rows]).all()
    assert torch.equal(_bits(out3[:rows]), _bits(_x3_def(out[:rows])))


# ---------------------------------------------------------------------------
# x3_cat against its definition
# ---------------------------------------------------------------------------
def _x3_values(rows, K):
    g = _gen("x3", rows, K)
    n = rows * K
    e = torch.randint(-100, 101, (n,), generator=g)
    x = torch.ldexp(1.0 + torch.rand(n, generator=g), e)
    x = torch.where(torch.rand(n, generator=g) < 0.5, -x, x)
    t8 = 2.0 ** -8
    special = torch.tensor([0.0, -0.0, 1 + t8, -(1 + t8), 1 + 3 * t8, -(1 + 3 * t8), 2.0 ** -126, -(2.0 ** -126),
                            3e38, -3e38, 1.0, -1.0])
    x[:12] = special          # the first rows ...
    x[n - 12:] = special.flip(0)  # ... and the last thread's elements
    return x.view(rows, K)


@gpu
@pytest.mark.parametrize("rows,K", [(6, 4), (5, 1028), (1025, 4100)])
def test_x3_cat_is_its_definition(rows, K):
    """x3_cat bitwise against hi = x.bfloat16(), lo = (x - hi.float()).bfloat16(),
    laid out [hi | hi | lo]: K = 4, a K that is no multiple of the block, and
    rows * K / 4 > 1,048,576 float4s (the grid-stride loop's second pass).
    Values: +-0, the round-to-nearest-even ties 1 + 2^-8 and 1 + 3 * 2^-8 and
    their negatives, the smallest normal fp32, 3e38, and random signs and
    mantissas over exponents 2^-100 .. 2^100.  Left out: non-finite values,
    denormals (inputs or a denormal lo), and values that round to infinity in
    bf16 -- the kernel's contract is the finite normal range."""
    _need_gpu()
    hip = _hip()
    if rows == 1025:
        assert rows * (K // 4) > 1048576
    x = _x3_values(rows, K).to(DEV)
    out = torch.full((rows + 2, 3 * K), float("nan"), device=DEV, dtype=torch.bfloat16)
    hip.x3_cat(x.data_ptr(), out.data_ptr(), rows, K)
    torch.cuda.synchronize()
    assert torch.isnan(out[rows:]).all(), "rows past the output were written"
    hi = x.bfloat16()
    lo = (x - hi.float()).bfloat16()
    assert torch.isfinite(hi.float()).all()
    got = out[:rows]
    assert torch.equal(_bits(got[:, :K]), _bits(hi)), "hi"
    assert torch.equal(_bits(got[:, K:2 * K]), _bits(hi)), "second hi"
    assert torch.equal(_bits(got[:, 2 * K:]), _bits(lo)), "lo"
    # the ties went to the even neighbour: 1 + 2^-8 -> 1, 1 + 3 * 2^-8 -> 1 + 2^-6
    assert got[0, :4].float().tolist()[2:] == [1.0, -1.0] and got.view(-1)[:2].float().tolist() == [0.0, 0.0]
    assert _bits(got.reshape(-1)[:2]).tolist() == [0, -32768]  # +0, -0
    if K >= 8:
        assert got[0, 4:6].float().tolist() == [1 + 2.0 ** -6, -(1 + 2.0 ** -6)]


# ---------------------------------------------------------------------------
# LayerNorm family and the QA head
# ---------------------------------------------------------------------------
WIDTHS = [512, 1024, 2048, 4096]
ROWS = [1, 3, 37]


def _ln_ref(v, gamma, beta, eps):
    return torch.nn.functional.layer_norm(v, (v.shape[-1],), gamma.double(), beta.double(), eps)


def _row_rel(got, ref):
    return ((got.double() - ref).norm(dim=1) / ref.norm(dim=1)).max().item()


def _ln_params(H, dt, g):
    gamma = (torch.rand(H, generator=g) + 0.5).to(dt).to(DEV)
    beta = torch.randn(H, generator=g).to(dt).to(DEV)
    return gamma, beta


def _canaried(rows, H, dt):
    return torch.full((rows + CANARY_ROWS, H), float("nan"), device=DEV, dtype=dt)


def _ln_inputs(rows, H, g):
    """Row classes of an add+LayerNorm input pair (fp32 on the CPU, exact in
    bf16 where it matters): row 0 constant (x + y = 2^-1 everywhere), the other
    rows ordinary."""
    x = torch.randn(rows + CANARY_ROWS, H, generator=g) * 3 + 1
    y = torch.randn(rows + CANARY_ROWS, H, generator=g)
    x[0], y[0] = 0.375, 0.125
    return x, y


@gpu
@pytest.mark.parametrize("H", WIDTHS)
@pytest.mark.parametrize("rows", ROWS)
def test_add_layernorm_rows_eps_and_canary(rows, H):
    """K11 per row against fp64 (the neighbouring file's 1e-2), nothing past
    ``rows`` written, a constant row gives beta bitwise, and eps = 1e-5 on
    rows whose variance is about 1e-5 (a dropped eps is off by sqrt(2))."""
    _need_gpu()
    hip = _hip()
    g = _gen("k11", rows, H)
    gamma, beta = _ln_params(H, torch.bfloat16, g)
    x, y = _ln_inputs(rows, H, g)
    x, y = x.bfloat16().to(DEV), y.bfloat16().to(DEV)
    out = _canaried(rows, H, torch.bfloat16)
    hip.add_layernorm(x.data_ptr(), y.data_ptr(), gamma.data_ptr(), beta.data_ptr(), out.data_ptr(), rows, H, 1e-12)
    torch.cuda.synchronize()
    assert torch.isnan(out[rows:]).all(), "rows past the output were written"
    ref = _ln_ref(x[:rows].double() + y[:rows].double(), gamma, beta, 1e-12)
    assert torch.equal(_bits(out[0]), _bits(beta)), "constant row"
    e1 = _row_rel(out[1:rows], ref[1:]) if rows > 1 else 0.0
    assert e1 < 1e-2, e1
    # variance ~ 1e-5 around a zero mean, eps = 1e-5
    xs = (torch.randn(rows + CANARY_ROWS, H, generator=g) * 10 ** -2.5).bfloat16().to(DEV)
    ys = torch.zeros_like(xs)
    out = _canaried(rows, H, torch.bfloat16)
    hip.add_layernorm(xs.data_ptr(), ys.data_ptr(), gamma.data_ptr(), beta.data_ptr(), out.data_ptr(), rows, H, 1e-5)
    torch.cuda.synchronize()
    assert torch.isnan(out[rows:]).all(), "rows past the output were written"
    v = xs[:rows].double()
    var = v.var(dim=1, unbiased=False)
    assert (var > 0.5e-5).all() and (var < 2e-5).all()
    e2 = _row_rel(out[:rows], _ln_ref(v, gamma, beta, 1e-5))
    assert e2 < 1e-2, e2
    _report("K11 %dx%d" % (rows, H), worst_row_rel_l2=e1, worst_row_rel_l2_eps=e2)


@gpu
@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "f32"])
@pytest.mark.parametrize("H", WIDTHS)
@pytest.mark.parametrize("rows", ROWS)
def test_add_layernorm_parts_rows_eps_and_canary(rows, H, f32):
    """K11p per row against fp64 (test_gemm_gpu.py's 4e-3 in bf16, 1e-6 in
    fp32) with a bias and two partial slabs, nothing past ``rows`` written, a
    constant row gives beta bitwise, eps = 1e-5 at variance 1e-5; in fp32 also
    rows of mean 1000 and standard deviation 1 at the same 1e-6 (a one-pass
    variance misses that by percent).  Those rows lie on a 2^-1 grid, so every
    fp32 partial sum of the row (< 2^23) and its mean are exact and the bound
    measures the variance and the normalisation alone."""
    _need_gpu()
    hip = _hip()
    dt = torch.float32 if f32 else torch.bfloat16
    lim = 1e-6 if f32 else 4e-3
    g = _gen("k11p", rows, H, f32)
    gamma, beta = _ln_params(H, dt, g)
    R = rows + CANARY_ROWS
    st = torch.cuda.current_stream().cuda_stream

    def run(x, parts, bias, eps, out3=False):
        out = _canaried(rows, H, dt)
        o3 = torch.full((R, 3 * H), float("nan"), device=DEV, dtype=torch.bfloat16) if out3 else None
        hip.add_layernorm_parts(x.data_ptr(), parts.data_ptr(), parts.shape[0], R * H,
                                None if bias is None else bias.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                out.data_ptr(), rows, H, eps, f32=f32, stream=st,
                                out3=None if o3 is None else o3.data_ptr())
        torch.cuda.synchronize()
        assert torch.isnan(out[rows:]).all(), "rows past the output were written"
        v = x[:rows].double() + parts[:, :rows].double().sum(0) + (0 if bias is None else bias.double())
        if o3 is not None:
            assert torch.isnan(o3[rows:]).all(), "rows past the x3 operand were written"
            assert torch.equal(_bits(o3[:rows]), _bits(_x3_def(out[:rows]))), "x3 operand"
        return out, v

    # ordinary rows; row 0 constant: the bias lies on a 2^-6 grid, so (0.25 -
    # bias) is exact in bf16 and (0.25 - bias) + bias + 0.125 + 0.125 = 2^-1
    # at every fp32 step
    x = torch.randn(R, H, generator=g).to(dt).to(DEV)
    parts = (torch.randn(2, R, H, generator=g) * 0.3).to(DEV)
    bias = (torch.round(torch.randn(H, generator=g) * 6.4).clamp(-32, 32) / 64).to(DEV)
    x[0], parts[:, 0] = (0.25 - bias).to(dt), 0.125
    out, v = run(x, parts, bias, 1e-12, out3=f32)
    assert (v[0] == 0.5).all()
    assert torch.equal(out[0], beta), "constant row"
    e1 = _row_rel(out[1:rows], _ln_ref(v[1:], gamma, beta, 1e-12)) if rows > 1 else 0.0
    assert e1 < lim, e1
    # variance ~ 1e-5, eps = 1e-5
    xs = (torch.randn(R, H, generator=g) * 10 ** -2.5).to(dt).to(DEV)
    zero = torch.zeros(1, R, H, device=DEV)
    out, v = run(xs, zero, None, 1e-5)
    var = v.var(dim=1, unbiased=False)
    assert (var > 0.5e-5).all() and (var < 2e-5).all()
    e2 = _row_rel(out[:rows], _ln_ref(v, gamma, beta, 1e-5))
    assert e2 < lim, e2
    e3 = 0.0
    if f32:  # mean 1000, standard deviation 1, on a 2^-1 grid
        grid = lambda t: torch.round(t * 2) / 2  # noqa: E731
        xm = (1000 + grid(torch.randn(R, H, generator=g) * 0.9)).to(DEV)
        pm = grid(torch.randn(2, R, H, generator=g) * 0.3).to(DEV)
        bm = grid(torch.randn(H, generator=g) * 0.5).to(DEV)
        out, v = run(xm, pm, bm, 1e-12)
        sd = v.std(dim=1, unbiased=False)
        assert ((v.mean(dim=1) - 1000).abs() < 1).all() and (sd > 0.7).all() and (sd < 1.5).all()
        e3 = _row_rel(out[:rows], _ln_ref(v, gamma, beta, 1e-12))
        assert e3 < lim, e3
    _report("K11p %s %dx%d" % ("f32" if f32 else "bf16", rows, H), worst_row_rel_l2=e1, worst_row_rel_l2_eps=e2,
            worst_row_rel_l2_mean1000=e3)


@gpu
@pytest.mark.parametrize("H", WIDTHS)
def test_embed_layernorm_clamps_wraps_and_guards(H):
    """The embedding LayerNorm called directly, small tables (vocab 50, 3
    types, S = 7) and rows = 3 * 7 + 2, so the position wraps and the last
    block is partial: per row against fp64 (the neighbouring file's 1e-2); ids
    -5 and vocab + 7 and type 9 equal their clamped rows bitwise; a constant
    row gives beta bitwise; eps = 1e-5 at variance 1e-5; nothing past ``rows``
    written.  The tables sit inside larger buffers of 1e4, so an unclamped
    index or an unwrapped position reads that and not foreign memory."""
    _need_gpu()
    hip = _hip()
    vocab, ntypes, S, rows, PAD = 50, 3, 7, 23, 12
    g = _gen("embed", H)
    gamma, beta = _ln_params(H, torch.bfloat16, g)

    def table(n, scale, after):
        buf = torch.full((PAD + n + after, H), 1e4, dtype=torch.bfloat16)
        buf[PAD:PAD + n] = (torch.randn(n, H, generator=g) * scale).bfloat16()
        return buf

    ids = torch.randint(0, vocab, (rows + CANARY_ROWS,), generator=g)
    tys = torch.randint(0, ntypes, (rows + CANARY_ROWS,), generator=g)
    ids[3], ids[9], tys[11], tys[4] = -5, vocab + 7, 9, -2
    ids[0] = ids[21] = 17  # rows 0 and 21 = 3 * 7: position 0 both times -> the constant row, twice
    tys[0] = tys[21] = 1

    def run(scale, eps, const):
        word, pos, tok = table(vocab, scale, PAD), table(S, scale, rows), table(ntypes, scale, PAD)
        if const:
            word[PAD + 17], pos[PAD + 0], tok[PAD + 1] = 0.25, 0.125, 0.125
        word, pos, tok = word.to(DEV), pos.to(DEV), tok.to(DEV)
        outs = []
        for clamp in (False, True):
            i = (ids.clamp(0, vocab - 1) if clamp else ids).to(DEV)
            t = (tys.clamp(0, ntypes - 1) if clamp else tys).to(DEV)
            out = _canaried(rows, H, torch.bfloat16)
            hip.embed_layernorm(i.data_ptr(), t.data_ptr(), word[PAD].data_ptr(), pos[PAD].data_ptr(),
                                tok[PAD].data_ptr(), gamma.data_ptr(), beta.data_ptr(), out.data_ptr(), rows, S, H,
                                vocab, ntypes, eps)
            torch.cuda.synchronize()
            assert torch.isnan(out[rows:]).all(), "rows past the output were written"
            outs.append(out[:rows])
        assert torch.equal(_bits(outs[0]), _bits(outs[1])), "out-of-range ids / types are not their clamped rows"
        ic, tc = ids[:rows].clamp(0, vocab - 1).to(DEV), tys[:rows].clamp(0, ntypes - 1).to(DEV)
        p = (torch.arange(rows) % S).to(DEV)
        v = word[PAD + ic].double() + pos[PAD + p].double() + tok[PAD + tc].double()
        return outs[0], v, _ln_ref(v, gamma, beta, eps)

    out, v, ref = run(1.0, 1e-12, True)
    assert (v[[0, 21]] == 0.5).all()
    assert torch.equal(_bits(out[0]), _bits(beta)) and torch.equal(_bits(out[21]), _bits(beta)), "constant rows"
    keep = [r for r in range(rows) if r not in (0, 21)]
    e1 = _row_rel(out[keep], ref[keep])
    assert e1 < 1e-2, e1
    out, v, ref = run(10 ** -2.5 / 3 ** 0.5, 1e-5, False)
    var = v.var(dim=1, unbiased=False)
    assert (var > 0.5e-5).all() and (var < 2e-5).all()
    e2 = _row_rel(out, ref)
    assert e2 < 1e-2, e2
    _report("embed %d" % H, worst_row_rel_l2=e1, worst_row_rel_l2_eps=e2)


@gpu
@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "f32"])
@pytest.mark.parametrize("H", WIDTHS)
def test_qa_head_three_rows_and_canary(H, f32):
    """The span head at rows = 3 (one guarded wave) against fp64 (the
    neighbouring file's 1e-5), nothing past ``rows`` written in either plane."""
    _need_gpu()
    hip = _hip()
    rows = 3
    g = _gen("qa", H, f32)
    dt = torch.float32 if f32 else torch.bfloat16
    x = torch.randn(rows + CANARY_ROWS, H, generator=g).to(dt).to(DEV)
    w = (torch.randn(2, H, generator=g) * 0.05).to(dt).to(DEV)
    b = torch.randn(2, generator=g).to(DEV)
    out = torch.full((2, rows + CANARY_ROWS), float("nan"), device=DEV)
    hip.qa_head(x.data_ptr(), w.data_ptr(), b.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), rows, H, f32=f32)
    torch.cuda.synchronize()
    assert torch.isnan(out[:, rows:]).all(), "logits past rows were written"
    ref = (x[:rows].double() @ w.double().t() + b.double()).t()
    err = ((out[:, :rows].double() - ref).norm() / ref.norm()).item()
    assert err < 1e-5, err
    _report("qa_head %s 3x%d" % ("f32" if f32 else "bf16", H), rel_l2=err)

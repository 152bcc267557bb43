"""K32 ``pool_layernorm`` (csrc/kernels/bert_pool.hip) against a fp64 numpy
reference of its formula on the exact values of the device operands, its batch
invariance, and ``BertLargeQA.embed`` fused against unfused.  Both bounds are
measured ones; how, and the figures: profiles/r26_bert_embed.md."""

import numpy as np
import pytest

from tests.test_bert_embed_cpu import pool_ref

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

H = 1024
EPS = 1e-12
K32_BOUND = 4 * 6.9e-7  # max abs; 4 x the torch fp32 composition's largest error on the cases of test 1
EMBED_BF16_REL = 2 * 7.1e-3  # per-row rel-L2; 2 x the fused / unfused disagreement of forward's hidden states
FORMS = [("k11", False), ("k11", True), ("parts1", False), ("parts3", False), ("parts1", True), ("parts3", True)]


def operands(form, f32, rows, S, seed=0):
    """The device operands of one form: x, then y (k11) or bias and slabs."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    dt = torch.float32 if f32 else torch.bfloat16
    rnd = lambda *shape, scale=1.0, d=dt: (torch.randn(*shape, device="cuda", generator=g) * scale).to(d)
    op = {"x": rnd(rows, S, H), "gamma": (1 + rnd(H, scale=0.1, d=torch.float32)).to(dt), "beta": rnd(H, scale=0.1)}
    if form == "k11":
        op["y"] = rnd(rows, S, H, scale=0.5)
    else:
        op["bias"] = rnd(H, scale=0.1, d=torch.float32)
        op["parts"] = rnd(int(form[5:]), rows, S, H, scale=0.3, d=torch.float32)
    return op


def k32(op, mask, flags, sl):
    """K32 over the rows ``sl`` (a slice) of the operands."""
    from triton_client_amd.ops import hip

    x, m = op["x"][sl].contiguous(), mask[sl].contiguous()
    b, S, _ = x.shape
    f = torch.tensor(flags, device="cuda", dtype=torch.int32)
    ws = torch.empty(hip.pool_layernorm_workspace(b, S) // 4, device="cuda", dtype=torch.float32)
    out = torch.full((b, H), float("nan"), device="cuda")
    tail = (op["gamma"].data_ptr(), op["beta"].data_ptr(), m.data_ptr(), f.data_ptr(), ws.data_ptr(), out.data_ptr(),
            b, S, H, EPS)
    kw = dict(f32=x.dtype == torch.float32, stream=torch.cuda.current_stream().cuda_stream)
    if "y" in op:
        y = op["y"][sl].contiguous()
        hip.pool_layernorm(x.data_ptr(), y.data_ptr(), *tail, **kw)
    else:
        p = op["parts"][:, sl].contiguous()
        hip.pool_layernorm_parts(x.data_ptr(), p.data_ptr(), p.shape[0], b * S * H, op["bias"].data_ptr(), *tail, **kw)
    torch.cuda.synchronize()
    return out


def summed(op, dtype):
    """The LayerNorm's input, summed in ``dtype``."""
    v = op["x"].to(dtype)
    if "y" in op:
        return v + op["y"].to(dtype)
    return v + op["bias"].to(dtype) + op["parts"].to(dtype).sum(0)


def reference(op, mask, flags):
    """fp64 numpy: LayerNorm, then the pooling rules (tests/test_bert_embed_cpu.py pool_ref)."""
    v = summed(op, torch.float64).cpu().numpy()
    d = v - v.mean(-1, keepdims=True)
    h = d / np.sqrt((d * d).mean(-1, keepdims=True) + EPS) * op["gamma"].double().cpu().numpy()
    return pool_ref(h + op["beta"].double().cpu().numpy(), mask.cpu().numpy(), flags)


def masks(S):
    """9 rows: all ones, one token at 0 / at S - 1, the prefixes 47 / 48 / 49 (a slice edge), holes (any
    value >= 1 is valid), an all-zero row next to a full one."""
    t = torch.arange(S, device="cuda")
    return torch.stack([(m * 1).int() for m in (t >= 0, t == 0, t == S - 1, t < 47, t < 48, t < 49,
                                                 (t % 3 != 1) * 2, t < 0, t >= 0)])


@pytest.mark.parametrize("S", [1, 5, 48, 49, 384])
@pytest.mark.parametrize("form, f32", FORMS)
def test_k32_matches_the_fp64_reference(form, f32, S):
    from triton_client_amd.models import bert

    op, mask = operands(form, f32, 9, S), masks(S)
    flags = [0, 1, 2, 2, 0, 1, 1, 2, 0]  # every batch of 3 rows mixes mean, CLS and unnormalised
    want = reference(op, mask, flags)
    got = torch.cat([k32(op, mask, flags[r:r + 3], slice(r, r + 3)) for r in (0, 3, 6)]
                    + [k32(op, mask, flags[r:r + 1], slice(r, r + 1)) for r in (0, 7)]).cpu().numpy()
    h32 = torch.nn.functional.layer_norm(summed(op, torch.float32), (H,), op["gamma"].float(), op["beta"].float(), EPS)
    composed = bert._pool_torch(h32, mask, torch.tensor(flags, device="cuda")).cpu().numpy()
    err = np.abs(got - np.concatenate([want, want[[0, 7]]])).max()
    print("k32 err %.3g torch fp32 composition err %.3g (%s f32=%d S=%d)"
          % (err, np.abs(composed - want).max(), form, f32, S))
    assert not got[7].any() and not got[10].any()  # the all-zero row: exactly zeros
    assert err <= K32_BOUND


@pytest.mark.parametrize("form, f32", [("k11", False), ("parts3", True)])
@pytest.mark.parametrize("flag", [0, 1])
def test_a_row_is_the_same_bits_in_any_batch(form, f32, flag):
    S = 100
    op = operands(form, f32, 128, S, seed=3)
    mask = (torch.arange(S, device="cuda")[None] < torch.randint(1, S + 1, (128, 1), device="cuda")).int()
    for r, rows in ((1, slice(0, 3)), (127, slice(0, 128))):
        alone = k32(op, mask, [flag], slice(r, r + 1))
        batch = k32(op, mask, [flag] * (rows.stop - rows.start), rows)
        assert torch.isfinite(alone).all() and torch.equal(alone[0], batch[r])


@pytest.fixture(scope="module", params=["bf16", "fp32"])
def model(request):
    from triton_client_amd.models import bert

    return bert.build(layers=2) if request.param == "bf16" else bert.prepare_x3(bert.build(dtype=torch.float32, layers=2))


@pytest.mark.parametrize("b", [1, 3])
def test_embed_fused_against_unfused(model, b):
    from triton_client_amd.models import bert

    g = torch.Generator().manual_seed(b)
    ids = torch.randint(1000, 30000, (b, 384), generator=g).cuda()
    mask = (torch.arange(384)[None] < torch.tensor([[384], [100], [49]])[:b]).int().cuda()
    tt = torch.zeros(b, 384, dtype=torch.long, device="cuda")
    with torch.no_grad():
        before = model(ids, mask, tt)
        fused = model.embed(ids, mask, tt)
        after = model(ids, mask, tt)
        bert.FUSED = False
        try:
            plain = model.embed(ids, mask, tt)
        finally:
            bert.FUSED = True
    assert fused.shape == (b, H) and fused.dtype == torch.float32
    assert all(torch.equal(x, y) for x, y in zip(before, after))  # embed leaves forward as it was
    rel = ((fused - plain).norm(dim=1) / plain.norm(dim=1)).max().item()
    err = (fused - plain).abs().max().item()
    print("embed %s fused vs unfused: rel-L2 %.3g max abs %.3g (b=%d)" % (model.word.weight.dtype, rel, err, b))
    assert rel <= EMBED_BF16_REL if model.word.weight.dtype == torch.bfloat16 else err <= K32_BOUND

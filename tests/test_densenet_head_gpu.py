"""K10c x3_classifier (csrc/kernels/densenet_head.hip) and the head that feeds it."""

import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

DEV = "cuda"
SHAPES = [(1000, 1024), (16, 64), (17, 64), (1, 128)]


def _hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from triton_client_amd.ops import hip

    hip.lib()
    return hip


def _case(b, N, K, seed=0):
    """Model-like inputs: pooled >= 0 (after ReLU), weights of std 0.03."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    a = torch.randn(b, K, device=DEV, generator=g).relu()
    w = torch.randn(N, K, device=DEV, generator=g) * 0.03
    bias = torch.randn(N, device=DEV, generator=g) * 0.03
    return a, w, bias


def _split(t):
    return t.to(torch.bfloat16), (t - t.to(torch.bfloat16).float()).to(torch.bfloat16)


def _run(hip, a, w, bias, out, ldc=None):
    (ah, al), (wh, wl) = _split(a), hip.x3_classifier_weights(w)
    hip.x3_classifier(ah.data_ptr(), al.data_ptr(), wh.data_ptr(), wl.data_ptr(), bias.data_ptr(), out.data_ptr(),
                      a.shape[0], w.shape[0], w.shape[1], ldc=ldc, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("N,K", SHAPES)
@pytest.mark.parametrize("b", [1, 15, 16, 17, 33, 128])
def test_classifier_matches_fp64_and_stores_nothing_else(b, N, K):
    """max |err| / max |ref| under 1e-5, the bound of the bf16x3 GEMM tests (tests/test_gemm_gpu.py);
    with ldc = N + 3 every element outside [0, b) x [0, N), the row past b included, keeps its NaN."""
    hip, (a, w, bias) = _hip(), _case(b, N, K, seed=b * 7 + N)
    out = _run(hip, a, w, bias, torch.full((b + 1, N + 3), float("nan"), device=DEV), ldc=N + 3)
    ref = a.double() @ w.double().T + bias.double()
    err = ((out[:b, :N].double() - ref).abs().max() / ref.abs().max()).item()
    lib = ((torch.addmm(bias, a, w.T).double() - ref).abs().max() / ref.abs().max()).item()
    print("b=%d N=%d K=%d: K10c %.3g, fp32 addmm %.3g" % (b, N, K, err, lib))
    assert err < 1e-5
    assert torch.isnan(out[:b, N:]).all() and torch.isnan(out[b:]).all()


@pytest.mark.parametrize("N,K", SHAPES)
@pytest.mark.parametrize("b", [17, 128])
def test_a_row_has_the_same_bits_in_every_batch(b, N, K):
    hip, (a, w, bias) = _hip(), _case(b, N, K, seed=3)
    row = a[5:6].clone()
    alone = _run(hip, row, w, bias, torch.empty(1, N, device=DEV))
    for pos in (0, 15, 16, b - 1):
        batch = a.clone()
        batch[pos] = row[0]
        got = _run(hip, batch, w, bias, torch.empty(b, N, device=DEV))
        assert torch.equal(got[pos], alone[0]), pos


@pytest.mark.parametrize("b", [1, 3])
def test_head_pool_split(b):
    """hi + lo is x3_head_pool's value to one ulp of the lo plane; the fp32 rows are its rows, bitwise."""
    hip = _hip()
    HW, C, st = 49, 1024, torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device=DEV).manual_seed(b)
    x = torch.randn(b * HW, C, device=DEV, generator=g)
    s, t = torch.rand(C, device=DEV, generator=g) + 0.5, torch.randn(C, device=DEV, generator=g)
    ref, out = torch.empty(b, C, device=DEV), torch.empty(b, C, device=DEV)
    hi, lo = (torch.empty(b, C, device=DEV, dtype=torch.bfloat16) for _ in range(2))
    hip.x3_head_pool(x.data_ptr(), s.data_ptr(), t.data_ptr(), ref.data_ptr(), b, HW, C, stream=st)
    hip.x3_head_pool_split(x.data_ptr(), s.data_ptr(), t.data_ptr(), hi.data_ptr(), lo.data_ptr(), b, HW, C,
                           out=out.data_ptr(), stream=st)
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
    rh, rl = _split(ref)
    assert torch.equal(hi, rh) and torch.equal(lo, rl)
    ulp = torch.ldexp(torch.ones_like(ref), torch.frexp(lo.float()).exponent - 8)  # bf16: 8 significant bits
    assert ((hi.float() + lo.float() - ref).abs() <= ulp).all()


@pytest.fixture(scope="module")
def engines():
    _hip()
    from triton_client_amd.models import densenet_fp32

    fused, model = densenet_fp32.build(max_batch=3, device=DEV, classifier="fused")
    return fused, densenet_fp32.FusedDenseNetFP32(model, 3, DEV), model


@pytest.mark.parametrize("b", [1, 3])
def test_engine_with_the_fused_head(engines, b):
    """classifier="fused": logits within the engine tests' 1e-3 rel-L2 of the
    fp32 module; "lib" is still the library's GEMM on the fp32 pooled rows."""
    fused, lib, model = engines
    x = torch.randn(3, 3, 224, 224, device=DEV, generator=torch.Generator(device=DEV).manual_seed(11))[:b]
    out = torch.empty(3, 1000, device=DEV)
    with torch.no_grad():
        got, ref = fused(x), model.to(DEV).float()(x)
        got_lib = lib(x)
        assert torch.equal(got_lib, torch.nn.functional.linear(lib.pooled[:b], lib.wc, lib.bc))
        ret = lib(x, out=out)
        assert torch.equal(ret, torch.addmm(lib.bc, lib.pooled[:b], lib.wc.t())) and ret.data_ptr() == out.data_ptr()
    err = ((got.double() - ref.double()).norm() / ref.double().norm()).item()
    print("fused head b=%d rel-L2 vs fp32 module: %.3g" % (b, err))
    assert err < 1e-3


def test_engine_row_has_the_same_bits_at_b1_and_b3(engines):
    """A row's logits from the b = 1 and the b = 3 forward of the fused-head
    engine are the same bits: the body keeps to its batch-invariant routes."""
    fused = engines[0]
    x = torch.randn(3, 3, 224, 224, device=DEV, generator=torch.Generator(device=DEV).manual_seed(11))
    with torch.no_grad():
        got = fused(x).clone()
        alone = fused(x[2:3].contiguous())
    d = (alone[0] - got[2]).abs()
    print("logits differ at %d of 1000, max %.3g" % ((d > 0).sum().item(), d.max().item()))
    assert torch.equal(alone[0], got[2])


def test_classifier_argument_checks():
    hip, (a, w, bias), out = _hip(), _case(4, 16, 64), torch.full((4, 16), 7.0, device=DEV)
    (ah, al), (wh, wl) = _split(a), hip.x3_classifier_weights(w)
    args = [ah.data_ptr(), al.data_ptr(), wh.data_ptr(), wl.data_ptr(), bias.data_ptr(), out.data_ptr()]
    hip.x3_classifier(*args, 0, 16, 64)  # no rows: no launch
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    for bad in ([*args, 129, 16, 64], [*args, 4, 16, 96], [args[0] + 2, *args[1:], 4, 16, 64]):
        with pytest.raises(hip.HipError):
            hip.x3_classifier(*bad)

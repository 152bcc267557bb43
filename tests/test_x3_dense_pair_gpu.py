"""K14x pair (`x3_dense_small_pair_kernel<14, 2>`): dense layers j and j+1 of
a 14x14 block in one launch on one read of the block input, and the engine's
routing on top of it (`FusedDenseNetFP32.smallf_pair`).

Kernel level, against fp64 torch: 1, 3 and 9 images (none a multiple of 8:
every launch has blocks that leave at once, and every tile is a top-edge or a
bottom-edge tile), K = 64, 256 and 960 (K / 32 even and odd, the K rotation
wrapping, the widest K with K + 64 <= 1024), the block row length 1024 and
K + 64.  One launch per case, shared by the tests that read its result.
"""

import pytest

torch = pytest.importorskip("torch")
import torch.nn.functional as F  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
H = 14
TILES = 2  # every (W, tiles) the pair kernel is routed at: (14, 2)
CASES = [(imgs, K, 1024) for imgs in (1, 3, 9) for K in (64, 256, 960)] + [(3, 256, 256 + 64)]
PATTERN = 0x7FC5A5A5  # a NaN with a payload: a read of it shows, a write over it shows


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _hip():
    from triton_client_amd.ops import hip

    hip.lib()
    return hip


def _rel(got, ref):
    got, ref = got.double(), ref.double()
    assert torch.isfinite(got).all()
    return ((got - ref).norm() / ref.norm().clamp_min(1e-30)).item()


def _split(t):
    hi = t.to(torch.bfloat16)
    lo = (t - hi.float()).to(torch.bfloat16)
    return hi.contiguous(), lo.contiguous()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _layer(hip, g, K):
    """One dense layer's parameters for K input channels: the tensors and the K14x pointer tuple."""
    s = torch.rand(K, device=DEV, generator=g) + 0.5
    t = torch.randn(K, device=DEV, generator=g) * 0.2
    w1 = torch.randn(128, K, device=DEV, generator=g) / K ** 0.5
    b1 = torch.randn(128, device=DEV, generator=g) * 0.1
    w2 = torch.randn(32, 128, 3, 3, device=DEV, generator=g) / (9 * 128) ** 0.5
    f1h, f1l = (hip.x3_w1_fragments(u) for u in _split(w1))
    f2h, f2l = (hip.x3_w3f_fragments(u) for u in _split(w2.permute(0, 2, 3, 1).reshape(32, -1)))
    keep = (s, t, f1h, f1l, b1, f2h, f2l)
    return {"s": s, "t": t, "w1": w1, "b1": b1, "w2": w2, "keep": keep, "ptrs": tuple(u.data_ptr() for u in keep)}


def _ref(xin, L, imgs):
    """fp64 dense layer over [pixels][K] rows of 14x14 images."""
    a = torch.relu(xin.double() * L["s"].double() + L["t"].double())
    z = torch.relu(a @ L["w1"].double().t() + L["b1"].double()).reshape(imgs, H, H, 128).permute(0, 3, 1, 2)
    return F.conv2d(z, L["w2"].double(), padding=1).permute(0, 2, 3, 1).reshape(imgs * H * H, 32)


_RUNS = {}


def _run(case):
    """One pair launch per case (and the two single launches it replaces), kept for every test."""
    if case in _RUNS:
        return _RUNS[case]
    hip = _hip()
    imgs, K, ldx = case
    g = torch.Generator(device=DEV).manual_seed(imgs * 1009 + K * 3 + ldx)
    M = imgs * H * H
    # one more image than the launch is told of: its rows must come back untouched
    x = torch.empty((imgs + 1) * H * H, ldx, device=DEV)
    x.view(torch.int32).fill_(PATTERN)
    x[:M, :K] = torch.randn(M, K, device=DEV, generator=g)
    x[:M, K:K + 64] = float("nan")
    L1, L2 = _layer(hip, g, K), _layer(hip, g, K + 32)
    before = x.clone()
    hip.x3_dense_small_pair(x.data_ptr(), ldx, imgs, H, H, K, L1["ptrs"], L2["ptrs"], x.data_ptr() + 4 * K, ldx,
                            stream=_st(), tiles=TILES)
    single = before.clone()
    for L, k in ((L1, K), (L2, K + 32)):
        hip.x3_dense_small(single.data_ptr(), ldx, imgs, H, H, k, *L["ptrs"], single.data_ptr() + 4 * k, ldx,
                           stream=_st(), tiles=TILES)
    torch.cuda.synchronize()
    _RUNS[case] = {"x": x, "before": before, "single": single, "L1": L1, "L2": L2}
    return _RUNS[case]


def _check(name, got, ref, imgs):
    err = _rel(got, ref)
    per_img = (got.double() - ref).reshape(imgs, -1).norm(dim=1) / ref.reshape(imgs, -1).norm(dim=1)
    print("%s: rel %.3g, worst image %.3g" % (name, err, per_img.max().item()))
    assert err < 3e-5 and per_img.max().item() < 1e-4


@pytest.mark.parametrize("case", CASES)
def test_pair_layers_match_fp64(case):
    """Layer j against fp64 torch, and layer j+1 against fp64 torch on the y_j
    the kernel itself wrote (which isolates the second layer): rel-L2 < 3e-5
    and < 1e-4 per image, the bounds of test_x3_dense_small."""
    _need_gpu()
    imgs, K, ldx = case
    r = _run(case)
    M = imgs * H * H
    x = r["x"]
    _check("pair layer j   imgs %d K %d ldx %d" % case, x[:M, K:K + 32], _ref(x[:M, :K], r["L1"], imgs), imgs)
    _check("pair layer j+1 imgs %d K %d ldx %d" % case, x[:M, K + 32:K + 64], _ref(x[:M, :K + 32], r["L2"], imgs),
           imgs)


@pytest.mark.parametrize("case", CASES)
def test_pair_matches_two_single_launches(case):
    """Both outputs against two x3_dense_small launches at the same tiling:
    < 2e-5, the bound between two tilings of one layer."""
    _need_gpu()
    imgs, K, _ = case
    r = _run(case)
    M = imgs * H * H
    for lo in (K, K + 32):
        e = _rel(r["x"][:M, lo:lo + 32], r["single"][:M, lo:lo + 32])
        print("pair vs singles imgs %d K %d channels %d..: %.3g" % (imgs, K, lo, e))
        assert e < 2e-5


@pytest.mark.parametrize("case", CASES)
def test_pair_write_footprint(case):
    """Only channels [K, K + 64) of the launch's own images change, and every
    element of them is written: the NaN pre-fill is gone, the pattern in the
    channels past K + 64 and in the image after the last one is bit-identical,
    and the inputs are."""
    _need_gpu()
    imgs, K, _ = case
    r = _run(case)
    M = imgs * H * H
    x, before = r["x"].view(torch.int32), r["before"].view(torch.int32)
    assert torch.isfinite(r["x"][:M, K:K + 64]).all()
    assert torch.equal(x[:M, :K], before[:M, :K])
    assert torch.equal(x[:M, K + 64:], before[:M, K + 64:])
    assert torch.equal(x[M:], before[M:])
    assert (x[M:] == PATTERN).all() and (x[:M, K + 64:] == PATTERN).all()


def test_pair_supported_answers_the_routed_tilings():
    _need_gpu()
    hip = _hip()
    assert hip.x3_dense_small_pair_supported(14, 2)
    for W, tiles in [(14, 1), (14, 4), (14, 7), (7, 1), (7, 2), (7, 4), (28, 2), (14, 0)]:
        assert not hip.x3_dense_small_pair_supported(W, tiles)


def test_pair_rejects():
    """Bad W, tilings without a pair kernel, a block row shorter than K + 64,
    K off the grid, misaligned pointers: errors, nothing launched.  imgs <= 0:
    success, nothing launched."""
    _need_gpu()
    hip = _hip()
    ldx, K = 384, 256
    x = torch.zeros(2 * H * H, ldx, device=DEV)
    w = torch.zeros(128 * 320, device=DEV)
    p = (w.data_ptr(),) * 7

    def call(Hh=14, W=14, K=K, ldx=ldx, tiles=2, xp=x.data_ptr(), l1=p, l2=p, imgs=2, ldy=ldx, yoff=0):
        hip.x3_dense_small_pair(xp, ldx, imgs, Hh, W, K, l1, l2, x.data_ptr() + 4 * K + yoff, ldy, stream=_st(),
                                tiles=tiles)

    bad = [dict(Hh=28, W=28), dict(Hh=7, W=7, tiles=1), dict(Hh=7, W=7, tiles=2), dict(Hh=14, W=7),
           dict(tiles=1), dict(tiles=4), dict(tiles=7), dict(tiles=3),
           dict(ldx=K + 32), dict(K=250), dict(K=32), dict(K=2048, ldx=4096), dict(ldx=ldx + 2), dict(ldy=ldx + 2),
           dict(xp=x.data_ptr() + 4), dict(yoff=4)]
    bad += [dict(l1=p[:i] + (w.data_ptr() + 4,) + p[i + 1:]) for i in range(7)]
    bad += [dict(l2=p[:i] + (w.data_ptr() + 4,) + p[i + 1:]) for i in range(7)]
    bad += [dict(l2=p[:3] + (0,) + p[4:])]
    for kw in bad:
        with pytest.raises(Exception):
            call(**kw)
    x.fill_(3.0)
    for imgs in (0, -1):
        call(imgs=imgs)
    torch.cuda.synchronize()
    assert (x == 3.0).all()


@pytest.fixture(scope="module")
def fp32_engine():
    _need_gpu()
    from triton_client_amd.models import densenet_fp32

    eng, model = densenet_fp32.build(max_batch=8, device=DEV)
    return eng, model.to(DEV).float()


def test_engine_pairs_the_14x14_block(fp32_engine):
    """Half-image tiles forced and K14x on at every batch, so 3 images take the
    pair kernel through block 3 (block 4 stays on single layers).  Logits
    against TCAMD_X3_SMALLF_PAIR=0 (< 2e-5, two routes of one engine) and the
    fp32 torch module (< 1e-3, the bound of test_fp32_engine_matches_fp32_module);
    then the forward captured into a graph once and replayed twice: both
    replays within the same bound of the eager run."""
    eng, model = fp32_engine
    hip = _hip()
    b = 3
    g = torch.Generator(device=DEV).manual_seed(1300 + b)
    x = torch.randn(b, 3, 224, 224, device=DEV, generator=g)
    keep = eng.smallf_tiles, eng.smallf_min_blocks, eng.smallf_pair
    calls = []
    real = hip.x3_dense_small_pair

    def counted(*a, **k):
        calls.append(a[5])
        return real(*a, **k)

    try:
        eng.smallf_tiles, eng.smallf_min_blocks, eng.smallf_pair = 2, 1, 1
        assert eng._small_fused(b, 14) and eng._small_tiles(b, 14) == 2
        hip.x3_dense_small_pair = counted
        try:
            with torch.no_grad():
                got = eng(x).clone()
        finally:
            hip.x3_dense_small_pair = real
        n3 = len(eng.blocks[2])
        assert calls == [eng.blocks[2][j]["cin"] for j in range(0, n3 - 1, 2)]
        eng.smallf_pair = 0
        with torch.no_grad():
            single = eng(x).clone()
            ref = model(x)
        eng.smallf_pair = 1
        out = torch.empty(b, 1000, device=DEV)
        s = torch.cuda.Stream(DEV)
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s), torch.no_grad():
            eng(x, out=out)
            s.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=s):
                eng(x, out=out)
            replays = []
            for _ in range(2):
                out.zero_()
                graph.replay()
                s.synchronize()
                replays.append(out.clone())
    finally:
        eng.smallf_tiles, eng.smallf_min_blocks, eng.smallf_pair = keep
    torch.cuda.synchronize()
    e_single, e_ref = _rel(got, single), _rel(got, ref)
    e_rep = [_rel(r, got) for r in replays]
    print("pair engine b=%d: rel vs single layers %.3g, vs fp32 module %.3g, graph replays vs eager %.3g %.3g"
          % (b, e_single, e_ref, e_rep[0], e_rep[1]))
    assert e_single < 2e-5 and e_ref < 1e-3
    assert max(e_rep) < 2e-5

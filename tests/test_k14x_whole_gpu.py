"""K14x tiling when concurrent streams share the chip: whole 7x7 images (one
tile, `x3_dense_small_kernel<7, 1>`) once a stream's batch alone fills its
share of the CUs (`tcamd_x3_small_tiles_shared`), and the engine's routing
on top of it.

The `<7, 1>` kernel itself is covered per layer by
tests/test_densenet_fp32_gpu.py::test_x3_dense_small (tiles = 1 at 7x7, 1 to
130 images, K 64 to 1024).  A whole-image 14x14 kernel was built and measured
and is not part of the library (profiles/r7_k14x_whole.md: no gain on two
streams), so the shared rule answers for 14x14 what `tcamd_x3_small_tiles`
answers and there is no whole-image entry point to test.
"""

import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

DEV = "cuda"


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


def test_shared_rule_whole_7x7_images_from_a_full_share():
    """On a 256-CU device: 1 tile at 7x7 for 128 and 256 images on 2 streams
    (padded images >= CUs / streams); the one-stream answer on 1 stream, at
    64 images on 2 streams, and at 14x14 everywhere.  On any device: 1 exactly
    when W = 7, streams >= 2 and the padded image count reaches CUs // streams."""
    _need_gpu()
    hip = _hip()
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    if ncu == 256:
        for imgs in (128, 256):
            assert hip.x3_small_tiles_shared(imgs, 7, 2) == 1
            assert hip.x3_small_tiles_shared(imgs, 14, 2) == hip.x3_small_tiles(imgs, 14) == 2
            for W in (7, 14):
                assert hip.x3_small_tiles_shared(imgs, W, 1) == hip.x3_small_tiles(imgs, W)
        assert hip.x3_small_tiles(128, 7) == 2
        for W in (7, 14):
            assert hip.x3_small_tiles_shared(64, W, 2) == hip.x3_small_tiles(64, W) == 4
        assert hip.x3_small_tiles_shared(120, 7, 2) == hip.x3_small_tiles(120, 7)  # padded 120 < 128
        assert hip.x3_small_tiles_shared(121, 7, 2) == 1
    for W in (7, 14):
        for streams in (0, 1, 2, 3, 4):
            for imgs in (1, 8, 9, 24, 32, 40, 63, 64, 65, 88, 120, 121, 128, 129, 256, 1000):
                padded = (imgs + 7) // 8 * 8
                whole = W == 7 and streams >= 2 and padded >= ncu // streams
                want = 1 if whole else hip.x3_small_tiles(imgs, W)
                assert hip.x3_small_tiles_shared(imgs, W, streams) == want, (imgs, W, streams)


@pytest.fixture(scope="module")
def fp32_engine():
    _need_gpu()
    from triton_client_amd.models import densenet_fp32

    eng, model = densenet_fp32.build(max_batch=16, device=DEV)
    return eng, model.to(DEV).float()


def test_engine_tiles_follow_the_shared_rule(fp32_engine):
    """`_small_tiles`: whole 7x7 images exactly where the native shared rule
    says so for the engine's stream count; TCAMD_X3_SMALLF_SHARED=0 and one
    stream keep the one-stream tiling (so b <= 40 on 1 or 2 streams is what it
    was); 14x14 never takes 1 tile; a forced TCAMD_X3_SMALLF_TILES wins.
    (Batches beyond the engine's capacity: the rule reads only the counts.)"""
    eng, _ = fp32_engine
    hip = _hip()
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    keep = eng.smallf_tiles, eng.concurrent_streams, eng.smallf_shared
    try:
        eng.smallf_tiles = 0
        for b in (8, 16, 40, 64, 120, 121, 128, 256):
            padded = (b + 7) // 8 * 8
            for streams in (1, 2, 3):
                eng.concurrent_streams, eng.smallf_shared = streams, 0
                old7, old14 = eng._small_tiles(b, 7), eng._small_tiles(b, 14)
                assert old7 == hip.x3_small_tiles(b, 7) and old14 != 1
                eng.smallf_shared = 1
                whole = streams >= 2 and padded >= ncu // streams
                assert eng._small_tiles(b, 7) == (1 if whole else old7), (b, streams)
                assert eng._small_tiles(b, 14) == old14, (b, streams)
        eng.concurrent_streams, eng.smallf_shared, eng.smallf_tiles = 2, 1, 4
        assert eng._small_tiles(128, 7) == 4
    finally:
        eng.smallf_tiles, eng.concurrent_streams, eng.smallf_shared = keep


@pytest.mark.parametrize("b", [3, 9])  # 9: ragged against the grid's groups of 8 images
def test_engine_whole_7x7_images_on_shared_chip(fp32_engine, b):
    """The engine with K14x on at every batch and so many concurrent streams
    that b images already fill one stream's share of the CUs: the 7x7 block
    runs whole images by the shared rule.  Against the fp32 module and
    against the K8x + K9x pair path, with the bounds of
    test_fp32_engine_k14x_blocks_match_fp32_module (the same bound between
    two routes against the one-stream tiling, which TCAMD_X3_SMALLF_SHARED=0
    gives back)."""
    eng, model = fp32_engine
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    padded = (b + 7) // 8 * 8
    g = torch.Generator(device=DEV).manual_seed(700 + b)
    x = torch.randn(b, 3, 224, 224, device=DEV, generator=g)
    keep = eng.smallf_min_blocks, eng.concurrent_streams, eng.smallf_shared, eng.smallf_tiles
    try:
        eng.smallf_tiles, eng.smallf_shared = 0, 1
        eng.concurrent_streams = -(-ncu // padded)  # the fewest streams with ncu // streams <= padded
        eng.smallf_min_blocks = 1
        assert eng._small_tiles(b, 7) == 1 and eng._small_fused(b, 7) and eng._small_fused(b, 14)
        with torch.no_grad():
            got = eng(x).clone()
        eng.smallf_shared = 0
        assert eng._small_tiles(b, 7) > 1
        with torch.no_grad():
            split = eng(x).clone()
        eng.smallf_min_blocks = 0
        with torch.no_grad():
            base = eng(x).clone()
            ref = model(x)
    finally:
        eng.smallf_min_blocks, eng.concurrent_streams, eng.smallf_shared, eng.smallf_tiles = keep
    torch.cuda.synchronize()
    e_ref, e_base, e_split = _rel(got, ref), _rel(got, base), _rel(got, split)
    print("whole 7x7 engine b=%d: rel vs fp32 module %.3g, vs the pair path %.3g, vs split tiles %.3g"
          % (b, e_ref, e_base, e_split))
    assert e_ref < 1e-3 and e_base < 1e-4 and e_split < 1e-4

"""K11x (hip.x3_dense_fused, v1, and hip.x3_dense_fused3, v3) on the shapes that
reach every path of its tile-to-tile index carry (csrc/kernels/x3_ring_math.h):
the 3x3's row addresses are carried from one 64-pixel tile of a block to the
next instead of divided out per tile, so what matters is how many tiles a block
walks, where the ring, the image rows and the images wrap inside that walk, and
the ragged end.

Each shape is (imgs, H, W, K), stated for a 256-CU device (the grid is one
block per CU, tiles per block = ceil(tiles / CUs)); on another CU count the
image count is derived so that the tiles per block stay as stated.  Every
shape is checked three ways, for v1 and v3: against an fp64 torch reference of
the layer (rel-L2 < 3e-5 overall and < 1e-4 for every image, the bounds of the
K14x tests in tests/test_densenet_fp32_gpu.py), torch.equal between v1 and v3
(the two run the same products in the same order), and the write footprint
(every channel outside the layer's 32 untouched).  The inputs, the reference
and both outputs of a shape are computed once and shared by its tests."""

import functools

import pytest

torch = pytest.importorskip("torch")
F = torch.nn.functional

pytestmark = pytest.mark.gpu

DEV = "cuda"

# (imgs, H, W, K) at 256 CUs: tiles per block, what the walk crosses
SHAPES = [
    (257, 16, 16, 64),    # 5: the 192-row ring wraps inside a block
    (1300, 5, 17, 64),    # 7: odd W, H * W = 85, an image boundary in almost every tile
    (70, 20, 20, 96),     # 2: odd NST
    (330, 28, 28, 128),   # 16
    (21, 56, 56, 64),     # 5 at the widest ring band
    (1, 56, 56, 224),     # 1: prologue and last-tile path only
    (16, 28, 28, 480),    # 1: NST 15
    (3, 28, 28, 192),     # 1: M = 2352 ends 48 pixels into its last tile
]
IDS = ["%dx%dx%d_k%d" % s for s in SHAPES]


def _tiles_per_block(imgs, H, W, ncu):
    tiles = (imgs * H * W + 63) // 64
    return (tiles + min(tiles, ncu) - 1) // min(tiles, ncu)


def _imgs_for(shape, ncu):
    """The image count that walks the stated tiles per block on ncu CUs."""
    imgs, H, W, _ = shape
    want = _tiles_per_block(imgs, H, W, 256)
    if ncu == 256 or want == 1 and (imgs * H * W + 63) // 64 <= ncu:
        return imgs, want
    if want == 1:  # fewer CUs than the stated shape has tiles: one tile per block is all that is asked
        return max(1, ncu * 64 // (H * W)), 1
    n = ((want - 1) * ncu * 64 + H * W) // (H * W)  # the fewest images with more than (want - 1) * ncu tiles
    return n, want


def _split(t):
    hi = t.to(torch.bfloat16)
    lo = (t - hi.float()).to(torch.bfloat16)
    return hi.contiguous(), lo.contiguous()


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Runs v1 and v3 on one shape; the figures its tests assert on."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from triton_client_amd.ops import hip

    hip.lib()
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    imgs, tpb = _imgs_for(shape, ncu)
    _, H, W, K = shape
    assert _tiles_per_block(imgs, H, W, ncu) == tpb
    M, ldx = imgs * H * W, K + 64
    g = torch.Generator(device=DEV).manual_seed(H * 1009 + W * 31 + K)
    x0 = torch.randn(M, ldx, device=DEV, generator=g)
    s = torch.rand(K, device=DEV, generator=g) + 0.5
    t = torch.randn(K, device=DEV, generator=g) * 0.2
    w1 = torch.randn(128, K, device=DEV, generator=g) / K ** 0.5
    b1 = torch.randn(128, device=DEV, generator=g) * 0.1
    w2 = torch.randn(32, 128, 3, 3, device=DEV, generator=g) / (9 * 128) ** 0.5
    f1h, f1l = (hip.x3_w1_fragments(u) for u in _split(w1))
    f2h, f2l = (hip.x3_w3f_fragments(u) for u in _split(w2.permute(0, 2, 3, 1).reshape(32, -1)))
    a = torch.relu(x0[:, :K].double() * s.double() + t.double())
    z = torch.relu(a @ w1.double().t() + b1.double()).reshape(imgs, H, W, 128).permute(0, 3, 1, 2)
    ref = F.conv2d(z, w2.double(), padding=1).permute(0, 2, 3, 1).reshape(M, 32)
    del a, z
    st = torch.cuda.current_stream().cuda_stream
    out, ys = {"imgs": imgs, "tiles_per_block": tpb}, {}
    for v, fn in ((1, hip.x3_dense_fused), (3, hip.x3_dense_fused3)):
        x = x0.clone()
        fn(x.data_ptr(), ldx, imgs, H, W, K, s.data_ptr(), t.data_ptr(), f1h.data_ptr(), f1l.data_ptr(),
           b1.data_ptr(), f2h.data_ptr(), f2l.data_ptr(), x.data_ptr() + 4 * K, ldx, stream=st)
        torch.cuda.synchronize()
        y = x[:, K:K + 32]
        d = y.double() - ref
        out[v] = {
            "finite": bool(torch.isfinite(y).all()),
            "rel": (d.norm() / ref.norm()).item(),
            "worst_image": (d.reshape(imgs, -1).norm(dim=1) / ref.reshape(imgs, -1).norm(dim=1)).max().item(),
            "untouched": torch.equal(x[:, :K], x0[:, :K]) and torch.equal(x[:, K + 32:], x0[:, K + 32:]),
        }
        ys[v] = y.clone()
        del x
    out["v1_equals_v3"] = torch.equal(ys[1], ys[3])
    print("K11x %s: imgs %d, %d tiles per block, v1 rel %.3g worst image %.3g, v3 rel %.3g worst image %.3g, equal %s"
          % (shape, imgs, tpb, out[1]["rel"], out[1]["worst_image"], out[3]["rel"], out[3]["worst_image"],
             out["v1_equals_v3"]))
    return out


@pytest.mark.parametrize("version", [1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_against_fp64(shape, version):
    r = _case(shape)[version]
    assert r["finite"]
    assert r["rel"] < 3e-5 and r["worst_image"] < 1e-4, r


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_v1_and_v3_are_bit_identical(shape):
    assert _case(shape)["v1_equals_v3"]


@pytest.mark.parametrize("version", [1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_write_footprint(shape, version):
    assert _case(shape)[version]["untouched"]

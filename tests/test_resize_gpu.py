"""K20 resize_pack (csrc/kernels/resize.hip) against the project's definition
of image preprocessing, utils.image.preprocess evaluated in float64.

Tolerance (derived, not tuned): at most 8 fp32 roundings act on values <= 256
before the affine step, so
    |got - ref| <= 8 * 2^-24 * 256 * |scale_c| + 2^-23 * |ref|
(1.2e-4 on the 0..255 scale), plus one ulp of the format at |ref| for 16-bit
outputs.  Every destination is its own slice of one canary-filled buffer, and
every run checks that the bytes between and after the slices are intact."""

import functools

import numpy as np
import pytest

from triton_client_amd.utils import image

pytestmark = pytest.mark.gpu

CANARY = 0xA5
GAP = 64  # canary bytes before, between and after the destinations
_ESZ = {"FP32": 4, "FP16": 2, "BF16": 2}
_SCALE = {"NONE": 1.0, "INCEPTION": 1.0 / 127.5, "VGG": 1.0}

SHAPES = [
    ((1, 1, 3), (3, 4, 4)),
    ((5, 7, 3), (3, 8, 8)),
    ((17, 13, 3), (3, 4, 4)),
    ((8, 8, 3), (3, 8, 8)),
    ((9, 6, 1), (3, 5, 5)),
    ((6, 9, 3), (1, 7, 3)),
    ((3000, 2, 3), (3, 224, 224)),
    ((2, 16000, 1), (1, 4, 16384)),
    ((480, 640, 3), (3, 224, 224)),  # the served shape
]


@pytest.fixture(scope="module")
def env():
    import torch

    from triton_client_amd.ops import hip

    torch.cuda.set_device(0)
    return torch, hip


@functools.lru_cache(maxsize=None)
def _image(shape, seed=0):
    rng = np.random.default_rng(shape[0] * 1000003 + shape[1] * 1009 + shape[2] + seed)
    img = rng.integers(0, 256, shape, dtype=np.uint8)
    img.setflags(write=False)
    return img


def _ulp16(ref, dtype):
    """One ulp of the 16-bit format at |ref| (0 for FP32 outputs)."""
    if dtype == "FP32":
        return np.zeros_like(ref)
    mant, emin = (10, -14) if dtype == "FP16" else (7, -126)
    e = np.floor(np.log2(np.maximum(np.abs(ref), 2.0 ** emin)))
    return 2.0 ** (e - mant)


def _bound(ref, scaling, dtype):
    return 8 * 2.0 ** -24 * 256 * _SCALE[scaling] + 2.0 ** -23 * np.abs(ref) + _ulp16(ref, dtype)


def _decode(raw, dtype):
    if dtype == "FP32":
        return raw.view(np.float32).astype(np.float64)
    if dtype == "FP16":
        return raw.view(np.float16).astype(np.float64)
    return (raw.view(np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def _run(env, imgs, C, H, W, scaling, fmt, dtype="FP32", src_offsets=None, dst_shift=0, rounding="rne"):
    """Resize ``imgs`` in one resize_pack call; returns the outputs as float64
    arrays in ``fmt`` order after checking every canary byte."""
    torch, hip = env
    n = len(imgs)
    src_offsets = src_offsets or [0] * n
    pos, starts = 0, []
    for im, o in zip(imgs, src_offsets):
        pos = (pos + 15) // 16 * 16  # the offset is the source pointer's misalignment
        starts.append(pos + o)
        pos += o + im.size + 8
    host = np.zeros(pos, dtype=np.uint8)
    for im, s in zip(imgs, starts):
        host[s:s + im.size] = im.reshape(-1)
    src = torch.from_numpy(host).cuda()
    per = C * H * W * _ESZ[dtype]
    pitch = (per + GAP + 15) // 16 * 16
    first = GAP + dst_shift
    total = first + n * pitch + GAP
    buf = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    dsts = [buf.data_ptr() + first + i * pitch for i in range(n)]
    scale, bias = image._SCALE_BIAS[scaling](C)
    assert src.data_ptr() % 16 == 0
    hip.resize_pack([src.data_ptr() + s for s in starts], [im.shape for im in imgs], dsts, dtype, fmt, C, H, W,
                    scale=scale, bias=bias, rounding=rounding, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    raw = buf.cpu().numpy()
    mask = np.ones(total, dtype=bool)
    outs = []
    shape = (C, H, W) if fmt == "NCHW" else (H, W, C)
    for i in range(n):
        a = first + i * pitch
        mask[a:a + per] = False
        outs.append(_decode(raw[a:a + per].copy(), dtype).reshape(shape))
    assert (raw[mask] == CANARY).all(), "bytes outside the destinations were written"
    return outs


def _check(got, img, C, H, W, scaling, fmt, dtype, what):
    ref = image.preprocess(img, C, H, W, scaling, fmt, np.float64)
    err = np.abs(got - ref)
    bound = _bound(ref, scaling, dtype)
    print("%s: max err %.3g, smallest bound %.3g, worst err/bound %.3g" % (what, err.max(), bound.min(),
                                                                           (err / bound).max()))
    assert (err <= bound).all(), what


@pytest.mark.parametrize("fmt", ["NCHW", "NHWC"])
@pytest.mark.parametrize("scaling", ["NONE", "INCEPTION", "VGG"])
@pytest.mark.parametrize("src,dst", SHAPES)
def test_resize_matches_float64_preprocess(env, src, dst, scaling, fmt):
    C, H, W = dst
    img = _image(src)
    (got,) = _run(env, [img], C, H, W, scaling, fmt)
    _check(got, img, C, H, W, scaling, fmt, "FP32", "%s->%s %s %s" % (src, dst, scaling, fmt))


@pytest.mark.parametrize("dtype", ["FP16", "BF16"])
@pytest.mark.parametrize("fmt", ["NCHW", "NHWC"])
@pytest.mark.parametrize("src,dst", [((5, 7, 3), (3, 8, 8)), ((9, 6, 1), (3, 5, 5))])
def test_resize_16bit_outputs(env, src, dst, fmt, dtype):
    C, H, W = dst
    img = _image(src)
    for scaling in ("NONE", "INCEPTION", "VGG"):
        (got,) = _run(env, [img], C, H, W, scaling, fmt, dtype)
        _check(got, img, C, H, W, scaling, fmt, dtype, "%s->%s %s %s %s" % (src, dst, scaling, fmt, dtype))


@pytest.mark.parametrize("dtype,shift", [("FP32", 4), ("FP16", 2), ("FP32", 8)])
@pytest.mark.parametrize("fmt", ["NCHW", "NHWC"])
def test_unaligned_destination_takes_the_scalar_stores(env, fmt, dtype, shift):
    """W % 4 == 0 but the destination is not 16-byte aligned."""
    img = _image((8, 8, 3))
    (got,) = _run(env, [img], 3, 8, 8, "INCEPTION", fmt, dtype, dst_shift=shift)
    _check(got, img, 3, 8, 8, "INCEPTION", fmt, dtype, "shifted %d %s %s" % (shift, fmt, dtype))


@pytest.mark.parametrize("fmt", ["NCHW", "NHWC"])
def test_half_weights_are_bit_exact(env, fmt):
    """n_in = 2 * n_out on both axes: every weight is 0.5."""
    img = _image((16, 24, 3))
    (got,) = _run(env, [img], 3, 8, 12, "NONE", fmt)
    f = img.astype(np.float32)
    a, b, c, d = f[0::2, 0::2], f[0::2, 1::2], f[1::2, 0::2], f[1::2, 1::2]
    half = np.float32(0.5)
    ref = ((a + b) * half + (c + d) * half) * half
    assert ref.dtype == np.float32
    ref = ref.transpose(2, 0, 1) if fmt == "NCHW" else ref
    np.testing.assert_array_equal(got.astype(np.float32), ref)


@pytest.mark.parametrize("rounding", ["rne", "trunc"])
def test_bf16_rounding_follows_the_argument(env, rounding):
    """As K6: the bf16 output is the fp32 output rounded to nearest even, or truncated."""
    img = _image((17, 13, 3))
    (f32,) = _run(env, [img], 3, 8, 8, "INCEPTION", "NCHW")
    (b16,) = _run(env, [img], 3, 8, 8, "INCEPTION", "NCHW", "BF16", rounding=rounding)
    u = f32.astype(np.float32).view(np.uint32)
    if rounding == "rne":
        u = u + 0x7FFF + ((u >> 16) & 1)
    ref = (u & 0xFFFF0000).view(np.float32)
    assert len(np.unique(ref)) > 100
    np.testing.assert_array_equal(b16.astype(np.float32), ref)


def test_equal_sizes_copy_through(env):
    img = _image((8, 8, 3))
    (got,) = _run(env, [img], 3, 8, 8, "NONE", "NHWC")
    np.testing.assert_array_equal(got, img.astype(np.float64))


@pytest.mark.parametrize("fmt", ["NCHW", "NHWC"])
def test_mixed_sizes_and_unaligned_sources_in_one_launch(env, fmt):
    imgs = [_image((5, 7, 3)), _image((17, 13, 3)), _image((9, 6, 1))]
    outs = _run(env, imgs, 3, 8, 8, "INCEPTION", fmt, src_offsets=[0, 1, 3])
    for k, (got, img) in enumerate(zip(outs, imgs)):
        _check(got, img, 3, 8, 8, "INCEPTION", fmt, "FP32", "mixed image %d %s" % (k, fmt))


def test_65_images_cross_the_64_image_table(env):
    imgs = [_image((2, 3, 3), seed=k) for k in range(65)]
    outs = _run(env, imgs, 3, 4, 4, "VGG", "NCHW")
    assert len(outs) == 65
    for k, (got, img) in enumerate(zip(outs, imgs)):
        ref = image.preprocess(img, 3, 4, 4, "VGG", "NCHW", np.float64)
        assert (np.abs(got - ref) <= _bound(ref, "VGG", "FP32")).all(), k


@pytest.mark.parametrize("what,sizes,dst", [
    ("source dimension 16385", [(16385, 2, 3)], (3, 4, 4)),
    ("source width 16385", [(2, 16385, 3)], (3, 4, 4)),
    ("output dimension 16385", [(2, 2, 3)], (3, 4, 16385)),
    ("src_c 2", [(2, 2, 2)], (3, 4, 4)),
    ("C 4", [(2, 2, 3)], (4, 4, 4)),
])
def test_invalid_arguments_return_an_error_without_a_launch(env, what, sizes, dst):
    """Plain argument checks in the entry point: nothing is launched, the
    destination keeps its canary bytes."""
    torch, hip = env
    C, H, W = dst
    src = torch.from_numpy(_image((2, 2, 3)).copy()).cuda()
    buf = torch.full((2 * GAP + 4 * 4 * 4 * 4,), CANARY, dtype=torch.uint8, device="cuda")
    with pytest.raises(hip.HipError):
        hip.resize_pack([src.data_ptr()], sizes, [buf.data_ptr() + GAP], "FP32", "NCHW", C, H, W,
                        stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == CANARY).all(), what


def test_null_tables_are_rejected(env):
    torch, hip = env
    with pytest.raises(hip.HipError):
        hip.resize_pack([0], [(2, 2, 3)], [0], "FP32", "NCHW", 3, 4, 4)


@pytest.mark.parametrize("fmt,dtype", [("NCHW", "FP32"), ("NHWC", "FP16")])
def test_preprocess_raw_batch_device_matches_the_oracle(env, fmt, dtype):
    imgs = [_image((37, 53, 3)), _image((64, 20, 1))]
    out = image.preprocess_raw_batch_device(imgs, 3, 16, 24, "INCEPTION", fmt, dtype)
    assert out.shape == ((2, 3, 16, 24) if fmt == "NCHW" else (2, 16, 24, 3))
    assert out.dtype == (np.float32 if dtype == "FP32" else np.float16)
    for got, img in zip(out, imgs):
        _check(got.astype(np.float64), img, 3, 16, 24, "INCEPTION", fmt, dtype, "raw batch %s %s" % (fmt, dtype))
    assert image.preprocess_raw_batch_device(imgs, 3, 16, 24, "NONE", fmt, "UINT8") is None

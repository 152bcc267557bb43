"""K21 resize_pack_aa (csrc/kernels/resize.hip, ``resize_pack(antialias=True)``)
against the project's definition of antialiased preprocessing,
utils.image.preprocess(..., antialias=True) evaluated in float64, with the
method of tests/test_resize_gpu.py: every destination is its own slice of one
canary-filled buffer and every byte outside the slices is checked.

Tolerance (derived, not tuned).  With Ty, Tx the largest tap counts of the two
axes (area_axis_table): each tap adds at most one fp32 rounding per weight,
product and add on partial sums <= 256, and 8 more cover the channel mean and
the affine step as in K20's bound, so
    |got - ref| <= (Ty + Tx + 8) * 2^-24 * 256 * |scale_c| + 2^-23 * |ref|
plus one ulp of the format at |ref| for 16-bit outputs."""

import functools
import os
import re

import numpy as np
import pytest

from triton_client_amd.utils import image

pytestmark = pytest.mark.gpu

CANARY = 0xA5
GAP = 64  # canary bytes before, between and after the destinations
_ESZ = {"FP32": 4, "FP16": 2, "BF16": 2}
_SCALE = {"NONE": 1.0, "INCEPTION": 1.0 / 127.5, "VGG": 1.0}
COMBOS = [(s, f) for s in ("NONE", "INCEPTION", "VGG") for f in ("NCHW", "NHWC")]

# (source, destination (C, H, W)); each runs with every scaling and layout
SMALL = [
    ((1, 1, 3), (3, 4, 4)),       # upscale
    ((17, 13, 3), (3, 4, 4)),     # both axes down; W = 4 is the only vector store
    ((17, 13, 3), (3, 5, 5)),     # tail lanes and scalar stores
    ((9, 6, 1), (3, 5, 5)),       # 1 -> 3 channels
    ((6, 9, 3), (1, 7, 3)),       # h up, w down by exactly 3, 3 -> 1 channels
    ((8, 8, 3), (3, 8, 8)),       # identity
]
# (source, destination, scaling, layout)
LARGE = [
    ((3000, 2, 3), (3, 224, 224), "VGG", "NHWC"),        # 27 taps; the footprint crosses the LDS chunk
    ((3000, 2, 3), (3, 224, 224), "INCEPTION", "NCHW"),
    ((16384, 3, 1), (1, 1, 2), "NONE", "NCHW"),          # 16384 taps on one axis
    ((3, 16384, 1), (1, 2, 1), "VGG", "NHWC"),           # the same on the other axis
    ((2, 16000, 1), (1, 4, 16384), "INCEPTION", "NHWC"),  # widest upscale
    ((480, 640, 3), (3, 224, 224), "INCEPTION", "NCHW"),  # the served shape
    ((480, 640, 3), (3, 224, 224), "NONE", "NHWC"),
]
UPSCALES = [((1, 1, 3), (3, 4, 4)), ((5, 7, 3), (3, 8, 8)), ((8, 8, 3), (3, 8, 8)), ((2, 16000, 1), (1, 4, 16384))]


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


@functools.lru_cache(maxsize=None)
def _reference(shape, seed, C, H, W, scaling, fmt):
    ref = image.preprocess(_image(shape, seed), C, H, W, scaling, fmt, np.float64, antialias=True)
    ref.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def _taps(shape, H, W):
    """Ty + Tx of the bound: the largest tap counts of the two axes."""
    return int(image.area_axis_table(H, shape[0])[1].max()) + int(image.area_axis_table(W, shape[1])[1].max())


def _ulp16(ref, dtype):
    """One ulp of the 16-bit format at |ref| (0 for FP32 outputs)."""
    if dtype == "FP32":
        return np.zeros_like(ref)
    mant, emin = (10, -14) if dtype == "FP16" else (7, -126)
    e = np.floor(np.log2(np.maximum(np.abs(ref), 2.0 ** emin)))
    return 2.0 ** (e - mant)


def _bound(ref, taps, scaling, dtype):
    return (taps + 8) * 2.0 ** -24 * 256 * _SCALE[scaling] + 2.0 ** -23 * np.abs(ref) + _ulp16(ref, dtype)


def _decode(raw, dtype):
    if dtype == "FP32":
        return raw.view(np.float32).astype(np.float64)
    if dtype == "FP16":
        return raw.view(np.float16).astype(np.float64)
    return (raw.view(np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def _run(env, imgs, C, H, W, scaling, fmt, dtype="FP32", src_offsets=None, dst_shift=0, rounding="rne",
         antialias=True):
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
    assert buf.data_ptr() % 16 == 0 and src.data_ptr() % 16 == 0
    dsts = [buf.data_ptr() + first + i * pitch for i in range(n)]
    scale, bias = image._SCALE_BIAS[scaling](C)
    hip.resize_pack([src.data_ptr() + s for s in starts], [im.shape for im in imgs], dsts, dtype, fmt, C, H, W,
                    scale=scale, bias=bias, rounding=rounding, stream=torch.cuda.current_stream().cuda_stream,
                    antialias=antialias)
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


def _check(got, shape, C, H, W, scaling, fmt, dtype, what, seed=0):
    ref = _reference(shape, seed, C, H, W, scaling, fmt)
    err = np.abs(got - ref)
    bound = _bound(ref, _taps(shape, H, W), scaling, dtype)
    print("%s: taps %d, max err %.3g, smallest bound %.3g, worst err/bound %.3g"
          % (what, _taps(shape, H, W), err.max(), bound.min(), (err / bound).max()))
    assert (err <= bound).all(), what


@pytest.mark.parametrize("src,dst", SMALL)
def test_small_shapes_match_float64_preprocess_in_every_scaling_and_layout(env, src, dst):
    C, H, W = dst
    for scaling, fmt in COMBOS:
        (got,) = _run(env, [_image(src)], C, H, W, scaling, fmt)
        _check(got, src, C, H, W, scaling, fmt, "FP32", "%s->%s %s %s" % (src, dst, scaling, fmt))


@pytest.mark.parametrize("src,dst,scaling,fmt", LARGE)
def test_large_shapes_match_float64_preprocess(env, src, dst, scaling, fmt):
    C, H, W = dst
    (got,) = _run(env, [_image(src)], C, H, W, scaling, fmt)
    _check(got, src, C, H, W, scaling, fmt, "FP32", "%s->%s %s %s" % (src, dst, scaling, fmt))


@pytest.mark.parametrize("dtype,rounding", [("FP16", "rne"), ("BF16", "rne"), ("BF16", "trunc")])
@pytest.mark.parametrize("fmt", ["NCHW", "NHWC"])
@pytest.mark.parametrize("src,dst", [((17, 13, 3), (3, 4, 4)), ((9, 6, 1), (3, 5, 5))])
def test_16bit_outputs(env, src, dst, fmt, dtype, rounding):
    C, H, W = dst
    for scaling in ("NONE", "INCEPTION", "VGG"):
        (got,) = _run(env, [_image(src)], C, H, W, scaling, fmt, dtype, rounding=rounding)
        _check(got, src, C, H, W, scaling, fmt, dtype, "%s->%s %s %s %s %s" % (src, dst, scaling, fmt, dtype, rounding))


@pytest.mark.parametrize("rounding", ["rne", "trunc"])
def test_bf16_rounding_follows_the_argument(env, rounding):
    """The bf16 output is the fp32 output rounded to nearest even, or truncated."""
    img = _image((17, 13, 3))
    (f32,) = _run(env, [img], 3, 8, 8, "INCEPTION", "NCHW")
    (b16,) = _run(env, [img], 3, 8, 8, "INCEPTION", "NCHW", "BF16", rounding=rounding)
    u = f32.astype(np.float32).view(np.uint32)
    if rounding == "rne":
        u = u + 0x7FFF + ((u >> 16) & 1)
    ref = (u & 0xFFFF0000).view(np.float32)
    assert len(np.unique(ref)) > 100
    np.testing.assert_array_equal(b16.astype(np.float32), ref)


@pytest.mark.parametrize("dtype,shift", [("FP32", 4), ("FP16", 2), ("FP32", 8)])
@pytest.mark.parametrize("fmt", ["NCHW", "NHWC"])
def test_unaligned_destination_takes_the_scalar_stores(env, fmt, dtype, shift):
    """W % 4 == 0 but the destination is not 16-byte aligned."""
    src, (C, H, W) = (17, 13, 3), (3, 4, 4)
    (got,) = _run(env, [_image(src)], C, H, W, "INCEPTION", fmt, dtype, dst_shift=shift)
    _check(got, src, C, H, W, "INCEPTION", fmt, dtype, "shifted %d %s %s" % (shift, fmt, dtype))


@pytest.mark.parametrize("fmt", ["NCHW", "NHWC"])
def test_mixed_sizes_and_unaligned_sources_in_one_launch(env, fmt):
    shapes = [(5, 7, 3), (17, 13, 3), (9, 6, 1), (40, 300, 3)]
    outs = _run(env, [_image(s) for s in shapes], 3, 8, 8, "INCEPTION", fmt, src_offsets=[0, 1, 10, 15])
    for k, (got, s) in enumerate(zip(outs, shapes)):
        _check(got, s, 3, 8, 8, "INCEPTION", fmt, "FP32", "mixed image %d %s" % (k, fmt))


def test_70_images_of_mixed_sizes_cross_the_64_image_table(env):
    shapes = [(2, 3, 3), (17, 13, 3), (9, 6, 1), (5, 7, 3), (13, 29, 3)]
    picks = [(shapes[k % len(shapes)], k // len(shapes)) for k in range(70)]
    outs = _run(env, [_image(s, seed) for s, seed in picks], 3, 4, 4, "VGG", "NCHW")
    assert len(outs) == 70
    for k, (got, (s, seed)) in enumerate(zip(outs, picks)):
        ref = _reference(s, seed, 3, 4, 4, "VGG", "NCHW")
        assert (np.abs(got - ref) <= _bound(ref, _taps(s, 4, 4), "VGG", "FP32")).all(), k


@pytest.mark.parametrize("src,dst", UPSCALES)
def test_upscales_agree_with_the_bilinear_kernel(env, src, dst):
    """No axis shrinks: K21 has K20's two taps and weights."""
    C, H, W = dst
    for fmt in ("NCHW", "NHWC"):
        (aa,) = _run(env, [_image(src)], C, H, W, "INCEPTION", fmt)
        (plain,) = _run(env, [_image(src)], C, H, W, "INCEPTION", fmt, antialias=False)
        ref = _reference(src, 0, C, H, W, "INCEPTION", fmt)
        diff = np.abs(aa - plain)
        bound = _bound(ref, _taps(src, H, W), "INCEPTION", "FP32")
        print("%s->%s %s: K21 vs K20 max diff %.3g, worst diff/bound %.3g" % (src, dst, fmt, diff.max(),
                                                                            (diff / bound).max()))
        assert _taps(src, H, W) <= 4
        assert (diff <= bound).all()


def test_one_pixel_stripes_are_averaged_on_the_device(env):
    """The reason for K21: 672 -> 224 of alternating 0 / 255 columns."""
    img = np.zeros((6, 672, 1), dtype=np.uint8)
    img[:, 1::2] = 255
    (aa,) = _run(env, [img], 1, 6, 224, "NONE", "NCHW")
    (plain,) = _run(env, [img], 1, 6, 224, "NONE", "NCHW", antialias=False)
    tol = (5 + 1 + 8) * 2.0 ** -24 * 256 + 2.0 ** -23 * 256
    assert aa.min() >= 255 * 4 / 9 - tol and aa.max() <= 255 * 5 / 9 + tol
    assert plain.min() == 0.0 and plain.max() == 255.0


@pytest.mark.parametrize("what,sizes,dst", [
    ("source dimension 16385", [(16385, 2, 3)], (3, 4, 4)),
    ("source width 16385", [(2, 16385, 3)], (3, 4, 4)),
    ("output dimension 16385", [(2, 2, 3)], (3, 4, 16385)),
    ("src_c 2", [(2, 2, 2)], (3, 4, 4)),
    ("C 4", [(2, 2, 3)], (4, 4, 4)),
])
def test_invalid_arguments_return_an_error_without_a_launch(env, what, sizes, dst):
    torch, hip = env
    C, H, W = dst
    src = torch.from_numpy(_image((2, 2, 3)).copy()).cuda()
    buf = torch.full((2 * GAP + 4 * 4 * 4 * 4,), CANARY, dtype=torch.uint8, device="cuda")
    with pytest.raises(hip.HipError):
        hip.resize_pack([src.data_ptr()], sizes, [buf.data_ptr() + GAP], "FP32", "NCHW", C, H, W,
                        stream=torch.cuda.current_stream().cuda_stream, antialias=True)
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == CANARY).all(), what


def test_null_tables_are_rejected(env):
    torch, hip = env
    with pytest.raises(hip.HipError):
        hip.resize_pack([0], [(2, 2, 3)], [0], "FP32", "NCHW", 3, 4, 4, antialias=True)


@pytest.mark.parametrize("fmt,dtype", [("NCHW", "FP32"), ("NHWC", "FP16")])
def test_preprocess_raw_batch_device_takes_the_flag(env, fmt, dtype):
    shapes = [(37, 53, 3), (64, 20, 1)]
    out = image.preprocess_raw_batch_device([_image(s) for s in shapes], 3, 16, 24, "INCEPTION", fmt, dtype,
                                            antialias=True)
    assert out.shape == ((2, 3, 16, 24) if fmt == "NCHW" else (2, 16, 24, 3))
    assert out.dtype == (np.float32 if dtype == "FP32" else np.float16)
    for got, s in zip(out, shapes):
        _check(got.astype(np.float64), s, 3, 16, 24, "INCEPTION", fmt, dtype, "raw batch %s %s" % (fmt, dtype))


# -- the GPU preprocess_inception model class ------------------------------------------
SIZES = [(240, 320, 3), (97, 131, 3), (480, 640, 3), (64, 48, 1)]


def _request(blobs, antialias=None, ensemble_step=False):
    from triton_client_amd.server.types import InferRequest, InputTensor

    data = np.array(list(blobs), dtype=np.object_).reshape(len(blobs), 1)
    r = InferRequest(model_name="preprocess_inception", inputs=[InputTensor("INPUT", "BYTES", [len(blobs), 1], data)])
    if antialias is not None:
        r.parameters["antialias"] = antialias
    if ensemble_step:
        r.accepts_device_outputs = True  # what core._infer_ensemble sets on its sub-requests
    return r


def _assert_rows(got, shapes, antialias, what):
    """Flagged rows against the K21 bound, the others against K20's (tests/test_resize_gpu.py)."""
    for k, (g, s) in enumerate(zip(got, shapes)):
        if antialias:
            ref, taps = _reference(s, 0, 3, 224, 224, "INCEPTION", "NCHW"), _taps(s, 224, 224)
        else:
            ref, taps = image.preprocess(_image(s), 3, 224, 224, "INCEPTION", "NCHW", np.float64), 0
        err = np.abs(g.astype(np.float64) - ref)
        bound = _bound(ref, taps, "INCEPTION", "FP32")
        print("%s image %d antialias=%s: max err %.3g, worst err/bound %.3g" % (what, k, antialias, err.max(),
                                                                               (err / bound).max()))
        assert (err <= bound).all(), (what, k)


@pytest.fixture(scope="module")
def model():
    from triton_client_amd.server.gpu_models import PreprocessInception

    m = PreprocessInception()
    m.load()
    yield m
    m.unload()


def test_model_splits_a_mixed_batch_by_the_flag(model, monkeypatch):
    from triton_client_amd.ops import hip

    calls = []
    real = hip.resize_pack

    def spy(*a, **kw):
        calls.append((len(a[0]), bool(kw.get("antialias", False))))
        return real(*a, **kw)

    monkeypatch.setattr(hip, "resize_pack", spy)
    blobs = [image.encode_ppm(_image(s)) if s[2] == 3 else image.encode_raw(_image(s)) for s in SIZES]
    # one batch: flagged rows 0-1, unflagged row 2, flagged row 3, explicit false row 4
    reqs = [_request(blobs[:2], True), _request(blobs[2:3]), _request(blobs[3:], True), _request(blobs[:1], False)]
    res = model.execute(reqs)
    assert sorted(calls) == [(2, False), (3, True)]  # at most one K20 and one K21 call per batch
    for outs, shapes, aa in zip(res, (SIZES[:2], SIZES[2:3], SIZES[3:], SIZES[:1]), (True, False, True, False)):
        (o,) = outs
        assert isinstance(o.data, np.ndarray) and o.data.shape == (len(shapes), 3, 224, 224)
        _assert_rows(o.data, shapes, aa, "mixed batch")
    a, b = res[0][0].data[0], res[3][0].data[0]  # the same 320 -> 224 image, flagged and not
    assert np.abs(a - b).max() > 0.05


def test_model_ensemble_step_gets_a_device_view_with_the_flag(model):
    from triton_client_amd.server.types import DeviceView, InputTensor

    blobs = [image.encode_raw(_image(s)) for s in SIZES]
    res = model.execute([_request(blobs[:3], True, True), _request(blobs[3:], None, True)])
    for outs, shapes, aa in zip(res, (SIZES[:3], SIZES[3:]), (True, False)):
        (o,) = outs
        assert isinstance(o.data, DeviceView) and o.shape == [len(shapes), 3, 224, 224] and o.owner.is_cuda
        _assert_rows(InputTensor("x", "FP32", o.shape, o.data).numpy(), shapes, aa, "device view")


def test_model_host_fallback_uses_resize_area(model, monkeypatch):
    shapes = SIZES[:2]
    monkeypatch.setattr(model, "STAGE_BYTES", _image(shapes[0]).size)  # the second image does not fit
    (outs,) = model.execute([_request([image.encode_ppm(_image(s)) for s in shapes], True)])
    got = outs[0].data
    _assert_rows(got[:1], shapes[:1], True, "staged")
    np.testing.assert_array_equal(got[1], image.inception_preprocess(_image(shapes[1]), 224, 224, "NCHW",
                                                                     antialias=True))


# -- served ---------------------------------------------------------------------------------
def test_served_ensemble_honours_the_request_parameter(gpu_server):
    """densenet_onnx on host-preprocessed tensors is the reference, as in
    tests/test_preprocess_device_gpu.py (rel-L2 1e-3 on the logits)."""
    import tritonclient.http as httpclient

    shapes = [(480, 640, 3), (500, 700, 3), (600, 451, 3)]  # every axis shrinks by 2 or more
    c = httpclient.InferenceServerClient(gpu_server.http_url)
    refs = {}
    for aa in (False, True):
        x = np.stack([image.inception_preprocess(_image(s), 224, 224, "NCHW", antialias=aa) for s in shapes])
        inp = httpclient.InferInput("data_0", list(x.shape), "FP32")
        inp.set_data_from_numpy(x.astype(np.float32))
        refs[aa] = c.infer("densenet_onnx", [inp]).as_numpy("fc6_1")
    data = np.array([image.encode_raw(_image(s)) for s in shapes], dtype=np.object_).reshape(3, 1)
    inp = httpclient.InferInput("INPUT", [3, 1], "BYTES")
    inp.set_data_from_numpy(data)
    got = {aa: c.infer("preprocess_inception_ensemble", [inp],
                       parameters={"antialias": True} if aa else None).as_numpy("OUTPUT") for aa in (False, True)}
    c.close()

    def rel(a, b):
        return np.linalg.norm(a - b, axis=1) / np.linalg.norm(b, axis=1)

    print("flagged vs area reference %s, unflagged vs bilinear reference %s, between the references %s"
          % (rel(got[True], refs[True]), rel(got[False], refs[False]), rel(refs[True], refs[False])))
    # the references are more than twice the tolerance apart, so no output can pass against both:
    # a flagged request served by the bilinear path (or the reverse) fails below
    assert rel(refs[True], refs[False]).min() > 2e-3
    assert rel(got[True], refs[True]).max() < 1e-3
    assert rel(got[False], refs[False]).max() < 1e-3


def test_image_client_antialias_device_paths_classify_as_the_host_path(gpu_server, tmp_path):
    from tests.test_examples import run_example

    for i, s in enumerate(SIZES[:3]):
        with open(os.path.join(tmp_path, "img%d.ppm" % i), "wb") as f:
            f.write(image.encode_ppm(_image(s)))
    picks = []
    # host resize_area; K21; host resize_area then K6
    for extra in (["--antialias"], ["--antialias", "--device-resize"], ["--antialias", "--device-preprocess"]):
        r = run_example("image_client.py", gpu_server.http_url,
                        ["-m", "densenet_onnx", "-s", "INCEPTION", "-c", "1", "-b", "3"] + extra + [str(tmp_path)],
                        timeout=300)
        assert r.returncode == 0 and "PASS" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]
        picks.append(re.findall(r"\((\d+)\) = ", r.stdout))
    assert len(picks[0]) == 3 and picks[0] == picks[1] == picks[2], picks

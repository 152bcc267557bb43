"""area_axis_table (the integer rule K21 resize_pack_aa implements), resize_area
built on it, the ``antialias`` keyword of utils.image.preprocess, and the
``antialias`` request parameter through an in-process CPU server, alone and as
an ensemble step.  CPU only."""

import asyncio
from fractions import Fraction

import numpy as np
import pytest

from triton_client_amd.server.core import InferenceServer
from triton_client_amd.server.cpu_models import PreprocessInception
from triton_client_amd.server.model_base import Model, TensorSpec
from triton_client_amd.server.types import InferRequest, InputTensor
from triton_client_amd.utils import image
from triton_client_amd.utils.image import area_axis_table, resize_area, resize_axis_table, resize_bilinear

PAIRS = [(n_in, n_out) for n_in in range(1, 41) for n_out in range(1, 41)]
PAIRS += [(16000, 16384), (16384, 1), (3000, 224), (1, 224), (16383, 2)]


def _weights(n_out, n_in):
    """Per output index: {source index: exact weight} from the table."""
    first, count, t, total = area_axis_table(n_out, n_in)
    assert len(first) == len(count) == len(total) == t.shape[0] == n_out
    rows = []
    for i in range(n_out):
        n = int(count[i])
        assert not t[i, n:].any(), (n_in, n_out, i)
        rows.append({int(first[i]) + k: Fraction(int(t[i, k]), int(total[i])) for k in range(n)})
    return rows


def _bilinear_weights(n_out, n_in):
    i0, i1, num, den = resize_axis_table(n_out, n_in)
    rows = []
    for i in range(n_out):
        w = {}
        for j, f in ((int(i0[i]), Fraction(den - int(num[i]), den)), (int(i1[i]), Fraction(int(num[i]), den))):
            if f:
                w[j] = w.get(j, 0) + f
        rows.append(w)
    return rows


def _definition(n_out, n_in):
    """The rule as the issue states it, over every j, in Python integers."""
    big = 2 * max(n_in, n_out)
    rows = []
    for i in range(n_out):
        t = [max(0, big - abs((2 * j + 1) * n_out - (2 * i + 1) * n_in)) for j in range(n_in)]
        rows.append({j: Fraction(v, sum(t)) for j, v in enumerate(t) if v})
    return rows


def test_table_is_the_definition_on_small_sizes():
    for n_in, n_out in PAIRS:
        if n_in <= 40 and n_out <= 40:
            assert _weights(n_out, n_in) == _definition(n_out, n_in), (n_in, n_out)


def test_weights_are_positive_and_sum_to_one_exactly():
    for n_in, n_out in PAIRS:
        first, count, t, total = area_axis_table(n_out, n_in)
        assert (count >= 1).all() and (first >= 0).all() and (first + count <= n_in).all(), (n_in, n_out)
        listed = np.arange(t.shape[1])[None, :] < count[:, None]
        assert (t[listed] > 0).all(), (n_in, n_out)  # no tap of weight zero is listed
        assert not t[~listed].any(), (n_in, n_out)
        assert np.array_equal(t.sum(axis=1), total), (n_in, n_out)
        for w in _weights(n_out, n_in):
            assert sum(w.values()) == 1 and min(w.values()) > 0, (n_in, n_out)


def test_neighbours_of_the_listed_taps_have_weight_zero():
    """Nothing with t > 0 is left out: the tap before ``first`` and the one after the last are at or below zero."""
    for n_in, n_out in PAIRS:
        first, count, _, _ = area_axis_table(n_out, n_in)
        big = 2 * max(n_in, n_out)
        c = (2 * np.arange(n_out, dtype=np.int64) + 1) * n_in
        for j, inside in ((first - 1, first - 1 >= 0), (first + count, first + count <= n_in - 1)):
            t = big - np.abs((2 * j + 1) * n_out - c)
            assert (t[inside] <= 0).all(), (n_in, n_out)


def test_upscale_and_identity_are_the_bilinear_table():
    for n_in, n_out in PAIRS:
        if n_in <= n_out and n_out <= 224:
            assert _weights(n_out, n_in) == _bilinear_weights(n_out, n_in), (n_in, n_out)
    # 16000 -> 16384 without 16384 dict rows: the same comparison in integer arrays
    first, count, t, total = area_axis_table(16384, 16000)
    i0, i1, num, den = resize_axis_table(16384, 16000)
    assert count.max() == 2
    one = count == 1
    assert np.array_equal(first[one], i0[one]) and ((num[one] == 0) | (i0[one] == i1[one])).all()
    two = ~one
    assert np.array_equal(first[two], i0[two]) and np.array_equal(first[two] + 1, i1[two])
    # t1 / total == num / den, cross-multiplied
    assert np.array_equal(t[two, 1] * den, num[two] * total[two])


@pytest.mark.parametrize("n_in,n_out,taps", [(480, 224, 5), (640, 224, 6), (3000, 224, 27), (16384, 1, 16384)])
def test_tap_counts(n_in, n_out, taps):
    assert int(area_axis_table(n_out, n_in)[1].max()) == taps


def test_terms_fit_32_bits_at_the_size_limit():
    worst_total = 0
    for n_in, n_out in [(16384, 1), (16384, 16383), (1, 16384)]:
        first, count, t, total = area_axis_table(n_out, n_in)
        big = 2 * max(n_in, n_out)
        c = (2 * np.arange(n_out, dtype=np.int64) + 1) * n_in
        last = first + count - 1
        terms = [c, c - big - n_out, c + big - n_out - 1, (2 * first + 1) * n_out - c, (2 * last + 1) * n_out - c,
                 (2 * (n_in - 1) + 1) * np.int64(n_out), total, t]
        for v in terms:
            assert np.abs(v).max() < 2 ** 31, (n_in, n_out)
        worst_total = max(worst_total, int(total.max()))
    assert worst_total == 402653184


def _img(shape, seed=0):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


@pytest.mark.parametrize("src,dst", [((1, 1, 3), (4, 4)), ((5, 7, 3), (8, 8)), ((8, 8, 3), (8, 8))])
def test_resize_area_is_resize_bilinear_when_nothing_shrinks(src, dst):
    img = _img(src)
    np.testing.assert_array_equal(resize_area(img, *dst), resize_bilinear(img, *dst))


def test_resize_area_is_the_dense_definition():
    img = _img((17, 13, 3))
    got = resize_area(img, 4, 5)

    def dense(n_out, n_in):
        m = np.zeros((n_out, n_in))
        for i, w in enumerate(_definition(n_out, n_in)):
            for j, f in w.items():
                m[i, j] = float(f)
        return m

    ref = np.einsum("iy,jx,yxc->ijc", dense(4, 17), dense(5, 13), img.astype(np.float64))
    assert got.dtype == np.float64 and got.shape == (4, 5, 3)
    assert np.abs(got - ref).max() <= 1e-12 * 255


def test_one_pixel_stripes_are_averaged_not_aliased():
    img = np.zeros((6, 672, 1), dtype=np.uint8)
    img[:, 1::2] = 255
    area = resize_area(img, 6, 224)
    # a 3-pixel-wide triangle over alternating 0 / 255: weights 1/9, 2/9, 3/9, 2/9, 1/9 -> 4/9 or 5/9 of 255
    assert area.min() >= 255 * 4 / 9 - 1e-9 and area.max() <= 255 * 5 / 9 + 1e-9
    plain = resize_bilinear(img, 6, 224)
    assert plain.min() == 0.0 and plain.max() == 255.0


def test_resize_area_is_banded_at_the_size_limit():
    """16000 -> 16384 on one axis: a dense matrix would be 2 GB; the table is two taps wide."""
    img = _img((1, 16000, 1))
    assert area_axis_table(16384, 16000)[2].shape == (16384, 2)
    got = resize_area(img, 1, 16384)
    np.testing.assert_allclose(got, resize_bilinear(img, 1, 16384), rtol=0, atol=1e-9)


@pytest.mark.parametrize("shape,c,h,w,scaling,fmt", [
    ((5, 7, 3), 3, 8, 8, "INCEPTION", "NCHW"),
    ((17, 13, 3), 1, 4, 5, "VGG", "NHWC"),
    ((9, 6, 1), 3, 5, 5, "NONE", "NCHW"),
])
def test_preprocess_without_the_flag_is_unchanged_and_with_it_uses_resize_area(shape, c, h, w, scaling, fmt):
    img = _img(shape)
    x = img
    if c == 1 and shape[2] == 3:
        x = img.mean(axis=2, keepdims=True)
    elif c == 3 and shape[2] == 1:
        x = np.repeat(img, 3, axis=2)
    for aa, resized in ((False, resize_bilinear(x, h, w)), (True, resize_area(x, h, w))):
        ref = resized
        if scaling == "INCEPTION":
            ref = ref / 127.5 - 1.0
        elif scaling == "VGG":
            ref = ref - np.array([123.0, 117.0, 104.0] if c == 3 else [128.0], np.float32)
        for dtype in (np.float32, np.float64):
            want = ref.astype(dtype)
            want = np.transpose(want, (2, 0, 1)) if fmt == "NCHW" else want
            got = image.preprocess(img, c, h, w, scaling, fmt, dtype, antialias=aa)
            assert got.dtype == dtype
            np.testing.assert_array_equal(got, want)
            if not aa:
                np.testing.assert_array_equal(image.preprocess(img, c, h, w, scaling, fmt, dtype), want)
    if c == 3 and scaling == "INCEPTION":
        np.testing.assert_array_equal(image.inception_preprocess(img, h, w, fmt),
                                      image.preprocess(img, 3, h, w, "INCEPTION", fmt))
        np.testing.assert_array_equal(image.inception_preprocess(img, h, w, fmt, antialias=True),
                                      image.preprocess(img, 3, h, w, "INCEPTION", fmt, antialias=True))


# -- served -----------------------------------------------------------------------------
SEEN = {}


class _Recorder(Model):
    """Second step: passes the tensor through and records what its sub-request carried."""

    name = "area_recorder"
    max_batch_size = 8
    inputs = (TensorSpec("X", "FP32", [3, 224, 224]),)
    outputs = (TensorSpec("Y", "FP32", [3, 224, 224]),)

    def execute(self, requests):
        for r in requests:
            SEEN["parameters"] = dict(r.parameters)
        return [[self.out("Y", r.input("X").numpy())] for r in requests]


class _Ensemble(Model):
    name = "area_ensemble"
    platform = "ensemble"
    max_batch_size = 8
    inputs = (TensorSpec("INPUT", "BYTES", [1]),)
    outputs = (TensorSpec("Y", "FP32", [3, 224, 224]),)
    ensemble_steps = [
        ("preprocess_inception", {"INPUT": "INPUT"}, {"OUTPUT": "mid"}),
        ("area_recorder", {"X": "mid"}, {"Y": "Y"}),
    ]


@pytest.fixture(scope="module")
def server():
    s = InferenceServer([PreprocessInception, _Recorder, _Ensemble])
    s.load_all()
    yield s
    s.executor.shutdown(wait=False)


@pytest.fixture(scope="module")
def shrunk():
    """A downscale on both axes, where the two resizes differ: the server models are fixed at 224x224."""
    img = _img((300, 451, 3), seed=4)
    return img, {aa: image.inception_preprocess(img, 224, 224, "NCHW", antialias=aa) for aa in (False, True)}


def _infer(server, model, img, parameters=None):
    data = np.array([image.encode_raw(img)], dtype=np.object_).reshape(1, 1)
    req = InferRequest(model_name=model, inputs=[InputTensor("INPUT", "BYTES", [1, 1], data)],
                       parameters=dict(parameters or {}))
    resp = asyncio.run(server.infer(req))
    ((o, _),) = resp.outputs
    return np.asarray(o.data)[0]


@pytest.mark.parametrize("model", ["preprocess_inception", "area_ensemble"])
def test_request_parameter_selects_the_antialiased_resize(server, shrunk, model):
    img, ref = shrunk
    assert np.abs(ref[True] - ref[False]).max() > 0.05  # the two resizes are told apart
    np.testing.assert_array_equal(_infer(server, model, img, {"antialias": True}), ref[True])
    np.testing.assert_array_equal(_infer(server, model, img), ref[False])
    np.testing.assert_array_equal(_infer(server, model, img, {"antialias": False}), ref[False])


def test_ensemble_hands_custom_parameters_to_every_step_and_keeps_reserved_ones(server, shrunk):
    img, _ = shrunk
    SEEN.clear()
    _infer(server, "area_ensemble", img, {"antialias": True, "tenant": "a", "priority": 3, "timeout": 5})
    assert SEEN["parameters"] == {"antialias": True, "tenant": "a"}
    SEEN.clear()
    _infer(server, "area_ensemble", img)
    assert SEEN["parameters"] == {}


def test_ensemble_counts_a_wire_parameter_once(server, shrunk):
    img, _ = shrunk
    key = "param:antialias:bool:True"
    before = server.wire_stats[key]
    _infer(server, "area_ensemble", img, {"antialias": True})
    assert server.wire_stats[key] - before == 1

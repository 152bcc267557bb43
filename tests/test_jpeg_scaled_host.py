"""The reduced-size JPEG decode (scale 1/2, 1/4, 1/8) on the host: the numpy
reference of tests/jpeg_scaled_cases.py against float64, against Pillow's
recorded ``draft`` decodes and against the box average of the full decode; the
host decoder (csrc/host/jpeg.cc through ops.host_codec) against the reference,
bit for bit; ``jpeg_auto_scale``; the refusals; and the ``jpeg_scale`` request
parameter of the CPU ``preprocess_inception``.  No GPU and no Pillow."""

import numpy as np
import pytest

from tests import jpeg_cases as jc
from tests import jpeg_scaled_cases as js
from triton_client_amd.utils import image


@pytest.fixture(scope="module")
def hc():
    from triton_client_amd.ops import host_codec

    return host_codec.load()


@pytest.fixture(scope="module")
def reference():
    """Per decodable fixture: (entry, blob, parse, coefficients, {scale: pixels}) of the numpy reference."""
    out = []
    for e in jc.decodable():
        b = jc.blob(e)
        info = jc.parse(b)
        coefs = jc.entropy_decode(info)
        out.append((e, b, info, coefs, {s: js.pixels(info, coefs, s) for s in js.SCALES}))
    return out


# -- arithmetic ---------------------------------------------------------------------------
@pytest.mark.parametrize("amplitude", [16, 256, 2047])
def test_idct_n_is_within_one_of_the_float64_transform(amplitude):
    rng = np.random.default_rng(amplitude)
    for ny, nx in js.SIZES:
        v = rng.integers(-amplitude, amplitude + 1, (20000, ny, nx))
        f = js.idct_n_float(v)
        got = js.idct_n(v)
        err = np.abs(got - np.floor(f + 0.5)).max()
        raw = np.abs(got - f).max()
        print("amplitude %4d, %d x %d: worst |integer - round(float64)| = %d, |integer - float64| = %.3f"
              % (amplitude, ny, nx, err, raw))
        assert err <= 1, (ny, nx)


def test_a_dc_only_block_gives_dc_over_eight_for_every_size():
    dc = np.arange(jc.DEQ_MIN, jc.DEQ_MAX + 1)
    for ny, nx in js.SIZES:
        v = np.zeros((dc.size, ny, nx), dtype=np.int64)
        v[:, 0, 0] = dc
        assert (js.idct_n(v) == ((dc + 4) >> 3)[:, None, None]).all(), (ny, nx)


def test_eight_by_eight_is_the_full_size_transform():
    v = np.random.default_rng(8).integers(jc.DEQ_MIN, jc.DEQ_MAX + 1, (5000, 8, 8))
    np.testing.assert_array_equal(js.idct_n(v), jc.idct(v))
    assert (js.m1(8) == jc.M1).all() and (js.m2(8) == jc.M2).all()


def test_intermediates_stay_below_2_to_31_at_the_dequantise_clamp():
    """The worst block for each output sample: every coefficient at the clamp
    with the sign of its basis product."""
    worst = 0
    for ny, nx in js.SIZES:
        by, bx = js.basis(ny), js.basis(nx)
        for y in range(ny):
            for x in range(nx):
                v = np.where(np.outer(by[:, y], bx[:, x]) >= 0, jc.DEQ_MAX, jc.DEQ_MIN)
                ws = v @ js.m1(nx)
                out = ((ws + 1024) >> 11).T @ js.m2(ny)
                worst = max(worst, np.abs(ws).max(), np.abs(out).max() + (1 << 16))
    assert worst < 2 ** 31, worst


def test_the_small_transforms_use_the_constants_of_the_eight_point_one():
    """What csrc/kernels/jpeg_math.h relies on: no constant is new."""
    for m, big in ((js.m1, jc.M1), (js.m2, jc.M2)):
        c2, c4, c6 = big[2][0], big[0][0], big[6][0]
        assert m(1).tolist() == [[c4]]
        assert m(2).tolist() == [[c4, c4], [c4, -c4]]
        assert m(4).tolist() == [[c4] * 4, [c2, c6, -c6, -c2], [c4, -c4, -c4, c4], [c6, -c2, c2, -c6]]


# -- host against the reference -----------------------------------------------------------
@pytest.mark.parametrize("scale", [2, 4, 8])
def test_host_scaled_decode_equals_the_reference_bitwise(hc, reference, scale):
    for e, b, info, _, want in reference:
        got = hc.jpeg_decode(b, scale)
        assert got.shape == (-(-e["h"] // scale), -(-e["w"] // scale), len(info["comps"])), e["name"]
        np.testing.assert_array_equal(got, want[scale], err_msg=e["name"])
        np.testing.assert_array_equal(image.decode_image(b, jpeg_scale=scale), want[scale], err_msg=e["name"])


@pytest.mark.parametrize("scale", [1, 2, 4, 8])
def test_host_compact_coefficient_buffer_equals_the_reference(hc, reference, scale):
    for e, b, info, coefs, _ in reference:
        p = hc.jpeg_parse(b, scale)
        assert p.shape == js.shape(info, scale) and p.scale == scale, e["name"]
        assert [(p.ny[c], p.nx[c]) for c in range(p.ncomp)] == js.sizes(info, scale), e["name"]
        assert all(p.coef_off[c] % 16 == 0 for c in range(p.ncomp))
        want = js.coefficient_buffer(info, coefs, scale)
        assert p.coef_bytes == len(want), e["name"]
        buf = np.full(p.coef_bytes + 64, 0xA5, dtype=np.uint8)
        hc.jpeg_entropy_decode(b, buf[:p.coef_bytes], scale)
        assert buf[:p.coef_bytes].tobytes() == want, e["name"]
        assert (buf[p.coef_bytes:] == 0xA5).all()
        with pytest.raises(ValueError, match="malformed JPEG: coefficient buffer too small"):
            hc.jpeg_entropy_decode(b, buf[:p.coef_bytes - 1], scale)


def test_the_expected_coefficient_bytes_of_the_bench_fixture(hc):
    (e,) = jc.fixtures("bench")
    assert [hc.jpeg_parse(jc.blob(e), s).coef_bytes for s in (1, 2, 8)] == [921984, 461184, 29184]


def test_the_scaled_entry_points_at_scale_one_equal_the_existing_ones(hc, reference):
    """The C entry points themselves: ``HostCodec`` takes the existing ones at scale 1."""
    import ctypes

    from triton_client_amd.ops.host_codec import JpegInfo

    lib = hc._lib
    for e, b, _, _, _ in reference:
        msg = ctypes.create_string_buffer(96)
        old, new = JpegInfo(), JpegInfo()
        assert lib.tcamd_host_jpeg_parse(b, len(b), ctypes.byref(old), msg, 96) == 0
        assert lib.tcamd_host_jpeg_parse_scaled(b, len(b), 1, ctypes.byref(new), msg, 96) == 0
        assert bytes(old) == bytes(new), e["name"]
        assert (new.scale, list(new.ny)[:new.ncomp], list(new.nx)[:new.ncomp]) == (1, [8] * new.ncomp, [8] * new.ncomp)
        c0, c1 = np.full(old.coef_bytes, 1, np.uint8), np.full(old.coef_bytes, 2, np.uint8)
        assert lib.tcamd_host_jpeg_entropy_decode(b, len(b), c0.ctypes.data, c0.size, msg, 96) == 0
        assert lib.tcamd_host_jpeg_entropy_decode_scaled(b, len(b), 1, c1.ctypes.data, c1.size, msg, 96) == 0
        assert c0.tobytes() == c1.tobytes(), e["name"]
        p0, p1 = np.full(old.pixel_bytes, 1, np.uint8), np.full(old.pixel_bytes, 2, np.uint8)
        assert lib.tcamd_host_jpeg_decode(b, len(b), p0.ctypes.data, p0.size, msg, 96) == 0
        assert lib.tcamd_host_jpeg_decode_scaled(b, len(b), 1, p1.ctypes.data, p1.size, msg, 96) == 0
        assert p0.tobytes() == p1.tobytes(), e["name"]
        np.testing.assert_array_equal(hc.jpeg_decode(b, 1), hc.jpeg_decode(b))


# -- closeness ------------------------------------------------------------------------------
def test_reference_stays_within_the_recorded_distance_to_pillows_draft(reference):
    """The manifest's figures are fixed numbers: reference and fixture are both
    deterministic.  b01 measured mean 0.35 / 1.55 / 2.57 and max 4 / 7 / 14 at
    1/2, 1/4, 1/8; the noise fixture f11 is recorded (max 55 at 1/2: dropping
    frequencies of noise is not libjpeg-turbo's approximation of it either) and
    exempt from the mean cap."""
    by_name = {e["name"]: pix for e, _, _, _, pix in reference}
    cap = {2: 1.0, 4: 2.5, 8: 4.0}
    drafts = js.drafts()
    assert {(d["name"][:3], d["scale"]) for d in drafts} >= {(n, s) for n in ("f01", "f05", "f06", "f08", "f09", "f11",
                                                                             "b01") for s in (2, 4, 8)} | {("f03", 2)}
    for d in drafts:
        diff = np.abs(by_name[d["name"]][d["scale"]].astype(np.int64) - js.pillow_draft(d).astype(np.int64))
        print("%-28s 1/%d  max %3d  mean %.4f" % (d["name"], d["scale"], diff.max(), diff.mean()))
        assert diff.max() <= d["max"], d
        if d["name"].startswith("b01"):
            assert diff.mean() < cap[d["scale"]], d


def test_reference_is_close_to_the_box_average_of_its_own_full_decode(reference):
    """What a design that scales every component alike and then upsamples the
    chroma fails (up to 88 on the 4:2:0 fixtures).  Measured worst: 15.7, b01 at
    1/8.  The noise fixture f11 is exempt: dropping frequencies of noise is not
    a box filter."""
    for e, _, _, _, pix in reference:
        if e["name"].startswith("f11"):
            continue
        for s in (2, 4, 8):
            d = np.abs(pix[s].astype(np.float64) - js.box_average(pix[1], s)).max()
            print("%-28s 1/%d  max %.2f" % (e["name"], s, d))
            assert d <= 16, (e["name"], s)


# -- jpeg_auto_scale ------------------------------------------------------------------------
@pytest.mark.parametrize("n,want", [(224, 1), (447, 1), (448, 2), (895, 2), (896, 4), (1791, 4), (1792, 8),
                                    (100000, 8)])
def test_jpeg_auto_scale_boundaries_for_a_224_target(n, want):
    assert image.jpeg_auto_scale(n, n, 224, 224) == want
    assert image.jpeg_auto_scale(n, 100000, 224, 224) == want
    assert image.jpeg_auto_scale(100000, n, 224, 224) == want


def test_jpeg_auto_scale_of_an_image_smaller_than_the_target_on_one_axis():
    assert image.jpeg_auto_scale(100, 4000, 224, 224) == 1
    assert image.jpeg_auto_scale(4000, 223, 224, 224) == 1
    assert image.jpeg_auto_scale(1, 1, 224, 224) == 1
    for H, W in ((480, 640), (1080, 1920), (3000, 4000), (225, 5000)):
        s = image.jpeg_auto_scale(H, W, 224, 224)
        assert -(-H // s) >= 224 and -(-W // s) >= 224  # the resize that follows never upscales because of the scale
        assert s == 8 or H < 2 * s * 224 or W < 2 * s * 224


# -- errors ---------------------------------------------------------------------------------
def _outcome(hc, data, scale):
    """("image", shape) or ("error", message) of a decode at ``scale``."""
    try:
        got = hc.jpeg_decode(data, scale)
    except ValueError as err:
        assert str(err).startswith(("malformed JPEG: ", "unsupported JPEG: ")), err
        return "error", str(err)
    assert got.dtype == np.uint8
    return "image", got.shape


def _same_as_full(hc, data, scale, seen):
    full, red = _outcome(hc, data, 1), _outcome(hc, data, scale)
    assert full[0] == red[0], (full, red)
    if full[0] == "error":
        assert red[1] == full[1]  # where the full decode raises, the message is the full decode's
    else:
        H, W, c = full[1]
        assert red[1] == (-(-H // scale), -(-W // scale), c)
    seen[full[0]] += 1


def test_every_prefix_of_two_fixtures_gives_the_full_decodes_error_or_a_scaled_image(hc):
    for name, scale in (("f05", 4), ("f03", 2), ("f05", 8)):
        b = jc.blob(next(x for x in jc.fixtures("case") if x["name"].startswith(name)))
        seen = {"error": 0, "image": 0}
        for n in range(len(b) + 1):
            _same_as_full(hc, b[:n], scale, seen)
        print("%s at 1/%d: %s" % (name, scale, seen))
        assert seen["error"] > len(b) // 2 and seen["image"] >= 1


def test_400_corruptions_at_scale_4_give_the_full_decodes_error_or_a_scaled_image(hc):
    b = jc.blob(next(x for x in jc.fixtures("case") if x["name"].startswith("f05")))
    rng = np.random.default_rng(400)
    seen = {"error": 0, "image": 0}
    for _ in range(400):
        m = bytearray(b)
        m[int(rng.integers(2, len(b)))] = int(rng.integers(0, 256))
        _same_as_full(hc, bytes(m), 4, seen)
    print("corruptions %s" % seen)
    assert seen["error"] and seen["image"]


@pytest.mark.parametrize("scale", [1, 2, 4, 8])
def test_progressive_is_refused_at_every_scale(hc, scale):
    (e,) = jc.fixtures("refused")
    for decode in (hc.jpeg_decode, hc.jpeg_parse, lambda b, s: image.decode_image(b, jpeg_scale=s)):
        with pytest.raises(ValueError, match="^unsupported JPEG: progressive"):
            decode(jc.blob(e), scale)


@pytest.mark.parametrize("scale", [0, 3, -1, 16, True, 2.0])
def test_another_scale_is_a_value_error(hc, scale):
    b = jc.blob(jc.fixtures("case")[0])
    for call in (lambda: hc.jpeg_parse(b, scale), lambda: hc.jpeg_decode(b, scale),
                 lambda: image.decode_image(b, jpeg_scale=scale),
                 lambda: hc.jpeg_entropy_decode(b, np.empty(1 << 16, np.uint8), scale)):
        with pytest.raises(ValueError, match="1, 2, 4"):
            call()


def test_the_c_entry_points_refuse_another_scale(hc):
    import ctypes

    from triton_client_amd.ops.host_codec import JpegInfo

    b = jc.blob(jc.fixtures("case")[0])
    msg = ctypes.create_string_buffer(96)
    assert hc._lib.tcamd_host_jpeg_parse_scaled(b, len(b), 3, ctypes.byref(JpegInfo()), msg, 96) == 1
    assert msg.value == b"scale 3 (1, 2, 4 or 8)"


# -- the CPU preprocess_inception -----------------------------------------------------------
def _request(blobs, **params):
    from triton_client_amd.server.types import InferRequest, InputTensor

    data = np.array(list(blobs), dtype=np.object_).reshape(len(blobs), 1)
    r = InferRequest(model_name="preprocess_inception", inputs=[InputTensor("INPUT", "BYTES", [len(blobs), 1], data)])
    r.parameters.update(params)
    return r


@pytest.fixture(scope="module")
def blobs():
    """b01 (640 x 480: automatic scale 2), a small 4:2:2 JPEG (automatic scale 1) and a PPM."""
    pick = [jc.blob(next(e for e in jc.decodable() if e["name"].startswith(n))) for n in ("b01", "f03")]
    ppm = image.encode_ppm(np.random.default_rng(5).integers(0, 256, (37, 53, 3), dtype=np.uint8))
    return pick + [ppm]


@pytest.mark.parametrize("antialias", [False, True])
@pytest.mark.parametrize("scale", [0, 1, 2, 4, 8])
def test_cpu_preprocess_inception_honours_jpeg_scale(hc, blobs, scale, antialias):
    from triton_client_amd.server.cpu_models import PreprocessInception

    params = {"jpeg_scale": scale}
    if antialias:
        params["antialias"] = True
    (outs,) = PreprocessInception().execute([_request(blobs, **params)])
    want = []
    for b in blobs:
        if b[:2] == image.JPEG_SOI:
            p = hc.jpeg_parse(b)
            img = hc.jpeg_decode(b, scale or image.jpeg_auto_scale(p.h, p.w, 224, 224))
        else:
            img = image.decode_image(b)
        want.append(image.inception_preprocess(img, 224, 224, "NCHW", antialias=antialias))
    assert outs[0].shape == [3, 3, 224, 224]
    np.testing.assert_array_equal(outs[0].data, np.stack(want))
    if scale == 0:  # b01 at 1/2, the 40 x 50 image at full size
        np.testing.assert_array_equal(want[0], image.inception_preprocess(hc.jpeg_decode(blobs[0], 2), 224, 224, "NCHW",
                                                                          antialias=antialias))


@pytest.mark.parametrize("value", [3, -1, 16, True, "2"])
def test_cpu_preprocess_inception_rejects_another_jpeg_scale(blobs, value):
    from triton_client_amd.server.cpu_models import PreprocessInception

    with pytest.raises(ValueError, match=r"jpeg_scale must be one of 0, 1, 2, 4, 8"):
        PreprocessInception().execute([_request(blobs, jpeg_scale=value)])


def test_a_request_without_the_parameter_equals_jpeg_scale_one(blobs):
    from triton_client_amd.server.cpu_models import PreprocessInception

    m = PreprocessInception()
    (a,), (b,) = m.execute([_request(blobs), _request(blobs, jpeg_scale=1)])
    np.testing.assert_array_equal(a.data, b.data)
    np.testing.assert_array_equal(a.data[0], image.inception_preprocess(image.decode_image(blobs[0]), 224, 224))

"""Baseline JPEG on the host (csrc/host/jpeg.cc through ops.host_codec and
utils.image.decode_image) against the numpy reference of tests/jpeg_cases.py,
the reference against the float64 IDCT and against Pillow's recorded decodes,
and the decoder's refusals.  No GPU and no Pillow."""

import numpy as np
import pytest

from tests import jpeg_cases as jc
from triton_client_amd.utils import image


@pytest.fixture(scope="module")
def hc():
    from triton_client_amd.ops import host_codec

    return host_codec.load()


@pytest.fixture(scope="module")
def reference():
    """Per decodable fixture: (entry, blob, parse, coefficients, pixels) of the numpy reference."""
    out = []
    for e in jc.decodable():
        b = jc.blob(e)
        info = jc.parse(b)
        coefs = jc.entropy_decode(info)
        out.append((e, b, info, coefs, jc.pixels(info, coefs)))
    return out


# -- C1 -------------------------------------------------------------------------------
@pytest.mark.parametrize("amplitude", [5, 256, 300])
def test_reference_idct_is_within_one_of_the_float64_idct(amplitude):
    rng = np.random.default_rng(amplitude)
    v = rng.integers(-amplitude, amplitude + 1, (10000, 8, 8))
    err = np.abs(jc.idct(v) - np.floor(jc.idct_float(v) + 0.5))
    print("amplitude %d: worst |integer - round(float64)| = %d, off by one in %.4f of samples"
          % (amplitude, err.max(), (err > 0).mean()))
    assert err.max() <= 1


def test_reference_idct_of_a_dc_only_block_is_exact():
    dc = np.arange(jc.DEQ_MIN, jc.DEQ_MAX + 1)
    v = np.zeros((dc.size, 8, 8), dtype=np.int64)
    v[:, 0, 0] = dc
    want = np.floor(dc / 8.0 + 0.5).astype(np.int64)  # round(dc*Q/8), halves up
    assert (jc.idct(v) == want[:, None, None]).all()


def test_the_dequantise_clamp_keeps_every_intermediate_in_32_bits():
    """The worst block for each output sample: every coefficient at the clamp
    with the sign of its basis product."""
    b = jc._BASIS
    worst = 0
    for y in range(8):
        for x in range(8):
            v = np.where(np.outer(b[:, y], b[:, x]) >= 0, jc.DEQ_MAX, jc.DEQ_MIN)  # [v, u] = row, column
            ws = v @ jc.M1
            out = ((ws + 1024) >> 11).T @ jc.M2
            worst = max(worst, np.abs(ws).max(), np.abs(out).max() + (1 << 16))
    assert worst < 2 ** 31, worst


# -- C2 -------------------------------------------------------------------------------
def test_host_decode_equals_the_reference_bitwise(hc, reference):
    for e, b, info, coefs, want in reference:
        got = hc.jpeg_decode(b)
        assert got.shape == (e["h"], e["w"], 1 if e["mode"] == "grey" else 3), e["name"]
        np.testing.assert_array_equal(got, want, err_msg=e["name"])
        np.testing.assert_array_equal(image.decode_image(b), want, err_msg=e["name"])


def test_host_entropy_decode_equals_the_reference(hc, reference):
    for e, b, info, coefs, _ in reference:
        p = hc.jpeg_parse(b)
        hmax, vmax, mcux, mcuy = jc.geometry(info)
        assert (p.h, p.w, p.ncomp, p.hs, p.vs) == (e["h"], e["w"], len(coefs), hmax, vmax), e["name"]
        assert [(p.bh[c], p.bw[c]) for c in range(p.ncomp)] == [c.shape[:2] for c in coefs]
        assert all(p.coef_off[c] % 128 == 0 for c in range(p.ncomp))
        want = jc.coefficient_buffer(info, coefs)
        assert p.coef_bytes == len(want), e["name"]
        buf = np.full(p.coef_bytes + 64, 0xA5, dtype=np.uint8)
        hc.jpeg_entropy_decode(b, buf[:p.coef_bytes])
        assert buf[:p.coef_bytes].tobytes() == want, e["name"]
        assert (buf[p.coef_bytes:] == 0xA5).all()
        with pytest.raises(ValueError, match="malformed JPEG: coefficient buffer too small"):
            hc.jpeg_entropy_decode(b, buf[:p.coef_bytes - 1])


# -- C3 -------------------------------------------------------------------------------
def test_reference_is_close_to_pillows_decode(reference):
    """Measured (profiles/r10_jpeg.md): worst element off by 3, at least 94.7 % equal."""
    for e, _, _, _, got in reference:
        d = np.abs(got.astype(np.int64) - jc.pillow_decode(e).astype(np.int64))
        print("%-28s worst %d, equal %.4f" % (e["name"], d.max(), (d == 0).mean()))
        assert d.max() <= 3, e["name"]
        assert (d == 0).mean() >= 0.90, e["name"]


# -- C4 -------------------------------------------------------------------------------
def test_progressive_is_refused(hc):
    (e,) = jc.fixtures("refused")
    for decode in (hc.jpeg_decode, hc.jpeg_parse, image.decode_image, jc.decode):
        with pytest.raises(ValueError, match="^unsupported JPEG: progressive"):
            decode(jc.blob(e))


def _outcome(hc, data, shape):
    try:
        got = hc.jpeg_decode(data)
    except ValueError as err:
        assert str(err).startswith(("malformed JPEG: ", "unsupported JPEG: ")), err
        return "error"
    assert got.shape == shape and got.dtype == np.uint8
    return "image"


def test_every_prefix_and_2000_corruptions_give_an_error_or_an_image(hc):
    e = next(x for x in jc.fixtures("case") if x["name"].startswith("f05"))  # 4:2:0 with restart markers
    b = jc.blob(e)
    shape = (e["h"], e["w"], 3)
    seen = {"error": 0, "image": 0}
    for n in range(len(b)):
        seen[_outcome(hc, b[:n], shape)] += 1
    assert seen["error"] > len(b) // 2  # every cut inside the headers or the scan
    rng = np.random.default_rng(2000)
    hit = {"error": 0, "image": 0}
    for _ in range(2000):
        m = bytearray(b)
        m[int(rng.integers(2, len(b)))] = int(rng.integers(0, 256))
        try:
            info = hc.jpeg_parse(bytes(m))
            s = info.shape
        except ValueError:
            s = shape
        hit[_outcome(hc, bytes(m), s)] += 1
    print("prefixes %s, corruptions %s" % (seen, hit))
    assert hit["error"] and hit["image"]


@pytest.mark.parametrize("what,edit", [
    ("DC size category", lambda b: _with_dc_symbol(b, 12)),
    ("undefined table", lambda b: _with_scan_table(b, 0x33)),
    ("missing or wrong RSTn", lambda b: _with_wrong_rst(b)),
])
def test_named_malformations(hc, what, edit):
    e = next(x for x in jc.fixtures("case") if x["name"].startswith("f05"))
    with pytest.raises(ValueError, match="^malformed JPEG: " + what):
        hc.jpeg_decode(edit(jc.blob(e)))


def _segment(b, marker):
    i = b.index(bytes([0xFF, marker]))
    return i, i + 2 + ((b[i + 2] << 8) | b[i + 3])


def _with_dc_symbol(b, sym):
    """Every symbol of the first DC table becomes ``sym``."""
    i, _ = _segment(b, 0xC4)
    m = bytearray(b)
    assert m[i + 4] == 0x00  # class 0, id 0
    n = sum(m[i + 5:i + 21])
    m[i + 21:i + 21 + n] = bytes([sym]) * n
    return bytes(m)


def _with_scan_table(b, sel):
    i, _ = _segment(b, 0xDA)
    m = bytearray(b)
    m[i + 6] = sel  # the first component's table selectors
    return bytes(m)


def _with_wrong_rst(b):
    i = b.index(b"\xff\xd0", _segment(b, 0xDA)[1])
    return b[:i + 1] + b"\xd3" + b[i + 2:]


def test_a_blob_without_soi_fails_as_an_unknown_encoding():
    with pytest.raises(ValueError, match=r"^unsupported image encoding \(expected PPM/PGM/TCIMG"):
        image.decode_image(b"JFIF not an image")


def test_without_the_host_library_decode_image_says_so(monkeypatch):
    from triton_client_amd.ops import host_codec

    monkeypatch.setattr(host_codec, "_INSTANCE", None)
    monkeypatch.setattr(host_codec, "_PATH", host_codec._PATH + ".missing")
    with pytest.raises(ValueError, match="libtcamd_host.so"):
        image.decode_image(jc.blob(jc.fixtures("case")[0]))


# -- C5 -------------------------------------------------------------------------------
@pytest.mark.parametrize("antialias", [False, True])
def test_cpu_preprocess_inception_takes_jpeg(antialias):
    from triton_client_amd.server.cpu_models import PreprocessInception
    from triton_client_amd.server.types import InferRequest, InputTensor

    blobs = [jc.blob(e) for e in jc.fixtures("case") if e["name"][:3] in ("f03", "f04")]
    data = np.array(blobs, dtype=np.object_).reshape(len(blobs), 1)
    r = InferRequest(model_name="preprocess_inception", inputs=[InputTensor("INPUT", "BYTES", [len(blobs), 1], data)])
    if antialias:
        r.parameters["antialias"] = True
    (outs,) = PreprocessInception().execute([r])
    want = np.stack([image.inception_preprocess(image.decode_image(b), 224, 224, "NCHW", antialias=antialias)
                     for b in blobs])
    assert outs[0].shape == [2, 3, 224, 224]
    np.testing.assert_array_equal(outs[0].data, want)


def test_image_client_hands_jpeg_bytes_to_the_device_path(tmp_path):
    import importlib.util
    import os

    path = os.path.join(os.path.dirname(jc.GOLDEN), "..", "..", "examples", "python", "image_client.py")
    spec = importlib.util.spec_from_file_location("image_client_example", path)
    client = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(client)
    e = jc.fixtures("case")[2]
    jpg = os.path.join(jc.GOLDEN, e["name"] + ".jpg")
    assert client.load_for_device(jpg) == jc.blob(e)  # undecoded: preprocess_raw_batch_device decodes it
    ppm = tmp_path / "x.ppm"
    img = np.arange(5 * 7 * 3, dtype=np.uint8).reshape(5, 7, 3)
    ppm.write_bytes(image.encode_ppm(img))
    np.testing.assert_array_equal(client.load_for_device(str(ppm)), img)

"""PNG on the host (csrc/host/png.cc through ops.host_codec and
utils.image.decode_image) against the Python reference of tests/png_cases.py
and the Pillow-written goldens of tests/golden/png, bit for bit: the whole
decode, the staged route (``png_inflate`` then ``png_unfilter``, K25's host
twin), every error message, and the CPU ``preprocess_inception`` model.  The
parser's behaviour on arbitrary bytes is explored by csrc/cpp/tests/png_test.cc
under sanitizers."""

import json
import os
import struct
import zlib

import numpy as np
import pytest

from tests import png_cases as pc
from triton_client_amd.ops import host_codec

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "png")
CASES = pc.host_cases()


@pytest.fixture(scope="module")
def hc():
    return host_codec.load()


@pytest.fixture(scope="module")
def reference():
    """name -> the reference decode, computed once and read-only."""
    out = {}
    for name, blob in CASES:
        out[name] = pc.decode(blob)
        out[name].setflags(write=False)
    return out


def _staged(hc, blob):
    info = hc.png_parse(blob)
    buf = host_codec.aligned_buffer(info.stage_bytes)
    buf[:] = 0xA5
    hc.png_inflate(blob, buf)
    return info, buf


def test_the_case_list_covers_the_matrix():
    names = [n for n, _ in CASES]
    assert len(set(names)) == len(names)
    for ctype, depth in pc.PAIRS:
        for f in range(5):
            assert "t%dd%d_f%d" % (ctype, depth, f) in names
        assert any(n.startswith("adam7_t%dd%d_1x1" % (ctype, depth)) for n in names)
    assert len(pc.PAIRS) == 15


@pytest.mark.parametrize("name,blob", CASES, ids=[n for n, _ in CASES])
def test_decode_and_the_staged_route_equal_the_reference(hc, reference, name, blob):
    want = reference[name]
    info = hc.png_parse(blob)
    assert info.shape == want.shape and info.pixel_bytes == want.size
    assert info.bpp == pc.filter_bpp(info.ctype, info.depth)
    assert info.row_bytes == pc.row_bytes(info.w, info.ctype, info.depth)
    np.testing.assert_array_equal(hc.png_decode(blob), want)
    if info.interlace:
        with pytest.raises(ValueError, match="unsupported PNG: an interlaced file has no staged form"):
            hc.png_inflate(blob, host_codec.aligned_buffer(info.stage_bytes))
        return
    assert info.filtered_bytes == info.h * (1 + info.row_bytes)
    info, buf = _staged(hc, blob)
    np.testing.assert_array_equal(hc.png_unfilter(buf, info), want)


def test_the_staged_layout(hc):
    # colour type 3: scanlines, then 768 bytes of palette at the next multiple of 16, zero past PLTE
    blob = pc.make(3, 4, 7, 9, pc.CYCLE, palette_entries=5)
    info, buf = _staged(hc, blob)
    assert (info.h, info.w, info.depth, info.ctype, info.interlace, info.channels, info.bpp) == (7, 9, 4, 3, 0, 3, 1)
    assert info.row_bytes == 5 and info.filtered_bytes == 7 * 6 and info.palette_off == 48 and info.line_off == 0
    assert info.stage_bytes == 48 + 768
    pal = np.zeros((256, 3), dtype=np.uint8)
    pal[:5] = pc.palette_for(5)
    np.testing.assert_array_equal(buf[48:48 + 768], pal.reshape(-1))
    assert not buf[42:48].any()
    # no palette, no scratch: the scanlines are all of it
    info = hc.png_parse(pc.make(6, 16, 3, 5))
    assert info.stage_bytes == info.filtered_bytes == 3 * (1 + 40) and info.palette_off == 0
    # more rows than a pass of K25: one scanline of scratch that the host leaves alone
    blob = pc.make(3, 8, 257, 3, (2,))
    info, buf = _staged(hc, blob)
    assert info.filtered_bytes == 257 * 4 and info.palette_off == 1040 and info.line_off == 1040 + 768
    assert info.stage_bytes == info.line_off + 3
    assert (buf[info.line_off:] == 0xA5).all()
    np.testing.assert_array_equal(hc.png_unfilter(buf, info), pc.decode(blob))


def test_inflate_checks_its_buffer_and_unfilter_its_pairing(hc):
    blob = pc.make(2, 8, 4, 4)
    info = hc.png_parse(blob)
    with pytest.raises(ValueError, match="malformed PNG: output buffer too small"):
        hc.png_inflate(blob, host_codec.aligned_buffer(info.stage_bytes - 1))
    info, buf = _staged(hc, blob)
    with pytest.raises(ValueError, match="do not belong together"):
        hc.png_unfilter(buf[:-1], info)


def test_the_goldens_decode_to_what_pillow_made_of_them(hc):
    with open(os.path.join(GOLDEN, "manifest.json")) as f:
        manifest = json.load(f)
    assert len(manifest) >= 7
    for entry in manifest:
        with open(os.path.join(GOLDEN, entry["png"]), "rb") as f:
            blob = f.read()
        want = np.load(os.path.join(GOLDEN, entry["npy"]))
        got = hc.png_decode(blob)
        assert got.shape == tuple(entry["shape"])
        np.testing.assert_array_equal(got, want.reshape(got.shape), err_msg=entry["png"])
        np.testing.assert_array_equal(pc.decode(blob), got, err_msg=entry["png"])


# ---- errors: each made by editing a valid file's bytes ---------------------------------------
def _rechunk(blob, kind, edit):
    """``blob`` with the data of its first ``kind`` chunk replaced by ``edit(data)`` (None drops
    the chunk) and the CRC made right again."""
    out = pc.SIGNATURE
    done = False
    for k, at, n in pc.chunks(blob):
        data = blob[at:at + n]
        if k == kind and not done:
            done = True
            data = edit(data)
            if data is None:
                continue
        out += pc.chunk(k, data)
    assert done
    return out


def _ihdr(blob, **fields):
    def edit(data):
        v = dict(zip(("w", "h", "depth", "ctype", "comp", "filt", "lace"), struct.unpack(">IIBBBBB", data)))
        v.update(fields)
        return struct.pack(">IIBBBBB", *(v[k] for k in ("w", "h", "depth", "ctype", "comp", "filt", "lace")))

    return _rechunk(blob, b"IHDR", edit)


def _flip(blob, kind, offset):
    """One bit of the first ``kind`` chunk's data flipped, the CRC left as it was."""
    at = next(a for k, a, _ in pc.chunks(blob) if k == kind)
    b = bytearray(blob)
    b[at + offset] ^= 0x01
    return bytes(b)


def _refilter(blob, edit):
    """The inflated bytes of a one-IDAT file edited and deflated again."""
    return _rechunk(blob, b"IDAT", lambda d: zlib.compress(bytes(edit(bytearray(zlib.decompress(d))))))


def _set(data, at, value):
    data[at] = value
    return data


RGB = pc.make(2, 8, 5, 6, pc.CYCLE)
PAL = pc.make(3, 8, 5, 6, pc.CYCLE)
LACED = pc.make(2, 8, 5, 6, pc.CYCLE, adam7=True)
ERRORS = [
    ("unsupported PNG: colour type 2 with bit depth 4", _ihdr(RGB, depth=4)),
    ("unsupported PNG: colour type 5 with bit depth 8", _ihdr(RGB, ctype=5)),
    ("unsupported PNG: colour type 3 with bit depth 16", _ihdr(PAL, depth=16)),
    ("unsupported PNG: 16385 x 5, a side above 16384", _ihdr(RGB, w=16385)),
    ("unsupported PNG: 6 x 70000, a side above 16384", _ihdr(RGB, h=70000)),
    ("unsupported PNG: compression method 1", _ihdr(RGB, comp=1)),
    ("unsupported PNG: filter method 1", _ihdr(RGB, filt=1)),
    ("unsupported PNG: interlace method 2", _ihdr(RGB, lace=2)),
    ("malformed PNG: bad CRC in IHDR", _flip(RGB, b"IHDR", 3)),
    ("malformed PNG: bad CRC in PLTE", _flip(PAL, b"PLTE", 10)),
    ("malformed PNG: bad CRC in IDAT", _flip(RGB, b"IDAT", 20)),
    ("malformed PNG: truncated chunk", RGB[:-30]),
    ("malformed PNG: truncated chunk", RGB[:-12]),  # the file ends without IEND
    ("malformed PNG: missing IHDR", _rechunk(RGB, b"IHDR", lambda d: None)),
    ("malformed PNG: missing IHDR", pc.SIGNATURE),
    ("malformed PNG: missing PLTE", _rechunk(PAL, b"PLTE", lambda d: None)),
    ("malformed PNG: missing IDAT", _rechunk(RGB, b"IDAT", lambda d: None)),
    ("malformed PNG: zlib: ", _rechunk(RGB, b"IDAT", lambda d: d[:2] + b"\xff" * (len(d) - 2))),
    ("malformed PNG: zlib: the stream ends early", _rechunk(RGB, b"IDAT", lambda d: d[:-6])),
    ("malformed PNG: inflated length 94, not the 95 of the header", _refilter(RGB, lambda d: d[:-1])),
    ("malformed PNG: inflated length above the 95 of the header", _refilter(RGB, lambda d: d + b"\x00")),
    ("malformed PNG: inflated length above the 76 of the header", _ihdr(RGB, h=4)),
    ("malformed PNG: inflated length", _ihdr(LACED, w=7)),  # Adam7: the passes of a 7 x 5 image need more
    ("malformed PNG: filter type 5 in row 2", _refilter(RGB, lambda d: _set(d, 2 * 19, 5))),
    ("malformed PNG: filter type 255 in row 0", _refilter(RGB, lambda d: _set(d, 0, 255))),
    ("malformed PNG: filter type 9 in row", _refilter(LACED, lambda d: _set(d, 0, 9))),
    ("malformed PNG: no PNG signature", b"\x89PNG\r\n\x1a\r" + RGB[8:]),
]


@pytest.mark.parametrize("message,blob", ERRORS, ids=["%02d %s" % (i, m[:48]) for i, (m, _) in enumerate(ERRORS)])
def test_every_error_has_its_message(hc, message, blob):
    import re

    with pytest.raises(ValueError, match="^" + re.escape(message)):
        hc.png_decode(blob)
    # the parse alone sees what is wrong with the headers; the inflate sees the rest
    staged_only = ("IDAT" in message and "missing" not in message) or "zlib" in message or "inflated" in message \
        or "filter type" in message
    if staged_only:
        info = hc.png_parse(blob)
        if not info.interlace:
            with pytest.raises(ValueError, match="^" + re.escape(message)):
                hc.png_inflate(blob, host_codec.aligned_buffer(info.stage_bytes))
    else:
        with pytest.raises(ValueError, match="^" + re.escape(message)):
            hc.png_parse(blob)


def test_the_parse_inflates_nothing(hc):
    # a valid header over garbage image data: the parse succeeds, the inflate is what fails
    blob = _rechunk(RGB, b"IDAT", lambda d: b"\x00" * len(d))
    assert hc.png_parse(blob).shape == (5, 6, 3)
    with pytest.raises(ValueError, match="malformed PNG: zlib"):
        hc.png_decode(blob)


def test_decode_image_takes_png():
    from triton_client_amd.utils.image import decode_image

    for blob in (RGB, LACED, pc.make(0, 1, 5, 9, pc.CYCLE), pc.make(4, 16, 3, 3)):
        np.testing.assert_array_equal(decode_image(blob), pc.decode(blob))
        np.testing.assert_array_equal(decode_image(bytearray(blob), jpeg_scale=4), pc.decode(blob))
    with pytest.raises(ValueError, match="malformed PNG: bad CRC in IHDR"):
        decode_image(_flip(RGB, b"IHDR", 3))
    with pytest.raises(ValueError, match=r"unsupported image encoding \(expected PPM/PGM/TCIMG/JPEG/PNG\)"):
        decode_image(b"GIF89a" + bytes(20))


def test_the_cpu_preprocess_model_serves_png():
    from triton_client_amd.server.cpu_models import PreprocessInception
    from triton_client_amd.server.types import InferRequest, InputTensor
    from triton_client_amd.utils.image import inception_preprocess

    blobs = [pc.make(2, 8, 37, 29, pc.CYCLE), pc.make(3, 2, 33, 35, pc.CYCLE, adam7=True), pc.make(0, 16, 20, 31, (4,))]
    data = np.array(blobs, dtype=np.object_).reshape(len(blobs), 1)
    r = InferRequest(model_name="preprocess_inception", inputs=[InputTensor("INPUT", "BYTES", [len(blobs), 1], data)])
    (outs,) = PreprocessInception().execute([r])
    assert outs[0].shape == [3, 3, 224, 224]
    want = np.stack([inception_preprocess(pc.decode(b), 224, 224, "NCHW") for b in blobs])
    np.testing.assert_array_equal(outs[0].data, want)

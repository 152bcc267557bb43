"""K25 png_unfilter (csrc/kernels/png.hip) against its host twin
(``HostCodec.png_unfilter``, csrc/host/png.cc), bit for bit, and the PNG route
through the GPU ``preprocess_inception``, the served ensemble and
``preprocess_raw_batch_device``.  The host decoder itself is pinned to the
Python reference and to Pillow's goldens in tests/test_png_host.py; everything
PNG decides is lossless, so every comparison is ``array_equal``, but the one of
the served ensemble's logits, whose engine does not repeat itself bit for bit
(``test_served_ensemble_on_png_matches_the_tcimg_of_its_decode``).  The images that sit on
the kernel's decomposition take its constants from the library
(``hip.png_unfilter_geometry``), not from literals."""

import glob
import os
from collections import namedtuple

import numpy as np
import pytest

from tests import png_cases as pc
from triton_client_amd.utils import image

pytestmark = pytest.mark.gpu

CANARY = 0xA5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def hc():
    from triton_client_amd.ops import host_codec

    return host_codec.load()


def _stage(hc, blob):
    from triton_client_amd.ops import host_codec

    info = hc.png_parse(blob)
    buf = host_codec.aligned_buffer(info.stage_bytes)
    buf[:] = 0x3C  # what the scratch scanline holds before the kernel is nobody's business
    hc.png_inflate(blob, buf)
    return info, buf


def _k25(hc, blobs, name=""):
    """``blobs`` through ONE ``hip.png_unfilter`` call and against the host twin.  The staged bytes
    of all images lie in one device buffer at different multiples of 16, the outputs in another at
    odd addresses, a canary byte before and after each that must be left alone."""
    import torch

    from triton_client_amd.ops import hip

    dev = torch.device("cuda", 0)
    staged = [_stage(hc, b) for b in blobs]
    src_at, dst_at, up, only = [], [], 16, 0
    for k, (info, buf) in enumerate(staged):
        up = -(-up // 16) * 16 + 16 * (k % 3)  # 16-byte aligned, and not all at multiples of 32 or 64
        src_at.append(up)
        up += info.stage_bytes
        only += 1 + only % 2  # one or two canary bytes, then an odd address
        dst_at.append(only)
        only += info.pixel_bytes
    only += 1
    host = np.full(up, 0x3C, dtype=np.uint8)
    for at, (info, buf) in zip(src_at, staged):
        host[at:at + info.stage_bytes] = buf
    src = torch.from_numpy(host).to(dev)
    dst = torch.full((only,), CANARY, device=dev, dtype=torch.uint8)
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 2 == 0 and all(a % 2 == 1 for a in dst_at)
    hip.png_unfilter([src.data_ptr() + a for a in src_at], [i for i, _ in staged], [dst.data_ptr() + a for a in dst_at],
                     stream=torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    out = dst.cpu().numpy()
    mine = np.zeros(only, dtype=bool)
    for k, (at, (info, buf)) in enumerate(zip(dst_at, staged)):
        want = hc.png_unfilter(buf, info)
        np.testing.assert_array_equal(out[at:at + info.pixel_bytes].reshape(info.shape), want,
                                      err_msg="%s image %d %s type %d depth %d" % (name, k, info.shape, info.ctype,
                                                                                   info.depth))
        mine[at:at + info.pixel_bytes] = True
    assert (out[~mine] == CANARY).all(), "a byte outside an image's pixels was written"
    # the staged scanlines and palettes are only read
    back = src.cpu().numpy()
    for at, (info, buf) in zip(src_at, staged):
        end = info.line_off or info.stage_bytes
        np.testing.assert_array_equal(back[at:at + end], buf[:end])


# -- the colour type / depth x filter matrix --------------------------------------------------
def test_the_matrix_of_types_depths_and_filters_equals_the_host(hc):
    cases = [(n, b) for n, b in pc.host_cases() if not n.startswith("adam7")]
    assert len(cases) > 64 * 3  # several launches of one call
    for ctype, depth in pc.PAIRS:
        for f in range(5):
            assert any(n == "t%dd%d_f%d" % (ctype, depth, f) for n, _ in cases)
    _k25(hc, [b for _, b in cases], "matrix")
    # and one of each pair at the largest size of this test, all filters cycling
    _k25(hc, [pc.make(ctype, depth, 40, 37, pc.CYCLE) for ctype, depth in pc.PAIRS], "40x37")


def test_the_goldens(hc):
    blobs = []
    for path in sorted(glob.glob(os.path.join(GOLDEN, "png", "*.png"))):
        with open(path, "rb") as f:
            blobs.append(f.read())
    blobs = [b for b in blobs if not hc.png_parse(b).interlace]  # K25 takes no Adam7 file
    assert len(blobs) >= 7
    _k25(hc, blobs, "goldens")


# -- the edges of the decomposition -----------------------------------------------------------
@pytest.fixture(scope="module")
def geometry():
    from triton_client_amd.ops import hip

    rows_per_wave, rows_per_pass, col_chunk = hip.png_unfilter_geometry()
    assert 0 < rows_per_wave < rows_per_pass and rows_per_pass % rows_per_wave == 0 and col_chunk > 0
    return rows_per_wave, rows_per_pass, col_chunk


@pytest.mark.parametrize("schedule", [(4,), (3,)], ids=["paeth", "average"])
def test_heights_around_every_row_boundary(hc, geometry, schedule):
    rpw, rpp, _ = geometry
    heights = sorted({b + d for b in (rpw, 2 * rpw, rpp) for d in (-1, 0, 1)} | {2 * rpp + 1})
    blobs = [pc.make(2, 8, h, 3, schedule) for h in heights]
    # the other unit widths at the tallest: 8 bytes (two shuffles), 1 byte of 8 pixels, a palette
    blobs += [pc.make(6, 16, 2 * rpp + 1, 3, schedule), pc.make(0, 1, rpp + 1, 3, schedule),
              pc.make(3, 8, rpp + 1, 3, schedule), pc.make(4, 8, rpp + rpw + 1, 3, schedule)]
    _k25(hc, blobs, "heights %s" % (heights,))


@pytest.mark.parametrize("schedule", [(4,), (3,), (1, 4)], ids=["paeth", "average", "sub-paeth"])
def test_widths_around_every_column_boundary(hc, geometry, schedule):
    _, _, cc = geometry
    widths = sorted({b + d for b in (cc, 2 * cc) for d in (-1, 0, 1)} | {4 * cc + 1, 5 * cc + 1})
    blobs = [pc.make(2, 8, 2, w, schedule) for w in widths]
    # a unit of depth 4 is two pixels: the same boundaries in units, and the half-filled last byte
    blobs += [pc.make(0, 4, 2, w, schedule) for w in (2 * cc - 1, 2 * cc, 2 * cc + 1, 2 * cc + 2, 4 * cc + 1)]
    blobs += [pc.make(6, 16, 2, w, schedule) for w in (cc, cc + 1)]
    _k25(hc, blobs, "widths %s" % (widths,))


def test_both_sides_just_past_a_boundary_cycling_the_filters(hc, geometry):
    rpw, rpp, cc = geometry
    waves = rpp // rpw
    _k25(hc, [pc.make(2, 8, rpp + 1, cc + 1, pc.CYCLE),
              pc.make(2, 8, rpp + 1, (waves + 1) * cc + 1, pc.CYCLE),  # more chunks than waves: another pass period
              pc.make(3, 2, rpp + 1, 4 * cc + 1, pc.CYCLE),
              pc.make(4, 16, rpw + 1, cc + 1, pc.CYCLE)], "both sides")


# -- launches ---------------------------------------------------------------------------------
def test_one_launch_of_mixed_images(hc):
    sizes = [(1, 1), (5, 9), (33, 17), (2, 40), (40, 2), (7, 8), (31, 20), (9, 13), (16, 16), (3, 70), (12, 1),
             (1, 12), (20, 31), (8, 7), (39, 40)]
    blobs = [pc.make(ctype, depth, h, w, pc.CYCLE, seed=k) for k, ((ctype, depth), (h, w)) in enumerate(zip(pc.PAIRS, sizes))]
    blobs.append(pc.make(3, 8, 11, 6, pc.CYCLE, palette_entries=100))  # indices past the end of PLTE
    assert len(blobs) <= 64
    _k25(hc, blobs, "mixed")


def test_65_tiny_images_take_a_second_launch(hc):
    _k25(hc, [pc.make(*pc.PAIRS[k % len(pc.PAIRS)], 1 + k % 3, 1 + k % 5, pc.CYCLE, seed=k) for k in range(65)], "65")


Info = namedtuple("Info", "h w ctype depth interlace")


@pytest.mark.parametrize("what", ["interlaced", "too wide", "too tall", "zero side", "no such pair", "null source",
                                  "misaligned source", "null destination"])
def test_bad_arguments_are_refused_before_any_launch(what):
    import torch

    from triton_client_amd.ops import hip

    dev = torch.device("cuda", 0)
    src = torch.zeros(4096, device=dev, dtype=torch.uint8)
    dst = torch.full((4096,), CANARY, device=dev, dtype=torch.uint8)
    info, s, d = Info(4, 4, 2, 8, 0), src.data_ptr(), dst.data_ptr()
    if what == "interlaced":
        info = info._replace(interlace=1)
    elif what == "too wide":
        info = info._replace(w=hip.RESIZE_MAX_DIM + 1)
    elif what == "too tall":
        info = info._replace(h=hip.RESIZE_MAX_DIM + 1)
    elif what == "zero side":
        info = info._replace(h=0)
    elif what == "no such pair":
        info = info._replace(ctype=3, depth=16)
    elif what == "null source":
        s = 0
    elif what == "misaligned source":
        s += 8
    else:
        d = 0
    good = Info(4, 4, 2, 8, 0)
    with pytest.raises(hip.HipError) as err:
        hip.png_unfilter([src.data_ptr() + 1024, s], [good, info], [dst.data_ptr() + 1024, d])
    assert err.value.code == 1  # hipErrorInvalidValue
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == CANARY).all()  # the good image before it was not launched either
    with pytest.raises(ValueError):
        hip.png_unfilter([s], [good, good], [d])


# -- the GPU preprocess_inception -------------------------------------------------------------
def _request(blobs, ensemble_step=False, **parameters):
    from triton_client_amd.server.types import InferRequest, InputTensor

    data = np.array(list(blobs), dtype=np.object_).reshape(len(blobs), 1)
    r = InferRequest(model_name="preprocess_inception", inputs=[InputTensor("INPUT", "BYTES", [len(blobs), 1], data)])
    r.parameters.update(parameters)
    if ensemble_step:
        r.accepts_device_outputs = True
    return r


def _rows(outs):
    from triton_client_amd.server.types import DeviceView, InputTensor

    (o,) = outs
    if isinstance(o.data, DeviceView):
        return InputTensor("x", "FP32", o.shape, o.data).numpy()
    return o.data


@pytest.fixture(scope="module")
def models():
    """``PreprocessInception`` loaded with TCAMD_DEVICE_PNG=0 and =1."""
    from triton_client_amd.server.gpu_models import PreprocessInception

    mp = pytest.MonkeyPatch()
    out = {}
    for knob in ("0", "1"):
        mp.setenv("TCAMD_DEVICE_PNG", knob)
        out[knob] = PreprocessInception()
        out[knob].load()
    mp.undo()
    assert not out["0"].device_png and out["1"].device_png
    yield out
    for m in out.values():
        m.unload()


def _count(mp, name):
    from triton_client_amd.ops import hip

    real = getattr(hip, name)
    calls = []

    def counted(first, *a, **kw):
        calls.append(len(first))
        return real(first, *a, **kw)

    mp.setattr(hip, name, counted)
    return calls


def _jpeg(prefix):
    (path,) = glob.glob(os.path.join(GOLDEN, "jpeg", prefix + "_*.jpg"))
    with open(path, "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def pngs():
    """PNG blobs of the served tests: RGB, a 2-bit palette, 16-bit grey + alpha, taller than a pass, interlaced."""
    return [pc.make(2, 8, 97, 131, pc.CYCLE), pc.make(3, 2, 64, 48, pc.CYCLE), pc.make(4, 16, 50, 70, pc.CYCLE),
            pc.make(6, 8, 300, 41, pc.CYCLE), pc.make(2, 8, 37, 29, pc.CYCLE, adam7=True)]


def _twin(blob):
    """The TCIMG of a blob's host decode."""
    return image.encode_raw(image.decode_image(blob))


@pytest.mark.parametrize("parameters", [{}, {"antialias": True}, {"jpeg_scale": 2}, {"jpeg_scale": 0, "antialias": True}],
                         ids=["plain", "antialias", "jpeg_scale", "auto_scale_antialias"])
@pytest.mark.parametrize("ensemble_step", [False, True], ids=["direct", "ensemble_step"])
def test_png_blobs_give_the_rows_of_their_tcimg_twins(models, pngs, ensemble_step, parameters, monkeypatch):
    model = models["1"]
    tcimg = image.encode_raw(np.random.default_rng(5).integers(0, 256, (33, 47, 3), dtype=np.uint8))
    jpeg = _jpeg("f03")
    batches = [pngs[:3], [pngs[3], jpeg, tcimg, pngs[4]]]  # PNG alone; PNG, JPEG, TCIMG and an interlaced PNG
    k25 = _count(monkeypatch, "png_unfilter")
    got = model.execute([_request(b, ensemble_step, **parameters) for b in batches])
    assert k25 == [4]  # the four non-interlaced PNGs of two requests: one K25 call
    monkeypatch.undo()
    # the JPEG stays a JPEG in the twin batch (its scale is the request's); every PNG becomes its pixels
    twins = [[_twin(b) if b[:4] == b"\x89PNG" else b for b in batch] for batch in batches]
    want = model.execute([_request(b, ensemble_step, **parameters) for b in twins])
    for g, w in zip(got, want):
        assert not isinstance(g, Exception) and not isinstance(w, Exception), (g, w)
        np.testing.assert_array_equal(_rows(g), _rows(w))


def test_the_png_knob_changes_the_route_and_not_one_bit_of_the_rows(models, pngs, monkeypatch):
    tcimg = image.encode_raw(np.random.default_rng(6).integers(0, 256, (64, 48, 1), dtype=np.uint8))
    batches = [[pngs[0], tcimg, pngs[1]], [pngs[3], pngs[4], _jpeg("f05"), pngs[2]]]
    rows = {}
    for knob, model in models.items():
        k25 = _count(monkeypatch, "png_unfilter")
        for antialias in (False, True):
            rows[knob, antialias] = model.execute([_request(b, antialias=antialias) for b in batches])
        assert k25 == ([4, 4] if knob == "1" else [])  # the four non-interlaced PNGs: one K25 call a batch, or none
        monkeypatch.undo()
    for antialias in (False, True):
        for got, want in zip(rows["1", antialias], rows["0", antialias]):
            np.testing.assert_array_equal(got[0].data, want[0].data)


def test_a_malformed_png_fails_its_own_request_with_the_hosts_message(models, pngs, hc):
    bad = bytearray(pngs[0])
    at = next(a for k, a, _ in pc.chunks(pngs[0]) if k == b"IDAT")
    bad[at + 40] ^= 0x10  # inside the image data: the parse passes, the inflate finds the CRC
    bad = bytes(bad)
    with pytest.raises(ValueError) as host_err:
        hc.png_decode(bad)
    assert str(host_err.value) == "malformed PNG: bad CRC in IDAT"
    header = pngs[1][:25] + b"\x09" + pngs[1][26:]  # IHDR's colour type overwritten: the parse itself refuses
    with pytest.raises(ValueError) as header_err:
        hc.png_decode(header)
    for knob, model in models.items():
        requests = [_request([pngs[1]]), _request([pngs[2], bad]), _request([pngs[0], pngs[3]]), _request([header])]
        res = model.execute(requests)
        assert isinstance(res[1], ValueError) and str(res[1]) == str(host_err.value), knob
        assert isinstance(res[3], ValueError) and str(res[3]) == str(header_err.value), knob
        want = model.execute([_request([_twin(pngs[1])]), _request([_twin(pngs[0]), _twin(pngs[3])])])
        np.testing.assert_array_equal(_rows(res[0]), _rows(want[0]))
        np.testing.assert_array_equal(_rows(res[2]), _rows(want[1]))


# -- the client helper ------------------------------------------------------------------------
@pytest.mark.parametrize("antialias", [False, True])
def test_preprocess_raw_batch_device_with_png_bytes_equals_the_decoded_arrays(pngs, antialias, monkeypatch):
    arr = np.random.default_rng(9).integers(0, 256, (50, 70, 3), dtype=np.uint8)
    mixed = [pngs[0], arr, pngs[1], _jpeg("f03"), pngs[4], pngs[3], pngs[2]]
    decoded = [image.decode_image(b) if isinstance(b, bytes) else b for b in mixed]
    want = image.preprocess_raw_batch_device(decoded, 3, 224, 224, antialias=antialias)
    k25 = _count(monkeypatch, "png_unfilter")
    got = image.preprocess_raw_batch_device(mixed, 3, 224, 224, antialias=antialias)
    assert got.shape == (7, 3, 224, 224)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(image.preprocess_raw_batch_device(mixed, 3, 224, 224, antialias=antialias,
                                                                    device_png=False), want)
    monkeypatch.setenv("TCAMD_DEVICE_PNG", "0")
    np.testing.assert_array_equal(image.preprocess_raw_batch_device(mixed, 3, 224, 224, antialias=antialias), want)
    assert k25 == [4]  # the four non-interlaced PNGs, once: the other two calls had the knob off


# -- served -----------------------------------------------------------------------------------
def _served(gpu_server, proto, model, blobs, antialias):
    import tritonclient.grpc as grpcclient
    import tritonclient.http as httpclient

    mod = grpcclient if proto == "grpc" else httpclient
    c = mod.InferenceServerClient(gpu_server.grpc_url if proto == "grpc" else gpu_server.http_url)
    inp = mod.InferInput("INPUT", [len(blobs), 1], "BYTES")
    inp.set_data_from_numpy(np.array(blobs, dtype=np.object_).reshape(len(blobs), 1))
    kw = {"parameters": {"antialias": True}} if antialias else {}
    out = c.infer(model, [inp], **kw).as_numpy("OUTPUT")
    c.close()
    return out


@pytest.mark.parametrize("antialias", [False, True])
@pytest.mark.parametrize("proto", ["http", "grpc"])
def test_served_preprocess_on_png_equals_the_tcimg_of_its_decode(gpu_server, pngs, proto, antialias):
    """Everything PNG decides, through a real server: the rows that ``preprocess_inception`` serves, and
    hands to ``densenet_onnx`` inside the ensemble, are those of the TCIMG twins bit for bit."""
    got = _served(gpu_server, proto, "preprocess_inception", pngs, antialias)
    want = _served(gpu_server, proto, "preprocess_inception", [_twin(b) for b in pngs], antialias)
    assert got.shape == (len(pngs), 3, 224, 224)
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("antialias", [False, True])
@pytest.mark.parametrize("proto", ["http", "grpc"])
def test_served_ensemble_on_png_matches_the_tcimg_of_its_decode(gpu_server, pngs, proto, antialias):
    """The ensemble's logits.  Its second step, the served ``densenet_onnx`` engine, does not repeat
    itself bit for bit: on an MI355X two requests with the SAME five TCIMG blobs gave logits 2.6e-6
    apart (4.855096e-04 and 4.828870e-04 in one place), and the PNG request differed from the TCIMG
    request by at most 1.29e-5 absolute although the rows that went into the engine were equal bit
    for bit (the test above, and ``ensemble_step`` in
    ``test_png_blobs_give_the_rows_of_their_tcimg_twins``).  ``array_equal`` on the logits would test
    that noise and not PNG, so this one comparison takes the bound the served tests of this suite
    have for the engine (tests/test_jpeg_gpu.py, tests/test_preprocess_device_gpu.py): rel-L2 below
    1e-3 per row and the same top class."""
    got = _served(gpu_server, proto, "preprocess_inception_ensemble", pngs, antialias)
    ref = _served(gpu_server, proto, "preprocess_inception_ensemble", [_twin(b) for b in pngs], antialias)
    assert got.shape == (len(pngs), 1000)
    rel = np.linalg.norm(got - ref, axis=1) / np.linalg.norm(ref, axis=1)
    print("%s antialias=%s: per-row rel-L2 PNG vs TCIMG request %s, max abs %g" % (proto, antialias, rel,
                                                                                  np.abs(got - ref).max()))
    assert rel.max() < 1e-3, rel
    assert np.array_equal(got.argmax(axis=1), ref.argmax(axis=1))

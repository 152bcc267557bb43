"""The reduced-size decode of K22 jpeg_decode (csrc/kernels/jpeg.hip, scales
1/2, 1/4 and 1/8) against the host's scaled decode (csrc/host/jpeg.cc) and the
numpy reference of tests/jpeg_scaled_cases.py, bit for bit, and the
``jpeg_scale`` request parameter through the GPU ``preprocess_inception``, the
served ensemble and ``preprocess_raw_batch_device``.  The host decoder itself is
pinned to the reference in test_jpeg_scaled_host.py.

The scaled kernel's tile is 64 x 32 output pixels, as at full size."""

import numpy as np
import pytest

from tests import jpeg_cases as jc
from tests import jpeg_scaled_cases as js
from triton_client_amd.utils import image

pytestmark = pytest.mark.gpu

CANARY = 0xA5
GUARD = 64


@pytest.fixture(scope="module")
def hc():
    from triton_client_amd.ops import host_codec

    return host_codec.load()


@pytest.fixture(scope="module")
def cases(hc):
    """Per decodable fixture and scale 1, 2, 4, 8: (name, parse, coefficient buffer, host pixels)."""
    out = []
    for e in jc.decodable():
        b = jc.blob(e)
        for s in js.SCALES:
            info = hc.jpeg_parse(b, s)
            coef = np.empty(info.coef_bytes, dtype=np.uint8)
            hc.jpeg_entropy_decode(b, coef, s)
            out.append(("%s at 1/%d" % (e["name"], s), info, coef, hc.jpeg_decode(b, s)))
    return out


def _run(jobs, offsets):
    """Decode ``jobs`` [(name, info, coef, expected)] in one ``hip.jpeg_decode``
    call, job k's destination ``offsets[k % len(offsets)]`` bytes past a 64-byte
    boundary and fenced by canaries; returns the pixels and checks the fences."""
    import torch

    from triton_client_amd.ops import hip

    dev = torch.device("cuda", 0)
    srcs, dsts, bufs = [], [], []
    for k, (_, info, coef, _) in enumerate(jobs):
        src = torch.from_numpy(coef).to(dev)
        off = offsets[k % len(offsets)]
        buf = torch.full((GUARD + off + info.pixel_bytes + GUARD,), CANARY, device=dev, dtype=torch.uint8)
        assert src.data_ptr() % 16 == 0 and buf.data_ptr() % 64 == 0
        srcs.append(src)
        bufs.append((buf, off))
        dsts.append(buf.data_ptr() + GUARD + off)
    hip.jpeg_decode([s.data_ptr() for s in srcs], [j[1] for j in jobs], dsts,
                    stream=torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    got = []
    for (name, info, _, _), (buf, off) in zip(jobs, bufs):
        a = buf.cpu().numpy()
        assert (a[:GUARD + off] == CANARY).all() and (a[GUARD + off + info.pixel_bytes:] == CANARY).all(), \
            "%s: a byte outside the destination was written" % name
        got.append(a[GUARD + off:GUARD + off + info.pixel_bytes].reshape(info.shape))
    return got


# -- single images ----------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_every_fixture_alone_at_every_scale_equals_the_host_scaled_decode(cases, offset):
    for job in cases:
        if job[1].scale == 1:
            continue  # tests/test_jpeg_gpu.py
        (got,) = _run([job], [offset])
        np.testing.assert_array_equal(got, job[3], err_msg=job[0])


def test_all_fixtures_at_all_four_scales_in_one_mixed_call(cases):
    assert len(cases) == 4 * len(jc.decodable()) and {j[1].scale for j in cases} == {1, 2, 4, 8}
    for job, got in zip(cases, _run(cases, [0, 1, 2, 3])):
        np.testing.assert_array_equal(got, job[3], err_msg=job[0])


def test_65_scaled_copies_take_a_second_launch(cases):
    job = next(j for j in cases if j[0].startswith("f02") and j[1].scale == 2)
    for got in _run([job] * 65, [3, 0, 1, 2]):
        np.testing.assert_array_equal(got, job[3])


# -- tile edges --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def synthetic():
    """Random coefficient buffers of every sampling whose result is one to three
    pixels past the 64 x 32 tile both ways: (name, parse, compact buffer, the
    numpy reference's pixels).  b01 among the fixtures above covers 4:2:0 (80 x
    60 at 1/8); it is here too, for the sizes that leave a ragged last block."""
    out = []
    for k, (scale, (W, H)) in enumerate({8: (530, 270), 4: (270, 140), 2: (140, 70)}.items()):
        for m, mode in enumerate(("grey", "444", "422", "420")):
            info, coefs = js.synthetic(H, W, mode, seed=100 * k + m)
            buf = np.frombuffer(js.coefficient_buffer(info, coefs, scale), dtype=np.uint8).copy()
            out.append(("%s %dx%d at 1/%d" % (mode, W, H, scale), js.Parse(info, scale), buf,
                        js.pixels(info, coefs, scale)))
    return out


def test_results_one_past_the_tile_equal_the_numpy_reference(synthetic):
    for job in synthetic:
        assert job[1].w > 64 and job[1].h > 32 and job[3].shape == job[1].shape
    for job, got in zip(synthetic, _run(synthetic, [1, 0, 3, 2])):
        np.testing.assert_array_equal(got, job[3], err_msg=job[0])


# -- bad arguments -----------------------------------------------------------------------
class _Info:
    def __init__(self, info, **kw):
        for f in ("h", "w", "ncomp", "hs", "vs", "scale", "ny", "nx"):
            setattr(self, f, kw.get(f, getattr(info, f)))


@pytest.mark.parametrize("what", ["scale 3", "scale 16", "ny against the sampling", "nx of the full size",
                                  "a full-size image beside a bad one"])
def test_bad_scaled_arguments_are_refused_before_any_launch(cases, what):
    import torch

    from triton_client_amd.ops import hip

    _, info, coef, _ = next(j for j in cases if j[0].startswith("f02") and j[1].scale == 2)  # 4:2:0: ny = nx = 4, 8, 8
    _, full, fcoef, _ = next(j for j in cases if j[0].startswith("f02") and j[1].scale == 1)
    dev = torch.device("cuda", 0)
    src, fsrc = torch.from_numpy(coef).to(dev), torch.from_numpy(fcoef).to(dev)
    dst = torch.full((GUARD + full.pixel_bytes + GUARD,), CANARY, device=dev, dtype=torch.uint8)
    sp, fp, dp = src.data_ptr(), fsrc.data_ptr(), dst.data_ptr() + GUARD
    args = {
        "scale 3": ([sp], [_Info(info, scale=3)], [dp]),
        "scale 16": ([sp], [_Info(info, scale=16)], [dp]),
        "ny against the sampling": ([sp], [_Info(info, ny=[4, 4, 4])], [dp]),
        "nx of the full size": ([sp], [_Info(info, nx=[8, 8, 8])], [dp]),
        "a full-size image beside a bad one": ([fp, sp], [full, _Info(info, ny=[2, 8, 8])], [dp, dp]),
    }[what]
    with pytest.raises(hip.HipError) as err:
        hip.jpeg_decode(*args)
    assert err.value.code == 1  # hipErrorInvalidValue
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == CANARY).all()


# -- the GPU preprocess_inception ----------------------------------------------------------
def _request(blobs, ensemble_step=False, **params):
    from triton_client_amd.server.types import InferRequest, InputTensor

    data = np.array(list(blobs), dtype=np.object_).reshape(len(blobs), 1)
    r = InferRequest(model_name="preprocess_inception", inputs=[InputTensor("INPUT", "BYTES", [len(blobs), 1], data)])
    r.parameters.update(params)
    if ensemble_step:
        r.accepts_device_outputs = True
    return r


def _rows(outs):
    from triton_client_amd.server.types import DeviceView, InputTensor

    (o,) = outs
    if isinstance(o.data, DeviceView):
        return InputTensor("x", "FP32", o.shape, o.data).numpy()
    return o.data


def _count(name):
    """Counts the calls of ``hip.<name>`` and their images from here on."""
    from triton_client_amd.ops import hip

    real = getattr(hip, name)
    calls = []

    def counted(srcs, *a, **kw):
        calls.append(len(srcs))
        return real(srcs, *a, **kw)

    mp = pytest.MonkeyPatch()
    mp.setattr(hip, name, counted)

    def done():
        mp.undo()
        return calls

    return done


@pytest.fixture(scope="module")
def model():
    from triton_client_amd.server.gpu_models import PreprocessInception

    m = PreprocessInception()
    m.load()
    yield m
    m.unload()


def _blob(prefix):
    return jc.blob(next(e for e in jc.decodable() if e["name"].startswith(prefix)))


def _twin(hc, blob, scale):
    """The TCIMG of the host's decode of a JPEG at ``scale`` (0: automatic for 224 x 224)."""
    if blob[:2] != image.JPEG_SOI:
        return blob
    p = hc.jpeg_parse(blob)
    return image.encode_raw(hc.jpeg_decode(blob, scale or image.jpeg_auto_scale(p.h, p.w, 224, 224)))


@pytest.mark.parametrize("ensemble_step", [False, True])
def test_mixed_batch_of_scales_equals_the_batch_of_host_decoded_images(model, hc, ensemble_step):
    b01, f05, f03, t01 = _blob("b01"), _blob("f05"), _blob("f03"), _blob("t01")
    ppm = image.encode_ppm(np.random.default_rng(3).integers(0, 256, (97, 131, 3), dtype=np.uint8))
    # (blobs, parameters): automatic (b01 at 1/2, f05 at full size), 2, 8, none, a PPM under a scale, antialias
    batch = [([b01, f05], {"jpeg_scale": 0}), ([f03], {"jpeg_scale": 2}), ([b01], {"jpeg_scale": 8}), ([t01], {}),
             ([ppm], {"jpeg_scale": 4}), ([b01], {"jpeg_scale": 4, "antialias": True})]
    assert sum(len(b) for b, _ in batch) <= model.max_batch_size
    count = _count("jpeg_decode")
    got = model.execute([_request(b, ensemble_step, **p) for b, p in batch])
    assert count() == [6]  # the six JPEGs of every scale: one jpeg_decode call
    twins = [([_twin(hc, x, p.get("jpeg_scale", 1)) for x in b], {k: v for k, v in p.items() if k == "antialias"})
             for b, p in batch]
    want = model.execute([_request(b, ensemble_step, **p) for b, p in twins])
    for g, w in zip(got, want):
        np.testing.assert_array_equal(_rows(g), _rows(w))
    (alone,) = model.execute([_request(*batch[3][:1], ensemble_step)])
    np.testing.assert_array_equal(_rows(got[3]), _rows(alone))


def test_a_bad_jpeg_scale_fails_its_own_request(model):
    b01 = _blob("b01")
    res = model.execute([_request([b01], jpeg_scale=3), _request([b01], jpeg_scale=2)])
    assert isinstance(res[0], ValueError) and "jpeg_scale must be one of 0, 1, 2, 4, 8" in str(res[0])
    (ref,) = model.execute([_request([b01], jpeg_scale=2)])
    np.testing.assert_array_equal(res[1][0].data, ref[0].data)


def test_a_jpeg_past_the_staging_area_at_full_size_takes_the_device_route_at_scale_8(model, hc, monkeypatch):
    """b01 needs 921,984 + 921,600 bytes of a staging area at full size and
    29,184 + 14,400 at 1/8: with 100,000 bytes it is decoded by the host at
    scale 1 and by K22 at scale 8, as a 12-megapixel photo is with the real
    32 MiB."""
    b01 = _blob("b01")
    full, small = hc.jpeg_parse(b01), hc.jpeg_parse(b01, 8)
    monkeypatch.setattr(model, "STAGE_BYTES", 100000)
    assert full.coef_bytes + full.pixel_bytes > model.STAGE_BYTES > small.coef_bytes + small.pixel_bytes + 128
    got = {}
    for scale in (1, 8):
        count = _count("jpeg_decode")
        (outs,) = model.execute([_request([b01], jpeg_scale=scale)])
        assert count() == ([] if scale == 1 else [1])
        got[scale] = outs[0].data
    monkeypatch.undo()
    # the host route resizes in numpy, the device route with K20 like the TCIMG of the same pixels
    np.testing.assert_array_equal(got[1][0], image.inception_preprocess(hc.jpeg_decode(b01), 224, 224, "NCHW"))
    (ref,) = model.execute([_request([_twin(hc, b01, 8)])])
    np.testing.assert_array_equal(got[8][0], ref[0].data[0])


def test_with_the_device_huffman_knob_a_scaled_request_takes_the_host_entropy_decoder(hc, monkeypatch):
    from triton_client_amd.server.gpu_models import PreprocessInception

    monkeypatch.setenv("TCAMD_DEVICE_HUFFMAN", "1")
    m = PreprocessInception()
    m.load()
    try:
        assert m.device_huffman
        b01, f05 = _blob("b01"), _blob("f05")
        huff, k22 = _count("jpeg_huffman"), _count("jpeg_decode")
        got = m.execute([_request([b01, f05], jpeg_scale=4)])
        assert huff() == [] and k22() == [2]
        want = m.execute([_request([_twin(hc, b01, 4), _twin(hc, f05, 4)])])
        np.testing.assert_array_equal(_rows(got[0]), _rows(want[0]))
        huff = _count("jpeg_huffman")
        m.execute([_request([b01], jpeg_scale=2), _request([f05])])
        assert huff() == [1]  # the request without the parameter still takes K23
    finally:
        m.unload()


# -- served --------------------------------------------------------------------------------
def test_served_ensemble_with_automatic_scale_matches_the_tcimg_of_the_scaled_host_decode(gpu_server, hc):
    import tritonclient.grpc as grpcclient

    c = grpcclient.InferenceServerClient(gpu_server.grpc_url)
    pick = [_blob("b01"), _blob("f05")]
    res = []
    for blobs, kw in ((pick, {"parameters": {"jpeg_scale": 0}}), ([_twin(hc, b, 0) for b in pick], {})):
        inp = grpcclient.InferInput("INPUT", [len(blobs), 1], "BYTES")
        inp.set_data_from_numpy(np.array(blobs, dtype=np.object_).reshape(len(blobs), 1))
        res.append(c.infer("preprocess_inception_ensemble", [inp], **kw).as_numpy("OUTPUT"))
    with pytest.raises(Exception, match="jpeg_scale must be one of 0, 1, 2, 4, 8"):
        c.infer("preprocess_inception_ensemble", [inp], parameters={"jpeg_scale": 5})
    c.close()
    got, ref = res
    assert got.shape == (len(pick), 1000)
    # the tolerance of the served tests of tests/test_jpeg_gpu.py
    rel = np.linalg.norm(got - ref, axis=1) / np.linalg.norm(ref, axis=1)
    print("per-row rel-L2 jpeg_scale=0 vs TCIMG request %s" % rel)
    assert rel.max() < 1e-3, rel
    assert np.array_equal(got.argmax(axis=1), ref.argmax(axis=1))


# -- the client helper ---------------------------------------------------------------------
@pytest.mark.parametrize("scale", [0, 2, 8])
def test_preprocess_raw_batch_device_decodes_at_a_scale(hc, scale):
    arr = np.random.default_rng(9).integers(0, 256, (50, 70, 3), dtype=np.uint8)
    blobs = [_blob("b01"), _blob("f04"), _blob("f03")]
    p = [hc.jpeg_parse(b) for b in blobs]
    decoded = [hc.jpeg_decode(b, scale or image.jpeg_auto_scale(i.h, i.w, 224, 224)) for b, i in zip(blobs, p)]
    got = image.preprocess_raw_batch_device(blobs[:2] + [arr] + blobs[2:], 3, 224, 224, jpeg_scale=scale)
    want = image.preprocess_raw_batch_device(decoded[:2] + [arr] + decoded[2:], 3, 224, 224)
    assert got.shape == (4, 3, 224, 224)
    np.testing.assert_array_equal(got, want)

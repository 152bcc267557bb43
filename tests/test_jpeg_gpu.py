"""K22 jpeg_decode (csrc/kernels/jpeg.hip) against the host decoder
(csrc/host/jpeg.cc), bit for bit, and the JPEG route through the GPU
``preprocess_inception``, the served ensemble and ``preprocess_raw_batch_device``.
The host decoder itself is pinned to the numpy reference in test_jpeg_host.py."""

import numpy as np
import pytest

from tests import jpeg_cases as jc
from triton_client_amd.utils import image

pytestmark = pytest.mark.gpu

CANARY = 0xA5
GUARD = 64


@pytest.fixture(scope="module")
def cases():
    """Per decodable fixture: (entry, blob, parse, coefficient buffer, host pixels)."""
    from triton_client_amd.ops import host_codec

    hc = host_codec.load()
    out = []
    for e in jc.decodable():
        b = jc.blob(e)
        info = hc.jpeg_parse(b)
        coef = np.empty(info.coef_bytes, dtype=np.uint8)
        hc.jpeg_entropy_decode(b, coef)
        out.append((e, b, info, coef, hc.jpeg_decode(b)))
    return out


def _run(jobs, offsets):
    """Decode ``jobs`` [(info, coef, expected)] in one ``hip.jpeg_decode`` call,
    job k's destination ``offsets[k % len(offsets)]`` bytes past a 64-byte
    boundary and fenced by canaries; returns the pixels and checks the fences."""
    import torch

    from triton_client_amd.ops import hip

    dev = torch.device("cuda", 0)
    srcs, dsts, bufs = [], [], []
    for k, (info, coef, _) in enumerate(jobs):
        src = torch.from_numpy(coef).to(dev)
        off = offsets[k % len(offsets)]
        buf = torch.full((GUARD + off + info.pixel_bytes + GUARD,), CANARY, device=dev, dtype=torch.uint8)
        assert src.data_ptr() % 16 == 0 and buf.data_ptr() % 64 == 0
        srcs.append(src)
        bufs.append((buf, off))
        dsts.append(buf.data_ptr() + GUARD + off)
    hip.jpeg_decode([s.data_ptr() for s in srcs], [j[0] for j in jobs], dsts,
                    stream=torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    got = []
    for (info, _, _), (buf, off) in zip(jobs, bufs):
        a = buf.cpu().numpy()
        assert (a[:GUARD + off] == CANARY).all() and (a[GUARD + off + info.pixel_bytes:] == CANARY).all(), \
            "a byte outside the destination was written"
        got.append(a[GUARD + off:GUARD + off + info.pixel_bytes].reshape(info.shape))
    return got


# -- G1 -------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_every_fixture_alone_equals_the_host_decode(cases, offset):
    for e, _, info, coef, want in cases:
        if e["kind"] == "bench" and offset:
            continue  # the large image once; the small ones cover every offset
        (got,) = _run([(info, coef, want)], [offset])
        np.testing.assert_array_equal(got, want, err_msg=e["name"])


def test_all_fixtures_in_one_mixed_launch(cases):
    jobs = [(info, coef, want) for _, _, info, coef, want in cases]
    for (e, *_), got, (_, _, want) in zip(cases, _run(jobs, [0, 1, 2, 3]), jobs):
        np.testing.assert_array_equal(got, want, err_msg=e["name"])


def test_65_copies_take_a_second_launch(cases):
    _, _, info, coef, want = next(c for c in cases if c[0]["name"].startswith("f02"))
    for got in _run([(info, coef, want)] * 65, [3, 0, 1, 2]):
        np.testing.assert_array_equal(got, want)


# -- G2 -------------------------------------------------------------------------------
class _Info:
    def __init__(self, info, **kw):
        for f in ("h", "w", "ncomp", "hs", "vs"):
            setattr(self, f, kw.get(f, getattr(info, f)))


@pytest.mark.parametrize("what", ["sampling", "zero dimension", "misaligned coefficients", "null table",
                                  "component count", "dimension above the limit"])
def test_bad_arguments_are_refused_before_any_launch(cases, what):
    import torch

    from triton_client_amd.ops import hip

    _, _, info, coef, _ = next(c for c in cases if c[0]["name"].startswith("f02"))
    dev = torch.device("cuda", 0)
    src = torch.from_numpy(np.concatenate([coef, np.zeros(16, np.uint8)])).to(dev)
    dst = torch.full((GUARD + info.pixel_bytes + GUARD,), CANARY, device=dev, dtype=torch.uint8)
    sp, dp = src.data_ptr(), dst.data_ptr() + GUARD
    args = {
        "sampling": ([sp], [_Info(info, hs=1, vs=2)], [dp]),
        "zero dimension": ([sp], [_Info(info, h=0)], [dp]),
        "misaligned coefficients": ([sp + 8], [info], [dp]),
        "null table": ([0], [info], [dp]),
        "component count": ([sp], [_Info(info, ncomp=4)], [dp]),
        "dimension above the limit": ([sp], [_Info(info, w=hip.RESIZE_MAX_DIM + 1)], [dp]),
    }[what]
    with pytest.raises(hip.HipError) as err:
        hip.jpeg_decode(*args)
    assert err.value.code == 1  # hipErrorInvalidValue
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == CANARY).all()


# -- the GPU preprocess_inception ---------------------------------------------------------
def _request(blobs, ensemble_step=False, antialias=False):
    from triton_client_amd.server.types import InferRequest, InputTensor

    data = np.array(list(blobs), dtype=np.object_).reshape(len(blobs), 1)
    r = InferRequest(model_name="preprocess_inception", inputs=[InputTensor("INPUT", "BYTES", [len(blobs), 1], data)])
    if antialias:
        r.parameters["antialias"] = True
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
def model():
    from triton_client_amd.server.gpu_models import PreprocessInception

    m = PreprocessInception()
    m.load()
    yield m
    m.unload()


def _mixed_batch(cases):
    """JPEG, PPM and TCIMG blobs, and the same batch with every JPEG replaced
    by the TCIMG of its host decode."""
    rng = np.random.default_rng(3)
    pick = [c for c in cases if c[0]["name"][:3] in ("f03", "f04", "f05", "t01", "b01")]
    ppm = image.encode_ppm(rng.integers(0, 256, (97, 131, 3), dtype=np.uint8))
    raw = image.encode_raw(rng.integers(0, 256, (64, 48, 1), dtype=np.uint8))
    blobs = [pick[0][1], ppm, pick[1][1], raw, pick[2][1], pick[3][1], pick[4][1]]
    twins = [image.encode_raw(image.decode_image(b)) if b[:2] == b"\xff\xd8" else b for b in blobs]
    return blobs, twins


@pytest.mark.parametrize("antialias", [False, True])
@pytest.mark.parametrize("ensemble_step", [False, True])
def test_mixed_batch_equals_the_batch_of_decoded_images(model, cases, ensemble_step, antialias):
    blobs, twins = _mixed_batch(cases)
    launches = _count_launches(model)
    got = model.execute([_request(blobs[:4], ensemble_step, antialias), _request(blobs[4:], ensemble_step, antialias)])
    assert launches() == 1  # five JPEGs of two requests: one K22 launch
    want = model.execute([_request(twins[:4], ensemble_step, antialias), _request(twins[4:], ensemble_step, antialias)])
    for g, w in zip(got, want):
        np.testing.assert_array_equal(_rows(g), _rows(w))


def _count_launches(model):
    """Counts the ``hip.jpeg_decode`` calls and their images from here on."""
    from triton_client_amd.ops import hip

    real = hip.jpeg_decode
    calls = []

    def counted(srcs, *a, **kw):
        calls.append(len(srcs))
        return real(srcs, *a, **kw)

    mp = pytest.MonkeyPatch()
    mp.setattr(hip, "jpeg_decode", counted)

    def done():
        mp.undo()
        return sum(-(-n // 64) for n in calls)

    done.images = calls
    return done


def test_a_jpeg_past_the_staging_area_takes_the_host_route(model, cases, monkeypatch):
    first = next(c for c in cases if c[0]["name"].startswith("f03"))
    second = next(c for c in cases if c[0]["name"].startswith("f05"))
    need = -(-first[2].coef_bytes // 128) * 128 + first[2].pixel_bytes
    monkeypatch.setattr(model, "STAGE_BYTES", need + 100)  # the second JPEG's coefficients do not fit
    launches = _count_launches(model)
    (outs,) = model.execute([_request([first[1], second[1]])])
    assert launches() == 1 and launches.images == [1]  # the first image alone went through K22
    got = outs[0].data
    monkeypatch.undo()
    (ref,) = model.execute([_request([image.encode_raw(first[4])])])
    np.testing.assert_array_equal(got[0], ref[0].data[0])
    np.testing.assert_array_equal(got[1], image.inception_preprocess(second[4], 224, 224, "NCHW"))


def test_a_bad_jpeg_fails_its_own_request_with_the_cpu_models_error(model, cases):
    from triton_client_amd.server.cpu_models import PreprocessInception as HostModel

    good = next(c for c in cases if c[0]["name"].startswith("f03"))
    progressive = jc.blob(jc.fixtures("refused")[0])
    for bad in (good[1][:len(good[1]) // 2], progressive):
        with pytest.raises(Exception) as host_err:
            HostModel().execute([_request([bad])])
        assert isinstance(host_err.value, ValueError) and "JPEG" in str(host_err.value)
        res = model.execute([_request([bad]), _request([good[1]])])
        assert type(res[0]) is type(host_err.value) and str(res[0]) == str(host_err.value)
        (ref,) = model.execute([_request([image.encode_raw(good[4])])])
        np.testing.assert_array_equal(res[1][0].data, ref[0].data)


# -- served ---------------------------------------------------------------------------
@pytest.mark.parametrize("antialias", [False, True])
@pytest.mark.parametrize("proto", ["http", "grpc"])
def test_served_ensemble_on_jpeg_matches_the_tcimg_of_its_host_decode(gpu_server, cases, proto, antialias):
    import tritonclient.grpc as grpcclient
    import tritonclient.http as httpclient

    mod = grpcclient if proto == "grpc" else httpclient
    c = mod.InferenceServerClient(gpu_server.grpc_url if proto == "grpc" else gpu_server.http_url)
    pick = [x for x in cases if x[0]["name"][:3] in ("f03", "f05", "b01")]
    res = []
    for blobs in ([x[1] for x in pick], [image.encode_raw(x[4]) for x in pick]):
        inp = mod.InferInput("INPUT", [len(blobs), 1], "BYTES")
        inp.set_data_from_numpy(np.array(blobs, dtype=np.object_).reshape(len(blobs), 1))
        kw = {"parameters": {"antialias": True}} if antialias else {}
        res.append(c.infer("preprocess_inception_ensemble", [inp], **kw).as_numpy("OUTPUT"))
    c.close()
    got, ref = res
    assert got.shape == (len(pick), 1000)
    # the tolerance of the served tests of tests/test_preprocess_device_gpu.py
    rel = np.linalg.norm(got - ref, axis=1) / np.linalg.norm(ref, axis=1)
    print("%s antialias=%s: per-row rel-L2 JPEG vs TCIMG request %s" % (proto, antialias, rel))
    assert rel.max() < 1e-3, rel
    assert np.array_equal(got.argmax(axis=1), ref.argmax(axis=1))


# -- the client helper ---------------------------------------------------------------------
@pytest.mark.parametrize("antialias", [False, True])
def test_preprocess_raw_batch_device_takes_jpeg_bytes_among_arrays(cases, antialias):
    rng = np.random.default_rng(9)
    arr = rng.integers(0, 256, (50, 70, 3), dtype=np.uint8)
    grey = rng.integers(0, 256, (31, 17), dtype=np.uint8)
    pick = [c for c in cases if c[0]["name"][:3] in ("f02", "f04", "t04")]
    mixed = [pick[0][1], arr, pick[1][1], grey, pick[2][1]]
    decoded = [pick[0][4], arr, pick[1][4], grey, pick[2][4]]
    got = image.preprocess_raw_batch_device(mixed, 3, 224, 224, antialias=antialias)
    want = image.preprocess_raw_batch_device(decoded, 3, 224, 224, antialias=antialias)
    assert got.shape == (5, 3, 224, 224)
    np.testing.assert_array_equal(got, want)

"""K23 jpeg_huffman (csrc/kernels/jpeg_huff.hip) against the host entropy
decoder (csrc/host/jpeg.cc), byte for byte, and the device Huffman route
(``TCAMD_DEVICE_HUFFMAN=1``) through the GPU ``preprocess_inception``.  The
algorithm itself, the pack and untrusted bytes are covered without a GPU in
tests/test_jpeg_huffman.py and csrc/cpp/tests/jpeg_stream_test.cc; the only
corrupted streams a GPU sees are the three of G5, which the emulation rejects
in bounds."""

import numpy as np
import pytest

from tests import jpeg_huff_cases as jh
from triton_client_amd.utils import image

pytestmark = pytest.mark.gpu

CANARY = 0xA5
GUARD = 64
# single-byte corruptions of f05's scan data from csrc/cpp/tests/jpeg_stream_test.cc: the markers
# are intact (packable), the Huffman data is broken (the emulation's status is not 0)
BROKEN_F05 = ((818, 0x87), (771, 0x33), (716, 0x6A))


@pytest.fixture(scope="module")
def cases():
    """Per decodable fixture: (name, blob, parse, stream buffer, host coefficients, host pixels)."""
    from triton_client_amd.ops import host_codec

    hc = host_codec.load()
    out = []
    for name, b in jh.decodable():
        buf = host_codec.aligned_buffer(hc.jpeg_stream_bound(len(b)))
        info, used = hc.jpeg_stream_pack(b, buf)
        assert used is not None, name  # no fallback on a fixture
        coef = np.empty(info.coef_bytes, dtype=np.uint8)
        hc.jpeg_entropy_decode(b, coef)
        out.append((name, b, info, buf[:used].copy(), coef, hc.jpeg_decode(b)))
    return out


def _huffman(jobs):
    """``jobs`` [(stream buffer, parse)] through one ``hip.jpeg_huffman`` call,
    every coefficient buffer fenced by canaries; returns (the device tensors
    holding the coefficient buffers, their offsets, the status words)."""
    import torch

    from triton_client_amd.ops import hip

    dev = torch.device("cuda", 0)
    streams, bufs = [], []
    for stream, info in jobs:
        streams.append(torch.from_numpy(stream).to(dev))
        bufs.append(torch.full((GUARD + info.coef_bytes + GUARD,), CANARY, device=dev, dtype=torch.uint8))
        assert streams[-1].data_ptr() % 16 == 0 and bufs[-1].data_ptr() % 64 == 0
    status = torch.full((GUARD // 4 + len(jobs) + GUARD // 4,), 0x5A5A5A5A, device=dev, dtype=torch.int32)
    hip.jpeg_huffman([s.data_ptr() for s in streams], [b.data_ptr() + GUARD for b in bufs],
                     status.data_ptr() + GUARD, stream=torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    st = status.cpu().numpy()
    assert (st[:GUARD // 4] == 0x5A5A5A5A).all() and (st[GUARD // 4 + len(jobs):] == 0x5A5A5A5A).all()
    coefs = []
    for (_, info), buf in zip(jobs, bufs):
        a = buf.cpu().numpy()
        assert (a[:GUARD] == CANARY).all() and (a[GUARD + info.coef_bytes:] == CANARY).all(), \
            "a byte outside the coefficient buffer was written"
        coefs.append(a[GUARD:GUARD + info.coef_bytes])
    return bufs, coefs, st[GUARD // 4:GUARD // 4 + len(jobs)]


# -- G1 -------------------------------------------------------------------------------
def test_every_fixture_alone_equals_the_host_entropy_decode(cases):
    for name, _, info, stream, want, _ in cases:
        _, (got,), status = _huffman([(stream, info)])
        assert status[0] == 0, name  # no fallback on a fixture
        np.testing.assert_array_equal(got, want, err_msg=name)


# -- G2 -------------------------------------------------------------------------------
def test_all_fixtures_in_one_launch(cases):
    _, coefs, status = _huffman([(c[3], c[2]) for c in cases])
    assert (status == 0).all()
    for c, got in zip(cases, coefs):
        np.testing.assert_array_equal(got, c[4], err_msg=c[0])


def test_65_copies_take_a_second_launch(cases):
    _, _, info, stream, want, _ = next(c for c in cases if c[0].startswith("f01"))
    _, coefs, status = _huffman([(stream, info)] * 65)
    assert (status == 0).all()
    for got in coefs:
        np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("what", ["misaligned stream", "misaligned coefficients", "null stream", "null status"])
def test_bad_arguments_are_refused_before_any_launch(cases, what):
    import torch

    from triton_client_amd.ops import hip

    _, _, info, stream, _, _ = next(c for c in cases if c[0].startswith("f01"))
    dev = torch.device("cuda", 0)
    src = torch.from_numpy(np.concatenate([stream, np.zeros(16, np.uint8)])).to(dev)
    dst = torch.full((GUARD + info.coef_bytes + GUARD,), CANARY, device=dev, dtype=torch.uint8)
    status = torch.zeros(4, device=dev, dtype=torch.int32)
    sp, dp, tp = src.data_ptr(), dst.data_ptr() + GUARD, status.data_ptr()
    args = {
        "misaligned stream": ([sp + 8], [dp], tp),
        "misaligned coefficients": ([sp], [dp + 8], tp),
        "null stream": ([0], [dp], tp),
        "null status": ([sp], [dp], 0),
    }[what]
    with pytest.raises(hip.HipError) as err:
        hip.jpeg_huffman(*args)
    assert err.value.code == 1  # hipErrorInvalidValue
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == CANARY).all()


# -- G3 -------------------------------------------------------------------------------
def test_k23_then_k22_equals_the_host_pixels(cases):
    import torch

    from triton_client_amd.ops import hip

    bufs, _, status = _huffman([(c[3], c[2]) for c in cases])
    assert (status == 0).all()
    dev = bufs[0].device
    outs = [torch.empty(c[2].pixel_bytes, device=dev, dtype=torch.uint8) for c in cases]
    hip.jpeg_decode([b.data_ptr() + GUARD for b in bufs], [c[2] for c in cases], [o.data_ptr() for o in outs],
                    stream=torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    for c, o in zip(cases, outs):
        np.testing.assert_array_equal(o.cpu().numpy().reshape(c[2].shape), c[5], err_msg=c[0])


# -- the GPU preprocess_inception ---------------------------------------------------------
def _request(blobs, antialias=False):
    from triton_client_amd.server.types import InferRequest, InputTensor

    data = np.array(list(blobs), dtype=np.object_).reshape(len(blobs), 1)
    r = InferRequest(model_name="preprocess_inception", inputs=[InputTensor("INPUT", "BYTES", [len(blobs), 1], data)])
    if antialias:
        r.parameters["antialias"] = True
    return r


@pytest.fixture(scope="module")
def models():
    """``PreprocessInception`` loaded with TCAMD_DEVICE_HUFFMAN=0 and =1."""
    from triton_client_amd.server.gpu_models import PreprocessInception

    mp = pytest.MonkeyPatch()
    out = {}
    for knob in ("0", "1"):
        mp.setenv("TCAMD_DEVICE_HUFFMAN", knob)
        out[knob] = PreprocessInception()
        out[knob].load()
    mp.undo()
    assert not out["0"].device_huffman and out["1"].device_huffman
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


# -- G4 -------------------------------------------------------------------------------
@pytest.mark.parametrize("antialias", [False, True])
def test_the_knob_changes_the_route_and_not_one_bit_of_the_rows(models, cases, antialias, monkeypatch):
    rng = np.random.default_rng(4)
    pick = {c[0][:3]: c[1] for c in cases}
    raw = image.encode_raw(rng.integers(0, 256, (64, 48, 1), dtype=np.uint8))
    ppm = image.encode_ppm(rng.integers(0, 256, (97, 131, 3), dtype=np.uint8))
    batches = [[pick["f05"], raw, pick["h05"], pick["f11"]], [pick["b01"], ppm, pick["h02"], pick["h01"]]]
    rows = {}
    for knob, model in models.items():
        huffman = _count(monkeypatch, "jpeg_huffman")
        rows[knob] = model.execute([_request(b, antialias) for b in batches])
        assert huffman == ([6] if knob == "1" else [])  # the six JPEGs of two requests: one K23 launch, or none
        monkeypatch.undo()
    for got, want in zip(rows["1"], rows["0"]):
        np.testing.assert_array_equal(got[0].data, want[0].data)


# -- the client helper ---------------------------------------------------------------------
def test_preprocess_raw_batch_device_with_the_device_huffman_route(cases, monkeypatch):
    pick = {c[0][:3]: c[1] for c in cases}
    arr = np.random.default_rng(9).integers(0, 256, (50, 70, 3), dtype=np.uint8)
    m = bytearray(pick["f05"])
    m[BROKEN_F05[0][0]] = BROKEN_F05[0][1]
    mixed = [pick["f05"], arr, pick["h03"], pick["f11"]]
    want = image.preprocess_raw_batch_device(mixed, 3, 224, 224, device_huffman=False)
    huffman = _count(monkeypatch, "jpeg_huffman")
    np.testing.assert_array_equal(image.preprocess_raw_batch_device(mixed, 3, 224, 224, device_huffman=True), want)
    monkeypatch.setenv("TCAMD_DEVICE_HUFFMAN", "1")
    np.testing.assert_array_equal(image.preprocess_raw_batch_device(mixed, 3, 224, 224), want)
    assert huffman == [3, 3]
    # broken Huffman data: K23's status sends the batch to the host decoder, which raises its error
    with pytest.raises(ValueError) as host_err:
        image.preprocess_raw_batch_device([bytes(m)], 3, 224, 224, device_huffman=False)
    with pytest.raises(ValueError) as err:
        image.preprocess_raw_batch_device([pick["f03"], bytes(m)], 3, 224, 224, device_huffman=True)
    assert str(err.value) == str(host_err.value) and huffman == [3, 3, 2]


# -- G5 -------------------------------------------------------------------------------
def test_broken_huffman_data_fails_its_own_request_with_the_hosts_message(models, cases, monkeypatch):
    from triton_client_amd.ops import host_codec

    hc = host_codec.load()
    f05 = next(c[1] for c in cases if c[0].startswith("f05"))
    good = [c for c in cases if c[0][:3] in ("f03", "h05")]
    broken, messages = [], []
    for at, value in BROKEN_F05:
        m = bytearray(f05)
        m[at] = value
        m = bytes(m)
        buf = host_codec.aligned_buffer(hc.jpeg_stream_bound(len(m)))
        info, used = hc.jpeg_stream_pack(m, buf)
        assert used is not None  # the markers are intact
        assert hc.jpeg_huffman_emulate(buf[:used], np.empty(info.coef_bytes, dtype=np.uint8))[0] != 0
        with pytest.raises(ValueError) as err:
            hc.jpeg_decode(m)
        broken.append(m)
        messages.append(str(err.value))
    model = models["1"]
    seen = []
    real = model._read_status

    def spy(*a, **kw):
        seen.append(real(*a, **kw))
        return seen[-1]

    monkeypatch.setattr(model, "_read_status", spy)
    requests = [_request([good[0][1]]), _request([broken[0]]), _request([good[1][1], broken[1]]),
                _request([broken[2]]), _request([good[0][1], good[1][1]])]
    res = model.execute(requests)
    # the status words, in the order of the batch's JPEGs: non-zero for exactly the broken ones
    (status,) = seen
    assert [int(s != 0) for s in status] == [0, 1, 0, 1, 1, 0, 0]
    for k, msg in ((1, messages[0]), (2, messages[1]), (3, messages[2])):
        assert isinstance(res[k], ValueError) and str(res[k]) == msg
    ref = models["0"].execute([_request([good[0][1]]), _request([good[0][1], good[1][1]])])
    np.testing.assert_array_equal(res[0][0].data, ref[0][0].data)
    np.testing.assert_array_equal(res[4][0].data, ref[1][0].data)

"""The K24 jpeg_huffman_wide kernels (csrc/kernels/jpeg_huff_wide.hip) against
the host entropy decoder (csrc/host/jpeg.cc) at every scale, byte for byte, and
the wide device Huffman route (``TCAMD_DEVICE_HUFFMAN_WIDE``) through the GPU
``preprocess_inception``.  The launch sequence itself, the wide pack and
untrusted bytes are covered without a GPU in tests/test_jpeg_huffman_wide.py
and csrc/cpp/tests/jpeg_wide_test.cc; the only corrupted streams a GPU sees are
the three of ``BROKEN_F05``, which the emulation rejects in bounds."""

import os

import numpy as np
import pytest

from tests import jpeg_huff_cases as jh
from tests.test_jpeg_huffman import _one_block_intervals
from triton_client_amd.utils import image

pytestmark = pytest.mark.gpu

CANARY = 0xA5
GUARD = 64
SCALES = (1, 2, 4, 8)
# tests/test_jpeg_huffman_gpu.py: f05 with its markers intact and its Huffman data broken
BROKEN_F05 = ((818, 0x87), (771, 0x33), (716, 0x6A))
W01 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_wide", "w01_640x480_420_q95_noise.jpg")


def _w01():
    with open(W01, "rb") as f:
        return f.read()


def _small(name):
    """The small chunk of a fixture: f11, the near-serial one, in chunks of two."""
    return 2 if name.startswith("f11") else 8


class Case:
    def __init__(self, hc, name, blob, scale, decodable=True):
        from triton_client_amd.ops import host_codec

        self.name, self.blob, self.scale = name, blob, scale
        buf = host_codec.aligned_buffer(hc.jpeg_stream_bound_wide(len(blob)))
        self.info, used, self.nsub = hc.jpeg_stream_pack_wide(blob, buf, scale)
        assert used is not None, name  # no fallback on a fixture
        self.stream = buf[:used].copy()
        self.want = np.empty(self.info.coef_bytes, dtype=np.uint8) if decodable else None
        if decodable:
            hc.jpeg_entropy_decode(blob, self.want, scale)


@pytest.fixture(scope="module")
def hc():
    from triton_client_amd.ops import host_codec

    return host_codec.load()


@pytest.fixture(scope="module")
def cases(hc):
    """{scale: [Case of every decodable fixture and of w01]}, packed and host-decoded once."""
    blobs = jh.decodable() + [("w01_640x480_420_q95_noise", _w01())]
    return {s: [Case(hc, n, b, s) for n, b in blobs] for s in SCALES}


def _wide(jobs, chunk_subs=0):
    """``jobs`` (Cases) through one ``hip.jpeg_huffman_wide`` call, every
    coefficient buffer, the status words and the workspace fenced by canaries;
    returns (the device tensors holding the coefficient buffers, the
    coefficient bytes, the status words)."""
    import torch

    from triton_client_amd.ops import hip

    dev = torch.device("cuda", 0)
    streams = [torch.from_numpy(j.stream).to(dev) for j in jobs]
    bufs = [torch.full((GUARD + j.info.coef_bytes + GUARD,), CANARY, device=dev, dtype=torch.uint8) for j in jobs]
    assert all(s.data_ptr() % 16 == 0 for s in streams) and all(b.data_ptr() % 64 == 0 for b in bufs)
    status = torch.full((GUARD // 4 + len(jobs) + GUARD // 4,), 0x5A5A5A5A, device=dev, dtype=torch.int32)
    nsubs = [j.nsub for j in jobs]
    need = hip.jpeg_huffman_wide_workspace(nsubs, chunk_subs)
    ws = torch.full((GUARD + need + GUARD,), CANARY, device=dev, dtype=torch.uint8)
    hip.jpeg_huffman_wide([s.data_ptr() for s in streams], [b.data_ptr() + GUARD for b in bufs], nsubs,
                          status.data_ptr() + GUARD, ws.data_ptr() + GUARD, need, chunk_subs,
                          stream=torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    st = status.cpu().numpy()
    assert (st[:GUARD // 4] == 0x5A5A5A5A).all() and (st[GUARD // 4 + len(jobs):] == 0x5A5A5A5A).all()
    w = ws.cpu().numpy()
    assert (w[:GUARD] == CANARY).all() and (w[GUARD + need:] == CANARY).all(), "a byte outside the workspace was written"
    coefs = []
    for j, buf in zip(jobs, bufs):
        a = buf.cpu().numpy()
        assert (a[:GUARD] == CANARY).all() and (a[GUARD + j.info.coef_bytes:] == CANARY).all(), \
            "a byte outside the coefficient buffer was written"
        coefs.append(a[GUARD:GUARD + j.info.coef_bytes])
    return bufs, coefs, st[GUARD // 4:GUARD // 4 + len(jobs)]


@pytest.mark.parametrize("scale", SCALES)
def test_every_fixture_alone_equals_the_host_entropy_decode(cases, scale):
    for c in cases[scale]:
        for cs in (0, _small(c.name)):
            _, (got,), status = _wide([c], cs)
            assert status[0] == 0, (c.name, cs)  # no fallback on a fixture
            np.testing.assert_array_equal(got, c.want, err_msg="%s chunk_subs %d" % (c.name, cs))


def test_w01_is_what_it_is_for(cases, hc):
    from triton_client_amd.ops import hip, host_codec

    for nsubs in ([1], [1024], [1025, 1], [2808] * 3, [2048] * 64):  # the host library sizes the same workspace
        assert hc.jpeg_huffman_wide_workspace(nsubs) == hip.jpeg_huffman_wide_workspace(nsubs), nsubs
    w01 = cases[1][-1]
    assert w01.nsub > jh.MAX_SUB and -(-w01.nsub // 1024) == 3  # three chunks at the default
    assert int(w01.stream[:64].view("<u4")[10]) == 1  # one segment
    assert hc.jpeg_stream_pack(w01.blob, host_codec.aligned_buffer(hc.jpeg_stream_bound(len(w01.blob))))[1] is None


@pytest.mark.parametrize("chunk_subs", [0, 8])
def test_all_fixtures_in_one_call_with_mixed_scales(cases, chunk_subs):
    n = len(cases[1])
    jobs = [cases[SCALES[(i + k) % 4]][i] for k in range(2) for i in range(n)]
    _, coefs, status = _wide(jobs, chunk_subs)
    assert (status == 0).all()
    for j, got in zip(jobs, coefs):
        np.testing.assert_array_equal(got, j.want, err_msg="%s 1/%d" % (j.name, j.scale))


def test_65_copies_take_a_second_launch_sequence(cases):
    f01 = next(c for c in cases[2] if c.name.startswith("f01"))
    w01 = cases[8][-1]
    jobs = [f01] * 63 + [w01] + [f01] * 2  # the second sequence reuses the workspace of the first
    _, coefs, status = _wide(jobs)
    assert (status == 0).all()
    for j, got in zip(jobs, coefs):
        np.testing.assert_array_equal(got, j.want)


@pytest.mark.parametrize("scale", SCALES)
def test_k24_then_k22_equals_the_host_pixels(cases, hc, scale):
    import torch

    from triton_client_amd.ops import hip

    jobs = cases[scale]
    bufs, _, status = _wide(jobs)
    assert (status == 0).all()
    dev = bufs[0].device
    outs = [torch.empty(j.info.pixel_bytes, device=dev, dtype=torch.uint8) for j in jobs]
    hip.jpeg_decode([b.data_ptr() + GUARD for b in bufs], [j.info for j in jobs], [o.data_ptr() for o in outs],
                    stream=torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    for j, o in zip(jobs, outs):
        np.testing.assert_array_equal(o.cpu().numpy().reshape(j.info.shape), hc.jpeg_decode(j.blob, scale),
                                      err_msg=j.name)


@pytest.mark.parametrize("chunk_subs", [0, 8])
def test_one_block_intervals_above_k23s_workspace(hc, chunk_subs):
    """2,050 segments of one subsequence each, two more than K23 holds: three
    chunks at the default, 257 at 8."""
    c = Case(hc, "one block intervals", _one_block_intervals(jh.MAX_SUB // 2 + 1), 1)
    assert c.nsub == jh.MAX_SUB + 2
    _, (got,), status = _wide([c], chunk_subs)
    assert status[0] == 0
    np.testing.assert_array_equal(got, c.want)


BAD_ARGUMENTS = ["misaligned stream", "misaligned coefficients", "null stream", "null status", "null workspace",
                 "misaligned workspace", "short workspace", "chunk_subs 3", "chunk_subs 2048", "no subsequences"]


@pytest.mark.parametrize("what", BAD_ARGUMENTS)
def test_bad_arguments_are_refused_before_any_launch(cases, what):
    import torch

    from triton_client_amd.ops import hip

    c = next(c for c in cases[1] if c.name.startswith("f01"))
    dev = torch.device("cuda", 0)
    src = torch.from_numpy(np.concatenate([c.stream, np.zeros(16, np.uint8)])).to(dev)
    dst = torch.full((GUARD + c.info.coef_bytes + GUARD,), CANARY, device=dev, dtype=torch.uint8)
    status = torch.full((4,), 0x5A5A5A5A, device=dev, dtype=torch.int32)
    need = hip.jpeg_huffman_wide_workspace([c.nsub])
    ws = torch.full((need + 64,), CANARY, device=dev, dtype=torch.uint8)
    sp, dp, tp, wp = src.data_ptr(), dst.data_ptr() + GUARD, status.data_ptr(), ws.data_ptr()
    good = dict(streams=[sp], coefs=[dp], nsubs=[c.nsub], status=tp, workspace=wp, workspace_bytes=need, chunk_subs=0)
    change = {
        "misaligned stream": dict(streams=[sp + 8]),
        "misaligned coefficients": dict(coefs=[dp + 8]),
        "null stream": dict(streams=[0]),
        "null status": dict(status=0),
        "null workspace": dict(workspace=0),
        "misaligned workspace": dict(workspace=wp + 8),
        "short workspace": dict(workspace_bytes=need - 1),
        "chunk_subs 3": dict(chunk_subs=3),
        "chunk_subs 2048": dict(chunk_subs=2048),
        "no subsequences": dict(nsubs=[0]),
    }[what]
    with pytest.raises(hip.HipError) as err:
        hip.jpeg_huffman_wide(**dict(good, **change))
    assert err.value.code == 1  # hipErrorInvalidValue
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == CANARY).all() and (ws.cpu().numpy() == CANARY).all()
    assert (status.cpu().numpy() == 0x5A5A5A5A).all()


def _broken(hc, scale=1):
    """The three corruptions of f05 as Cases (the host decode of each raises), and the host's messages."""
    f05 = jh.blob("f05")
    out, messages = [], []
    for at, value in BROKEN_F05:
        m = bytearray(f05)
        m[at] = value
        m = bytes(m)
        with pytest.raises(ValueError) as err:
            hc.jpeg_decode(m, scale)
        messages.append(str(err.value))
        c = Case(hc, "broken f05", m, scale, decodable=False)  # packable: the markers are intact
        assert hc.jpeg_huffman_wide_emulate(c.stream, np.empty(c.info.coef_bytes, dtype=np.uint8), 2)[0] != 0
        out.append(c)
    return out, messages


@pytest.mark.parametrize("scale,chunk_subs", [(1, 0), (2, 2)])
def test_broken_huffman_data_ends_in_the_status_word_and_in_bounds(cases, hc, scale, chunk_subs):
    broken, _ = _broken(hc, scale)
    good = next(c for c in cases[scale] if c.name.startswith("f03"))
    _, coefs, status = _wide([good] + broken + [good], chunk_subs)  # the canaries are checked in _wide
    assert [int(s != 0) for s in status] == [0, 1, 1, 1, 0]
    np.testing.assert_array_equal(coefs[0], good.want)
    np.testing.assert_array_equal(coefs[4], good.want)


# -- the GPU preprocess_inception ---------------------------------------------------------
def _request(blobs, **params):
    from triton_client_amd.server.types import InferRequest, InputTensor

    data = np.array(list(blobs), dtype=np.object_).reshape(len(blobs), 1)
    r = InferRequest(model_name="preprocess_inception", inputs=[InputTensor("INPUT", "BYTES", [len(blobs), 1], data)])
    r.parameters.update(params)
    return r


# (TCAMD_DEVICE_HUFFMAN, TCAMD_DEVICE_HUFFMAN_WIDE)
KNOBS = (("0", "0"), ("0", "1"), ("1", "0"), ("1", "1"), ("0", "300000"), ("0", "400000"))


@pytest.fixture(scope="module")
def models():
    """``PreprocessInception`` loaded under every pair of ``KNOBS``."""
    from triton_client_amd.server.gpu_models import PreprocessInception

    mp = pytest.MonkeyPatch()
    out = {}
    for k23, k24 in KNOBS:
        mp.setenv("TCAMD_DEVICE_HUFFMAN", k23)
        mp.setenv("TCAMD_DEVICE_HUFFMAN_WIDE", k24)
        out[(k23, k24)] = PreprocessInception()
        out[(k23, k24)].load()
        assert out[(k23, k24)].device_huffman == (k23 == "1") and out[(k23, k24)].device_huffman_wide == int(k24)
    mp.undo()
    yield out
    for m in out.values():
        m.unload()


def _count(mp, obj, name):
    real = getattr(obj, name)
    calls = []

    def counted(first, *a, **kw):
        calls.append(len(first))
        return real(first, *a, **kw)

    mp.setattr(obj, name, counted)
    return calls


def test_the_wide_knob_changes_the_route_and_not_one_bit_of_the_rows(models, cases, hc, monkeypatch):
    from triton_client_amd.ops import hip

    rng = np.random.default_rng(24)
    pick = {c.name[:3]: c.blob for c in cases[1]}
    assert 300000 <= len(pick["w01"]) < 400000 and max(len(b) for n, b in pick.items() if n != "w01") < 300000
    raw = image.encode_raw(rng.integers(0, 256, (64, 48, 1), dtype=np.uint8))
    ppm = image.encode_ppm(rng.integers(0, 256, (97, 131, 3), dtype=np.uint8))

    def batch():
        return [_request([pick["f05"], raw, pick["h05"], pick["f11"]]),
                _request([pick["b01"], ppm, pick["w01"], pick["h01"]]),
                _request([pick["b01"], pick["w01"], pick["h02"]], jpeg_scale=2, antialias=True),
                _request([pick["w01"], ppm, pick["f03"]], jpeg_scale=8),
                _request([pick["b01"]], jpeg_scale=0)]

    # 12 JPEGs: 6 at full size, of which K23's pack declines w01; 3 at 1/2, 2 at 1/8, b01 at the automatic scale
    want = {  # calls of hip.jpeg_huffman, hip.jpeg_huffman_wide, and host entropy decodes
        ("0", "0"): ([], [], 12),
        ("0", "1"): ([], [12], 0),  # every JPEG, scaled ones included, in one wide call
        ("1", "0"): ([5], [], 7),  # K23 keeps its share; a scaled request makes no K23 call
        ("1", "1"): ([5], [7], 0),
        ("0", "300000"): ([], [3], 9),  # only the three w01
        ("0", "400000"): ([], [], 12),  # no blob of the batch is that large
    }
    rows = {}
    for knobs, model in models.items():
        huffman = _count(monkeypatch, hip, "jpeg_huffman")
        wide = _count(monkeypatch, hip, "jpeg_huffman_wide")
        host = _count(monkeypatch, hc, "jpeg_entropy_decode")
        rows[knobs] = model.execute(batch())
        assert (huffman, wide, len(host)) == want[knobs], knobs
        monkeypatch.undo()
    for knobs, res in rows.items():
        for got, ref in zip(res, rows[("0", "0")]):
            np.testing.assert_array_equal(got[0].data, ref[0].data, err_msg=str(knobs))


def test_broken_huffman_data_fails_its_own_request_with_the_hosts_message(models, cases, hc, monkeypatch):
    good = [c for c in cases[1] if c.name[:3] in ("f03", "h05")]
    for scale in (1, 2):
        broken, messages = _broken(hc, scale)
        model = models[("0", "1")]
        seen = []
        real = model._read_status

        def spy(*a, **kw):
            seen.append(real(*a, **kw))
            return seen[-1]

        monkeypatch.setattr(model, "_read_status", spy)
        params = {} if scale == 1 else {"jpeg_scale": scale}
        requests = [_request([good[0].blob], **params), _request([broken[0].blob], **params),
                    _request([good[1].blob, broken[1].blob], **params), _request([broken[2].blob], **params),
                    _request([good[0].blob, good[1].blob], **params)]
        res = model.execute(requests)
        (status,) = seen  # the status words, in the order of the batch's JPEGs
        assert [int(s != 0) for s in status] == [0, 1, 0, 1, 1, 0, 0]
        for k, msg in ((1, messages[0]), (2, messages[1]), (3, messages[2])):
            assert isinstance(res[k], ValueError) and str(res[k]) == msg
        ref = models[("0", "0")].execute([_request([good[0].blob], **params),
                                          _request([good[0].blob, good[1].blob], **params)])
        np.testing.assert_array_equal(res[0][0].data, ref[0][0].data)
        np.testing.assert_array_equal(res[4][0].data, ref[1][0].data)
        monkeypatch.undo()


# -- the client helper ---------------------------------------------------------------------
def test_preprocess_raw_batch_device_with_the_wide_route(cases, hc, monkeypatch):
    from triton_client_amd.ops import hip

    pick = {c.name[:3]: c.blob for c in cases[1]}
    arr = np.random.default_rng(9).integers(0, 256, (50, 70, 3), dtype=np.uint8)
    mixed = [pick["f05"], arr, pick["w01"], pick["f11"]]
    huffman = _count(monkeypatch, hip, "jpeg_huffman")
    wide = _count(monkeypatch, hip, "jpeg_huffman_wide")
    for scale in (1, 4, 0):
        want = image.preprocess_raw_batch_device(mixed, 3, 224, 224, device_huffman=False, jpeg_scale=scale,
                                                 device_huffman_wide=0)
        assert (huffman, wide) == ([], [])
        got = image.preprocess_raw_batch_device(mixed, 3, 224, 224, jpeg_scale=scale, device_huffman_wide=1)
        np.testing.assert_array_equal(got, want)
        assert (huffman, wide) == ([], [3])
        del wide[:]
    monkeypatch.setenv("TCAMD_DEVICE_HUFFMAN_WIDE", "300000")
    got = image.preprocess_raw_batch_device(mixed, 3, 224, 224, device_huffman=True)
    np.testing.assert_array_equal(got, image.preprocess_raw_batch_device(mixed, 3, 224, 224, device_huffman=False,
                                                                         device_huffman_wide=0))
    assert (huffman, wide) == ([2], [1])  # K23 keeps f05 and f11; w01, which it declines, goes wide
    # broken Huffman data: K24's status sends the batch to the host decoder, which raises its error
    (m, _, _), (message, _, _) = _broken(hc, 1)
    with pytest.raises(ValueError) as err:
        image.preprocess_raw_batch_device([pick["f03"], m.blob], 3, 224, 224, device_huffman=False,
                                          device_huffman_wide=1)
    assert str(err.value) == message

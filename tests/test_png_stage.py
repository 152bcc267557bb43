"""The PNG route and its part of the staging layout
(triton_client_amd/utils/jpeg_stage.py: ``StagePlan.add_png``, ``PngJob``,
``launch_decode``) without a GPU: a batch is planned over a host buffer, the
plan is executed by the host twin of K25 (``HostCodec.png_unfilter``), and the
offsets are checked against the documented contract.  The same plans run on the
device in tests/test_png_gpu.py."""

import glob
import os

import numpy as np
import pytest

from tests import png_cases as pc
from triton_client_amd.ops import host_codec
from triton_client_amd.utils import jpeg_stage

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MAX_DIM = 16384
RGB = pc.make(2, 8, 9, 13, pc.CYCLE)
PAL = pc.make(3, 4, 7, 9, pc.CYCLE, palette_entries=5)
TALL = pc.make(0, 8, 259, 5, (2, 1))  # more rows than a pass of K25: a scratch scanline
LACED = pc.make(2, 8, 9, 13, pc.CYCLE, adam7=True)


@pytest.fixture(scope="module")
def hc():
    return host_codec.load()


def _jpeg(prefix):
    (path,) = glob.glob(os.path.join(GOLDEN, "jpeg*", prefix + "_*.jpg"))
    with open(path, "rb") as f:
        return f.read()


def _plan(hc, capacity, codec=None, **knobs):
    return jpeg_stage.StagePlan(host_codec.aligned_buffer(capacity), codec or hc, knobs.get("huffman", False),
                                knobs.get("huffman_wide", 0), MAX_DIM)


def _key(job):
    """A PngJob with its parse by value."""
    return job._replace(info=bytes(job.info))


def check_png_layout(plan):
    """What the module's docstring promises of the PNGs of a plan, and that nothing in the plan overlaps."""
    host, device = [], []
    for j in plan.pngs:
        assert j.stream % 16 == 0
        assert j.info.palette_off % 16 == 0 and j.info.line_off % 16 == 0
        host.append((j.stream, j.stream + j.info.stage_bytes, "staged PNG"))
        device.append((j.pix, j.pix + j.info.pixel_bytes, "PNG pixels"))
    for j in plan.jpegs:
        (host if j.route == jpeg_stage.HOST else device).append((j.coef, j.coef + j.info.coef_bytes, "coefficients"))
        if j.stream is not None:
            host.append((j.stream, j.stream + 1, "stream"))  # its length is the JPEG tests' business
        device.append((j.pix, j.pix + j.info.pixel_bytes, "JPEG pixels"))
    host += [(r.pix, r.pix + r.image.size, "raw") for r in plan.raws if r.pix is not None]
    assert 0 <= plan.used <= plan.top - plan.ws_need and plan.top <= plan.stage.size
    for start, end, what in host:
        assert 0 <= start < end <= plan.used, what
    for start, end, what in device:
        assert plan.top - plan.ws_need <= start < end <= plan.stage.size, what
    ranges = sorted(host + device)
    for (_, end, a), (start, _, b) in zip(ranges, ranges[1:]):
        assert end <= start, (a, b)
    assert sorted(j.row for j in plan.jpegs + plan.pngs + plan.raws) == list(range(plan.rows))


def test_offsets_alignments_and_the_palette(hc):
    plan = _plan(hc, 1 << 20)
    plan.add_raw(np.full((3, 3, 1), 7, dtype=np.uint8))  # 9 bytes: the next PNG starts at 16
    infos = [hc.png_parse(b) for b in (PAL, RGB, TALL)]
    jobs = [plan.add_png(b, i, aa, request) for request, (b, i, aa) in
            enumerate(zip((PAL, RGB, TALL), infos, (False, True, False)))]
    assert [j.stream for j in jobs] == [16, 16 + 816, 16 + 816 + 368]
    assert infos[0].stage_bytes == 816 and infos[1].stage_bytes == 9 * 40 and plan.used == 1200 + infos[2].stage_bytes
    assert infos[2].line_off == -(-259 * 6 // 16) * 16 and infos[2].stage_bytes == infos[2].line_off + 5
    top = 1 << 20
    for j, info in zip(jobs, infos):
        top -= info.pixel_bytes
        assert j.pix == top and j.shape == info.shape
    assert plan.top == top and plan.ws_need == 0
    assert [(j.row, j.antialias, j.request) for j in jobs] == [(1, False, 0), (2, True, 1), (3, False, 2)]
    assert [j.blob for j in jobs] == [PAL, RGB, TALL] and plan.pngs == jobs and plan.rows == 4
    # the palette lies behind the scanlines of its image, in the upload region
    pal = np.zeros((256, 3), dtype=np.uint8)
    pal[:5] = pc.palette_for(5)
    at = jobs[0].stream + infos[0].palette_off
    assert infos[0].palette_off == 48
    np.testing.assert_array_equal(plan.stage[at:at + 768], pal.reshape(-1))
    check_png_layout(plan)
    # executed on the CPU: K25's host twin on the staged bytes gives the reference's pixels
    for j, blob in zip(jobs, (PAL, RGB, TALL)):
        np.testing.assert_array_equal(hc.png_unfilter(plan.stage[j.stream:j.stream + j.info.stage_bytes], j.info),
                                      pc.decode(blob))


class CountingCodec:
    """A codec that counts the inflates it is asked for."""

    def __init__(self, real):
        self.real, self.inflates = real, 0

    def png_inflate(self, blob, out):
        self.inflates += 1
        return self.real.png_inflate(blob, out)

    def __getattr__(self, name):
        return getattr(self.real, name)


@pytest.mark.parametrize("blob", [RGB, PAL, TALL], ids=["rgb", "palette", "tall"])
@pytest.mark.parametrize("before", [0, 9], ids=["first", "after9bytes"])
def test_the_fit_test_is_the_documented_formula_and_inflates_nothing_when_it_fails(hc, blob, before):
    info = hc.png_parse(blob)
    at = -(-before // 16) * 16
    least = at + info.stage_bytes + info.pixel_bytes
    for capacity, fits in ((least, True), (least - 1, False), (least + 1, True), (least - 100, False)):
        codec = CountingCodec(hc)
        plan = _plan(hc, capacity, codec)
        if before:
            assert plan.add_raw(np.zeros((before, 1, 1), dtype=np.uint8)).pix == 0
        state = plan.mark()
        job = plan.add_png(blob, info)
        assert (job is not None) == fits, capacity
        assert codec.inflates == (1 if fits else 0)
        if fits:
            assert job.stream == at and job.pix == capacity - info.pixel_bytes and plan.used == at + info.stage_bytes
            check_png_layout(plan)
        else:
            assert plan.mark() == state
            # the caller's fallback: the host's pixels as a raw image (which may not fit either)
            plan.add_raw(hc.png_decode(blob))
            assert plan.rows == (2 if before else 1)


def test_the_workspace_of_a_k24_jpeg_counts_against_a_png(hc):
    w01 = _jpeg("w01")
    jinfo, info = hc.jpeg_parse(w01, 8), hc.png_parse(RGB)
    need = info.stage_bytes + info.pixel_bytes
    for extra, fits in ((0, True), (1, False)):
        plan = _plan(hc, 4 << 20, huffman_wide=1)
        assert plan.add_jpeg(w01, jinfo).route == jpeg_stage.K24 and plan.ws_need > 16
        # a filler that leaves the PNG exactly its bytes under the workspace, then one byte more
        filler = (plan.top - plan.ws_need - need) // 16 * 16 - plan.used + extra
        for shape in ((filler // 1024, 1024, 1), (filler % 1024 or 1024, 1, 1))[:2 if filler % 1024 else 1]:
            assert plan.add_raw(np.zeros(shape, dtype=np.uint8)).pix is not None
        at = -(-plan.used // 16) * 16
        assert (at + need <= plan.top - plan.ws_need) == fits
        assert (plan.add_png(RGB, info) is not None) == fits
        check_png_layout(plan)


def test_an_interlaced_or_oversized_png_is_not_staged(hc):
    plan = _plan(hc, 1 << 20, CountingCodec(hc))
    assert plan.add_png(LACED, hc.png_parse(LACED)) is None
    small = jpeg_stage.StagePlan(host_codec.aligned_buffer(1 << 20), plan.codec, max_dim=8)
    assert small.add_png(RGB, hc.png_parse(RGB)) is None  # 13 wide: the resize of this plan does not take it
    assert plan.codec.inflates == 0 and plan.rows == small.rows == 0


def test_rollback_after_a_malformed_second_blob(hc):
    bad = bytearray(RGB)
    at = next(a for k, a, _ in pc.chunks(RGB) if k == b"IDAT")
    bad[at + 9] ^= 0x40  # the parse passes (it does not read IDAT), the inflate finds the CRC
    bad = bytes(bad)
    plan = _plan(hc, 1 << 20)
    plan.add_png(PAL, hc.png_parse(PAL), request=0)
    before = (plan.mark(), list(plan.pngs), plan.stage[:plan.used].copy())
    # inside one request: a good PNG, then the broken one; the request is taken back out
    mark = plan.mark()
    assert plan.add_png(RGB, hc.png_parse(RGB), request=1) is not None and len(plan.pngs) == 2
    state = plan.mark()
    with pytest.raises(ValueError, match="malformed PNG: bad CRC in IDAT"):
        plan.add_png(bad, hc.png_parse(bad), request=1)
    assert plan.mark() == state  # the raise left the plan as it was
    plan.rollback(mark)
    assert (plan.mark(), plan.pngs) == before[:2]
    np.testing.assert_array_equal(plan.stage[:plan.used], before[2])
    # and the plan goes on as if nothing had been added
    fresh = _plan(hc, 1 << 20)
    fresh.add_png(PAL, hc.png_parse(PAL), request=0)
    for p in (plan, fresh):
        p.add_png(TALL, hc.png_parse(TALL), True, 2)
        check_png_layout(p)
    assert plan.mark() == fresh.mark() and [_key(j) for j in plan.pngs] == [_key(j) for j in fresh.pngs]


def test_a_mixed_plan_of_jpeg_png_and_raw_images(hc):
    f03, f05 = _jpeg("f03"), _jpeg("f05")
    raw = np.random.default_rng(3).integers(0, 256, (33, 47, 3), dtype=np.uint8)
    for knobs in ({}, {"huffman": True}, {"huffman_wide": 1}):
        plan = _plan(hc, 4 << 20, **knobs)
        plan.add_jpeg(f03, hc.jpeg_parse(f03), False, 0)
        plan.add_png(PAL, hc.png_parse(PAL), False, 1)
        plan.add_raw(raw)
        plan.add_png(TALL, hc.png_parse(TALL), True, 2)
        plan.add_jpeg(f05, hc.jpeg_parse(f05), True, 3)
        plan.add_png(RGB, hc.png_parse(RGB), False, 4)
        assert plan.rows == 6 and [j.row for j in plan.pngs] == [1, 3, 5] and [j.row for j in plan.jpegs] == [0, 4]
        check_png_layout(plan)
        for j, blob in zip(plan.pngs, (PAL, TALL, RGB)):
            np.testing.assert_array_equal(hc.png_unfilter(plan.stage[j.stream:j.stream + j.info.stage_bytes], j.info),
                                          pc.decode(blob))


class RecordingHip:
    """Records the kernel calls ``launch_decode`` makes."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args, **kw):
            self.calls.append((name, args, kw))

        return call


class Status:
    def data_ptr(self):
        return 0x5000


def test_launch_decode_issues_k25_once_after_the_jpeg_kernels(hc):
    f03 = _jpeg("f03")
    plan = _plan(hc, 4 << 20, huffman=True)
    plan.add_png(PAL, hc.png_parse(PAL))
    plan.add_jpeg(f03, hc.jpeg_parse(f03))
    plan.add_png(RGB, hc.png_parse(RGB))
    assert plan.jpegs[0].route == jpeg_stage.K23
    hip = RecordingHip()
    upload, only = 0x10000000, 0x20000000
    ran = jpeg_stage.launch_decode(hip, plan.jpegs, upload, only, only + plan.workspace, 0, lambda n: Status(), 77,
                                   pngs=plan.pngs)
    assert [c[0] for c in hip.calls] == ["jpeg_huffman", "jpeg_decode", "png_unfilter"]
    assert len(ran) == 1
    name, (srcs, infos, dsts), kw = hip.calls[-1]
    assert srcs == [upload + j.stream for j in plan.pngs] and all(s % 16 == 0 for s in srcs)
    assert dsts == [only + j.pix for j in plan.pngs]
    assert [i.shape for i in infos] == [(7, 9, 3), (9, 13, 3)] and kw == {"stream": 77}
    # the callers issue the resize after this call; without PNGs, and with the arguments of before, no K25
    hip = RecordingHip()
    jpeg_stage.launch_decode(hip, plan.jpegs, upload, only, only + plan.workspace, 0, lambda n: Status(), 77)
    assert [c[0] for c in hip.calls] == ["jpeg_huffman", "jpeg_decode"]
    hip = RecordingHip()
    assert jpeg_stage.launch_decode(hip, [], upload, only, 0, 0, lambda n: Status(), None, pngs=plan.pngs[:1]) == []
    assert [c[0] for c in hip.calls] == ["png_unfilter"]


def test_the_knob_reader(monkeypatch):
    monkeypatch.delenv("TCAMD_DEVICE_PNG", raising=False)
    default = jpeg_stage.device_png_knob()
    from triton_client_amd.utils.knobs import BY_NAME

    assert default == bool(BY_NAME["TCAMD_DEVICE_PNG"].default)
    monkeypatch.setenv("TCAMD_DEVICE_PNG", "0")
    assert jpeg_stage.device_png_knob() is False
    monkeypatch.setenv("TCAMD_DEVICE_PNG", "1")
    assert jpeg_stage.device_png_knob() is True

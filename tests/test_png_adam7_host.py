"""The host side of the interlaced (Adam7) PNG route, without a GPU: the layout of the staged bytes
K25i reads (``stage_layout_adam7``), ``HostCodec.png_inflate_adam7`` and the kernel's host twin
``png_unfilter_adam7`` against the reference decoder of tests/png_cases.py, bit for bit, and the
planner's part (``StagePlan.add_png`` with ``png_adam7``, the ``TCAMD_DEVICE_PNG_ADAM7`` knob)."""

import numpy as np
import pytest

from tests import png_cases as pc
from triton_client_amd.ops import host_codec
from triton_client_amd.utils import jpeg_stage

ROWS_PER_PASS = 256  # kRowsPerPass: a sub-image of more rows has a scratch scanline
CASES = [(n, b) for n, b in pc.host_cases() if n.startswith("adam7")] \
    + [("adam7_tall", pc.make(3, 4, 2 * ROWS_PER_PASS + 3, 5, pc.CYCLE, adam7=True))]  # passes 6 and 7 have scratch
RGB = pc.make(2, 8, 9, 13, pc.CYCLE)
LACED = pc.make(2, 8, 9, 13, pc.CYCLE, adam7=True)
LACED_PAL = pc.make(3, 2, 33, 35, pc.CYCLE, adam7=True)


@pytest.fixture(scope="module")
def hc():
    return host_codec.load()


@pytest.mark.parametrize("name,blob", CASES, ids=[n for n, _ in CASES])
def test_layout_inflate_and_unfilter_of_an_interlaced_file(hc, name, blob):
    info = hc.png_parse(blob)
    lay = hc.png_adam7_layout(info)
    end = 0
    for p, (x0, y0, dx, dy) in enumerate(pc.ADAM7):
        pw, ph = len(range(x0, info.w, dx)), len(range(y0, info.h, dy))
        assert (lay.off[p], lay.h[p], lay.w[p]) == (end, ph, pw)
        end += ph * (1 + pc.row_bytes(pw, info.ctype, info.depth)) if pw and ph else 0
    assert lay.filtered_bytes == end == info.filtered_bytes == info.stage_bytes
    assert lay.palette_off == (-(-end // 16) * 16 if info.ctype == 3 else 0)
    end = lay.palette_off + 768 if info.ctype == 3 else end
    scratch = []
    for p in range(7):
        tall = lay.w[p] and lay.h[p] > ROWS_PER_PASS
        assert lay.line_off[p] == (-(-end // 16) * 16 if tall else 0)
        if tall:
            end = lay.line_off[p] + pc.row_bytes(lay.w[p], info.ctype, info.depth)
            scratch.append((lay.line_off[p], end))
    assert lay.stage_bytes == end and (name != "adam7_tall" or len(scratch) == 2)
    buf = host_codec.aligned_buffer(lay.stage_bytes)
    buf[:] = 0x5A
    hc.png_inflate_adam7(blob, buf)
    assert all((buf[a:b] == 0x5A).all() for a, b in scratch)  # the scratch scanlines are left alone
    np.testing.assert_array_equal(hc.png_unfilter_adam7(buf, info), pc.decode(blob))


def test_each_entry_point_refuses_the_other_kind_of_file(hc):
    info, buf = hc.png_parse(RGB), host_codec.aligned_buffer(4096)
    for call, msg in ((lambda: hc.png_inflate_adam7(RGB, buf), "unsupported PNG: not an interlaced file"),
                      (lambda: hc.png_adam7_layout(info), ""), (lambda: hc.png_unfilter_adam7(buf, info), ""),
                      (lambda: hc.png_inflate(LACED, buf), "an interlaced file has no staged form")):
        with pytest.raises(ValueError, match=msg):
            call()


def test_the_planner_stages_an_interlaced_png_only_with_the_knob(hc, monkeypatch):
    def _plan(codec, capacity=1 << 20, **kw):
        return jpeg_stage.StagePlan(host_codec.aligned_buffer(capacity), codec, **kw)

    inflates, real = [], hc.png_inflate_adam7
    monkeypatch.setattr(hc, "png_inflate_adam7", lambda blob, out: (inflates.append(1), real(blob, out)))
    monkeypatch.delenv("TCAMD_DEVICE_PNG_ADAM7", raising=False)
    monkeypatch.delenv("TCAMD_DEVICE_PNG", raising=False)
    assert jpeg_stage.device_png_adam7_knob() is False
    off = _plan(hc, png_adam7=jpeg_stage.device_png_adam7_knob())
    assert off.add_png(LACED, hc.png_parse(LACED)) is None and not inflates and off.rows == 0
    monkeypatch.setenv("TCAMD_DEVICE_PNG_ADAM7", "1")
    assert jpeg_stage.device_png_adam7_knob() is True
    monkeypatch.setenv("TCAMD_DEVICE_PNG", "0")
    assert jpeg_stage.device_png_adam7_knob() is False  # effective only with the PNG route itself
    # staged between a raw image, a non-interlaced PNG and another interlaced one; nothing overlaps
    plan = _plan(hc, png_adam7=True)
    raw = plan.add_raw(np.full((3, 3, 1), 7, dtype=np.uint8))
    png = plan.add_png(RGB, hc.png_parse(RGB))
    mark = plan.mark()
    jobs = [plan.add_png(b, hc.png_parse(b), aa, 3) for b, aa in ((LACED, False), (LACED_PAL, True))]
    assert plan.adam7s == jobs and plan.pngs == [png] and isinstance(png, jpeg_stage.PngJob) and plan.rows == 4
    assert [(j.row, j.antialias, j.request) for j in jobs] == [(2, False, 3), (3, True, 3)] and len(inflates) == 2
    ranges = [(raw.pix, raw.pix + 9), (png.stream, png.stream + png.info.stage_bytes)]
    top = plan.stage.size - png.info.pixel_bytes
    for j, blob in zip(jobs, (LACED, LACED_PAL)):
        assert j.stream == -(-ranges[-1][1] // 16) * 16
        ranges.append((j.stream, j.stream + j.layout.stage_bytes))
        top -= j.info.pixel_bytes
        assert j.pix == top and j.shape == j.info.shape
        np.testing.assert_array_equal(hc.png_unfilter_adam7(plan.stage[ranges[-1][0]:ranges[-1][1]], j.info),
                                      pc.decode(blob))
    assert plan.used == ranges[-1][1] <= plan.top == top
    # a truncated IDAT raises and leaves the plan as it was; a rollback forgets the interlaced jobs
    state = plan.mark()
    kind, at, n = next(c for c in pc.chunks(LACED) if c[0] == b"IDAT")
    bad = LACED[:at - 8] + pc.chunk(b"IDAT", LACED[at:at + n // 2]) + pc.chunk(b"IEND", b"")
    with pytest.raises(ValueError, match="malformed PNG: zlib: the stream ends early"):
        plan.add_png(bad, hc.png_parse(bad))
    assert plan.mark() == state and len(plan.adam7s) == 2
    plan.rollback(mark)
    assert plan.mark() == mark and plan.adam7s == [] and plan.pngs == [png] and plan.rows == 2
    # the fit rule is add_png's: with one byte less nothing is inflated
    info, need = hc.png_parse(LACED), hc.png_adam7_layout(hc.png_parse(LACED)).stage_bytes
    del inflates[:]
    assert _plan(hc, need + info.pixel_bytes - 1, png_adam7=True).add_png(LACED, info) is None and not inflates
    assert _plan(hc, need + info.pixel_bytes, png_adam7=True).add_png(LACED, info) is not None and len(inflates) == 1

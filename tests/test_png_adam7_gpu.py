"""K25i png_unfilter_adam7 (csrc/kernels/png.hip) against the reference decoder of tests/png_cases.py,
bit for bit, and the interlaced PNG route (``TCAMD_DEVICE_PNG_ADAM7``) through the GPU
``preprocess_inception`` and ``preprocess_raw_batch_device``."""

from collections import namedtuple

import numpy as np
import pytest

from tests import png_cases as pc
from triton_client_amd.utils import image

pytestmark = pytest.mark.gpu

CANARY = 0xA5
Info = namedtuple("Info", "h w ctype depth interlace")


def _k25i(blobs):
    """``blobs`` through ONE ``hip.png_unfilter_adam7`` call: sources at multiples of 16, destinations at
    odd addresses with canary bytes between them; pixels, canaries and the staged bytes are checked."""
    import torch
    from triton_client_amd.ops import hip, host_codec
    hc = host_codec.load()
    infos = [hc.png_parse(b) for b in blobs]
    lays = [hc.png_adam7_layout(i) for i in infos]
    src_at, dst_at, up, only = [], [], 0, 0
    for k, (info, lay) in enumerate(zip(infos, lays)):
        src_at.append(-(-up // 16) * 16 + 16 * (k % 3))
        up = src_at[-1] + lay.stage_bytes
        dst_at.append(only + 1 + only % 2)  # one or two canary bytes, then an odd address
        only = dst_at[-1] + info.pixel_bytes
    host = np.full(up, 0x3C, dtype=np.uint8)
    scratch, mine = np.zeros(up, dtype=bool), np.zeros(only + 1, dtype=bool)
    for at, dat, blob, info, lay in zip(src_at, dst_at, blobs, infos, lays):
        buf = host_codec.aligned_buffer(lay.stage_bytes)
        buf[:] = 0x3C
        hc.png_inflate_adam7(blob, buf)
        host[at:at + lay.stage_bytes] = buf
        mine[dat:dat + info.pixel_bytes] = True
        for p in range(7):
            if lay.line_off[p]:
                scratch[at + lay.line_off[p]:at + lay.line_off[p] + pc.row_bytes(lay.w[p], info.ctype, info.depth)] = True
    src = torch.from_numpy(host).cuda()
    dst = torch.full((only + 1,), CANARY, device="cuda", dtype=torch.uint8)
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 2 == 0
    hip.png_unfilter_adam7([src.data_ptr() + a for a in src_at], infos, [dst.data_ptr() + a for a in dst_at],
                           stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = dst.cpu().numpy()
    for k, (at, info) in enumerate(zip(dst_at, infos)):
        np.testing.assert_array_equal(out[at:at + info.pixel_bytes].reshape(info.shape), pc.decode(blobs[k]),
                                      err_msg="image %d %s type %d depth %d" % (k, info.shape, info.ctype, info.depth))
    assert (out[~mine] == CANARY).all(), "a byte outside an image's pixels was written"
    np.testing.assert_array_equal(src.cpu().numpy()[~scratch], host[~scratch])  # only the scratch lines are written
    return lays


def test_the_matrix_of_types_depths_and_sizes_equals_the_reference():
    cases = [b for n, b in pc.host_cases() if n.startswith("adam7")]
    assert len(cases) > 64 * 3  # several launches of one call
    _k25i(cases)


def test_the_edges_of_the_decomposition():
    from triton_client_amd.ops import hip
    rpw, rpp, cc = hip.png_unfilter_geometry()
    lays = _k25i([pc.make(2, 8, 131, 5, pc.CYCLE, adam7=True),   # a wave edge inside pass 7: 65 rows
                  pc.make(3, 8, 515, 3, pc.CYCLE, adam7=True),   # a pass edge inside pass 7: 257 rows, a scratch line
                  pc.make(0, 8, 2057, 9, pc.CYCLE, adam7=True),  # a pass edge in pass 1: 258 rows
                  pc.make(2, 8, 9, 259, pc.CYCLE, adam7=True),   # a column-chunk edge: 129 units in pass 6
                  pc.make(0, 1, 3, 1033, pc.CYCLE, adam7=True)])  # the same at depth 1: 130 bytes in pass 7
    assert lays[0].h[6] == rpw + 1 and lays[1].h[6] == rpp + 1 and lays[1].line_off[6] and lays[2].h[0] == rpp + 2
    assert lays[2].line_off[0] and lays[3].w[5] == cc + 1 and -(-lays[4].w[6] // 8) == cc + 2


@pytest.mark.parametrize("what", ["not interlaced", "too wide", "too tall", "zero side", "no such pair", "null source",
                                  "misaligned source", "null destination"])
def test_bad_arguments_are_refused_before_any_launch(what):
    import torch
    from triton_client_amd.ops import hip
    src = torch.zeros(4096, device="cuda", dtype=torch.uint8)
    dst = torch.full((4096,), CANARY, device="cuda", dtype=torch.uint8)
    good = Info(4, 4, 2, 8, 1)
    info = {"not interlaced": good._replace(interlace=0), "too wide": good._replace(w=hip.RESIZE_MAX_DIM + 1),
            "too tall": good._replace(h=hip.RESIZE_MAX_DIM + 1), "zero side": good._replace(h=0),
            "no such pair": good._replace(ctype=3, depth=16)}.get(what, good)
    s = {"null source": 0, "misaligned source": src.data_ptr() + 8}.get(what, src.data_ptr())
    d = 0 if what == "null destination" else dst.data_ptr()
    with pytest.raises(hip.HipError) as err:
        hip.png_unfilter_adam7([src.data_ptr() + 1024, s], [good, info], [dst.data_ptr() + 1024, d])
    assert err.value.code == 1  # hipErrorInvalidValue
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == CANARY).all()  # the good image before it was not launched either


@pytest.mark.parametrize("route", ["served", "client"])
def test_the_adam7_knob_changes_the_route_and_not_one_bit_of_the_rows(route, monkeypatch):
    from triton_client_amd.ops import hip
    from triton_client_amd.server.gpu_models import PreprocessInception
    from triton_client_amd.server.types import InferRequest, InputTensor
    raw = np.random.default_rng(4).integers(0, 256, (33, 47, 3), dtype=np.uint8)
    laced = [pc.make(2, 8, 97, 131, pc.CYCLE, adam7=True), pc.make(3, 2, 64, 48, pc.CYCLE, adam7=True)]
    plain = pc.make(6, 8, 300, 41, pc.CYCLE)
    real, calls, rows = hip.png_unfilter_adam7, [], {}
    monkeypatch.setattr(hip, "png_unfilter_adam7", lambda srcs, *a, **kw: (calls.append(len(srcs)), real(srcs, *a, **kw)))
    for knob in ("1", None):
        monkeypatch.delenv("TCAMD_DEVICE_PNG_ADAM7", raising=False)
        if knob:
            monkeypatch.setenv("TCAMD_DEVICE_PNG_ADAM7", knob)
        if route == "client":
            rows[knob] = image.preprocess_raw_batch_device([laced[0], plain, raw, laced[1]], 3, 224, 224)
        else:
            blobs = [laced[0], plain, image.encode_raw(raw), laced[1]]
            data = np.array(blobs, dtype=np.object_).reshape(len(blobs), 1)
            model = PreprocessInception()
            model.load()
            (out,), = model.execute([InferRequest(model_name=model.name,
                                                  inputs=[InputTensor("INPUT", "BYTES", [len(blobs), 1], data)])])
            rows[knob] = out.data.copy()
            model.unload()
        assert calls == [2]  # once per batch with the two interlaced files, and never with the knob unset
    assert rows["1"].shape == (4, 3, 224, 224)
    np.testing.assert_array_equal(rows["1"], rows[None])

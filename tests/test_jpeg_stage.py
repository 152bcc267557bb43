"""The JPEG route and the staging layout (triton_client_amd/utils/jpeg_stage.py)
without a GPU: a batch is planned over a host buffer, the plan is executed by
the host emulations of K23 and K24, and every coefficient buffer must be the
host entropy decoder's; the offsets are checked against the documented
contract after every step.  The same plans run on the device in
tests/test_jpeg_huffman_gpu.py, test_jpeg_huffman_wide_gpu.py,
test_jpeg_scaled_gpu.py and test_jpeg_gpu.py, which compare output rows."""

import glob
import os

import numpy as np
import pytest

from triton_client_amd.utils import jpeg_stage
from triton_client_amd.utils.image import jpeg_auto_scale
from triton_client_amd.utils.jpeg_stage import HOST, K23, K24

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _blob(prefix):
    (path,) = glob.glob(os.path.join(GOLDEN, "jpeg*", prefix + "_*.jpg"))
    with open(path, "rb") as f:
        return f.read()


BLOBS = {name: _blob(name) for name in ("f01", "f03", "f05", "f12", "h05", "b01", "w01")}
BATCH = (("f05", 1), ("w01", 1), ("h05", 2), ("w01", 8), ("f03", 1), ("b01", 1))
KNOBS = ((0, 0), (0, 1), (1, 0), (1, 1), (0, 300000))  # (TCAMD_DEVICE_HUFFMAN, TCAMD_DEVICE_HUFFMAN_WIDE)
CAPACITIES = (32 << 20, 3000000, 1500000)
ROUTES_AT_32_MIB = {
    (0, 0): [HOST] * 6,
    (0, 1): [K24] * 6,
    (1, 0): [K23, HOST, HOST, HOST, K23, K23],
    (1, 1): [K23, K24, K24, K24, K23, K23],
    (0, 300000): [HOST, K24, HOST, K24, HOST, HOST],
}
WORKSPACE_LISTS = ([1], [1024], [1025, 1], [2808] * 3, [2048] * 64)
MAX_DIM = 16384


@pytest.fixture(scope="module")
def hc():
    from triton_client_amd.ops import host_codec

    return host_codec.load()


@pytest.fixture(scope="module")
def batch(hc):
    """[(blob, parse at the scale, the host entropy decoder's coefficients)] of ``BATCH``, decoded once."""
    out = []
    for name, scale in BATCH:
        info = hc.jpeg_parse(BLOBS[name], scale)
        want = np.empty(info.coef_bytes, dtype=np.uint8)
        hc.jpeg_entropy_decode(BLOBS[name], want, scale)
        want.setflags(write=False)
        out.append((BLOBS[name], info, want))
    return out


def _new_plan(hc, capacity, knobs):
    from triton_client_amd.ops import host_codec

    return jpeg_stage.StagePlan(host_codec.aligned_buffer(capacity), hc, bool(knobs[0]), knobs[1], MAX_DIM)


def _stream_bytes(plan, job):
    return int(plan.stage[job.stream:job.stream + 8].view("<u4")[1])  # the header's second word: total bytes


def check_layout(plan):
    """The documented contract of the staging area, on the plan as it stands."""
    capacity = plan.stage.size
    host, device = [], []  # (start, end, what) of what the host wrote / of what exists on the device only
    for j in plan.jpegs:
        if j.route == HOST:
            assert j.stream is None
            host.append((j.coef, j.coef + j.info.coef_bytes, "coefficients"))
        else:
            assert j.stream % 16 == 0
            host.append((j.stream, j.stream + _stream_bytes(plan, j), "stream"))
            device.append((j.coef, j.coef + j.info.coef_bytes, "coefficients"))
        assert j.coef % 128 == 0  # K22 needs 16
        device.append((j.pix, j.pix + j.info.pixel_bytes, "pixels"))
    host += [(r.pix, r.pix + r.image.size, "raw") for r in plan.raws if r.pix is not None]
    if plan.ws_need:
        assert plan.workspace % 16 == 0
        assert plan.ws_need == 16 + _workspace_formula(plan)
        device.append((plan.workspace, plan.workspace + plan.ws_need - 16, "workspace"))
    else:
        assert not any(j.route == K24 for j in plan.jpegs)
    assert 0 <= plan.used <= plan.top - plan.ws_need and plan.top <= capacity
    for start, end, what in host:
        assert 0 <= start < end <= plan.used, what
    for start, end, what in device:
        assert plan.top - plan.ws_need <= start < end <= capacity, what
    ranges = sorted(host + device)
    for (_, end, a), (start, _, b) in zip(ranges, ranges[1:]):
        assert end <= start, (a, b)
    assert sorted(j.row for j in plan.jpegs + plan.raws) == list(range(plan.rows))


def _workspace_formula(plan):
    nsubs = [j.nsub for j in plan.jpegs if j.route == K24]
    return (sum(-(-n // 1024) for n in nsubs) * 72 + sum(nsubs) * 28 + 15) // 16 * 16


def _plan_batch(hc, batch, capacity, knobs):
    """``batch`` through a new plan as a caller does it, the layout checked after every add; returns
    (plan, the route of every JPEG, None for one that fits no route)."""
    plan = _new_plan(hc, capacity, knobs)
    routes = []
    for request, (blob, info, _) in enumerate(batch):
        job = plan.add_jpeg(blob, info, False, request)
        routes.append(job and job.route)
        if job is None:
            plan.add_raw(hc.jpeg_decode(blob, info.scale))
        check_layout(plan)
    return plan, routes


@pytest.mark.parametrize("capacity", CAPACITIES)
@pytest.mark.parametrize("knobs", KNOBS)
def test_the_plan_executed_on_the_cpu_gives_the_host_decoders_coefficients(hc, batch, knobs, capacity):
    from triton_client_amd.ops import host_codec

    plan, routes = _plan_batch(hc, batch, capacity, knobs)
    if capacity == 32 << 20:
        assert routes == ROUTES_AT_32_MIB[knobs]
    elif capacity == 3000000:  # the last JPEG, b01, fits no route
        assert routes[-1] is None and None not in routes[:-1]
    else:  # nor does the full-size w01
        assert [k for k, r in enumerate(routes) if r is None] == [1, 5]
    device = host_codec.aligned_buffer(capacity)  # what the device has: the upload, nothing else
    device[:] = 0
    device[:plan.used] = plan.stage[:plan.used]
    assert [j.request for j in plan.jpegs] == [k for k, r in enumerate(routes) if r is not None]
    for j in plan.jpegs:
        got = device[j.coef:j.coef + j.info.coef_bytes]
        if j.route == K23:
            assert hc.jpeg_huffman_emulate(device[j.stream:], got)[0] == 0
        elif j.route == K24:
            assert hc.jpeg_huffman_wide_emulate(device[j.stream:], got)[0] == 0
        np.testing.assert_array_equal(got, batch[j.request][2], err_msg="%s %s" % (BATCH[j.request], j.route))


def _f03_alone(hc, capacity, knobs):
    plan = _new_plan(hc, capacity, knobs)
    job = plan.add_jpeg(BLOBS["f03"], hc.jpeg_parse(BLOBS["f03"]))
    if job is not None:
        check_layout(plan)
    return job and job.route


def test_the_fit_thresholds_are_the_documented_formulas(hc):
    from triton_client_amd.ops import host_codec

    blob = BLOBS["f03"]
    info = hc.jpeg_parse(blob)
    coef_bytes, pixel_bytes = info.coef_bytes, info.pixel_bytes
    room = host_codec.aligned_buffer(hc.jpeg_stream_bound_wide(len(blob)))
    n23 = hc.jpeg_stream_pack(blob, room)[1]
    _, n24, nsub = hc.jpeg_stream_pack_wide(blob, room)
    assert n23 is not None and n24 is not None and nsub == 5
    need = 16 + (72 + nsub * 28 + 15) // 16 * 16  # one chunk

    def expected(capacity, knobs):
        coef = (capacity - pixel_bytes - coef_bytes) // 128 * 128
        if knobs[0] and n23 <= coef:
            return K23
        if knobs[1] and n24 <= coef - need:
            return K24
        return HOST if coef_bytes + pixel_bytes <= capacity else None

    def up128(n):
        return -(-n // 128) * 128

    # the smallest capacity that fits each route, and what one byte less gives: the next route in the order
    least = {HOST: coef_bytes + pixel_bytes, K23: pixel_bytes + coef_bytes + up128(n23),
             K24: pixel_bytes + coef_bytes + up128(n24 + need)}
    assert _f03_alone(hc, least[HOST], (0, 0)) == HOST and _f03_alone(hc, least[HOST] - 1, (0, 0)) is None
    assert _f03_alone(hc, least[K23], (1, 0)) == K23 and _f03_alone(hc, least[K23] - 1, (1, 0)) == HOST
    assert _f03_alone(hc, least[K24], (0, 1)) == K24 and _f03_alone(hc, least[K24] - 1, (0, 1)) == HOST
    assert _f03_alone(hc, least[K24] - 1, (1, 1)) == K23 and _f03_alone(hc, least[K23] - 1, (1, 1)) == HOST
    for knobs in ((0, 0), (1, 0), (0, 1), (1, 1)):
        for capacity in sorted({c + d for c in least.values() for d in (-129, -100, -1, 0, 1, 63, 100, 127, 128)}):
            assert _f03_alone(hc, capacity, knobs) == expected(capacity, knobs), (capacity, knobs)


def test_the_workspace_counts_against_what_follows_a_k24_jpeg(hc, batch):
    """w01 at 1/8 on K24, then f03 (below the knob: the host's) or a raw image: either has what is left
    under the workspace, ``top - ws_need - used`` bytes, by the formulas and not by the planner."""
    (blob, info, _), f03 = batch[3], hc.jpeg_parse(BLOBS["f03"])
    from triton_client_amd.ops import host_codec

    _, used, n = hc.jpeg_stream_pack_wide(blob, host_codec.aligned_buffer(hc.jpeg_stream_bound_wide(len(blob))), 8)
    need = 16 + (-(-n // 1024) * 72 + n * 28 + 15) // 16 * 16

    def left(capacity):  # for the upload, once w01 is in
        return (capacity - info.pixel_bytes - info.coef_bytes) // 128 * 128 - need - used

    for size, add in ((-(-used // 128) * 128 - used + f03.coef_bytes + f03.pixel_bytes,
                       lambda plan: plan.add_jpeg(BLOBS["f03"], f03)),
                      (3 * 41 * 37, lambda plan: plan.add_raw(np.zeros((41, 37, 3), dtype=np.uint8)).pix)):
        least = info.pixel_bytes + info.coef_bytes + -(-(used + need + size) // 128) * 128
        assert left(least) >= size > left(least - 1)
        for capacity, fits in ((least, True), (least - 1, False), (least + 100, True), (least - 100, False)):
            plan = _new_plan(hc, capacity, (0, 300000))
            assert plan.add_jpeg(blob, info).route == K24 and (add(plan) is not None) == fits, (capacity, size)
            check_layout(plan)


def test_rollback_restores_every_cursor_and_the_plan_goes_on_as_if_nothing_was_added(hc, batch):
    raw = np.random.default_rng(15).integers(0, 256, (33, 47, 3), dtype=np.uint8)

    def state(plan):
        return plan.rows, plan.used, plan.top, plan.ws_need, list(plan.jpegs), list(plan.raws)

    def add(plan, k):
        return plan.add_jpeg(batch[k][0], batch[k][1], False, k)

    plan = _new_plan(hc, 32 << 20, (0, 1))
    assert add(plan, 0).route == K24
    plan.add_raw(raw)
    before, mark = state(plan), plan.mark()
    assert add(plan, 1).route == K24 and add(plan, 3).route == K24
    assert plan.add_raw(raw).pix is not None
    assert plan.ws_need > before[3] and plan.rows == before[0] + 3
    plan.rollback(mark)
    assert state(plan) == before
    fresh = _new_plan(hc, 32 << 20, (0, 1))
    add(fresh, 0)
    fresh.add_raw(raw)
    for p in (plan, fresh):
        assert add(p, 2).route == K24 and add(p, 5).route == K24
        p.add_raw(raw, antialias=True)
        check_layout(p)
    assert state(plan) == state(fresh)
    np.testing.assert_array_equal(plan.stage[:plan.used], fresh.stage[:fresh.used])


def test_a_raw_image_that_the_device_resize_does_not_take_or_that_does_not_fit_is_the_hosts(hc):
    plan = _new_plan(hc, 1000, (0, 0))
    fits, wide, large = (np.zeros(s, dtype=np.uint8) for s in ((10, 10, 3), (1, MAX_DIM + 1, 1), (20, 20, 3)))
    assert plan.add_raw(fits).pix == 0 and plan.add_raw(wide).pix is None and plan.add_raw(large).pix is None
    assert plan.add_raw(fits[:, :, :1]).pix == 300 and plan.add_raw(np.zeros((5, 5, 2), dtype=np.uint8)).pix is None
    assert (plan.rows, plan.used) == (5, 400) and [r.row for r in plan.raws] == list(range(5))


def test_parse_at_scale(hc):
    def fields(info):
        return info.shape, info.scale, info.coef_bytes, list(info.ny), list(info.nx)

    auto = jpeg_auto_scale(480, 640, 224, 224)
    assert auto == 2
    assert fields(jpeg_stage.parse_at_scale(hc, BLOBS["b01"], 0, 224, 224)) == fields(hc.jpeg_parse(BLOBS["b01"], auto))
    assert fields(jpeg_stage.parse_at_scale(hc, BLOBS["f01"], 0, 224, 224)) == fields(hc.jpeg_parse(BLOBS["f01"]))
    for scale in (1, 2, 4, 8):
        assert fields(jpeg_stage.parse_at_scale(hc, BLOBS["b01"], scale, 224, 224)) == \
            fields(hc.jpeg_parse(BLOBS["b01"], scale))
    for scale in (0, 1, 4):
        with pytest.raises(ValueError, match="unsupported JPEG: progressive"):
            jpeg_stage.parse_at_scale(hc, BLOBS["f12"], scale, 224, 224)


def test_the_automatic_scale_of_a_small_image_costs_one_parse(hc, monkeypatch):
    calls = []
    real = hc.jpeg_parse
    monkeypatch.setattr(hc, "jpeg_parse", lambda *a: calls.append(a[1:]) or real(*a))
    jpeg_stage.parse_at_scale(hc, BLOBS["f01"], 0, 224, 224)
    assert len(calls) == 1
    jpeg_stage.parse_at_scale(hc, BLOBS["b01"], 0, 224, 224)
    assert len(calls) == 3


@pytest.mark.parametrize("nsubs", WORKSPACE_LISTS, ids=str)
def test_the_host_library_sizes_the_k24_workspace(hc, nsubs):
    chunks = sum(-(-n // 1024) for n in nsubs)
    assert hc.jpeg_huffman_wide_workspace(nsubs) == (chunks * 72 + sum(nsubs) * 28 + 15) // 16 * 16
    assert hc.jpeg_huffman_wide_workspace(nsubs, 8) == (sum(-(-n // 8) for n in nsubs) * 72 + sum(nsubs) * 28 + 15) // 16 * 16


def test_the_knob_readers(monkeypatch):
    for name in ("TCAMD_DEVICE_HUFFMAN", "TCAMD_DEVICE_HUFFMAN_WIDE"):
        monkeypatch.delenv(name, raising=False)
    assert (jpeg_stage.device_huffman_knob(), jpeg_stage.device_huffman_wide_knob()) == (False, 0)
    monkeypatch.setenv("TCAMD_DEVICE_HUFFMAN", "1")
    monkeypatch.setenv("TCAMD_DEVICE_HUFFMAN_WIDE", "300000")
    assert (jpeg_stage.device_huffman_knob(), jpeg_stage.device_huffman_wide_knob()) == (True, 300000)
    monkeypatch.setenv("TCAMD_DEVICE_HUFFMAN_WIDE", "")
    assert jpeg_stage.device_huffman_wide_knob() == 0
    monkeypatch.setenv("TCAMD_DEVICE_HUFFMAN_WIDE", "-5")
    assert jpeg_stage.device_huffman_wide_knob() == 0

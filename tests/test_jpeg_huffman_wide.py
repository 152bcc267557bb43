"""The K24 jpeg_huffman_wide launch sequence without a GPU: the wide stream pack
(``tcamd_host_jpeg_stream_pack_wide``) and the host emulation of the kernels
(``tcamd_host_jpeg_huffman_wide_emulate``: the kernels' own phases from
csrc/kernels/jpeg_huff_wide_core.h, launch by launch, workgroup by workgroup,
thread by thread) against the host entropy decoder and the numpy reference at
every scale, and against K23's emulation where K23 packs.  The kernels
themselves are compared with the host decoder in
tests/test_jpeg_huffman_wide_gpu.py; untrusted bytes are explored by
csrc/cpp/tests/jpeg_wide_test.cc under sanitizers."""

import os

import numpy as np
import pytest

from tests import jpeg_cases as jc
from tests import jpeg_huff_cases as jh
from tests import jpeg_scaled_cases as js
from tests.test_jpeg_huffman import TAILS, _one_block_intervals, aligned

WIDE_MAGIC = 0x3157544A  # "JTW1"
SCALES = (1, 2, 4, 8)
CHUNKS = (1, 2, 8, 1024)
W01 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_wide", "w01_640x480_420_q95_noise.jpg")


def _w01():
    with open(W01, "rb") as f:
        return f.read()


FIXTURES = jh.decodable() + [("w01_640x480_420_q95_noise", _w01())]
NAMES = [n for n, _ in FIXTURES]

# (fixture, chunk_subs) -> (chunks, the inter-chunk launches in which a chunk took a new entry), as
# observed: f11 (q100 noise, 41 subsequences, 27 of K23's rounds) is the near-serial case
CHANGED = {
    ("f11", 2): (21, 13),
    ("h04", 8): (30, 2),
    ("w01", 1024): (3, 1),
}


@pytest.fixture(scope="module")
def hc():
    from triton_client_amd.ops import host_codec

    return host_codec.load()


def wide_pack(hc, blob, scale=1, cap=None):
    """(parse at the scale, the wide stream buffer as a uint8 array or None when not packable, subsequences)."""
    buf = aligned(hc.jpeg_stream_bound_wide(len(blob)) if cap is None else cap, 0xEE)
    info, used, nsub = hc.jpeg_stream_pack_wide(blob, buf, scale)
    return info, (None if used is None else buf[:used]), nsub


def host_coefficients(hc, blob, scale=1):
    out = aligned(hc.jpeg_parse(blob, scale).coef_bytes)
    hc.jpeg_entropy_decode(blob, out, scale)
    return out


@pytest.fixture(scope="module")
def reference():
    """Per fixture the numpy reference's parse and coefficients, decoded once."""
    out = {}
    for name, blob in FIXTURES:
        info = jc.parse(blob)
        out[name] = (info, jc.entropy_decode(info))
    return out


@pytest.mark.parametrize("name,blob", FIXTURES, ids=NAMES)
def test_pack_and_emulation_agree_with_the_host_and_the_reference(hc, reference, name, blob):
    k23 = aligned(hc.jpeg_stream_bound(len(blob)), 0xEE)
    k23_info, k23_used = hc.jpeg_stream_pack(blob, k23)
    for scale in SCALES:
        info, stream, nsub = wide_pack(hc, blob, scale)
        assert stream is not None  # no fallback on a fixture
        head = stream[:64].view("<u4")
        assert (int(head[0]), int(head[11]), int(head[15])) == (WIDE_MAGIC, nsub, scale)
        want = host_coefficients(hc, blob, scale)
        assert want.tobytes() == js.coefficient_buffer(*reference[name], scale)
        if k23_used is not None:
            # the same pack: only the magic word and the scale differ
            twin = k23[:k23_used].copy()
            twin[:64].view("<u4")[[0, 15]] = (WIDE_MAGIC, scale)
            assert stream.tobytes() == twin.tobytes()
        for cs in CHUNKS:
            got = aligned(info.coef_bytes, 0x5A)
            status, _ = hc.jpeg_huffman_wide_emulate(stream, got, cs)
            assert status == 0, (scale, cs)  # no fallback on a fixture
            assert got.tobytes() == want.tobytes(), (scale, cs)
        if scale == 1 and k23_used is not None:
            got = aligned(k23_info.coef_bytes, 0x5A)
            assert hc.jpeg_huffman_emulate(k23[:k23_used], got)[0] == 0 and got.tobytes() == want.tobytes()


def test_w01_is_above_k23_and_spans_three_chunks_of_one_segment(hc):
    blob = _w01()
    _, stream, nsub = wide_pack(hc, blob)
    assert nsub > jh.MAX_SUB and -(-nsub // 1024) == 3 and int(stream[:64].view("<u4")[10]) == 1
    assert hc.jpeg_stream_pack(blob, aligned(hc.jpeg_stream_bound(len(blob))))[1] is None


def test_the_cross_chunk_launches_really_run(hc):
    seen = {}
    for (prefix, cs) in CHANGED:
        blob = next(b for n, b in FIXTURES if n.startswith(prefix))
        info, stream, nsub = wide_pack(hc, blob)
        got = aligned(info.coef_bytes, 0x5A)
        status, changed = hc.jpeg_huffman_wide_emulate(stream, got, cs)
        assert status == 0 and got.tobytes() == host_coefficients(hc, blob).tobytes()
        chunks = -(-nsub // cs)
        assert changed <= chunks - 1
        if prefix != "w01":
            assert changed > 1  # an entry travels on through more than one chunk boundary
        seen[(prefix, cs)] = (chunks, changed)
    print("chunks, launches that changed something:", seen)
    assert seen == CHANGED


@pytest.mark.parametrize("chunk_subs", [4, 8])
def test_segments_start_inside_chunks_and_chunks_span_segments(hc, chunk_subs):
    blob = jh.blob("h05")  # DRI 7: 12 segments over 142 subsequences
    info, stream, nsub = wide_pack(hc, blob)
    head = stream[:64].view("<u4")
    nseg, ntab = int(head[10]), int(head[12])
    first = stream[448 + 1416 * ntab:][:16 * nseg].view("<u4").reshape(nseg, 4)[:, 3]
    assert nseg == 12 and (first[1:] % chunk_subs != 0).any()  # segments start inside chunks
    assert (np.diff(first)[:-1] > chunk_subs).all()  # and every full interval spans more than one chunk
    for scale in SCALES:
        info, stream, _ = wide_pack(hc, blob, scale)
        got = aligned(info.coef_bytes, 0x5A)
        assert hc.jpeg_huffman_wide_emulate(stream, got, chunk_subs)[0] == 0
        assert got.tobytes() == host_coefficients(hc, blob, scale).tobytes()


@pytest.mark.parametrize("chunk_subs", [1, 8, 1024])
def test_one_block_intervals_above_k23s_workspace(hc, chunk_subs):
    blob = _one_block_intervals(jh.MAX_SUB // 2 + 1)  # one-subsequence segments, two more than K23 holds
    assert hc.jpeg_stream_pack(blob, aligned(hc.jpeg_stream_bound(len(blob))))[1] is None
    info, stream, nsub = wide_pack(hc, blob)
    assert stream is not None and nsub == jh.MAX_SUB + 2 == int(stream[:64].view("<u4")[10])
    got = aligned(info.coef_bytes, 0x5A)
    status, changed = hc.jpeg_huffman_wide_emulate(stream, got, chunk_subs)
    assert (status, changed) == (0, 0)  # no entry ever crosses a segment
    assert got.tobytes() == host_coefficients(hc, blob).tobytes()


# -- refusals -------------------------------------------------------------------------------
def test_the_emulation_rejects_a_stream_buffer_that_does_not_hold(hc):
    b = jh.blob("f05")
    info, stream, _ = wide_pack(hc, b)
    words = ((0, 0), (2, 0), (4, 2), (9, 0), (10, 7), (11, 4096), (12, 7), (13, 0x77), (14, 4), (15, 3), (15, 0),
             (15, 16))
    for word, value in words:
        bad = aligned(len(stream))
        bad[:] = stream
        bad[:64].view("<u4")[word] = value
        for cs in (2, 1024):
            got = aligned(info.coef_bytes, 0x5A)
            assert hc.jpeg_huffman_wide_emulate(bad, got, cs)[0] == 1, (word, value)  # kBadHeader
    ntab = int(stream[:64].view("<u4")[12])
    bad = aligned(len(stream))
    bad[:] = stream
    bad[448 + 1416:][:1024].view("<u2")[:] = 0x0000 | 0x00F0  # every short AC code a ZRL of length 0
    assert hc.jpeg_huffman_wide_emulate(bad, aligned(info.coef_bytes), 2)[0] == 2  # kBadCode
    for field, value in ((0, 2), (1, 1 << 20), (2, 1), (3, 9)):  # segment 1: offset, bits, first MCU, first subsequence
        bad = aligned(len(stream))
        bad[:] = stream
        bad[448 + 1416 * ntab + 16:][:16].view("<u4")[field] = value
        for cs in (2, 1024):
            assert hc.jpeg_huffman_wide_emulate(bad, aligned(info.coef_bytes), cs)[0] == 1, field
    for cs in (3, 2048, 1 << 31):  # not a power of two up to 1024
        assert hc.jpeg_huffman_wide_emulate(stream, aligned(info.coef_bytes), cs)[0] == 1
    assert hc.jpeg_huffman_wide_emulate(stream, aligned(info.coef_bytes - 1), 2)[0] == 1  # a buffer too small


def test_neither_kernel_accepts_the_others_buffer(hc):
    b = jh.blob("f05")
    info, wide, _ = wide_pack(hc, b)
    k23 = aligned(hc.jpeg_stream_bound(len(b)), 0xEE)
    _, used = hc.jpeg_stream_pack(b, k23)
    got = aligned(info.coef_bytes, 0x5A)
    assert hc.jpeg_huffman_wide_emulate(k23[:used], got)[0] == 1
    assert hc.jpeg_huffman_emulate(wide, got)[0] == 1
    assert (got == 0x5A).all()


def test_a_scale_that_is_none_raises_as_the_parse_does(hc):
    b = jh.blob("f01")
    with pytest.raises(ValueError, match="jpeg scale must be 1, 2, 4 or 8"):
        wide_pack(hc, b, 3)


@pytest.mark.parametrize("tail,packable,error", TAILS, ids=[t[0].hex() or "nothing" for t in TAILS])
def test_what_follows_the_scan(hc, tail, packable, error):
    """The wide pack declines what K23's pack declines."""
    b = jh.blob("f01")
    blob = b[:-2] + tail
    for scale in (1, 4):
        info, stream, _ = wide_pack(hc, blob, scale)
        assert (stream is not None) == packable
        if error:
            with pytest.raises(ValueError) as err:
                host_coefficients(hc, blob, scale)
            assert str(err.value) == error
        elif packable:
            want = host_coefficients(hc, blob, scale)
            got = aligned(len(want), 0x5A)
            assert hc.jpeg_huffman_wide_emulate(stream, got, 2)[0] == 0 and got.tobytes() == want.tobytes()


def test_a_misaligned_buffer_is_declined(hc):
    b = jh.blob("f01")
    buf = aligned(hc.jpeg_stream_bound_wide(len(b)) + 8, 0xEE)
    info, used, nsub = hc.jpeg_stream_pack_wide(b, buf[8:], 2)
    assert used is None and nsub is None and info.shape == (8, 8, 3) and (buf == 0xEE).all()


def test_a_buffer_too_small_is_declined_and_nothing_past_it_is_written(hc):
    b = jh.blob("b01")
    _, whole, _ = wide_pack(hc, b)
    for cap in (0, 64, 6000, len(whole) - 1):
        buf = aligned(cap + 64, 0xEE)
        info, used, _ = hc.jpeg_stream_pack_wide(b, buf[:cap])
        assert used is None and info.shape == (480, 640, 3)
        assert (buf[cap:] == 0xEE).all()
    # the bound follows the blob (a segment costs two bytes of it and 20 of the buffer), not the 32 MiB ceiling
    assert len(whole) <= hc.jpeg_stream_bound_wide(len(b)) <= 11 * len(b) + 16384


def test_misnumbered_rst_and_malformed_blobs_are_the_host_decoders_business(hc):
    b = jh.blob("f05")
    i = b.index(b"\xff\xd1", b.index(b"\xff\xda"))
    assert wide_pack(hc, b[:i + 1] + b"\xd3" + b[i + 2:])[1] is None
    for blob in (jc.blob(jc.fixtures("refused")[0]), b[:len(b) // 3], b"\xff\xd8\xff"):
        with pytest.raises(ValueError) as host_err:
            hc.jpeg_parse(blob)
        with pytest.raises(ValueError) as pack_err:
            wide_pack(hc, blob, 2)
        assert str(pack_err.value) == str(host_err.value)

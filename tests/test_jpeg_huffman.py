"""The Huffman stage of K23 ``jpeg_huffman`` without a GPU: the stream pack
(``tcamd_host_jpeg_stream_pack``) and the host emulation of the kernel
(``tcamd_host_jpeg_huffman_emulate``, the kernel's own phases from
csrc/kernels/jpeg_huff_core.h run thread by thread) against the Python twin of
tests/jpeg_huff_cases.py and the host entropy decoder.  The kernel itself is
compared with the host decoder in tests/test_jpeg_huffman_gpu.py; untrusted
bytes are explored by csrc/cpp/tests/jpeg_stream_test.cc under sanitizers."""

import struct

import numpy as np
import pytest

from tests import jpeg_cases as jc
from tests import jpeg_huff_cases as jh

FIXTURES = jh.decodable()
NAMES = [n for n, _ in FIXTURES]

# subsequences and sync rounds of every fixture at S = 128 bytes (kSubBits = 1024): a round is one
# barrier interval in which at least one subsequence is decoded, the first (all from their own
# first bit) included.  f11 (q100 noise) is the near-serial case: no small cap on the rounds works.
ROUNDS = {
    "f01_16x16_444_q90": (1, 1),
    "f02_17x23_420_q75": (1, 1),
    "f03_40x50_422_q85": (5, 2),
    "f04_33x47_grey_q80": (2, 2),
    "f05_64x48_420_q60_rst2": (6, 1),
    "f06_48x40_420_rstrow": (3, 1),
    "f07_37x29_420_q95_opt": (4, 3),
    "f08_1x1_420": (1, 1),
    "f09_8x8_444_q100": (1, 1),
    "f10_9x70_422_q30": (1, 1),
    "f11_32x40_444_q100_noise": (41, 27),
    "t01_65x24_420": (3, 2),
    "t02_40x33_420": (3, 2),
    "t03_65x24_444": (4, 2),
    "t04_40x33_444": (3, 2),
    "b01_640x480_420_q75": (343, 6),
}


@pytest.fixture(scope="module")
def hc():
    from triton_client_amd.ops import host_codec

    return host_codec.load()


def aligned(n, fill=0):
    a = np.full(n + 16, fill, dtype=np.uint8)
    o = -a.ctypes.data % 16
    return a[o:o + n]


def host_pack(hc, blob, cap=None):
    """(parse, the stream buffer as a uint8 array, or None when not packable)."""
    buf = aligned(hc.jpeg_stream_bound(len(blob)) if cap is None else cap, 0xEE)
    info, used = hc.jpeg_stream_pack(blob, buf)
    return info, (None if used is None else buf[:used])


def host_coefficients(hc, blob):
    info = hc.jpeg_parse(blob)
    out = aligned(info.coef_bytes)
    hc.jpeg_entropy_decode(blob, out)
    return out


@pytest.fixture(scope="module")
def twin():
    """Per fixture the twin's (coefficient bytes, rounds, subsequences, stream buffer), computed once."""
    out = {}
    for name, blob in FIXTURES:
        coefs, rounds, nsub = jh.decode(blob)
        assert coefs is not None, name
        out[name] = (jc.coefficient_buffer(jc.parse(blob), coefs), rounds, nsub, jh.pack(blob))
    return out


@pytest.mark.parametrize("name,blob", FIXTURES, ids=NAMES)
def test_twin_pack_and_emulation_agree_with_the_reference_and_the_host(hc, twin, name, blob):
    info = jc.parse(blob)
    want = jc.coefficient_buffer(info, jc.entropy_decode(info))
    coefs, _, _, packed = twin[name]
    assert coefs == want  # the subsequence algorithm, in Python
    pinfo, stream = host_pack(hc, blob)
    assert stream is not None and packed is not None  # no fallback on a fixture
    assert stream.tobytes() == packed  # the pack, byte for byte
    got = aligned(pinfo.coef_bytes, 0x5A)
    status, _ = hc.jpeg_huffman_emulate(stream, got)
    assert status == 0  # no fallback on a fixture
    assert got.tobytes() == host_coefficients(hc, blob).tobytes() == want


def test_round_counts(hc, twin):
    seen = {}
    for name, blob in FIXTURES:
        _, stream = host_pack(hc, blob)
        nsub = int(stream[:64].view("<u4")[11])
        _, rounds = hc.jpeg_huffman_emulate(stream, aligned(hc.jpeg_parse(blob).coef_bytes))
        assert (nsub, rounds) == (twin[name][2], twin[name][1]), name  # the twin takes the same rounds
        seen[name] = (nsub, rounds)
    print("subsequences, rounds:", seen)
    assert {k: v for k, v in seen.items() if k in ROUNDS} == ROUNDS
    new = {k: v for k, v in seen.items() if k not in ROUNDS}
    # the jpeg_huff fixtures: about a hundred subsequences or more of dense data per sampling, more
    # blocks than a hundred in one subsequence of the flat image, intervals longer than a subsequence
    assert new == HUFF_ROUNDS


HUFF_ROUNDS = {
    "h01_256x256_420_flat": (9, 2),
    "h02_200x200_grey_q90_noise": (246, 12),
    "h03_128x128_422_q90_noise": (153, 12),
    "h04_128x128_444_q90_noise": (240, 20),
    "h05_160x120_420_q90_rst7": (142, 10),
}


def test_the_new_fixtures_are_what_they_are_for(hc):
    _, stream = host_pack(hc, jh.blob("h01"))
    # 1536 blocks in 9 subsequences: EOB-only blocks, well over a hundred per subsequence
    assert 6 * 256 / int(stream[:64].view("<u4")[11]) > 100
    _, stream = host_pack(hc, jh.blob("h05"))
    head = stream[:64].view("<u4")
    nseg, ntab = int(head[10]), int(head[12])
    mcux = int(head[7])
    assert int(head[9]) == 7 and nseg == 12 and mcux == 10 and mcux % int(head[9])  # intervals cut MCU rows; RSTn wraps
    segs = stream[448 + 1416 * ntab:][:16 * nseg].view("<u4").reshape(nseg, 4)
    assert (segs[:-1, 1] > jh.SUB_BITS).all()  # every full interval is longer than a subsequence


# -- refusals: the pack declines, the host route gives today's answer -------------------------
def _scan_start(b):
    i = b.index(b"\xff\xda")
    return i + 2 + ((b[i + 2] << 8) | b[i + 3])


def _misnumbered_rst(b):
    i = b.index(b"\xff\xd1", _scan_start(b))
    return b[:i + 1] + b"\xd3" + b[i + 2:]


def _surplus_rst(b):
    i = b.rindex(b"\xff\xd9")
    return b[:i] + b"\xff\xd5" + b[i:]


def _one_block_intervals(cols):
    """A flat grey JPEG of 2 x cols blocks with DRI 1: restart intervals of one
    block each, DC difference 0 and EOB ('00' '1010', padded with ones: 0x2B)
    in the standard tables of the grey fixture."""
    n = 2 * cols
    b = jh.blob("f04")
    i = b.index(b"\xff\xc0")
    sof = bytearray(b[i:i + 2 + ((b[i + 2] << 8) | b[i + 3])])
    sof[5:9] = struct.pack(">HH", 16, 8 * cols)
    s = b.index(b"\xff\xda")
    scan = b"".join(b"\x2b" + (bytes([0xFF, 0xD0 + (k & 7)]) if k + 1 < n else b"") for k in range(n))
    dri = b"\xff\xdd\x00\x04\x00\x01"
    return b[:i] + bytes(sof) + b[i + len(sof):s] + dri + b[s:_scan_start(b)] + scan + b"\xff\xd9"


def test_misnumbered_and_surplus_rst_are_declined(hc):
    b = jh.blob("f05")
    _, stream = host_pack(hc, _misnumbered_rst(b))
    assert stream is None
    with pytest.raises(ValueError, match="^malformed JPEG: missing or wrong RSTn"):
        host_coefficients(hc, _misnumbered_rst(b))
    _, stream = host_pack(hc, _surplus_rst(b))
    assert stream is None
    assert host_coefficients(hc, _surplus_rst(b)).tobytes() == host_coefficients(hc, b).tobytes()


# what may follow the scan of f01 once its EOI is cut off: (tail, packable, the host decoder's error)
TAILS = [
    (b"\xff\xd9", True, None),
    (b"", True, None),
    (b"\xff", True, None),
    (b"\xff\xff\xff\xd9", True, None),  # fill before the marker
    (b"\xff\xe0\x00\x02\xff\xda\x00\x02\xff\xd9", True, None),  # the host looks no further than the first marker
    (b"\xff\xda\x00\x02\xff\xd9", False, "unsupported JPEG: multi-scan"),
    (b"\xff\xdc\x00\x04\x00\x10\xff\xd9", False, "unsupported JPEG: DNL"),
    # fill, then 00: the data ends at the fill, but the host's look for another scan reads on
    (b"\xff\xff\x00\xff\xda\x00\x02\xff\xd9", False, "unsupported JPEG: multi-scan"),
    (b"\xff\xff\x00\xff\xdc\x00\x04\x00\x10\xff\xd9", False, "unsupported JPEG: DNL"),
    (b"\xff\xff\xff\x00\x12\xff\xd9", False, None),
    (b"\xff\xd3\xff\xd9", False, None),  # an RSTn without DRI
]


@pytest.mark.parametrize("tail,packable,error", TAILS, ids=[t[0].hex() or "nothing" for t in TAILS])
def test_what_follows_the_scan(hc, tail, packable, error):
    """The pack takes a blob only where the host decoder's look past the scan
    sees what the pack saw; then the emulation and the host agree.  Declined
    blobs get the host's answer, an image or its error."""
    b = jh.blob("f01")
    assert b.endswith(b"\xff\xd9")
    blob = b[:-2] + tail
    _, stream = host_pack(hc, blob)
    assert (stream is not None) == packable
    assert (jh.pack(blob) is not None) == packable  # the twin, from the reference decoder's reading
    if error:
        with pytest.raises(ValueError) as err:
            host_coefficients(hc, blob)
        assert str(err.value) == error
        with pytest.raises(ValueError) as ref_err:
            jc.decode(blob)
        assert str(ref_err.value) == error
    else:
        want = host_coefficients(hc, blob)
        assert want.tobytes() == host_coefficients(hc, b).tobytes()
        if packable:
            assert stream.tobytes() == jh.pack(blob)
            got = aligned(len(want), 0x5A)
            assert hc.jpeg_huffman_emulate(stream, got)[0] == 0 and got.tobytes() == want.tobytes()


def test_fill_then_zero_between_intervals_is_declined(hc):
    b = jh.blob("f05")
    i = b.index(b"\xff\xd0", _scan_start(b))
    blob = b[:i] + b"\xff\xff\x00" + b[i:]
    assert host_pack(hc, blob)[1] is None and jh.pack(blob) is None
    with pytest.raises(ValueError, match="^malformed JPEG: missing or wrong RSTn"):
        host_coefficients(hc, blob)
    blob = b[:i] + b"\xff\xff" + b[i:]  # fill alone is what a restart accepts
    _, stream = host_pack(hc, blob)
    assert stream is not None and stream.tobytes() == jh.pack(blob) == host_pack(hc, b)[1].tobytes()
    assert host_coefficients(hc, blob).tobytes() == host_coefficients(hc, b).tobytes()


def test_a_misaligned_buffer_is_declined(hc):
    b = jh.blob("f01")
    buf = aligned(hc.jpeg_stream_bound(len(b)) + 8, 0xEE)
    info, used = hc.jpeg_stream_pack(b, buf[8:])
    assert used is None and info.shape == (16, 16, 3) and (buf == 0xEE).all()


def test_a_stream_above_the_workspace_is_declined(hc):
    fits, above = _one_block_intervals(jh.MAX_SUB // 2), _one_block_intervals(jh.MAX_SUB // 2 + 1)
    info, stream = host_pack(hc, fits)
    assert stream is not None and int(stream[:64].view("<u4")[11]) == jh.MAX_SUB
    got = aligned(info.coef_bytes, 0x5A)
    assert hc.jpeg_huffman_emulate(stream, got)[0] == 0
    assert got.tobytes() == host_coefficients(hc, fits).tobytes()
    _, stream = host_pack(hc, above)
    assert stream is None
    px = hc.jpeg_decode(above)  # today's answer: a flat image
    assert px.shape == (16, 8 * (jh.MAX_SUB // 2 + 1), 1) and (px == px[0, 0, 0]).all()


def test_a_buffer_too_small_is_declined_and_nothing_past_it_is_written(hc):
    b = jh.blob("b01")
    _, whole = host_pack(hc, b)
    for cap in (0, 64, 6000, len(whole) - 1):
        buf = aligned(cap + 64, 0xEE)
        info, used = hc.jpeg_stream_pack(b, buf[:cap])
        assert used is None and info.shape == (480, 640, 3)
        assert (buf[cap:] == 0xEE).all()


def test_progressive_and_malformed_blobs_raise_as_the_host_route_does(hc):
    b = jh.blob("f05")
    bad = [jc.blob(jc.fixtures("refused")[0]), b[:len(b) // 3], b"\xff\xd8\xff", b[:2] + b"\x00" + b[3:]]
    for blob in bad:
        with pytest.raises(ValueError) as host_err:
            hc.jpeg_parse(blob)
        with pytest.raises(ValueError) as pack_err:
            host_pack(hc, blob)
        assert str(pack_err.value) == str(host_err.value)
    # broken inside the scan: packable or not, the answer is the host decoder's
    cut = b[:_scan_start(b) + 40]
    _, stream = host_pack(hc, cut)
    assert stream is None  # the RSTn markers that should follow are missing
    with pytest.raises(ValueError, match="^malformed JPEG: "):
        host_coefficients(hc, cut)


def test_the_emulation_rejects_a_stream_buffer_that_does_not_hold(hc):
    b = jh.blob("f05")
    info, stream = host_pack(hc, b)
    for word, value in ((0, 0), (2, 0), (4, 2), (9, 0), (10, 7), (11, 4096), (12, 7), (13, 0x77), (14, 4)):
        bad = aligned(len(stream))
        bad[:] = stream
        bad[:64].view("<u4")[word] = value
        got = aligned(info.coef_bytes, 0x5A)
        assert hc.jpeg_huffman_emulate(bad, got)[0] == 1, word  # kBadHeader
    ntab = int(stream[:64].view("<u4")[12])
    # a lookup entry of length 0 (the pack writes none) would be a symbol that consumes no bit
    bad = aligned(len(stream))
    bad[:] = stream
    bad[448 + 1416:][:1024].view("<u2")[:] = 0x0000 | 0x00F0  # the first AC table: every short code a ZRL of length 0
    assert hc.jpeg_huffman_emulate(bad, aligned(info.coef_bytes))[0] == 2  # kBadCode
    for field, value in ((0, 2), (1, 1 << 20), (2, 1), (3, 9)):  # segment 1: offset, bits, first MCU, first subsequence
        bad = aligned(len(stream))
        bad[:] = stream
        bad[448 + 1416 * ntab + 16:][:16].view("<u4")[field] = value
        assert hc.jpeg_huffman_emulate(bad, aligned(info.coef_bytes))[0] == 1, field

"""The PNG contract in Python: a reference decoder written from the standard
(independently of csrc/host/png.cc and csrc/kernels/png_math.h), a PNG writer
that can force what an imaging library chooses by itself (the filter of every
row, the IDAT split, Adam7, a short PLTE), and the case lists of the PNG tests.
Needs ``zlib`` and numpy only.

Output contract: uint8 HWC, C = 1 for colour types 0 and 4, C = 3 for 2, 3 and
6; a 16-bit sample gives its high byte; grey of depth 1 / 2 / 4 is multiplied
by 255 / 85 / 17; a palette index reads its PLTE entry, (0, 0, 0) past the end
of PLTE; alpha is dropped.
"""

import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
FILE_CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
OUT_CHANNELS = {0: 1, 2: 3, 3: 3, 4: 1, 6: 3}
PAIRS = [(0, 1), (0, 2), (0, 4), (0, 8), (0, 16), (2, 8), (2, 16), (3, 1), (3, 2), (3, 4), (3, 8), (4, 8), (4, 16),
         (6, 8), (6, 16)]
ADAM7 = [(0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2)]  # x0 y0 dx dy


def row_bytes(w, ctype, depth):
    return (w * FILE_CHANNELS[ctype] * depth + 7) // 8


def filter_bpp(ctype, depth):
    return max(1, FILE_CHANNELS[ctype] * depth // 8)


def chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xffffffff)


def chunks(blob):
    """[(type, data offset, data length)] of a well-formed file."""
    out, pos = [], 8
    while pos < len(blob):
        n = struct.unpack_from(">I", blob, pos)[0]
        out.append((blob[pos + 4:pos + 8], pos + 8, n))
        pos += 12 + n
    return out


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    if pa <= pb and pa <= pc:
        return a
    return b if pb <= pc else c


def filter_rows(raw, bpp, schedule):
    """Filter the scanlines ``raw`` (uint8 [h, row_bytes]) with filter type
    ``schedule[y % len(schedule)]`` on row y -> the bytes a PNG deflates."""
    h, rb = raw.shape
    out = bytearray()
    zero = np.zeros(rb, dtype=np.int32)
    for y in range(h):
        ft = schedule[y % len(schedule)]
        cur = raw[y].astype(np.int32)
        up = raw[y - 1].astype(np.int32) if y else zero
        left = np.concatenate([zero[:bpp], cur[:-bpp]]) if rb > bpp else zero[:rb] * 0
        upleft = np.concatenate([zero[:bpp], up[:-bpp]]) if rb > bpp else zero[:rb] * 0
        if ft == 0:
            pred = zero
        elif ft == 1:
            pred = left
        elif ft == 2:
            pred = up
        elif ft == 3:
            pred = (left + up) >> 1
        else:
            pred = np.array([_paeth(int(a), int(b), int(c)) for a, b, c in zip(left, up, upleft)], dtype=np.int32)
        out.append(ft)
        out += ((cur - pred) & 0xff).astype(np.uint8).tobytes()
    return bytes(out)


def pack_samples(samples, depth):
    """Samples [h, w, file channels] (values below 2 ** depth) -> scanlines uint8 [h, row_bytes]."""
    h, w, c = samples.shape
    flat = samples.reshape(h, w * c).astype(np.uint32)
    if depth == 16:
        return np.stack([flat >> 8, flat & 0xff], axis=2).reshape(h, -1).astype(np.uint8)
    if depth == 8:
        return flat.astype(np.uint8)
    per = 8 // depth
    pad = (-flat.shape[1]) % per
    flat = np.concatenate([flat, np.zeros((h, pad), dtype=np.uint32)], axis=1).reshape(h, -1, per)
    shifts = np.array([8 - depth * (k + 1) for k in range(per)], dtype=np.uint32)
    return (flat << shifts).sum(axis=2).astype(np.uint8)


def write_png(samples, ctype, depth, schedule=(0,), idat_splits=1, adam7=False, palette=None, split_at=None,
              level=6, extra=()):
    """A PNG file of ``samples`` (integer array [h, w, file channels] or [h, w]
    for one channel, values below ``2 ** depth``).  ``schedule``: the filter
    types, cycled over the rows (of every Adam7 sub-image on its own).
    ``idat_splits``: the number of IDAT chunks of about equal size, or
    ``split_at``: the byte offsets of the zlib stream at which a new chunk
    starts.  ``palette``: uint8 [n, 3] for colour type 3, n <= 256 and possibly
    fewer than the indices used.  ``extra``: ``(type, data)`` ancillary chunks
    put before the first IDAT."""
    samples = np.asarray(samples)
    if samples.ndim == 2:
        samples = samples[:, :, None]
    h, w, c = samples.shape
    assert c == FILE_CHANNELS[ctype]
    bpp = filter_bpp(ctype, depth)
    if adam7:
        filt = b""
        for x0, y0, dx, dy in ADAM7:
            sub = samples[y0::dy, x0::dx]
            if sub.shape[0] and sub.shape[1]:
                filt += filter_rows(pack_samples(sub, depth), bpp, schedule)
    else:
        filt = filter_rows(pack_samples(samples, depth), bpp, schedule)
    stream = zlib.compress(filt, level)
    if split_at is None:
        n = max(1, int(idat_splits))
        split_at = [len(stream) * i // n for i in range(1, n)]
    cuts = [0] + list(split_at) + [len(stream)]
    out = SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, 1 if adam7 else 0))
    if palette is not None:
        out += chunk(b"PLTE", np.asarray(palette, dtype=np.uint8).tobytes())
    for kind, data in extra:
        out += chunk(kind, data)
    for a, b in zip(cuts[:-1], cuts[1:]):
        out += chunk(b"IDAT", stream[a:b])
    return out + chunk(b"IEND", b"")


def _unfilter(filt, h, rb, bpp):
    """Filtered bytes of h scanlines -> uint8 [h, rb], byte by byte as the standard states it."""
    out = np.zeros((h, rb), dtype=np.uint8)
    prev = [0] * rb
    pos = 0
    for y in range(h):
        ft = filt[pos]
        assert ft <= 4
        line = filt[pos + 1:pos + 1 + rb]
        pos += 1 + rb
        cur = [0] * rb
        for i in range(rb):
            a = cur[i - bpp] if i >= bpp else 0
            b = prev[i]
            c = prev[i - bpp] if i >= bpp else 0
            pred = (0, a, b, (a + b) // 2, _paeth(a, b, c))[ft]
            cur[i] = (line[i] + pred) & 0xff
        out[y] = cur
        prev = cur
    return out


def _to_pixels(lines, w, ctype, depth, palette):
    """Reconstructed scanlines uint8 [h, rb] -> the contract's uint8 [h, w, C]."""
    h = lines.shape[0]
    c = FILE_CHANNELS[ctype]
    if depth == 16:
        s = lines.reshape(h, w * c, 2)[:, :, 0]
    elif depth == 8:
        s = lines[:, :w * c]
    else:
        per = 8 // depth
        shifts = np.array([8 - depth * (k + 1) for k in range(per)], dtype=np.uint8)
        s = ((lines[:, :, None] >> shifts) & ((1 << depth) - 1)).reshape(h, -1)[:, :w]
    s = s.reshape(h, w, c)
    if ctype == 3:
        pal = np.zeros((256, 3), dtype=np.uint8)
        pal[:len(palette)] = palette
        return pal[s[:, :, 0]]
    if ctype == 0 and depth < 8:
        return (s * (255 // ((1 << depth) - 1))).astype(np.uint8)
    return np.ascontiguousarray(s[:, :, :OUT_CHANNELS[ctype]]).astype(np.uint8)


def decode(blob):
    """The reference decode of a well-formed PNG -> uint8 [h, w, 1 or 3]."""
    assert blob[:8] == SIGNATURE
    w = h = depth = ctype = lace = None
    palette, stream = None, b""
    for kind, at, n in chunks(blob):
        data = blob[at:at + n]
        if kind == b"IHDR":
            w, h, depth, ctype, _, _, lace = struct.unpack(">IIBBBBB", data)
        elif kind == b"PLTE":
            palette = np.frombuffer(data, dtype=np.uint8).reshape(-1, 3)
        elif kind == b"IDAT":
            stream += data
    filt = zlib.decompress(stream)
    bpp = filter_bpp(ctype, depth)
    if not lace:
        rb = row_bytes(w, ctype, depth)
        assert len(filt) == h * (1 + rb)
        return _to_pixels(_unfilter(filt, h, rb, bpp), w, ctype, depth, palette)
    out = np.zeros((h, w, OUT_CHANNELS[ctype]), dtype=np.uint8)
    pos = 0
    for x0, y0, dx, dy in ADAM7:
        pw, ph = len(range(x0, w, dx)), len(range(y0, h, dy))
        if not pw or not ph:
            continue
        rb = row_bytes(pw, ctype, depth)
        out[y0::dy, x0::dx] = _to_pixels(_unfilter(filt[pos:pos + ph * (1 + rb)], ph, rb, bpp), pw, ctype, depth, palette)
        pos += ph * (1 + rb)
    assert pos == len(filt)
    return out


def samples_for(ctype, depth, h, w, seed=0):
    """Deterministic samples [h, w, file channels]: smooth ramps plus noise, so
    that every filter has something to predict and something to miss."""
    rng = np.random.default_rng(1000 * ctype + 10 * depth + seed + 7 * h + 13 * w)
    c = FILE_CHANNELS[ctype]
    top = (1 << depth) - 1
    y, x = np.mgrid[0:h, 0:w]
    base = ((x * 5 + y * 3)[:, :, None] * (np.arange(c) + 1) * max(1, top // 64)) % (top + 1)
    noise = rng.integers(0, top + 1, size=(h, w, c))
    pick = rng.random((h, w, 1)) < 0.3
    return np.where(pick, noise, base).astype(np.uint32)


def palette_for(n, seed=0):
    return np.random.default_rng(seed + n).integers(0, 256, size=(n, 3)).astype(np.uint8)


def make(ctype, depth, h, w, schedule=(0,), seed=0, palette_entries=None, **kw):
    """``write_png`` of :func:`samples_for`; colour type 3 gets a palette of
    ``palette_entries`` colours (default: all ``2 ** depth``)."""
    pal = None
    if ctype == 3:
        pal = palette_for((1 << depth) if palette_entries is None else palette_entries, seed)
    return write_png(samples_for(ctype, depth, h, w, seed), ctype, depth, schedule, palette=pal, **kw)


CYCLE = (4, 3, 2, 1, 0, 4, 4, 3)
# each filter on every row; each as the first row only (the rest None ... and the rest Paeth, so the
# first row is what the next rows predict from); a schedule cycling all five
SCHEDULES = [(f,) for f in range(5)] + [(f,) + (0,) * 63 for f in range(1, 5)] + [(f,) + (4,) * 63 for f in range(4)] \
    + [CYCLE]
LOW_WIDTHS = (1, 2, 7, 8, 9)
ADAM7_SIZES = [(h, w) for h in range(1, 10) for w in range(1, 10) if (h, w) in
               {(1, 1), (1, 2), (2, 1), (2, 2), (3, 3), (1, 9), (9, 1), (4, 5), (5, 4), (8, 8), (9, 9), (5, 8), (8, 3)}]


def host_cases():
    """``[(name, blob)]``: the matrix of tests/test_png_host.py."""
    out = []
    for ctype, depth in PAIRS:
        for sch in SCHEDULES:
            out.append(("t%dd%d_f%s" % (ctype, depth, "".join(map(str, sch[:8]))), make(ctype, depth, 6, 11, sch)))
        if depth < 8:
            for w in LOW_WIDTHS:
                out.append(("t%dd%d_w%d" % (ctype, depth, w), make(ctype, depth, 5, w, CYCLE)))
        out.append(("t%dd%d_1x1" % (ctype, depth), make(ctype, depth, 1, 1, (4,))))
        out.append(("t%dd%d_1xN" % (ctype, depth), make(ctype, depth, 1, 13, (3,))))
        out.append(("t%dd%d_Nx1" % (ctype, depth), make(ctype, depth, 13, 1, CYCLE)))
    for n in (1, 2, 17):
        out.append(("idat%d" % n, make(2, 8, 9, 13, CYCLE, idat_splits=n)))
    out.append(("idat_split_in_zlib_header", make(2, 8, 9, 13, CYCLE, split_at=[1])))
    out.append(("idat_with_an_empty_chunk", make(6, 8, 9, 13, CYCLE, split_at=[0, 5, 5])))
    out.append(("ancillary_chunks", make(6, 8, 4, 4, CYCLE, extra=[(b"gAMA", struct.pack(">I", 45455)),
                                                                    (b"tRNS", b"\x00\x01"), (b"tEXt", b"k\x00v")])))
    for ctype, depth in PAIRS:
        for h, w in ADAM7_SIZES:
            out.append(("adam7_t%dd%d_%dx%d" % (ctype, depth, h, w), make(ctype, depth, h, w, CYCLE, adam7=True)))
    out.append(("adam7_larger", make(2, 8, 37, 29, CYCLE, adam7=True, idat_splits=3)))
    out.append(("adam7_larger_low", make(3, 2, 33, 35, CYCLE, adam7=True)))
    for depth in (1, 2, 4, 8):
        out.append(("short_plte_d%d" % depth, make(3, depth, 7, 9, CYCLE, palette_entries=max(1, (1 << depth) // 2 - 1))))
    return out

"""A Python twin of the stream pack (``tcamd_host_jpeg_stream_pack``,
csrc/host/jpeg.cc) and of the subsequence algorithm of K23 ``jpeg_huffman``
(csrc/kernels/jpeg_huff_core.h), and the fixture list of tests/golden/jpeg_huff.
Written from the documented layout and algorithm with the parser and the
bit-by-bit Huffman tables of tests/jpeg_cases.py, not from the C++: the pack
must produce the same bytes, the algorithm the coefficients of
``jpeg_cases.entropy_decode``.

The stream buffer (little endian):

* header, 16 uint32: magic "JTS1", total bytes, h, w, ncomp, hs, vs, mcux, mcuy,
  MCUs per segment (DRI, or all MCUs), segments, subsequences, tables, table
  map (component c: DC table index in bits [8c, 8c+4), AC in [8c+4, 8c+8)),
  data bytes, 0;
* uint16 q[3][64], natural order, unused components zero;
* the distinct Huffman tables in order of first use (component 0 DC, AC,
  component 1 DC, ...), each ``uint16 look[512]`` (9 leading bits -> length << 8
  | symbol, 0 for longer codes), ``int32 maxcode[17]``, ``int32 valoff[17]``
  (entry 0 of both zero), ``uint8 vals[256]`` (zero past the last symbol);
* per segment 4 uint32: byte offset in the data, bits, first MCU, first
  subsequence;
* the data from the next 16-byte boundary: each segment's bytes without FF 00
  stuffing from a 4-byte boundary, zeros between, the whole rounded up to 16
  bytes plus 16 zero bytes.
"""

import json
import os
import struct

import numpy as np

from tests import jpeg_cases as jc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_huff")

SUB_BITS = 1024  # kSubBits
MAX_SUB = 2048   # kMaxSub
MAGIC = 0x3153544A
NOT_PACKABLE = None


def manifest():
    with open(os.path.join(GOLDEN, "manifest.json")) as f:
        return json.load(f)


def decodable():
    """(name, blob) of every decodable fixture, tests/golden/jpeg and jpeg_huff."""
    out = [(e["name"], jc.blob(e)) for e in jc.decodable()]
    for e in manifest()["fixtures"]:
        with open(os.path.join(GOLDEN, e["name"] + ".jpg"), "rb") as f:
            out.append((e["name"], f.read()))
    return out


def blob(prefix):
    return next(b for n, b in decodable() if n.startswith(prefix))


def subs_of(bits):
    return max(1, -(-bits // SUB_BITS))


# ---- the scan, cut the way the reference decoder reads it -----------------------------------
def _data_end(d, p):
    """Where ``jpeg_cases._Bits`` stops reading entropy-coded bytes from ``p``: the
    first FF that no 00 follows, or the end of the blob."""
    while True:
        p = d.find(b"\xff", p)
        if p < 0:
            return len(d)
        if p + 1 < len(d) and d[p + 1] == 0:
            p += 2
            continue
        return p


def _next_marker(d, p):
    """The index of the first FF xx from ``p`` with xx neither 00 nor FF, as the
    loop at the end of ``jpeg_cases.entropy_decode`` finds it, or None."""
    while p + 1 < len(d):
        if d[p] == 0xFF and d[p + 1] not in (0x00, 0xFF):
            return p
        p += 1
    return None


def segments(info):
    """(the unstuffed bytes of every restart interval, MCUs per interval), or
    None unless the scan is plain in the reference decoder's own terms: between
    two intervals exactly what ``_Bits.restart`` accepts (FF fill, then the RSTn
    whose turn it is); after the last interval the marker that the decoder's
    look for another scan finds first stands right behind the data, FF fill
    alone between them (so that look cannot read on into anything the pack
    dropped), and is no RSTn, SOS or DNL; or nothing but FF up to the blob's end."""
    d, p = info["data"], info["pos"]
    _, _, mcux, mcuy = jc.geometry(info)
    mcus = mcux * mcuy
    interval = info["dri"] if 0 < info["dri"] < mcus else mcus
    nseg = -(-mcus // interval)
    segs = []
    for k in range(nseg):
        end = _data_end(d, p)
        segs.append(d[p:end].replace(b"\xff\x00", b"\xff"))
        if k + 1 < nseg:
            q = end
            while q < len(d) and d[q] == 0xFF:  # _Bits.restart
                q += 1
            if q == end or q >= len(d) or d[q] != 0xD0 + (k & 7):
                return None
            p = q + 1
    m = _next_marker(d, end)
    tail = d[end:] if m is None else d[end:m]
    if tail.strip(b"\xff"):
        return None  # something other than fill between the data and the next marker
    if m is not None and (0xD0 <= d[m + 1] <= 0xD7 or d[m + 1] in (0xDA, 0xDC)):
        return None
    return segs, interval


def huff_table(table):
    """The lookup form of a {(length, code): symbol} table, as bytes."""
    look = np.zeros(512, dtype="<u2")
    maxcode = np.zeros(17, dtype="<i4")
    valoff = np.zeros(17, dtype="<i4")
    vals = np.zeros(256, dtype=np.uint8)
    code = k = 0
    for length in range(1, 17):
        codes = sorted(c for (n, c) in table if n == length)
        assert codes == list(range(code, code + len(codes)))  # canonical
        valoff[length] = k - code
        for c in codes:
            vals[k] = table[(length, c)]
            if length <= 9:
                look[c << (9 - length):(c + 1) << (9 - length)] = (length << 8) | int(vals[k])
            k += 1
        code += len(codes)
        maxcode[length] = code - 1 if codes else -1
        code <<= 1
    return look.tobytes() + maxcode.tobytes() + valoff.tobytes() + vals.tobytes()


def pack(data):
    """The stream buffer of a blob as bytes, or None when it is not packable."""
    info = jc.parse(data)
    cut = segments(info)
    if cut is None:
        return None
    segs, interval = cut
    hmax, vmax, mcux, mcuy = jc.geometry(info)
    comps = info["comps"]
    tabs, tabmap = [], 0
    for c, (_, _, _, _, td, ta) in enumerate(comps):
        for cls, t in ((0, td), (1, ta)):
            if (cls, t) not in tabs:
                tabs.append((cls, t))
            tabmap |= tabs.index((cls, t)) << (8 * c + 4 * cls)
    seg_table, body, nsub = b"", bytearray(), 0
    for k, s in enumerate(segs):
        if len(s) > MAX_SUB * SUB_BITS // 8:
            return None
        seg_table += struct.pack("<4I", len(body), 8 * len(s), k * interval, nsub)
        nsub += subs_of(8 * len(s))
        body += s + bytes(-len(s) % 4)
    if nsub > MAX_SUB:
        return None
    body += bytes(-len(body) % 16) + bytes(16)
    q = np.zeros((3, 64), dtype="<u2")
    for c, comp in enumerate(comps):
        q[c] = info["qt"][comp[3]]
    head = q.tobytes() + b"".join(huff_table(info["huff"][t]) for t in tabs) + seg_table
    head += bytes(-(64 + len(head)) % 16)
    total = 64 + len(head) + len(body)
    header = struct.pack("<2I7i7I", MAGIC, total, info["H"], info["W"], len(comps), hmax, vmax, mcux, mcuy, interval,
                         len(segs), nsub, len(tabs), tabmap, len(body), 0)
    return header + head + bytes(body)


# ---- the subsequence algorithm ---------------------------------------------------------------
class Invalid(Exception):
    pass


class _Image:
    def __init__(self, info):
        self.info = info
        self.comps = info["comps"]
        self.hmax, self.vmax, self.mcux, self.mcuy = jc.geometry(info)
        # the blocks of an MCU in scan order: (component, bx, by)
        self.mcu_blocks = [(ci, bx, by) for ci, (_, h, v, _, _, _) in enumerate(self.comps)
                           for by in range(v) for bx in range(h)]
        self.bpm = len(self.mcu_blocks)


def _decode(img, seg, pos, state, stop, budget, emit):
    """From bit ``pos`` of the segment's bytes ``seg`` in ``state`` (block in
    the MCU, zigzag index) whole symbols until ``pos >= stop`` or ``budget``
    blocks are complete.  Returns (pos, state, blocks done); Invalid for bad
    data, bits past the segment's end included."""
    limit = 8 * len(seg)

    def bits(p, n):  # n <= 16 bits from p; past the end: Invalid
        if p + n > limit:
            raise Invalid("data ends early")
        v = int.from_bytes(seg[p >> 3:(p >> 3) + 3], "big") << (8 * max(0, (p >> 3) + 3 - len(seg)))
        return (v >> (24 - (p & 7) - n)) & ((1 << n) - 1)

    def symbol(p, table):
        # a code that needs a bit past the end is invalid, whatever that bit would read as
        v = bits(p, min(16, limit - p)) << max(0, 16 - (limit - p))
        for length in range(1, min(16, limit - p) + 1):
            s = table.get((length, v >> (16 - length)))
            if s is not None:
                return s, length
        raise Invalid("bad code or data ends early")

    def extend(v, s):
        return v if s == 0 or v >= (1 << (s - 1)) else v - (1 << s) + 1

    blk, zz = state
    done = 0
    huff = img.info["huff"]
    while pos < stop and done < budget:
        ci = img.mcu_blocks[blk][0]
        td, ta = img.comps[ci][4], img.comps[ci][5]
        complete = False
        if zz == 0:
            s, n = symbol(pos, huff[(0, td)])
            if s > 11:
                raise Invalid("DC category")
            emit(done, blk, 0, extend(bits(pos + n, s), s))
            pos += n + s
            zz = 1
        else:
            rs, n = symbol(pos, huff[(1, ta)])
            r, s = rs >> 4, rs & 15
            if s == 0:
                pos += n
                if r != 15:
                    complete = True
                else:
                    zz += 16
                    if zz > 64:
                        raise Invalid("run")
                    complete = zz == 64
            else:
                if s > 10:
                    raise Invalid("AC category")
                zz += r
                if zz > 63:
                    raise Invalid("run")
                emit(done, blk, zz, extend(bits(pos + n, s), s))
                pos += n + s
                zz += 1
                complete = zz == 64
        if complete:
            done += 1
            zz = 0
            blk = (blk + 1) % img.bpm
    return pos, (blk, zz), done


def decode(data):
    """The subsequence algorithm on a packable blob.  Returns (coefficients per
    component as jpeg_cases.entropy_decode gives them, or None when the data is
    invalid; sync rounds; subsequences)."""
    info = jc.parse(data)
    img = _Image(info)
    segs, interval = segments(info)
    mcus = img.mcux * img.mcuy
    rounds_max = 0
    out = [np.zeros((img.mcuy * c[2], img.mcux * c[1], 64), dtype=np.int16) for c in img.comps]
    ok = True
    nsub_all = 0
    for k, seg in enumerate(segs):
        limit = 8 * len(seg)
        n = subs_of(limit)
        nsub_all += n
        stops = [min((j + 1) * SUB_BITS, limit) for j in range(n)]
        entry = [(min(j * SUB_BITS, limit), (0, 0)) for j in range(n)]
        exits = [None] * n
        counts = [0] * n
        sums = [[0, 0, 0] for _ in range(n)]
        todo = list(range(n))
        rounds = 0
        while todo:
            rounds += 1
            for j in todo:
                acc = [0, 0, 0]

                def add(done, blk, zz, val, acc=acc):
                    if zz == 0:
                        acc[img.mcu_blocks[blk][0]] += val

                try:
                    pos, state, counts[j] = _decode(img, seg, entry[j][0], entry[j][1], stops[j], 1 << 30, add)
                    exits[j] = (pos, state)
                except Invalid:
                    exits[j], counts[j] = None, 0  # the count of an invalid subsequence is never used
                sums[j] = acc
            # the next round: whoever's predecessor now has another valid exit (read for all, then decode)
            todo = [j for j in range(1, n) if exits[j - 1] is not None and exits[j - 1] != entry[j]]
            for j in todo:
                entry[j] = exits[j - 1]
        rounds_max = max(rounds_max, rounds)
        # count and write
        blocks = min(interval, mcus - k * interval) * img.bpm
        first, pred = 0, [0, 0, 0]
        reached = False
        for j in range(n):
            if j and exits[j - 1] is None:
                break
            if first >= blocks:
                break
            p = list(pred)

            def store(done, blk, zz, val, first=first, p=p):
                b = first + done
                mcu = k * interval + b // img.bpm
                ci, bx, by = img.mcu_blocks[blk]
                my, mx = divmod(mcu, img.mcux)
                _, h, v = img.comps[ci][:3]
                if zz == 0:
                    p[ci] += val
                    if not -32768 <= p[ci] <= 32767:
                        raise Invalid("DC out of range")
                    val = p[ci]
                out[ci][my * v + by, mx * h + bx, jc.ZIGZAG[zz]] = val

            try:
                pos, _, done = _decode(img, seg, entry[j][0], entry[j][1], stops[j], blocks - first, store)
            except Invalid:
                ok = False
                break
            if first + done == blocks:
                reached = True
                if k + 1 < len(segs) and limit - pos >= 8:
                    ok = False
            first += counts[j]
            pred = [a + b for a, b in zip(pred, sums[j])]
        if not reached:
            ok = False
    return (out if ok else None), rounds_max, nsub_all

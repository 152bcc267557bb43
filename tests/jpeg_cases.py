"""numpy reference of the baseline JPEG decode that csrc/host/jpeg.cc (host) and
K22 ``jpeg_decode`` (csrc/kernels/jpeg.hip, device) implement, and the fixture
list of tests/golden/jpeg.  A complete, independent decoder: marker parse, a
bit-by-bit Huffman decode in Python, and the per-sample arithmetic below, which
the two native decoders must reproduce bit for bit.

The arithmetic contract, all in integers (``>>`` is an arithmetic shift):

1. dequantise: ``v = clamp(coef * Q, DEQ_MIN, DEQ_MAX)`` with the range
   [-2048, 2047].  The forward DCT of 8-bit samples is below 1024 in magnitude
   and quantisation adds at most Q/2, so a legitimate encoder never reaches the
   clamp; with it the largest intermediate below is
   ``2048 * 7.48 * 7.48 * 2**(PASS1_BITS + C2_BITS) < 2**31``
   (7.48 = the largest absolute column sum of the scaled basis).
2. 8x8 inverse DCT, separable, rows first: the basis
   ``b[u][x] = s(u) * cos((2x+1) u pi / 16)`` with ``s(0) = 1, s(u>0) = sqrt(2)``
   is the orthonormal one times sqrt(8) per pass, so the DC column is exactly
   a power of two.  ``M1 = round(b * 2**C1_BITS)``, ``M2 = round(b * 2**C2_BITS)``:
     row pass     ws[y][x]  = (sum_u M1[u][x] * v[y][u] + 2**(C1_BITS-PASS1_BITS-1)) >> (C1_BITS - PASS1_BITS)
     column pass  out[y][x] = (sum_v M2[v][y] * ws[v][x] + 2**(C2_BITS+PASS1_BITS+2)) >> (C2_BITS + PASS1_BITS + 3)
   A DC-only block gives ``(dc*Q + 4) >> 3`` everywhere.
3. level shift: ``clamp(out + 128, 0, 255)``.
4. chroma upsampling by the triangle filter over the valid chroma extent
   ``cw = ceil(W / hmax), ch = ceil(H / vmax)``, edges replicated there.
5. YCbCr -> RGB with 16 fractional bits (``ycc_to_rgb``).
"""

import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg")

DEQ_MIN, DEQ_MAX = -2048, 2047
C1_BITS, C2_BITS, PASS1_BITS = 13, 12, 2
MAX_DIM = 16384  # ops.hip.RESIZE_MAX_DIM

_BASIS = np.array([[(1.0 if u == 0 else np.sqrt(2.0)) * np.cos((2 * x + 1) * u * np.pi / 16) for x in range(8)]
                   for u in range(8)])
M1 = np.rint(_BASIS * (1 << C1_BITS)).astype(np.int64)
M2 = np.rint(_BASIS * (1 << C2_BITS)).astype(np.int64)

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13,
                   6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45,
                   38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])


def manifest():
    with open(os.path.join(GOLDEN, "manifest.json")) as f:
        return json.load(f)


def fixtures(kind=None):
    """Manifest entries (dicts with name, h, w, mode, kind ...); ``kind`` is
    "case", "tile", "bench" or "refused"."""
    return [e for e in manifest()["fixtures"] if kind is None or e["kind"] == kind]


def decodable():
    return [e for e in manifest()["fixtures"] if e["kind"] != "refused"]


def blob(entry):
    with open(os.path.join(GOLDEN, entry["name"] + ".jpg"), "rb") as f:
        return f.read()


def pillow_decode(entry):
    a = np.load(os.path.join(GOLDEN, entry["name"] + ".npy"))
    return a[:, :, None] if a.ndim == 2 else a


# ---- arithmetic -------------------------------------------------------------------
def dequantise(coef, q):
    return np.clip(coef.astype(np.int64) * q.astype(np.int64), DEQ_MIN, DEQ_MAX)


def idct(v):
    """[..., 8, 8] dequantised coefficients (row y, column u) -> samples before
    the level shift, int64."""
    v = np.asarray(v, dtype=np.int64)
    ws = (v @ M1 + (1 << (C1_BITS - PASS1_BITS - 1))) >> (C1_BITS - PASS1_BITS)
    out = np.swapaxes(np.swapaxes(ws, -1, -2) @ M2, -1, -2)
    assert np.abs(out).max(initial=0) < 2 ** 31
    return (out + (1 << (C2_BITS + PASS1_BITS + 2))) >> (C2_BITS + PASS1_BITS + 3)


def idct_float(v):
    """The float64 separable IDCT of the same coefficients."""
    b = _BASIS / np.sqrt(8.0)
    v = np.asarray(v, dtype=np.float64)
    return np.swapaxes(np.swapaxes(v @ b, -1, -2) @ b, -1, -2)


def _shift(p, d, axis):
    """p[i + d] along axis with the edge replicated."""
    n = p.shape[axis]
    return np.take(p, np.clip(np.arange(n) + d, 0, n - 1), axis=axis)


def upsample_h2v1(p):
    p = p.astype(np.int64)
    out = np.empty((p.shape[0], 2 * p.shape[1]), dtype=np.int64)
    out[:, 0::2] = (3 * p + _shift(p, -1, 1) + 1) >> 2
    out[:, 1::2] = (3 * p + _shift(p, 1, 1) + 2) >> 2
    return out


def upsample_h2v2(p):
    p = p.astype(np.int64)
    rows = np.empty((2 * p.shape[0], p.shape[1]), dtype=np.int64)
    rows[0::2] = 3 * p + _shift(p, -1, 0)
    rows[1::2] = 3 * p + _shift(p, 1, 0)
    out = np.empty((rows.shape[0], 2 * rows.shape[1]), dtype=np.int64)
    out[:, 0::2] = (3 * rows + _shift(rows, -1, 1) + 8) >> 4
    out[:, 1::2] = (3 * rows + _shift(rows, 1, 1) + 7) >> 4
    return out


def ycc_to_rgb(y, cb, cr):
    y, cb, cr = y.astype(np.int64), cb.astype(np.int64) - 128, cr.astype(np.int64) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


# ---- parse + entropy decode ----------------------------------------------------------
def _bad(what):
    return ValueError("malformed JPEG: " + what)


def _no(what):
    return ValueError("unsupported JPEG: " + what)


def _u16(d, p):
    if p + 2 > len(d):
        raise _bad("truncated")
    return (d[p] << 8) | d[p + 1]


def parse(data):
    """Markers up to the first SOS.  Returns a dict: H, W, comps [(id, h, v, tq,
    td, ta)], qt {tq: int64[64] natural order}, huff {(tc, th): {(len, code):
    symbol}}, dri, pos (first entropy-coded byte)."""
    d = bytes(data)
    if d[:2] != b"\xff\xd8":
        raise _bad("no SOI")
    p = 2
    qt, huff, frame, dri, adobe = {}, {}, None, 0, None
    while True:
        if p >= len(d):
            raise _bad("truncated")
        if d[p] != 0xFF:
            raise _bad("marker expected")
        while p < len(d) and d[p] == 0xFF:
            p += 1
        if p >= len(d):
            raise _bad("truncated")
        m = d[p]
        p += 1
        if m == 0xD8 or m == 0x01 or 0xD0 <= m <= 0xD7:
            raise _bad("unexpected marker")
        if m == 0xD9:
            raise _bad("no scan")
        n = _u16(d, p)
        if n < 2 or p + n > len(d):
            raise _bad("truncated")
        seg = d[p + 2:p + n]
        p += n
        if m == 0xDB:
            s = 0
            while s < len(seg):
                pq, tq = seg[s] >> 4, seg[s] & 15
                if pq > 1 or tq > 3 or s + 1 + 64 * (pq + 1) > len(seg):
                    raise _bad("DQT")
                t = np.frombuffer(seg, dtype=">u2" if pq else np.uint8, count=64, offset=s + 1).astype(np.int64)
                q = np.zeros(64, dtype=np.int64)
                q[ZIGZAG] = t
                qt[tq] = q
                s += 1 + 64 * (pq + 1)
        elif m == 0xC4:
            s = 0
            while s < len(seg):
                if s + 17 > len(seg):
                    raise _bad("DHT")
                tc, th = seg[s] >> 4, seg[s] & 15
                counts = list(seg[s + 1:s + 17])
                if tc > 1 or th > 3 or s + 17 + sum(counts) > len(seg):
                    raise _bad("DHT")
                table, code, k = {}, 0, s + 17
                for length in range(1, 17):
                    if code + counts[length - 1] > (1 << length):
                        raise _bad("DHT")
                    for _ in range(counts[length - 1]):
                        table[(length, code)] = seg[k]
                        code += 1
                        k += 1
                    code <<= 1
                huff[(tc, th)] = table
                s = k
        elif m in (0xC0, 0xC1):
            if frame is not None:
                raise _bad("second SOF")
            if len(seg) < 6:
                raise _bad("SOF")
            if seg[0] != 8:
                raise _no("%d-bit precision" % seg[0])
            H, W, nc = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            if H == 0:
                raise _no("DNL")
            if W == 0:
                raise _bad("zero width")
            if nc not in (1, 3):
                raise _no("%d components" % nc)
            if len(seg) != 6 + 3 * nc:
                raise _bad("SOF")
            if H > MAX_DIM or W > MAX_DIM:
                raise _no("dimension above %d" % MAX_DIM)
            comps = [(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]) for i in range(nc)]
            if nc == 1:
                comps = [(comps[0][0], 1, 1, comps[0][3])]
            elif [c[1:3] for c in comps] not in ([(1, 1)] * 3, [(2, 1), (1, 1), (1, 1)], [(2, 2), (1, 1), (1, 1)]):
                raise _no("sampling factors")
            if any(c[3] > 3 for c in comps):
                raise _bad("SOF")
            frame = (H, W, comps)
        elif 0xC2 <= m <= 0xCF and m != 0xC8:
            raise _no({0xC2: "progressive"}.get(m, "SOF%d" % (m - 0xC0)))
        elif m == 0xDC:
            raise _no("DNL")
        elif m == 0xDD:
            if len(seg) != 2:
                raise _bad("DRI")
            dri = (seg[0] << 8) | seg[1]
        elif m == 0xEE:
            if len(seg) >= 12 and seg[:5] == b"Adobe":
                adobe = seg[11]
        elif m == 0xDA:
            if frame is None:
                raise _bad("SOS before SOF")
            H, W, comps = frame
            if len(comps) == 3 and adobe not in (None, 1):
                raise _no("Adobe colour transform %d" % adobe)
            if len(seg) < 1 or len(seg) != 4 + 2 * seg[0]:
                raise _bad("SOS")
            if seg[0] != len(comps):
                raise _no("multi-scan")
            full = []
            for i, c in enumerate(comps):
                if seg[1 + 2 * i] != c[0]:
                    raise _no("scan component order")
                td, ta = seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15
                if (0, td) not in huff or (1, ta) not in huff or c[3] not in qt:
                    raise _bad("undefined table")
                full.append(c + (td, ta))
            if tuple(seg[-3:]) != (0, 63, 0):
                raise _bad("SOS")
            return {"H": H, "W": W, "comps": full, "qt": qt, "huff": huff, "dri": dri, "pos": p, "data": d}
        # APPn, COM and the rest carry nothing the decode needs


class _Bits:
    def __init__(self, d, p):
        self.d, self.p, self.acc, self.n = d, p, 0, 0

    def bit(self):
        if self.n == 0:
            d, p = self.d, self.p
            if p >= len(d):
                raise _bad("entropy-coded data ends early")
            b = d[p]
            if b == 0xFF:
                if p + 1 < len(d) and d[p + 1] == 0:
                    p += 1
                else:
                    raise _bad("entropy-coded data ends early")
            self.p, self.acc, self.n = p + 1, b, 8
        self.n -= 1
        return (self.acc >> self.n) & 1

    def symbol(self, table):
        code = 0
        for length in range(1, 17):
            code = (code << 1) | self.bit()
            s = table.get((length, code))
            if s is not None:
                return s
        raise _bad("bad Huffman code")

    def value(self, s):
        if s == 0:
            return 0
        v = 0
        for _ in range(s):
            v = (v << 1) | self.bit()
        return v if v >= (1 << (s - 1)) else v - (1 << s) + 1

    def restart(self, k):
        d, p = self.d, self.p
        self.n = 0
        if p >= len(d) or d[p] != 0xFF:
            raise _bad("missing or wrong RSTn")
        while p < len(d) and d[p] == 0xFF:
            p += 1
        if p >= len(d) or d[p] != 0xD0 + (k & 7):
            raise _bad("missing or wrong RSTn")
        self.p = p + 1


def geometry(info):
    """(hmax, vmax, mcux, mcuy) of a parsed image."""
    hmax, vmax = info["comps"][0][1], info["comps"][0][2]
    mcux = -(-info["W"] // (8 * hmax))
    mcuy = -(-info["H"] // (8 * vmax))
    return hmax, vmax, mcux, mcuy


def entropy_decode(info):
    """Per component an int16 [block rows, block columns, 64] array over the
    MCU-padded block grid, natural order, DC prediction carried through, not
    dequantised."""
    hmax, vmax, mcux, mcuy = geometry(info)
    comps = info["comps"]
    out = [np.zeros((mcuy * c[2], mcux * c[1], 64), dtype=np.int16) for c in comps]
    bits = _Bits(info["data"], info["pos"])
    pred = [0] * len(comps)
    dri, rst = info["dri"], 0
    for mcu in range(mcux * mcuy):
        if dri and mcu and mcu % dri == 0:
            bits.restart(rst)
            rst += 1
            pred = [0] * len(comps)
        my, mx = divmod(mcu, mcux)
        for ci, (_, h, v, _, td, ta) in enumerate(comps):
            dc_t, ac_t = info["huff"][(0, td)], info["huff"][(1, ta)]
            for by in range(v):
                for bx in range(h):
                    blk = out[ci][my * v + by, mx * h + bx]
                    s = bits.symbol(dc_t)
                    if s > 11:
                        raise _bad("DC size category %d" % s)
                    pred[ci] += bits.value(s)
                    if not -32768 <= pred[ci] <= 32767:
                        raise _bad("DC out of range")
                    blk[0] = pred[ci]
                    k = 1
                    while k < 64:
                        rs = bits.symbol(ac_t)
                        r, s = rs >> 4, rs & 15
                        if s == 0:
                            if r != 15:
                                break
                            k += 16
                            if k > 64:
                                raise _bad("run passes coefficient 63")
                            continue
                        if s > 10:
                            raise _bad("AC size category %d" % s)
                        k += r
                        if k > 63:
                            raise _bad("run passes coefficient 63")
                        blk[ZIGZAG[k]] = bits.value(s)
                        k += 1
    # what follows the scan: another scan or DNL is refused
    d, p = info["data"], bits.p
    while p + 1 < len(d):
        if d[p] == 0xFF and d[p + 1] not in (0x00, 0xFF):
            if d[p + 1] == 0xDA:
                raise _no("multi-scan")
            if d[p + 1] == 0xDC:
                raise _no("DNL")
            break
        p += 1
    return out


def planes(info, coefs):
    """The decoded sample planes, each cropped to its valid extent."""
    hmax, vmax, _, _ = geometry(info)
    res = []
    for (_, h, v, tq, _, _), c in zip(info["comps"], coefs):
        bh, bw = c.shape[:2]
        s = np.clip(idct(dequantise(c, info["qt"][tq]).reshape(bh, bw, 8, 8)) + 128, 0, 255)
        plane = s.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)
        res.append(plane[:-(-info["H"] * v // vmax), :-(-info["W"] * h // hmax)])
    return res


def decode(data):
    """Blob -> uint8 [H, W, 1 or 3]."""
    info = parse(data)
    return pixels(info, entropy_decode(info))


def pixels(info, coefs):
    """The per-sample half: entropy-decoded coefficients -> uint8 [H, W, 1 or 3]."""
    H, W = info["H"], info["W"]
    p = planes(info, coefs)
    if len(p) == 1:
        return p[0].astype(np.uint8)[:, :, None]
    hmax, vmax, _, _ = geometry(info)
    if (hmax, vmax) == (2, 1):
        p[1:] = [upsample_h2v1(c) for c in p[1:]]
    elif (hmax, vmax) == (2, 2):
        p[1:] = [upsample_h2v2(c) for c in p[1:]]
    return ycc_to_rgb(p[0], p[1][:H, :W], p[2][:H, :W])


def coefficient_buffer(info, coefs):
    """The layout the host entropy decoder writes: uint16 quantisation tables
    [ncomp][64], then each component's blocks, as bytes."""
    q = np.stack([info["qt"][c[3]] for c in info["comps"]]).astype("<u2")
    return q.tobytes() + b"".join(c.astype("<i2").tobytes() for c in coefs)

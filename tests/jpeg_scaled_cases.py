"""numpy reference of the reduced-size JPEG decode (scale 1/2, 1/4, 1/8) that
csrc/host/jpeg.cc (host) and K22 ``jpeg_decode`` (csrc/kernels/jpeg.hip, device)
implement, built on tests/jpeg_cases.py, and the fixture list of
tests/golden/jpeg_scaled (Pillow ``draft`` decodes of the fixtures of
tests/golden/jpeg).

The contract, all in integers (``>>`` is an arithmetic shift).  The scale is
``s`` in {1, 2, 4, 8} and ``N = 8 / s``; ``s = 1`` is tests/jpeg_cases.py.

1. output size: ``h = ceil(H / s)``, ``w = ceil(W / s)``.
2. component ``c`` with sampling ``hc x vc`` under the maximum ``hmax x vmax``
   is transformed with ``Nx = min(8, N * hmax / hc)`` columns and
   ``Ny = min(8, N * vmax / vc)`` rows: for ``s >= 2`` every component comes out
   at the output resolution, subsampled chroma through a transform twice as
   large and not through the triangle filter, which is used at ``s = 1`` only.
3. dequantise as at full size; only the coefficients with vertical frequency
   below ``Ny`` and horizontal frequency below ``Nx`` are used.
4. ``Ny x Nx`` inverse DCT, separable, rows first, with the bit widths and
   shifts of the 8 x 8: ``b_n[u][x] = s(u) cos((2x+1) u pi / (2n))``,
   ``M1 = round(b_Nx * 2**13)``, ``M2 = round(b_Ny * 2**12)``,
   ``ws = (v @ M1 + 2**10) >> 11``, ``out = (M2^T ws + 2**16) >> 17``.  (The
   n-point orthonormal inverse of coefficients of an 8-point forward transform,
   rescaled by sqrt(n/8), has the 8-point's 1/sqrt(8) per pass.)  A 1 x 1
   transform gives ``(dc*Q + 4) >> 3``.
5. level shift and clamp, every plane cropped to ``h x w``, three components
   through ``ycc_to_rgb``.

The compact coefficient buffer: uint16 ``q[ncomp][64]``, then component ``c``'s
blocks at the next multiple of 16 bytes, each ``Ny * Nx`` int16, vertical
frequency major.  At ``s = 1`` that is the layout of ``jpeg_cases``.
"""

import json
import os

import numpy as np

from tests import jpeg_cases as jc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_scaled")
SCALES = (1, 2, 4, 8)
# every (Ny, Nx) the rule of point 2 gives for sampling factors 1 and 2
SIZES = [(1, 1), (2, 2), (4, 4), (8, 8), (1, 2), (2, 4), (4, 8), (2, 1), (4, 2), (8, 4)]
MODES = {"grey": [(1, 1)], "444": [(1, 1)] * 3, "422": [(2, 1), (1, 1), (1, 1)], "420": [(2, 2), (1, 1), (1, 1)]}


def basis(n):
    return np.array([[(1.0 if u == 0 else np.sqrt(2.0)) * np.cos((2 * x + 1) * u * np.pi / (2 * n)) for x in range(n)]
                     for u in range(n)])


def m1(n):
    return np.rint(basis(n) * (1 << jc.C1_BITS)).astype(np.int64)


def m2(n):
    return np.rint(basis(n) * (1 << jc.C2_BITS)).astype(np.int64)


def idct_n(v):
    """[..., Ny, Nx] dequantised coefficients (row = vertical frequency) ->
    [..., Ny, Nx] samples before the level shift, int64."""
    v = np.asarray(v, dtype=np.int64)
    ny, nx = v.shape[-2:]
    ws = (v @ m1(nx) + (1 << (jc.C1_BITS - jc.PASS1_BITS - 1))) >> (jc.C1_BITS - jc.PASS1_BITS)
    out = np.swapaxes(np.swapaxes(ws, -1, -2) @ m2(ny), -1, -2)
    assert max(np.abs(v @ m1(nx)).max(initial=0), np.abs(out).max(initial=0) + (1 << 16)) < 2 ** 31
    return (out + (1 << (jc.C2_BITS + jc.PASS1_BITS + 2))) >> (jc.C2_BITS + jc.PASS1_BITS + 3)


def idct_n_float(v):
    """The float64 transform of the same coefficients."""
    v = np.asarray(v, dtype=np.float64)
    ny, nx = v.shape[-2:]
    return np.swapaxes(np.swapaxes(v @ (basis(nx) / np.sqrt(8.0)), -1, -2) @ (basis(ny) / np.sqrt(8.0)), -1, -2)


def sizes(info, scale):
    """Per component (Ny, Nx)."""
    hmax, vmax = info["comps"][0][1], info["comps"][0][2]
    n = 8 // scale
    return [(min(8, n * vmax // c[2]), min(8, n * hmax // c[1])) for c in info["comps"]]


def shape(info, scale):
    return -(-info["H"] // scale), -(-info["W"] // scale), len(info["comps"])


def planes(info, coefs, scale):
    """The decoded planes of a scale >= 2, each cropped to the output size."""
    h, w, _ = shape(info, scale)
    res = []
    for comp, c, (ny, nx) in zip(info["comps"], coefs, sizes(info, scale)):
        bh, bw = c.shape[:2]
        v = jc.dequantise(c, info["qt"][comp[3]]).reshape(bh, bw, 8, 8)[:, :, :ny, :nx]
        s = np.clip(idct_n(v) + 128, 0, 255)
        res.append(s.transpose(0, 2, 1, 3).reshape(bh * ny, bw * nx)[:h, :w])
    return res


def pixels(info, coefs, scale=1):
    """Entropy-decoded coefficients (``jpeg_cases.entropy_decode``) -> uint8 [h, w, 1 or 3]."""
    if scale == 1:
        return jc.pixels(info, coefs)
    p = planes(info, coefs, scale)
    if len(p) == 1:
        return p[0].astype(np.uint8)[:, :, None]
    return jc.ycc_to_rgb(*p)


def decode(data, scale=1):
    info = jc.parse(data)
    return pixels(info, jc.entropy_decode(info), scale)


def coefficient_buffer(info, coefs, scale=1):
    """The compact layout the host entropy decoder writes at ``scale``, as bytes."""
    out = bytearray(np.stack([info["qt"][c[3]] for c in info["comps"]]).astype("<u2").tobytes())
    for c, (ny, nx) in zip(coefs, sizes(info, scale)):
        out += b"\0" * (-len(out) % 16)
        bh, bw = c.shape[:2]
        out += np.ascontiguousarray(c.reshape(bh, bw, 8, 8)[:, :, :ny, :nx]).astype("<i2").tobytes()
    return bytes(out)


def synthetic(H, W, mode, seed, amplitude=40):
    """A parse (the keys the functions above read) of an ``H x W`` image of
    sampling ``mode`` and random coefficient arrays over its block grid, with
    the DC near mid-grey so that few samples clamp."""
    rng = np.random.default_rng(seed)
    comps = [(i + 1, h, v, min(i, 1), 0, 0) for i, (h, v) in enumerate(MODES[mode])]
    qt = {t: rng.integers(1, 24, 64).astype(np.int64) for t in (0, 1)}
    info = {"H": H, "W": W, "comps": comps, "qt": qt}
    _, _, mcux, mcuy = jc.geometry(info)
    coefs = []
    for _, h, v, _, _, _ in comps:
        c = rng.integers(-amplitude, amplitude + 1, (mcuy * v, mcux * h, 64)).astype(np.int16)
        c[:, :, 0] = rng.integers(-300, 301, c.shape[:2])
        coefs.append(c)
    return info, coefs


class Parse:
    """What ``ops.hip.jpeg_decode`` reads of a parse, for a synthetic image."""

    def __init__(self, info, scale):
        self.h, self.w, self.ncomp = shape(info, scale)
        self.hs, self.vs = info["comps"][0][1], info["comps"][0][2]
        self.scale = scale
        sz = sizes(info, scale) + [(0, 0)] * (3 - self.ncomp)
        self.ny, self.nx = [s[0] for s in sz], [s[1] for s in sz]
        self.shape = (self.h, self.w, self.ncomp)
        self.pixel_bytes = self.h * self.w * self.ncomp


def box_average(img, scale):
    """The mean over ``scale x scale`` boxes of a uint8 HWC image whose edges are
    replicated to a multiple of ``scale``, float64."""
    h, w, c = img.shape
    p = np.pad(img.astype(np.float64), ((0, -h % scale), (0, -w % scale), (0, 0)), mode="edge")
    return p.reshape(p.shape[0] // scale, scale, p.shape[1] // scale, scale, c).mean(axis=(1, 3))


# ---- fixtures ---------------------------------------------------------------------
def manifest():
    with open(os.path.join(GOLDEN, "manifest.json")) as f:
        return json.load(f)


def drafts():
    """Manifest entries: name (a fixture of tests/golden/jpeg), scale, file, max, mean."""
    return manifest()["drafts"]


def pillow_draft(entry):
    a = np.load(os.path.join(GOLDEN, entry["file"]))
    return a[:, :, None] if a.ndim == 2 else a

#!/usr/bin/env python3
"""Write the JPEG fixtures of tests/golden/jpeg: each ``.jpg``, Pillow's decode
of it as ``.npy`` and ``manifest.json``.  Needs Pillow, so it runs on a
development machine only; nothing under tests/ imports Pillow.  The images are
seeded, so a rerun with the same Pillow / libjpeg-turbo rewrites the same files.

Sizes are width x height.  The tile fixtures are one pixel wider / taller than
K22's workgroup tile (kTileW x kTileH in csrc/kernels/jpeg.hip).

``--huff`` writes tests/golden/jpeg_huff instead: the streams that exercise K23
``jpeg_huffman`` (csrc/kernels/jpeg_huff.hip) beyond what the fixtures above do,
each ``.jpg`` under 64 KB and its own ``manifest.json``, without Pillow's
decodes: the oracle of the Huffman stage is the host entropy decoder.

``--scaled`` writes tests/golden/jpeg_scaled: Pillow's ``draft`` decode (the
DCT-domain 1/2, 1/4 and 1/8 decode of libjpeg-turbo) of the existing ``.jpg``
files of tests/golden/jpeg, as ``.npy``, for each scale at which the draft
comes out at exactly ``ceil(H / s) x ceil(W / s)``, and a ``manifest.json``
with the max and mean absolute difference of the numpy reference
(tests/jpeg_scaled_cases.py) to each.  It writes no JPEG file.

``--wide`` writes tests/golden/jpeg_wide: one stream of more than 2048
subsequences, which K23 declines and the K24 ``jpeg_huffman_wide`` kernels
(csrc/kernels/jpeg_huff_wide.hip) decode in several chunks; ``.jpg`` and
``manifest.json`` only, as for ``--huff``."""

import io
import json
import os
import sys

import numpy as np
from PIL import Image, features

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "jpeg")
TILE_W, TILE_H = 64, 32
SUBSAMPLING = {"444": 0, "422": 1, "420": 2}


def smooth(w, h, c, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    chans = []
    for _ in range(c):
        fx, fy, ph = rng.uniform(0.02, 0.25, 2).tolist() + [rng.uniform(0, 6.28)]
        base = 128 + 90 * np.sin(fx * x + ph) * np.cos(fy * y - ph) + 25 * np.sin(0.7 * fx * (x + y))
        chans.append(base + rng.normal(0, 3, (h, w)))
    return np.clip(np.rint(np.stack(chans, axis=-1)), 0, 255).astype(np.uint8)


def noise(w, h, c, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, c), dtype=np.uint8)


def flat(w, h, c, seed):
    return np.full((h, w, c), 90 + seed % 7, dtype=np.uint8)


# name, width, height, mode, kind, image maker, save() parameters
FIXTURES = [
    ("f01_16x16_444_q90", 16, 16, "444", "case", smooth, {"quality": 90}),
    ("f02_17x23_420_q75", 17, 23, "420", "case", smooth, {"quality": 75}),
    ("f03_40x50_422_q85", 40, 50, "422", "case", smooth, {"quality": 85}),
    ("f04_33x47_grey_q80", 33, 47, "grey", "case", smooth, {"quality": 80}),
    ("f05_64x48_420_q60_rst2", 64, 48, "420", "case", smooth, {"quality": 60, "restart_marker_blocks": 2}),
    ("f06_48x40_420_rstrow", 48, 40, "420", "case", smooth, {"restart_marker_rows": 1}),
    ("f07_37x29_420_q95_opt", 37, 29, "420", "case", smooth, {"quality": 95, "optimize": True}),
    ("f08_1x1_420", 1, 1, "420", "case", smooth, {}),
    ("f09_8x8_444_q100", 8, 8, "444", "case", smooth, {"quality": 100}),
    ("f10_9x70_422_q30", 9, 70, "422", "case", smooth, {"quality": 30}),
    ("f11_32x40_444_q100_noise", 32, 40, "444", "case", noise, {"quality": 100}),
    ("f12_24x24_progressive", 24, 24, "420", "refused", smooth, {"progressive": True}),
    ("t01_%dx24_420" % (TILE_W + 1), TILE_W + 1, 24, "420", "tile", smooth, {"quality": 80}),
    ("t02_40x%d_420" % (TILE_H + 1), 40, TILE_H + 1, "420", "tile", smooth, {"quality": 80}),
    ("t03_%dx24_444" % (TILE_W + 1), TILE_W + 1, 24, "444", "tile", smooth, {"quality": 80}),
    ("t04_40x%d_444" % (TILE_H + 1), 40, TILE_H + 1, "444", "tile", smooth, {"quality": 80}),
    ("b01_640x480_420_q75", 640, 480, "420", "bench", smooth, {"quality": 75}),
]

# K23: EOB-only blocks (hundreds of blocks in one subsequence); about a hundred subsequences of
# dense data per sampling; restart intervals longer than a subsequence, unaligned with the MCU
# rows (10 MCUs a row) and more than 8 of them, so the RSTn numbers wrap
HUFF_OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "jpeg_huff")
HUFF_FIXTURES = [
    ("h01_256x256_420_flat", 256, 256, "420", "case", flat, {}),
    ("h02_200x200_grey_q90_noise", 200, 200, "grey", "case", noise, {"quality": 90}),
    ("h03_128x128_422_q90_noise", 128, 128, "422", "case", noise, {"quality": 90}),
    ("h04_128x128_444_q90_noise", 128, 128, "444", "case", noise, {"quality": 90}),
    ("h05_160x120_420_q90_rst7", 160, 120, "420", "case", noise, {"quality": 90, "restart_marker_blocks": 7}),
]

# K24: more than 2048 subsequences in one segment (no restart markers): three chunks of 1024
WIDE_OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "jpeg_wide")
WIDE_FIXTURES = [
    ("w01_640x480_420_q95_noise", 640, 480, "420", "case", noise, {"quality": 95}),
]


def main(out=OUT, fixtures=FIXTURES, first_seed=1000, decodes=True):
    os.makedirs(out, exist_ok=True)
    entries = []
    for seed, (name, w, h, mode, kind, make, params) in enumerate(fixtures):
        a = make(w, h, 1 if mode == "grey" else 3, first_seed + seed)
        im = Image.fromarray(a[:, :, 0], "L") if mode == "grey" else Image.fromarray(a, "RGB")
        kw = dict(params)
        if mode != "grey":
            kw["subsampling"] = SUBSAMPLING[mode]
        buf = io.BytesIO()
        im.save(buf, "JPEG", **kw)
        data = buf.getvalue()
        with open(os.path.join(out, name + ".jpg"), "wb") as f:
            f.write(data)
        if decodes:
            np.save(os.path.join(out, name + ".npy"), np.asarray(Image.open(io.BytesIO(data))))
        entries.append({"name": name, "w": w, "h": h, "mode": mode, "kind": kind, "params": params,
                        "bytes": len(data)})
        print("%-28s %6d bytes" % (name, len(data)))
    with open(os.path.join(out, "manifest.json"), "w") as f:
        json.dump({"pillow": features.version("pil"), "libjpeg_turbo": features.version_feature("libjpeg_turbo"),
                   "tile": [TILE_W, TILE_H], "fixtures": entries}, f, indent=1)
        f.write("\n")


SCALED_OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "jpeg_scaled")


def scaled(out=SCALED_OUT):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    from tests import jpeg_cases as jc
    from tests import jpeg_scaled_cases as js

    os.makedirs(out, exist_ok=True)
    entries = []
    for e in jc.decodable():
        data = jc.blob(e)
        for s in (2, 4, 8):
            im = Image.open(io.BytesIO(data))
            im.draft(im.mode, (-(-e["w"] // s), -(-e["h"] // s)))
            a = np.asarray(im)
            if a.shape[:2] != (-(-e["h"] // s), -(-e["w"] // s)):
                continue  # Pillow picked another scale for this size
            name = "%s_s%d.npy" % (e["name"], s)
            np.save(os.path.join(out, name), a)
            d = np.abs(js.decode(data, s).astype(np.int64) - (a[:, :, None] if a.ndim == 2 else a))
            entries.append({"name": e["name"], "scale": s, "file": name, "max": int(d.max()),
                            "mean": round(float(d.mean()), 4)})
            print("%-28s 1/%d  max %3d  mean %.4f" % (e["name"], s, d.max(), d.mean()))
    with open(os.path.join(out, "manifest.json"), "w") as f:
        json.dump({"pillow": features.version("pil"), "libjpeg_turbo": features.version_feature("libjpeg_turbo"),
                   "drafts": entries}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    if sys.argv[1:] == ["--scaled"]:
        scaled()
    elif sys.argv[1:] == ["--huff"]:
        main(HUFF_OUT, HUFF_FIXTURES, first_seed=2000, decodes=False)
    elif sys.argv[1:] == ["--wide"]:
        main(WIDE_OUT, WIDE_FIXTURES, first_seed=3000, decodes=False)
    else:
        main()

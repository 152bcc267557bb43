#!/usr/bin/env python3
"""Write the PNG fixtures of tests/golden/png: each ``.png`` as Pillow writes it,
Pillow's own ``.convert("RGB")`` / ``.convert("L")`` of it as ``.npy``, and
``manifest.json``.  Needs Pillow, so it runs on a development machine only;
nothing under tests/ imports Pillow.  The images are seeded, so a rerun with
the same Pillow / zlib rewrites the same files.

A file is committed only if Pillow's result equals the contract of
tests/png_cases.py (alpha dropped, not composited; a 16-bit sample gives its
high byte): the tool reports a file on which the two differ instead of
writing it.  Sizes are width x height.

Pillow writes neither Adam7 nor a filter of one's choosing, so three more files
(``c01`` .. ``c03``) come from the writer of tests/png_cases.py, with the
reference decode as their ``.npy`` (Pillow reads them back to the same pixels
where its conversion is the contract's, which the tool checks too): they give
csrc/cpp/tests/png_test.cc, which reads this directory, an interlaced file, a
16-bit file and a short PLTE."""

import io
import json
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
from tests import png_cases  # noqa: E402

OUT = os.path.join(HERE, "..", "tests", "golden", "png")


def picture(w, h, c, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([(x * (3 + k) + y * (5 - k) + 40 * k) % 256 for k in range(c)], axis=2)
    noise = rng.integers(-12, 13, size=(h, w, c))
    return np.clip(base + noise, 0, 255).astype(np.uint8)


def fixtures():
    rgb = picture(31, 20, 3, 1)
    yield "g01_rgb_31x20", Image.fromarray(rgb, "RGB"), {}
    yield "g02_rgba_31x20", Image.fromarray(picture(31, 20, 4, 2), "RGBA"), {}
    yield "g03_l_31x20", Image.fromarray(picture(31, 20, 1, 3)[:, :, 0], "L"), {}
    yield "g04_la_17x9", Image.fromarray(picture(17, 9, 2, 4), "LA"), {}
    yield "g05_p200_31x20", Image.fromarray(rgb, "RGB").quantize(200), {}
    yield "g06_p_bits2_13x11", Image.fromarray(picture(13, 11, 3, 6), "RGB").quantize(4), {"bits": 2}
    yield "g07_1bit_29x15", Image.fromarray(picture(29, 15, 1, 7)[:, :, 0] > 127), {}
    yield "g08_rgb_optimized_64x48", Image.fromarray(picture(64, 48, 3, 8), "RGB"), {"optimize": True}
    yield "g09_rgb_1x1", Image.fromarray(picture(1, 1, 3, 9), "RGB"), {}


def written_cases():
    """(name, blob, whether Pillow's conversion is expected to be the contract's)."""
    yield "c01_adam7_rgb_9x7", png_cases.make(2, 8, 7, 9, png_cases.CYCLE, adam7=True, idat_splits=2), True
    yield "c02_rgba16_5x4", png_cases.make(6, 16, 4, 5, png_cases.CYCLE), False  # Pillow keeps 8 bits its own way
    yield "c03_adam7_p2_short_plte_11x9", png_cases.make(3, 2, 9, 11, png_cases.CYCLE, adam7=True,
                                                         palette_entries=3), False  # Pillow has no rule for it


def main():
    os.makedirs(OUT, exist_ok=True)
    manifest, differ = [], []
    for name, blob, pillow_agrees in written_cases():
        ours = png_cases.decode(blob)
        if pillow_agrees:
            back = np.asarray(Image.open(io.BytesIO(blob)).convert("RGB"), dtype=np.uint8)
            if not np.array_equal(back.reshape(ours.shape), ours):
                differ.append(name)
                continue
        with open(os.path.join(OUT, name + ".png"), "wb") as f:
            f.write(blob)
        np.save(os.path.join(OUT, name + ".npy"), ours)
        manifest.append({"name": name, "png": name + ".png", "npy": name + ".npy", "mode": "png_cases",
                         "shape": list(ours.shape), "bytes": len(blob)})
    for name, im, opts in fixtures():
        buf = io.BytesIO()
        im.save(buf, "PNG", **opts)
        blob = buf.getvalue()
        back = Image.open(io.BytesIO(blob))
        ours = png_cases.decode(blob)
        want = np.asarray(back.convert("L" if ours.shape[2] == 1 else "RGB"), dtype=np.uint8).reshape(ours.shape)
        if not np.array_equal(want, ours):
            differ.append(name)
            continue
        with open(os.path.join(OUT, name + ".png"), "wb") as f:
            f.write(blob)
        np.save(os.path.join(OUT, name + ".npy"), want)
        manifest.append({"name": name, "png": name + ".png", "npy": name + ".npy", "mode": back.mode,
                         "shape": list(want.shape), "bytes": len(blob)})
    with open(os.path.join(OUT, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1)
        f.write("\n")
    print("wrote %d fixtures to %s" % (len(manifest), os.path.normpath(OUT)))
    for name in differ:
        print("NOT written, Pillow's conversion differs from the contract: %s" % name)
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())

"""The route a JPEG or a PNG takes to the device and the layout of the staging area
it is routed into: the one place where both are decided, for the GPU
``preprocess_inception`` (server/gpu_models.py) and for
``utils.image.preprocess_raw_batch_device``.  Planning is integer arithmetic
and calls into a ``HostCodec`` (ops/host_codec.py), so it runs, and is tested
(tests/test_jpeg_stage.py), without a GPU: nothing here imports torch or the
device library, which :func:`launch_decode` receives as an argument.

The routes of a JPEG, tried in this order:

1. ``K23``: ``TCAMD_DEVICE_HUFFMAN=1``, the parse is at scale 1 and
   ``HostCodec.jpeg_stream_pack`` succeeds in the room that is left.  The host
   only packs the scan; K23 ``jpeg_huffman`` writes the coefficients.
2. ``K24``: ``TCAMD_DEVICE_HUFFMAN_WIDE=N`` with N > 0, the blob has at least N
   bytes, ``HostCodec.jpeg_stream_pack_wide`` succeeds, and the stream still
   fits under the workspace this JPEG enlarges.  The K24 ``jpeg_huffman_wide``
   kernels write the coefficients, at any scale.
3. ``HOST``: ``HostCodec.jpeg_entropy_decode`` writes the coefficients straight
   into the staging area.
4. None of them fits: the caller decodes the blob on the host and offers the
   pixels as a raw image; a raw image that does not fit is resized on the host.

K22 ``jpeg_decode`` turns the coefficients of every route into pixels.

A PNG has one device route, under ``TCAMD_DEVICE_PNG=1`` and for a file that is
not interlaced: ``HostCodec.png_inflate`` inflates the IDAT stream straight
into the staging area (filtered scanlines, then the palette of colour type 3,
then, for an image of more rows than a pass of the kernel, one scanline of
scratch that only the kernel touches), and K25 ``png_unfilter`` reverses the
filters and converts the samples into pixels.  The fit test needs the parse
alone, so a PNG that does not fit is never inflated twice: like an interlaced
one, or any PNG with the knob off, the caller decodes it on the host
(``HostCodec.png_decode``) and offers the pixels as a raw image.

The staging area of a :class:`StagePlan` is ``capacity`` bytes that exist on
the host (the view) and on the device:

* the *upload region* ``[0, used)`` is what the host writes and the H2D copy
  carries: raw pixels at any alignment, ``HOST`` coefficient buffers at
  multiples of 128, packed streams and the staged bytes of a PNG at multiples
  of 16;
* the *device-only region* ``[top, capacity)`` is written by kernels alone: for
  a ``K23`` or ``K24`` JPEG the pixels at ``top - pixel_bytes`` and the
  coefficients at ``(top - pixel_bytes - coef_bytes) // 128 * 128``, which is
  the new ``top``; for a ``HOST`` JPEG and for a PNG only the pixels;
* K24's workspace, ``ws_need = 16 + workspace(the K24 subsequence counts so
  far)`` bytes (16: it starts at a 16-byte boundary), lies below ``top`` at
  :attr:`StagePlan.workspace` once the plan is complete, so at every step
  nothing in the upload region reaches past ``top - ws_need``.
"""

import os
from collections import namedtuple

from .image import jpeg_auto_scale

K23, K24, HOST = "K23", "K24", "HOST"


def device_huffman_knob():
    """``TCAMD_DEVICE_HUFFMAN``: 1 = the host packs a JPEG's scan and K23
    ``jpeg_huffman`` decodes it on the device; 0 (the default) is off."""
    return os.environ.get("TCAMD_DEVICE_HUFFMAN", "0") == "1"


def device_huffman_wide_knob():
    """``TCAMD_DEVICE_HUFFMAN_WIDE``: the smallest JPEG blob, in bytes, whose
    Huffman stage the K24 ``jpeg_huffman_wide`` kernels take; 0 (the default)
    is off, 1 is every JPEG."""
    return max(0, int(os.environ.get("TCAMD_DEVICE_HUFFMAN_WIDE", "0") or 0))


def device_png_knob():
    """``TCAMD_DEVICE_PNG``: 1 (the default) = the host inflates a
    non-interlaced PNG into the staging area and K25 ``png_unfilter`` makes the
    pixels on the device; 0 = the host decodes it and the pixels go up."""
    return os.environ.get("TCAMD_DEVICE_PNG", "1") != "0"


def parse_at_scale(codec, blob, jpeg_scale, h_out, w_out):
    """The parse of a JPEG blob at ``jpeg_scale`` (1, 2, 4 or 8); 0 picks
    :func:`utils.image.jpeg_auto_scale` for an ``h_out x w_out`` target."""
    if jpeg_scale == 0:
        full = codec.jpeg_parse(blob)
        jpeg_scale = jpeg_auto_scale(full.h, full.w, h_out, w_out)
        if jpeg_scale == 1:
            return full
    return codec.jpeg_parse(blob, jpeg_scale)


class JpegJob(namedtuple("JpegJob", "route stream coef pix info nsub row blob antialias request")):
    """A routed JPEG: its ``route``; the offsets of its packed ``stream``
    (None on ``HOST``), its coefficients and its pixels; its parse; its K24
    subsequences (0 on the other routes); its row of the batch, its blob, its
    antialias flag and the index of its request."""

    __slots__ = ()

    @property
    def shape(self):
        return self.info.shape


class PngJob(namedtuple("PngJob", "stream pix info row blob antialias request")):
    """A staged PNG: the offsets of its staged bytes (``info.stage_bytes`` in
    the upload region) and of its pixels; its parse; its row of the batch, its
    blob, its antialias flag and the index of its request."""

    __slots__ = ()

    @property
    def shape(self):
        return self.info.shape


class RawImage(namedtuple("RawImage", "row image pix antialias")):
    """A decoded uint8 HWC image: its row of the batch, and the offset of its
    pixels in the upload region, or None when it takes the host resize."""

    __slots__ = ()

    @property
    def shape(self):
        return self.image.shape


def pack_stream(codec, blob, info, room, huffman, huffman_wide):
    """Pack the scan of ``blob`` (parse ``info``) into the 16-byte aligned
    uint8 array ``room`` for the first device Huffman route that takes it under
    the two knobs: ``(route, bytes written, subsequences)``, or None when the
    host's entropy decoder is to have it."""
    if huffman and info.scale == 1:
        n = codec.jpeg_stream_pack(blob, room)[1]
        if n is not None:
            return K23, n, 0
    if huffman_wide and len(blob) >= huffman_wide:
        n, nsub = codec.jpeg_stream_pack_wide(blob, room, info.scale)[1:]
        if n is not None:
            return K24, n, nsub
    return None


class StagePlan:
    """The plan of one batch over ``stage``, a uint8 numpy view whose first
    byte is 16-byte aligned and whose size is the capacity (the layout: the
    module's docstring).  ``huffman`` and ``huffman_wide`` are the two knobs,
    ``max_dim`` the largest image side the device resize takes.  ``jpegs``,
    ``pngs`` and ``raws`` list the batch's images in the order they were added;
    ``rows`` counts them."""

    def __init__(self, stage, codec, huffman=False, huffman_wide=0, max_dim=16384):
        self.stage, self.codec = stage, codec
        self.huffman, self.huffman_wide, self.max_dim = huffman, huffman_wide, max_dim
        self.rows = self.used = self.ws_need = 0
        self.top = stage.size
        self.jpegs, self.raws, self.pngs = [], [], []

    @property
    def workspace(self):
        """The offset of K24's ``ws_need - 16`` bytes of workspace."""
        return (self.top - self.ws_need + 15) // 16 * 16

    def mark(self):
        return self.rows, self.used, self.top, self.ws_need, len(self.jpegs), len(self.raws), len(self.pngs)

    def rollback(self, mark):
        """Forget everything added since ``mark``."""
        self.rows, self.used, self.top, self.ws_need = mark[:4]
        del self.jpegs[mark[4]:], self.raws[mark[5]:], self.pngs[mark[6]:]

    def add_raw(self, image, antialias=False):
        """Stage a uint8 HWC array if the device resize takes it and it fits."""
        h, w, c = image.shape
        pix = None
        if 1 <= h <= self.max_dim and 1 <= w <= self.max_dim and c in (1, 3) \
                and self.used + image.size <= self.top - self.ws_need:
            pix = self.used
            self.stage[pix:pix + image.size] = image.reshape(-1)
            self.used += image.size
        self.raws.append(RawImage(self.rows, image, pix, antialias))
        self.rows += 1
        return self.raws[-1]

    def add_jpeg(self, blob, info, antialias=False, request=0):
        """Route a JPEG blob with parse ``info`` and stage what its route has
        the host write; None when no route fits.  An undecodable blob raises
        the host decoder's error and leaves the plan as it was."""
        job = None
        at = -(-self.used // 16) * 16
        coef = (self.top - info.pixel_bytes - info.coef_bytes) // 128 * 128
        if at < coef - self.ws_need:
            packed = pack_stream(self.codec, blob, info, self.stage[at:coef - self.ws_need], self.huffman,
                                 self.huffman_wide)
            if packed is not None:
                route, n, nsub = packed
                need = self.ws_need
                if route == K24:
                    need = 16 + self.codec.jpeg_huffman_wide_workspace(
                        [j.nsub for j in self.jpegs if j.route == K24] + [nsub])
                if at + n <= coef - need:
                    job = JpegJob(route, at, coef, self.top - info.pixel_bytes, info, nsub, self.rows, blob,
                                  antialias, request)
                    self.used, self.top, self.ws_need = at + n, coef, need
        if job is None:
            coef = -(-self.used // 128) * 128
            if coef + info.coef_bytes + info.pixel_bytes > self.top - self.ws_need:
                return None
            self.codec.jpeg_entropy_decode(blob, self.stage[coef:coef + info.coef_bytes], info.scale)
            self.used = coef + info.coef_bytes
            self.top -= info.pixel_bytes
            job = JpegJob(HOST, None, coef, self.top, info, 0, self.rows, blob, antialias, request)
        self.jpegs.append(job)
        self.rows += 1
        return job


    def add_png(self, blob, info, antialias=False, request=0):
        """Stage a non-interlaced PNG blob with parse ``info`` for K25: None,
        with nothing inflated, when its staged bytes and its pixels do not fit
        (or the device resize does not take its size).  A blob that does not
        inflate raises the host decoder's error and leaves the plan as it was."""
        at = -(-self.used // 16) * 16
        if info.interlace or not (1 <= info.h <= self.max_dim and 1 <= info.w <= self.max_dim) \
                or at + info.stage_bytes > self.top - info.pixel_bytes - self.ws_need:
            return None
        self.codec.png_inflate(blob, self.stage[at:at + info.stage_bytes])
        self.used = at + info.stage_bytes
        self.top -= info.pixel_bytes
        job = PngJob(at, self.top, info, self.rows, blob, antialias, request)
        self.pngs.append(job)
        self.rows += 1
        return job


def launch_decode(hip, jobs, upload, device_only, workspace, workspace_bytes, alloc_status, stream, pngs=()):
    """Issue K23, then K24, then K22 for the :class:`JpegJob` list ``jobs`` and
    K25, once, for the :class:`PngJob` list ``pngs`` on ``stream``.  ``upload`` and ``device_only`` are the device addresses that
    the offsets of the two regions count from (the same address for a
    :class:`StagePlan`); ``workspace`` is the device address of K24's
    ``workspace_bytes``; ``alloc_status(n)`` gives ``n`` int32 status words on
    the device, an object with ``data_ptr()``.  Returns ``[(jobs, status)]`` of
    K23 and of K24, for each that ran, the status words in the order of its jobs:
    an image whose word is not 0 after the stream's synchronise has no pixels."""
    ran = []
    for route in (K23, K24):
        mine = [j for j in jobs if j.route == route]
        if not mine:
            continue
        status = alloc_status(len(mine))
        streams, coefs = [upload + j.stream for j in mine], [device_only + j.coef for j in mine]
        if route == K23:
            hip.jpeg_huffman(streams, coefs, status.data_ptr(), stream=stream)
        else:
            hip.jpeg_huffman_wide(streams, coefs, [j.nsub for j in mine], status.data_ptr(), workspace,
                                  workspace_bytes, stream=stream)
        ran.append((mine, status))
    if jobs:
        hip.jpeg_decode([(upload if j.route == HOST else device_only) + j.coef for j in jobs],
                        [j.info for j in jobs], [device_only + j.pix for j in jobs], stream=stream)
    if pngs:
        hip.png_unfilter([upload + j.stream for j in pngs], [j.info for j in pngs],
                         [device_only + j.pix for j in pngs], stream=stream)
    return ran

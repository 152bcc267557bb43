"""Image decoding + classification preprocessing without an imaging library.

Mirrors the preprocessing of reference src/python/examples/image_client.py:154-194
(INCEPTION scaling ``x/127.5 - 1``, VGG mean subtraction, NCHW/NHWC) using
numpy only.  Decodes binary PPM (P6) / PGM (P5), a raw ``TCIMG`` container
(``b"TCIMG" + u16 H + u16 W + u8 C + HWC bytes``) used by the examples, and,
through the host decoders of libtcamd_host.so, baseline JPEG (csrc/host/jpeg.cc)
and PNG of every standard colour type and bit depth, interlaced or not, to 8
bits per sample without alpha (csrc/host/png.cc).
"""

import struct

import numpy as np


def encode_raw(img):
    img = np.ascontiguousarray(img, dtype=np.uint8)
    if img.ndim == 2:
        img = img[:, :, None]
    h, w, c = img.shape
    return b"TCIMG" + struct.pack("<HHB", h, w, c) + img.tobytes()


def encode_ppm(img):
    img = np.ascontiguousarray(img, dtype=np.uint8)
    h, w = img.shape[:2]
    return b"P6\n%d %d\n255\n" % (w, h) + img.tobytes()


JPEG_SOI = b"\xff\xd8"
PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"


def _jpeg_codec():
    from triton_client_amd.ops import host_codec

    try:
        return host_codec.load()
    except (OSError, AttributeError) as e:
        raise ValueError("JPEG decoding needs libtcamd_host.so, which is not built (run make): %s" % e) from e


def _png_codec():
    from triton_client_amd.ops import host_codec

    try:
        return host_codec.load()
    except (OSError, AttributeError) as e:
        raise ValueError("PNG decoding needs libtcamd_host.so, which is not built (run make): %s" % e) from e


JPEG_SCALES = (1, 2, 4, 8)


def jpeg_auto_scale(H, W, h_out, w_out):
    """The largest reduced-size JPEG decode that a resize to ``h_out x w_out``
    does not have to upscale: the largest ``s`` in {1, 2, 4, 8} with
    ``H >= s * h_out`` and ``W >= s * w_out``, so that the ``ceil(H / s) x
    ceil(W / s)`` decode has ``h_out x w_out`` whole samples (the last row and
    column of a size that ``s`` does not divide cover fewer source pixels and
    do not count: 447 -> 1, 448 -> 2 for a 224 target); 1 for an image that is
    already smaller than the target on an axis."""
    for s in (8, 4, 2):
        if int(H) >= s * h_out and int(W) >= s * w_out:
            return s
    return 1


def check_jpeg_scale(value, auto=True):
    """``value`` as a JPEG scale: 1, 2, 4 or 8, or (with ``auto``) 0 for
    :func:`jpeg_auto_scale`; anything else raises ``ValueError``."""
    allowed = ((0,) if auto else ()) + JPEG_SCALES
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or int(value) not in allowed:
        raise ValueError("jpeg_scale must be one of %s, not %r" % (", ".join(str(a) for a in allowed), value))
    return int(value)


def decode_image(blob, jpeg_scale=1):
    """PPM / PGM / TCIMG / baseline JPEG / PNG blob -> uint8 [H, W, C].  A JPEG
    or PNG the decoder does not cover raises ``ValueError("unsupported JPEG:
    ...")`` / ``("unsupported PNG: ...")``, a broken one ``("malformed JPEG:
    ...")`` / ``("malformed PNG: ...")``.  A PNG gives C = 1 for grey and C = 3
    otherwise: 16-bit samples give their high byte and alpha is dropped.
    ``jpeg_scale`` 2, 4 or 8 decodes a JPEG in the DCT domain at that fraction
    of its size, ``ceil(H / s) x ceil(W / s)``; the other encodings ignore it."""
    blob = bytes(blob)
    if blob[:8] == PNG_SIGNATURE:
        return _png_codec().png_decode(blob)
    if blob[:2] == JPEG_SOI:
        return _jpeg_codec().jpeg_decode(blob, check_jpeg_scale(jpeg_scale, auto=False))
    if blob[:5] == b"TCIMG":
        h, w, c = struct.unpack_from("<HHB", blob, 5)
        return np.frombuffer(blob, dtype=np.uint8, offset=10, count=h * w * c).reshape(h, w, c)
    if blob[:2] in (b"P6", b"P5"):
        parts = []
        pos = 2
        while len(parts) < 3:
            while blob[pos : pos + 1].isspace():
                pos += 1
            if blob[pos : pos + 1] == b"#":
                while blob[pos : pos + 1] not in (b"\n", b""):
                    pos += 1
                continue
            start = pos
            while not blob[pos : pos + 1].isspace():
                pos += 1
            parts.append(int(blob[start:pos]))
        pos += 1
        w, h, _ = parts
        c = 3 if blob[:2] == b"P6" else 1
        return np.frombuffer(blob, dtype=np.uint8, offset=pos, count=h * w * c).reshape(h, w, c)
    raise ValueError("unsupported image encoding (expected PPM/PGM/TCIMG/JPEG/PNG)")


def resize_bilinear(img, h, w):
    ih, iw = img.shape[:2]
    if (ih, iw) == (h, w):
        return img.astype(np.float32)
    ys = (np.arange(h) + 0.5) * ih / h - 0.5
    xs = (np.arange(w) + 0.5) * iw / w - 0.5
    y0 = np.clip(np.floor(ys).astype(int), 0, ih - 1)
    x0 = np.clip(np.floor(xs).astype(int), 0, iw - 1)
    y1 = np.clip(y0 + 1, 0, ih - 1)
    x1 = np.clip(x0 + 1, 0, iw - 1)
    wy = np.clip(ys - y0, 0, 1)[:, None, None]
    wx = np.clip(xs - x0, 0, 1)[None, :, None]
    f = img.astype(np.float32)
    top = f[y0][:, x0] * (1 - wx) + f[y0][:, x1] * wx
    bot = f[y1][:, x0] * (1 - wx) + f[y1][:, x1] * wx
    return top * (1 - wy) + bot * wy


def resize_axis_table(n_out, n_in):
    """``(i0, i1, frac_num, den)`` of ``resize_bilinear`` along one axis, in
    integers: output index ``i`` blends source ``i0[i]`` and ``i1[i]`` with
    weight ``frac_num[i] / den`` on ``i1``.  The written contract of K20
    ``resize_pack`` (csrc/kernels/resize.hip), which computes the same terms
    per thread: ``num = (2i+1)*n_in - n_out``, ``den = 2*n_out``,
    ``floor(num/den)`` clamped to the source, weight 0 before the first sample
    and 1 past the last.  No fp32 coordinate is formed, so the weights are
    exact ratios at any size (up to 16384 ``num`` fits 32 bits)."""
    i = np.arange(n_out, dtype=np.int64)
    den = 2 * int(n_out)
    num = (2 * i + 1) * int(n_in) - int(n_out)
    f = num // den  # numpy floors toward -inf
    frac = num - f * den
    frac = np.where(f < 0, 0, np.where(f > n_in - 1, den, frac))
    i0 = np.clip(f, 0, n_in - 1)
    i1 = np.clip(i0 + 1, 0, n_in - 1)
    return i0, i1, frac, den


def area_axis_table(n_out, n_in):
    """``(first, count, t, total)`` of the antialiased resize along one axis,
    in integers: output index ``i`` is
    ``sum_k t[i, k] * src[first[i] + k] / total[i]`` over ``k < count[i]``,
    with ``D = 2 * max(n_in, n_out)`` and
    ``t = D - |(2j+1)*n_out - (2i+1)*n_in|`` at source index ``j``: the triangle
    filter with half-pixel centres and support ``max(1, n_in/n_out)``,
    renormalised at the borders (the coefficients of Pillow's BILINEAR
    ``resize``, kept as exact ratios).  Only taps with ``t > 0`` are listed;
    ``t`` is zero past ``count[i]``.  For ``n_in <= n_out`` these are the two
    taps and weights of :func:`resize_axis_table`.  The written contract of K21
    ``resize_pack_aa`` (csrc/kernels/resize.hip), which walks the same taps;
    up to 16384 every term fits 32 bits signed.  The table has
    ``n_out * max(count)`` entries, about ``2 * max(n_in, n_out)``."""
    n_out, n_in = int(n_out), int(n_in)
    i = np.arange(n_out, dtype=np.int64)
    big = 2 * max(n_in, n_out)
    den = 2 * n_out
    c = (2 * i + 1) * n_in
    # t > 0  <=>  c - big < (2j+1)*n_out < c + big
    first = np.maximum((c - big - n_out) // den + 1, 0)
    last = np.minimum((c + big - n_out - 1) // den, n_in - 1)
    count = last - first + 1
    j = first[:, None] + np.arange(int(count.max()), dtype=np.int64)[None, :]
    t = big - np.abs((2 * j + 1) * n_out - c[:, None])
    t = np.where(j <= last[:, None], t, 0)
    return first, count, t, t.sum(axis=1)


def _area_axis(x, n_out):
    """Antialiased resize of float64 ``x`` along axis 0, one pass per tap."""
    n_in = x.shape[0]
    first, count, t, total = area_axis_table(n_out, n_in)
    tail = (1,) * (x.ndim - 1)
    out = np.zeros((n_out,) + x.shape[1:], dtype=np.float64)
    for k in range(t.shape[1]):
        rows = np.nonzero(count > k)[0]
        out[rows] += (t[rows, k] / total[rows]).reshape((-1,) + tail) * x[first[rows] + k]
    return out


def resize_area(img, h, w):
    """Antialiased (support-scaled triangle filter) resize of an HWC image to
    ``h x w`` in float64: :func:`area_axis_table` along x, then along y.  A
    downscaled axis averages every source pixel under the widened filter; an
    upscaled axis is :func:`resize_bilinear`.  Banded: the work is
    ``n_out * taps`` per axis, never an ``n_out x n_in`` matrix."""
    x = np.asarray(img, dtype=np.float64)
    x = _area_axis(x.transpose(1, 0, 2), w).transpose(1, 0, 2)
    return _area_axis(x, h)


def preprocess(img, c, h, w, scaling="INCEPTION", fmt="NCHW", dtype=np.float32, antialias=False):
    """``antialias`` resizes with :func:`resize_area` instead of
    :func:`resize_bilinear`; everything else is the same."""
    if c == 1 and img.shape[2] == 3:
        img = img.mean(axis=2, keepdims=True)
    elif c == 3 and img.shape[2] == 1:
        img = np.repeat(img, 3, axis=2)
    x = resize_area(img, h, w) if antialias else resize_bilinear(img, h, w)
    if scaling == "INCEPTION":
        x = x / 127.5 - 1.0
    elif scaling == "VGG":
        mean = np.array([123.0, 117.0, 104.0] if c == 3 else [128.0], np.float32)
        x = x - mean
    x = x.astype(dtype)
    if fmt == "NCHW":
        x = np.transpose(x, (2, 0, 1))
    return np.ascontiguousarray(x)


def inception_preprocess(img, h, w, fmt="NCHW", antialias=False):
    return preprocess(img, 3, h, w, "INCEPTION", fmt, antialias=antialias)


_SCALE_BIAS = {
    "NONE": lambda c: ([1.0] * c, [0.0] * c),
    "INCEPTION": lambda c: ([1.0 / 127.5] * c, [-1.0] * c),
    "VGG": lambda c: ([1.0] * c, [-m for m in ([123.0, 117.0, 104.0] if c == 3 else [128.0])]),
}
_DEVICE_DTYPES = {"FP32": np.float32, "FP16": np.float16}


def preprocess_batch_device(resized, scaling="INCEPTION", fmt="NCHW", dtype="FP32", device=0):
    """Scale + HWC->CHW transpose + dtype convert of a batch of resized HWC
    fp32 images in ONE K6 ``layout_pack`` launch on the GPU (LDS-tiled
    transpose; replaces the numpy scale/transpose of ``preprocess``, reference
    src/python/examples/image_client.py:154-194 and
    src/c++/examples/image_client.cc:86-188).  The images are uploaded once as
    a host->device copy, the packed [n, C, H, W] (or [n, H, W, C]) batch comes
    back as numpy.  ``dtype`` is the model's Triton datatype (FP32 or FP16).
    Returns None when the datatype has no device path (integer models)."""
    if dtype not in _DEVICE_DTYPES:
        return None
    import torch

    from triton_client_amd.ops import hip

    imgs = [np.ascontiguousarray(r, dtype=np.float32) for r in resized]
    h, w, c = imgs[0].shape
    dev = torch.device("cuda", device)
    src = torch.from_numpy(np.stack(imgs, axis=0)).to(dev, non_blocking=False)
    shape = (len(imgs), c, h, w) if fmt == "NCHW" else (len(imgs), h, w, c)
    dst = torch.empty(shape, device=dev, dtype=torch.float32 if dtype == "FP32" else torch.float16)
    scale, bias = _SCALE_BIAS[scaling](c)
    stream = torch.cuda.current_stream(dev).cuda_stream
    per = c * h * w * dst.element_size()
    for i0 in range(0, len(imgs), 64):  # K6 takes up to 64 source pointers per launch
        n = min(64, len(imgs) - i0)
        hip.layout_pack([src[i].data_ptr() for i in range(i0, i0 + n)], "FP32", "NHWC", dst.data_ptr() + i0 * per,
                        dtype, fmt, c, h, w, scale=scale, bias=bias, stream=stream)
    return dst.cpu().numpy()


def preprocess_raw_batch_device(images, c, h, w, scaling="INCEPTION", fmt="NCHW", dtype="FP32", device=0,
                                antialias=False, device_huffman=None, jpeg_scale=1, device_huffman_wide=None,
                                device_png=None):
    """``preprocess`` of a batch of decoded uint8 HWC images of any sizes on
    the GPU: the raw pixels go up in ONE uint8 host->device copy (a quarter of
    the bytes of the resized fp32 images, and no host resize), K20
    ``resize_pack`` launches (64 images each) resample, adapt the channels,
    scale, convert and pack them, and the [n, C, H, W] (or [n, H, W, C]) batch
    comes back as numpy.  ``antialias`` runs K21 ``resize_pack_aa`` (the
    device form of :func:`resize_area`) instead of K20.  An element may also be
    the ``bytes`` of a baseline JPEG file, which takes the first route of
    ``utils.jpeg_stage`` that the knobs allow: with ``device_huffman`` (default:
    ``TCAMD_DEVICE_HUFFMAN`` in the environment) K23, with
    ``device_huffman_wide`` (default: ``TCAMD_DEVICE_HUFFMAN_WIDE`` in the
    environment; the smallest blob in bytes, 0 is off) K24, and otherwise the
    host's entropy decoder, straight into the same upload.  K22 ``jpeg_decode``
    turns the coefficients into pixels in a device buffer that K20 / K21 read.
    If K23 or K24 leaves a non-zero status word the whole batch is done again
    with the host's entropy decoder, which gives the answer or raises the
    error.  ``jpeg_scale`` 2, 4 or 8 decodes the JPEGs at that fraction of
    their size (the host stores, and the upload carries, only the coefficients
    the reduced transform uses), 0 picks :func:`jpeg_auto_scale` per JPEG for
    the ``h x w`` target.  A ``bytes`` element with the PNG signature takes the
    PNG route of ``utils.jpeg_stage``: with ``device_png`` (default:
    ``TCAMD_DEVICE_PNG`` in the environment, 1 unless set to 0) and for a file
    that is not interlaced the host inflates the IDAT stream straight into the
    upload and K25 ``png_unfilter`` writes the pixels into the device-only
    allocation; otherwise the host decodes it and the pixels go up like an
    array's.  The result is the same bit for bit.  Returns None when the
    datatype has no device path (integer models)."""
    if dtype not in _DEVICE_DTYPES:
        return None
    import torch

    from triton_client_amd.ops import hip, host_codec
    from triton_client_amd.utils import jpeg_stage

    jpeg_scale = check_jpeg_scale(jpeg_scale)
    if device_huffman is None:
        device_huffman = jpeg_stage.device_huffman_knob()
    if device_huffman_wide is None:
        device_huffman_wide = jpeg_stage.device_huffman_wide_knob()
    if device_png is None:
        device_png = jpeg_stage.device_png_knob()
    items = []  # a uint8 HWC array, or (blob, parse) of a JPEG or of a PNG that K25 takes
    for im in images:
        if isinstance(im, (bytes, bytearray, memoryview)):
            blob = bytes(im)
            if blob[:8] == PNG_SIGNATURE:
                info = _png_codec().png_parse(blob)
                if device_png and not info.interlace:
                    items.append((blob, info))
                else:
                    items.append(_png_codec().png_decode(blob))
                continue
            items.append((blob, jpeg_stage.parse_at_scale(_jpeg_codec(), blob, jpeg_scale, h, w)))
            continue
        im = np.ascontiguousarray(im, dtype=np.uint8)
        items.append(im[:, :, None] if im.ndim == 2 else im)
    if any(max(im.shape[:2]) > hip.RESIZE_MAX_DIM or im.shape[2] not in (1, 3)
           for im in items if not isinstance(im, tuple)):
        return None
    dev = torch.device("cuda", device)
    # The upload (``up`` bytes): arrays as they are, host-decoded JPEG coefficient buffers at 128-byte
    # boundaries, packed JPEG streams and the staged bytes of PNGs at 16-byte boundaries.  In a second
    # allocation, on the device only (``only`` bytes): the coefficient buffers K23 / K24 write, at 128-byte
    # boundaries, and the pixels K22 / K25 write.
    codec = _jpeg_codec() if any(isinstance(im, tuple) for im in items) else None
    raws, jobs, pngs, up, only = [], [], [], 0, 0
    packs = {}  # row -> the stream its pack wrote
    for row, im in enumerate(items):
        if not isinstance(im, tuple):
            raws.append(jpeg_stage.RawImage(row, im, up, antialias))
            up += im.size
            continue
        blob, info = im
        if isinstance(info, host_codec.PngInfo):
            at = -(-up // 16) * 16
            up = at + info.stage_bytes
            pngs.append(jpeg_stage.PngJob(at, only, info, row, blob, antialias, 0))
            only += info.pixel_bytes
            continue
        room = None
        if device_huffman or device_huffman_wide:
            room = host_codec.aligned_buffer(max(codec.jpeg_stream_bound(len(blob)),
                                                 codec.jpeg_stream_bound_wide(len(blob))))
        packed = jpeg_stage.pack_stream(codec, blob, info, room, device_huffman, device_huffman_wide)
        if packed is not None:
            route, n, nsub = packed
            packs[row] = room[:n]
            at = -(-up // 16) * 16
            up = at + n
            coef = -(-only // 128) * 128
            only = coef + info.coef_bytes
        else:
            route, nsub, at = jpeg_stage.HOST, 0, None
            coef = -(-up // 128) * 128
            up = coef + info.coef_bytes
        jobs.append(jpeg_stage.JpegJob(route, at, coef, only, info, nsub, row, blob, antialias, 0))
        only += info.pixel_bytes
    raw = np.empty(up, dtype=np.uint8)
    for r in raws:
        raw[r.pix:r.pix + r.image.size] = r.image.reshape(-1)
    for j in jobs:
        if j.route == jpeg_stage.HOST:
            codec.jpeg_entropy_decode(j.blob, raw[j.coef:j.coef + j.info.coef_bytes], j.info.scale)
        else:
            raw[j.stream:j.stream + packs[j.row].size] = packs[j.row]
    for j in pngs:
        codec.png_inflate(j.blob, raw[j.stream:j.stream + j.info.stage_bytes])
    src = torch.from_numpy(raw).to(dev, non_blocking=False)
    stream = torch.cuda.current_stream(dev).cuda_stream
    scratch = torch.empty(only, device=dev, dtype=torch.uint8)
    nsubs = [j.nsub for j in jobs if j.route == jpeg_stage.K24]
    need = hip.jpeg_huffman_wide_workspace(nsubs) if nsubs else 0
    workspace = torch.empty(need, device=dev, dtype=torch.uint8)
    ran = jpeg_stage.launch_decode(hip, jobs, src.data_ptr(), scratch.data_ptr(), workspace.data_ptr(), need,
                                   lambda n: torch.empty(n, device=dev, dtype=torch.int32), stream, pngs=pngs)
    staged = sorted(jobs + pngs + raws, key=lambda j: j.row)
    shape = (len(items), c, h, w) if fmt == "NCHW" else (len(items), h, w, c)
    dst = torch.empty(shape, device=dev, dtype=torch.float32 if dtype == "FP32" else torch.float16)
    scale, bias = _SCALE_BIAS[scaling](c)
    per = c * h * w * dst.element_size()
    hip.resize_pack([(src if isinstance(j, jpeg_stage.RawImage) else scratch).data_ptr() + j.pix for j in staged],
                    [j.shape for j in staged], [dst.data_ptr() + j.row * per for j in staged], dtype, fmt, c, h, w,
                    scale=scale, bias=bias, stream=stream, antialias=antialias)
    out = dst.cpu().numpy()
    if any(status.cpu().numpy().any() for _, status in ran):
        return preprocess_raw_batch_device(images, c, h, w, scaling, fmt, dtype, device, antialias,
                                           device_huffman=False, jpeg_scale=jpeg_scale, device_huffman_wide=0,
                                           device_png=device_png)
    return out

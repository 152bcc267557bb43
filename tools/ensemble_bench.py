"""Closed-loop raw-image load on preprocess_inception_ensemble, and K20's own time.

    python tools/ensemble_bench.py                # served: bs 1, one 640x480 image, concurrency 1 and 8, gRPC
    python tools/ensemble_bench.py --kernel       # K20 resize_pack alone: 8 images 640x480 -> 224x224, HIP events
    python tools/ensemble_bench.py --antialias    # either mode with the antialiased resize (K21 resize_pack_aa)
    python tools/ensemble_bench.py --jpeg         # served: the committed 640x480 JPEG fixture instead of a TCIMG blob
    python tools/ensemble_bench.py --kernel --jpeg  # K22 jpeg_decode, K23 jpeg_huffman alone: 8 copies of that fixture
    python tools/ensemble_bench.py --png          # served: that fixture's pixels as a PNG, TCAMD_DEVICE_PNG 1 against 0
    python tools/ensemble_bench.py --kernel --png # K25 png_unfilter alone, next to the host's unfilter and inflate

The served mode starts the bench server (densenet_onnx, preprocess_inception
and the ensemble, 2 instances) as a child process, keeps ``--concurrency``
gRPC ``async_infer`` requests in flight, each one raw TCIMG blob (BYTES
[1, 1]), and prints one JSON line per concurrency: infer/s, p50/p99 request
latency and the server's time per preprocess_inception request.  It uses only
the public client API, so it runs unchanged on a tree whose
preprocess_inception is the numpy model.  ``--antialias`` sends the request
parameter ``antialias=true`` with every request (served) or times K21 in
place of K20 (``--kernel``).  ``--jpeg`` sends tests/golden/jpeg's 640x480
4:2:0 file, which the server Huffman-decodes on the host and finishes with K22
(``TCAMD_DEVICE_PREPROCESS=0`` in the environment: decodes on the host);
``--kernel --jpeg`` also times the host's entropy decode and full decode, and in
further JSON lines the wide stream pack (host) and the K24 ``jpeg_huffman_wide``
launch sequence on one and on 8 copies, with its chunks, launches and the
inter-chunk launches that changed something, and the stream pack (host) and K23
``jpeg_huffman`` on one and on 8 copies.  ``--huffman-wide N`` starts the served
loop's server with ``TCAMD_DEVICE_HUFFMAN_WIDE=N``.  ``--jpeg-scale N`` (1, 2, 4, 8, or 0 for the automatic scale of a
224 x 224 target) sends the request parameter ``jpeg_scale`` (served) or times
the reduced-size decode of K22 and of the host and prints the bytes of the
compact coefficient buffer (``--kernel --jpeg``; the K23 line is left out: K23
writes the full layout only).  ``--jpeg-file PATH`` takes another baseline JPEG
than the fixture, a large photo for instance.  ``TCAMD_DEVICE_HUFFMAN=1`` in the environment of a served run makes
the server pack the scan and run K23 instead of the host's entropy decode.

``--png`` is the counterpart of ``--jpeg``: the pixels of that fixture (its host
decode, 640 x 480 RGB) written as a PNG by this tool, with ``--png-filter``
choosing the filter of every row (``adaptive``, the default, picks per row the
filter with the smallest sum of absolute differences, as encoders do), or
``--png-file PATH`` for a file of another writer.  Served, it starts TWO
servers, ``TCAMD_DEVICE_PNG=1`` and ``=0``, and for ``--reps`` rounds and each
concurrency loads them in turn (only one at a time), each with the PNG blob and
with the TCIMG blob of the same pixels: one JSON line per round, concurrency,
arm and encoding, so that the arms alternate within one session on one box.
``--kernel --png`` times K25 ``png_unfilter`` on one image and on ``--images``
copies (HIP events around the launch), next to the host's ``png_unfilter`` and
``png_inflate`` on the same file.
"""

import argparse
import json
import os
import sys
import threading
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def kernel_time(n, h, w, iters, antialias=False):
    import numpy as np
    import torch

    from triton_client_amd.ops import hip
    from triton_client_amd.utils import image

    torch.cuda.set_device(0)
    rng = np.random.default_rng(0)
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(n)]
    src = torch.from_numpy(np.stack(imgs)).cuda()
    dst = torch.zeros(n, 3, 224, 224, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    srcs = [src[i].data_ptr() for i in range(n)]
    dsts = [dst[i].data_ptr() for i in range(n)]
    sizes = [(h, w, 3)] * n

    def launch():
        hip.resize_pack(srcs, sizes, dsts, "FP32", "NCHW", 3, 224, 224, scale=[1 / 127.5] * 3, bias=[-1.0] * 3,
                        stream=s, **({"antialias": True} if antialias else {}))

    for _ in range(10):
        launch()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launch()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    ref = image.preprocess(imgs[n - 1], 3, 224, 224, "INCEPTION", "NCHW", np.float64,
                           **({"antialias": True} if antialias else {}))
    err = float(np.abs(dst[n - 1].cpu().numpy().astype(np.float64) - ref).max())
    t0 = time.perf_counter()
    image.inception_preprocess(imgs[0], 224, 224, "NCHW", **({"antialias": True} if antialias else {}))
    host_ms = (time.perf_counter() - t0) * 1e3
    moved = n * (h * w * 3 + 3 * 224 * 224 * 4)
    print(json.dumps({"kernel": "K21 resize_pack_aa" if antialias else "K20 resize_pack", "images": n,
                      "src": [h, w, 3], "dst": [3, 224, 224],
                      "launches": iters, "mean_us": round(float(np.mean(times)), 2),
                      "min_us": round(float(np.min(times)), 2), "max_us": round(float(np.max(times)), 2),
                      "bytes_read_plus_written": moved, "gb_per_s_at_min": round(moved / np.min(times) / 1e3, 1),
                      "max_abs_err_vs_float64": err, "numpy_host_ms_per_image": round(host_ms, 3)}))


def jpeg_fixture(path=None):
    import glob

    if path:
        with open(path, "rb") as f:
            return f.read()
    (path,) = glob.glob(os.path.join(REPO, "tests", "golden", "jpeg", "b01_*.jpg"))
    with open(path, "rb") as f:
        return f.read()


def jpeg_kernel_time(n, iters, scale=1, path=None):
    import numpy as np
    import torch

    from triton_client_amd.ops import hip, host_codec

    torch.cuda.set_device(0)
    hc = host_codec.load()
    blob = jpeg_fixture(path)
    if scale == 0:
        from triton_client_amd.utils.image import jpeg_auto_scale

        full = hc.jpeg_parse(blob)
        scale = jpeg_auto_scale(full.h, full.w, 224, 224)
    info = hc.jpeg_parse(blob, scale)
    coef = np.empty(info.coef_bytes, dtype=np.uint8)
    host = {}
    for what, fn in (("entropy_decode", lambda: hc.jpeg_entropy_decode(blob, coef, scale)),
                     ("full_decode", lambda: hc.jpeg_decode(blob, scale))):
        fn()
        ts = []
        for _ in range(20):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        host[what] = ts
    want = hc.jpeg_decode(blob, scale)
    stride = -(-info.coef_bytes // 128) * 128
    src = torch.from_numpy(np.concatenate([np.pad(coef, (0, stride - coef.size))] * n)).cuda()
    dst = torch.zeros(n, info.pixel_bytes, device="cuda", dtype=torch.uint8)
    s = torch.cuda.current_stream().cuda_stream
    srcs = [src.data_ptr() + i * stride for i in range(n)]
    dsts = [dst[i].data_ptr() for i in range(n)]

    def launch():
        hip.jpeg_decode(srcs, [info] * n, dsts, stream=s)

    for _ in range(10):
        launch()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launch()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    equal = bool((dst.cpu().numpy().reshape((n,) + want.shape) == want).all())
    moved = n * (info.coef_bytes + info.pixel_bytes)
    print(json.dumps({"kernel": "K22 jpeg_decode", "images": n, "jpeg_scale": scale, "image": list(info.shape),
                      "sampling": [info.hs, info.vs], "jpeg_bytes": len(blob), "coef_bytes": int(info.coef_bytes),
                      "launches": iters, "mean_us": round(float(np.mean(times)), 2),
                      "min_us": round(float(np.min(times)), 2), "max_us": round(float(np.max(times)), 2),
                      "bytes_read_plus_written": moved, "gb_per_s_at_min": round(moved / np.min(times) / 1e3, 1),
                      "equals_host_decode": equal,
                      "host_entropy_decode_ms_min_mean": [round(float(np.min(host["entropy_decode"])), 3),
                                                          round(float(np.mean(host["entropy_decode"])), 3)],
                      "host_full_decode_ms_min_mean": [round(float(np.min(host["full_decode"])), 3),
                                                       round(float(np.mean(host["full_decode"])), 3)]}))
    jpeg_wide_line(hc, hip, blob, info, scale, coef, host, n, iters)
    if scale != 1:
        return  # K23 writes the full layout only

    # K23: the pack on the host, the Huffman stage on the device, against the host's entropy decode above
    packed = host_codec.aligned_buffer(hc.jpeg_stream_bound(len(blob)))
    _, used = hc.jpeg_stream_pack(blob, packed)
    if used is None:  # a scan above what K23's workspace holds (--jpeg-file): the host's entropy decoder's turn
        print(json.dumps({"kernel": "K23 jpeg_huffman", "packable": False}))
        return
    pack_ms = []
    for _ in range(20):
        t0 = time.perf_counter()
        hc.jpeg_stream_pack(blob, packed)
        pack_ms.append((time.perf_counter() - t0) * 1e3)
    sstride = -(-used // 16) * 16
    streams = torch.from_numpy(np.concatenate([np.pad(packed[:used], (0, sstride - used))] * n)).cuda()
    out = torch.zeros(n * stride, device="cuda", dtype=torch.uint8)
    status = torch.ones(n, device="cuda", dtype=torch.int32)
    sp = [streams.data_ptr() + i * sstride for i in range(n)]
    cp = [out.data_ptr() + i * stride for i in range(n)]
    huff = {}
    for m in (1, n):
        for _ in range(10):
            hip.jpeg_huffman(sp[:m], cp[:m], status.data_ptr(), stream=s)
        torch.cuda.synchronize()
        ts = []
        for _ in range(iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            hip.jpeg_huffman(sp[:m], cp[:m], status.data_ptr(), stream=s)
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b) * 1e3)
        huff[m] = ts
    got = out.cpu().numpy().reshape(n, stride)[:, :coef.size]
    print(json.dumps({"kernel": "K23 jpeg_huffman", "image": list(info.shape), "jpeg_bytes": len(blob),
                      "stream_bytes": int(used), "coef_bytes": int(info.coef_bytes), "launches": iters,
                      "one_image_us_min_mean": [round(float(np.min(huff[1])), 2), round(float(np.mean(huff[1])), 2)],
                      "images": n,
                      "all_images_us_min_mean": [round(float(np.min(huff[n])), 2), round(float(np.mean(huff[n])), 2)],
                      "status_all_zero": bool((status.cpu().numpy() == 0).all()),
                      "equals_host_entropy_decode": bool((got == coef).all()),
                      "host_stream_pack_ms_min_mean": [round(float(np.min(pack_ms)), 4),
                                                       round(float(np.mean(pack_ms)), 4)],
                      "host_entropy_decode_ms_min_mean": [round(float(np.min(host["entropy_decode"])), 3),
                                                          round(float(np.mean(host["entropy_decode"])), 3)]}))


_PNG_FILTERS = ("none", "sub", "up", "average", "paeth")


def write_png(img, how="adaptive"):
    """An 8-bit RGB or grey PNG of the uint8 HWC array ``img``: filter type ``how`` on every row, or
    per row the one of the five with the smallest sum of absolute (signed) differences."""
    import struct
    import zlib

    import numpy as np

    h, w, c = img.shape
    raw = img.reshape(h, w * c).astype(np.int16)
    left = np.concatenate([np.zeros((h, c), np.int16), raw[:, :-c]], axis=1)
    up = np.concatenate([np.zeros((1, w * c), np.int16), raw[:-1]], axis=0)
    upleft = np.concatenate([np.zeros((h, c), np.int16), up[:, :-c]], axis=1)
    p = left + up - upleft
    pa, pb, pc = np.abs(p - left), np.abs(p - up), np.abs(p - upleft)
    paeth = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, upleft))
    cand = np.stack([(raw - pred) & 0xff for pred in (0 * raw, left, up, (left + up) >> 1, paeth)]).astype(np.uint8)
    if how == "adaptive":
        pick = np.abs(cand.view(np.int8).astype(np.int32)).sum(axis=2).argmin(axis=0)
    else:
        pick = np.full(h, _PNG_FILTERS.index(how))
    rows = cand[pick, np.arange(h)]
    filt = np.concatenate([pick[:, None].astype(np.uint8), rows], axis=1).tobytes()

    def chunk(kind, data):
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xffffffff)

    return b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2 if c == 3 else 0, 0, 0, 0)) \
        + chunk(b"IDAT", zlib.compress(filt, 6)) + chunk(b"IEND", b"")


def png_fixture(args):
    """(the PNG blob, its pixels): ``--png-file``, or the JPEG fixture's host decode written by :func:`write_png`."""
    from triton_client_amd.ops import host_codec

    hc = host_codec.load()
    if args.png_file:
        with open(args.png_file, "rb") as f:
            blob = f.read()
    else:
        blob = write_png(hc.jpeg_decode(jpeg_fixture()), args.png_filter)
    return blob, hc.png_decode(blob)


def _host_ms(fn, n=20):
    fn()
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def png_kernel_time(args):
    import numpy as np
    import torch

    from triton_client_amd.ops import hip, host_codec

    torch.cuda.set_device(0)
    hc = host_codec.load()
    blob, want = png_fixture(args)
    info = hc.png_parse(blob)
    staged = host_codec.aligned_buffer(info.stage_bytes)
    inflate = _host_ms(lambda: hc.png_inflate(blob, staged))
    unfilter = _host_ms(lambda: hc.png_unfilter(staged, info))
    decode = _host_ms(lambda: hc.png_decode(blob))
    n = max(1, args.images)
    stride = -(-info.stage_bytes // 16) * 16
    src = torch.from_numpy(np.concatenate([np.pad(staged, (0, stride - staged.size))] * n)).cuda()
    dst = torch.zeros(n, info.pixel_bytes, device="cuda", dtype=torch.uint8)
    s = torch.cuda.current_stream().cuda_stream
    srcs = [src.data_ptr() + i * stride for i in range(n)]
    dsts = [dst[i].data_ptr() for i in range(n)]
    line = {"kernel": "K25 png_unfilter", "image": list(info.shape), "colour_type": info.ctype, "depth": info.depth,
            "filter": "file" if args.png_file else args.png_filter, "png_bytes": len(blob),
            "stage_bytes": int(info.stage_bytes), "pixel_bytes": int(info.pixel_bytes), "timed_launches": args.iters}
    rows = np.frombuffer(staged[:info.filtered_bytes], dtype=np.uint8).reshape(info.h, -1)[:, 0]
    line["rows_per_filter_type"] = [int((rows == f).sum()) for f in range(5)]
    for m in sorted({1, n}):
        def launch():
            hip.png_unfilter(srcs[:m], [info] * m, dsts[:m], stream=s)

        for _ in range(5):
            launch()
        torch.cuda.synchronize()
        times = []
        for _ in range(args.iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            launch()
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b) * 1e3)
        line["images_%d_us_min_mean_max" % m] = [round(float(f(times)), 1) for f in (np.min, np.mean, np.max)]
    line["equals_host_decode"] = bool((dst.cpu().numpy().reshape((n,) + want.shape) == want).all())
    for what, ts in (("host_png_inflate", inflate), ("host_png_unfilter", unfilter), ("host_png_decode", decode)):
        line[what + "_ms_min_mean"] = [round(float(np.min(ts)), 3), round(float(np.mean(ts)), 3)]
    print(json.dumps(line), flush=True)


def served_png(args):
    """Two servers, TCAMD_DEVICE_PNG=1 and =0, loaded in turn with the PNG and with its TCIMG twin."""
    import numpy as np

    import tritonclient.grpc as grpcclient
    from triton_client_amd.perf.harness import ServerProcess
    from triton_client_amd.utils.image import encode_raw

    blob, pixels = png_fixture(args)
    blobs = {"PNG": blob, "TCIMG": encode_raw(pixels)}
    log = os.path.abspath(args.server_log) if args.server_log else None
    if log:
        os.makedirs(os.path.dirname(log), exist_ok=True)
    servers, clients = {}, {}
    try:
        for knob in ("1", "0"):
            servers[knob] = ServerProcess(device=0, models="densenet_onnx,preprocess_inception,preprocess_inception_ensemble",
                                          log_path=log and "%s.png%s" % (log, knob), extra_args=["--instance-count", "2"],
                                          env={"TCAMD_DEVICE_PNG": knob})
        first = {}
        for knob, srv in servers.items():
            srv.wait_ready(timeout=900, model="preprocess_inception_ensemble")
            clients[knob] = grpcclient.InferenceServerClient(srv.grpc_url)
        inputs = {}
        for enc, b in blobs.items():
            inputs[enc] = grpcclient.InferInput("INPUT", [1, 1], "BYTES")
            inputs[enc].set_data_from_numpy(np.array([b], dtype=np.object_).reshape(1, 1))
        params = {"antialias": True} if args.antialias else None
        for knob, c in clients.items():
            for enc in blobs:
                first[knob, enc] = c.infer("preprocess_inception_ensemble", [inputs[enc]], parameters=params).as_numpy("OUTPUT")
        same = all(np.array_equal(v, first["1", "PNG"]) for v in first.values())
        for rep_ in range(args.reps):
            for conc in args.concurrency:
                for knob in ("1", "0"):
                    for enc in ("PNG", "TCIMG"):
                        res = closed_loop(clients[knob], grpcclient, inputs[enc], conc, args.warmup, args.seconds, params)
                        res.update(round=rep_, device_png=int(knob), encoding=enc, image=list(pixels.shape),
                                   blob_bytes=len(blobs[enc]), antialias=args.antialias,
                                   filter="file" if args.png_file else args.png_filter,
                                   all_four_first_answers_equal=bool(same))
                        print(json.dumps(res), flush=True)
        for c in clients.values():
            c.close()
    finally:
        for srv in servers.values():
            srv.stop()


def jpeg_wide_line(hc, hip, blob, info, scale, coef, host, n, iters):
    """K24: the wide pack on the host, the launch sequence of ``hip.jpeg_huffman_wide`` on one image and on
    ``n`` copies, against the host's entropy decode of the same run."""
    import numpy as np
    import torch

    from triton_client_amd.ops import host_codec

    packed = host_codec.aligned_buffer(hc.jpeg_stream_bound_wide(len(blob)))
    _, used, nsub = hc.jpeg_stream_pack_wide(blob, packed, scale)
    if used is None:
        print(json.dumps({"kernel": "K24 jpeg_huffman_wide", "packable": False}))
        return
    pack_ms = []
    for _ in range(20):
        t0 = time.perf_counter()
        hc.jpeg_stream_pack_wide(blob, packed, scale)
        pack_ms.append((time.perf_counter() - t0) * 1e3)
    _, changed = hc.jpeg_huffman_wide_emulate(packed[:used], np.empty(info.coef_bytes, dtype=np.uint8))
    chunks = -(-nsub // hip.JPEG_WIDE_CHUNK_SUBS)
    stride = -(-info.coef_bytes // 128) * 128
    sstride = -(-used // 16) * 16
    streams = torch.from_numpy(np.concatenate([np.pad(packed[:used], (0, sstride - used))] * n)).cuda()
    out = torch.zeros(n * stride, device="cuda", dtype=torch.uint8)
    status = torch.ones(n, device="cuda", dtype=torch.int32)
    need = hip.jpeg_huffman_wide_workspace([nsub] * n)
    ws = torch.empty(need, device="cuda", dtype=torch.uint8)
    s = torch.cuda.current_stream().cuda_stream
    sp = [streams.data_ptr() + i * sstride for i in range(n)]
    cp = [out.data_ptr() + i * stride for i in range(n)]
    wide = {}
    for m in (1, n):
        def call():
            hip.jpeg_huffman_wide(sp[:m], cp[:m], [nsub] * m, status.data_ptr(), ws.data_ptr(), need, stream=s)

        for _ in range(10):
            call()
        torch.cuda.synchronize()
        ts = []
        for _ in range(iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b) * 1e3)
        wide[m] = ts
    got = out.cpu().numpy().reshape(n, stride)[:, :coef.size]
    print(json.dumps({"kernel": "K24 jpeg_huffman_wide", "image": list(info.shape), "jpeg_scale": scale,
                      "jpeg_bytes": len(blob), "stream_bytes": int(used), "coef_bytes": int(info.coef_bytes),
                      "subsequences": nsub, "chunks": chunks, "launches_per_call": 6 + chunks,
                      "inter_chunk_launches_that_changed": changed, "workspace_bytes_one_image":
                      hip.jpeg_huffman_wide_workspace([nsub]), "timed_calls": iters,
                      "one_image_us_min_mean": [round(float(np.min(wide[1])), 2), round(float(np.mean(wide[1])), 2)],
                      "images": n,
                      "all_images_us_min_mean": [round(float(np.min(wide[n])), 2), round(float(np.mean(wide[n])), 2)],
                      "status_all_zero": bool((status.cpu().numpy() == 0).all()),
                      "equals_host_entropy_decode": bool((got == coef).all()),
                      "host_stream_pack_ms_min_mean": [round(float(np.min(pack_ms)), 4),
                                                       round(float(np.mean(pack_ms)), 4)],
                      "host_entropy_decode_ms_min_mean": [round(float(np.min(host["entropy_decode"])), 3),
                                                          round(float(np.mean(host["entropy_decode"])), 3)]}))


def closed_loop(c, grpcclient, inp, conc, warmup, seconds, params=None):
    lock = threading.Lock()
    done = threading.Event()
    state = {"lat": [], "errors": 0, "stop": False, "inflight": conc, "measure": False}

    def send():
        t0 = time.perf_counter()

        def cb(result, error):
            t1 = time.perf_counter()
            with lock:
                if error is not None:
                    state["errors"] += 1
                elif state["measure"]:
                    state["lat"].append(t1 - t0)
                again = not state["stop"]
                if not again:
                    state["inflight"] -= 1
                    if state["inflight"] == 0:
                        done.set()
            if again:
                send()

        c.async_infer("preprocess_inception_ensemble", [inp], callback=cb, parameters=params)

    def pre_stats():
        s = c.get_inference_statistics("preprocess_inception", as_json=True)["model_stats"][0]
        ok = s["inference_stats"]["success"]
        return int(ok.get("count", 0)), int(ok.get("ns", 0))

    for _ in range(conc):
        send()
    time.sleep(warmup)
    n0, ns0 = pre_stats()
    with lock:
        state["measure"] = True
        state["lat"] = []
    t0 = time.perf_counter()
    time.sleep(seconds)
    with lock:
        lat = list(state["lat"])
        state["measure"] = False
    dt = time.perf_counter() - t0
    n1, ns1 = pre_stats()
    with lock:
        state["stop"] = True
    done.wait(30)
    lat.sort()
    n = len(lat)
    return {
        "model": "preprocess_inception_ensemble", "batch": 1, "concurrency": conc, "seconds": round(dt, 2),
        "requests": n, "errors": state["errors"], "infer_per_s": round(n / dt, 1),
        "p50_ms": round(lat[n // 2] * 1e3, 3) if n else None,
        "p99_ms": round(lat[min(n - 1, int(n * 0.99))] * 1e3, 3) if n else None,
        "preprocess_us_per_request": round((ns1 - ns0) / 1e3 / max(1, n1 - n0), 1),
    }


def served(args):
    import numpy as np

    import tritonclient.grpc as grpcclient
    from triton_client_amd.perf.harness import ServerProcess
    from triton_client_amd.utils.image import encode_raw
    from triton_client_amd.utils.jpeg_stage import device_huffman_knob, device_huffman_wide_knob

    if args.huffman_wide is not None:
        os.environ["TCAMD_DEVICE_HUFFMAN_WIDE"] = str(args.huffman_wide)  # the server process inherits it
    log = os.path.abspath(args.server_log) if args.server_log else None
    if log:
        os.makedirs(os.path.dirname(log), exist_ok=True)
    srv = ServerProcess(device=0, models="densenet_onnx,preprocess_inception,preprocess_inception_ensemble",
                        log_path=log, extra_args=["--instance-count", "2"])
    try:
        srv.wait_ready(timeout=900, model="preprocess_inception_ensemble")
        img = np.random.default_rng(0).integers(0, 256, (args.height, args.width, 3), dtype=np.uint8)
        data = np.array([jpeg_fixture(args.jpeg_file) if args.jpeg else encode_raw(img)],
                        dtype=np.object_).reshape(1, 1)
        shape = [args.height, args.width, 3]
        if args.jpeg:
            from triton_client_amd.ops import host_codec

            shape = list(host_codec.load().jpeg_parse(data[0, 0]).shape)
        c = grpcclient.InferenceServerClient(srv.grpc_url)
        inp = grpcclient.InferInput("INPUT", [1, 1], "BYTES")
        inp.set_data_from_numpy(data)
        params = {"antialias": True} if args.antialias else {}
        if args.jpeg_scale is not None:
            params["jpeg_scale"] = args.jpeg_scale
        params = params or None
        first = c.infer("preprocess_inception_ensemble", [inp], parameters=params).as_numpy("OUTPUT")
        assert first.shape == (1, 1000), first.shape
        kind = c.get_model_config("preprocess_inception", as_json=True)["config"]["instance_group"][0]["kind"]
        for conc in args.concurrency:
            res = closed_loop(c, grpcclient, inp, conc, args.warmup, args.seconds, params)
            res.update(antialias=args.antialias, image=shape, preprocess_kind=kind,
                       encoding="JPEG" if args.jpeg else "TCIMG", jpeg_scale=args.jpeg_scale,
                       blob_bytes=len(data[0, 0]),
                       device_preprocess=os.environ.get("TCAMD_DEVICE_PREPROCESS", "1") != "0",
                       device_huffman=device_huffman_knob(), device_huffman_wide=device_huffman_wide_knob(),
                       top1=int(first[0].argmax()))
            print(json.dumps(res), flush=True)
        c.close()
    finally:
        srv.stop()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--kernel", action="store_true", help="time K20 alone instead of the served loop")
    ap.add_argument("--antialias", action="store_true",
                    help="the antialiased resize: request parameter antialias=true (served), K21 (--kernel)")
    ap.add_argument("--jpeg", action="store_true",
                    help="the committed 640x480 JPEG fixture: as the request's blob (served), K22 alone (--kernel)")
    ap.add_argument("--jpeg-scale", type=int, choices=[0, 1, 2, 4, 8], default=None,
                    help="the reduced-size JPEG decode: request parameter jpeg_scale (served), K22 at that scale "
                         "(--kernel --jpeg); 0 is the automatic scale for 224 x 224")
    ap.add_argument("--jpeg-file", default="", metavar="PATH", help="--jpeg: this baseline JPEG instead of the fixture")
    ap.add_argument("--huffman-wide", type=int, default=None, metavar="N",
                    help="served: start the server with TCAMD_DEVICE_HUFFMAN_WIDE=N (JPEG blobs of at least N bytes "
                         "take the K24 jpeg_huffman_wide kernels; 0 = off)")
    ap.add_argument("--png", action="store_true",
                    help="the JPEG fixture's pixels as a PNG: served by two servers, TCAMD_DEVICE_PNG=1 and =0, in turn, "
                         "next to the TCIMG of the same pixels; K25 alone (--kernel)")
    ap.add_argument("--png-filter", choices=("adaptive",) + _PNG_FILTERS, default="adaptive",
                    help="--png: the filter type of every row of the PNG this tool writes")
    ap.add_argument("--png-file", default="", metavar="PATH", help="--png: this PNG file instead")
    ap.add_argument("--reps", type=int, default=3, help="--png, served: rounds over the concurrencies and arms")
    ap.add_argument("--concurrency", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--warmup", type=float, default=3.0)
    ap.add_argument("--images", type=int, default=8, help="--kernel: images per launch")
    ap.add_argument("--iters", type=int, default=50, help="--kernel: timed launches (after 10 warm-up)")
    ap.add_argument("--server-log", default="", metavar="PATH", help="keep the server's log in this file")
    args = ap.parse_args()
    if args.png:
        (png_kernel_time if args.kernel else served_png)(args)
    elif args.kernel and args.jpeg:
        jpeg_kernel_time(args.images, args.iters, 1 if args.jpeg_scale is None else args.jpeg_scale, args.jpeg_file)
    elif args.kernel:
        kernel_time(args.images, args.height, args.width, args.iters, args.antialias)
    else:
        served(args)


if __name__ == "__main__":
    main()

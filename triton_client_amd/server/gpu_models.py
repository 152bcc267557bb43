"""GPU model backends of the bench server (torch-ROCm + in-tree HIP kernels).

``densenet_onnx`` — the BASELINE model (FP32 ``data_0`` [3,224,224] NCHW in,
FP32 ``fc6_1`` [1000] out; same I/O contract as Triton's densenet_onnx example)
served with dynamic batching on one MI355X:

  request inputs (device shm views / host tensors)
    --pointer table (one 1 KB H2D)--> HIP graph replay of DenseNet-121 on
        hand-written MFMA kernels whose first kernel reads every image
        straight from its request's fp32 NCHW region (the batch is never
        assembled).  engine="fp32" (default, the model's FP32 contract):
        split-precision bf16x3 kernels K8x-K10x (models/densenet_fp32.py),
        logits within ~4e-5 rel-L2 of the fp32 module.  engine="fused": the
        bf16 K8-K10 kernels (models/densenet_fused.py), ~2.2x faster, ~3e-2
        off fp32 — a labelled reduced-precision operating point.
        engine="torch" keeps the MIOpen per-op bf16 module, fed by K6
        layout_pack (gather+transpose+cvt into one bf16 NHWC batch buffer)
    --K7 batched_copy--> each request's fp32 logits straight into its output
                         device-shm region (one launch per batch)

Host (non-shm) inputs are staged through pinned memory; host outputs come back
with one D2H of the whole batch.  Each model instance owns a torch stream, its
graphs (one per batch bucket) and static buffers, so ``instance_count``
batches pipeline on separate HIP streams.

The other models here follow the same pattern; the slot pool, the base classes
and the staging helpers they share are in server/device_slots.py.
"""

import ctypes
import os

import numpy as np

from triton_client_amd.utils import jpeg_stage, roctx

from . import cpu_models as _cpu
from .device_slots import (DeviceModel, Ensemble, download, pinned_view, place_input, plan_errors, stage_input,
                           stage_texts)
from .model_base import TensorSpec
from .types import DeviceView, OutputTensor, ServerError

# HIP-graph batch buckets: powers of two up to 16, then every 8 rows to 128 and
# every 16 to 256.  A batch runs the smallest bucket that holds it, and the
# padding rows cost full compute: under the headline load (bs8 requests, 128-row
# preferred batches) batches average 109-124 rows, which power-of-two buckets
# padded to 128 (3-15% of the device time spent on padding)
BUCKETS = (1, 2, 4, 8, 12, 16, 20) + tuple(range(24, 129, 8)) + tuple(range(144, 257, 16))


class DensenetOnnx(DeviceModel):
    name = "densenet_onnx"
    platform = "onnxruntime_onnx"
    backend = "onnxruntime"
    max_batch_size = 128
    inputs = (TensorSpec("data_0", "FP32", [3, 224, 224], fmt="NCHW"),)
    outputs = (TensorSpec("fc6_1", "FP32", [1000], label_filename="densenet_labels.txt"),)
    # pipelined: tcserve dispatches a partial batch to a free instance once the
    # queue holds as many rows as the last batch (bs1 closed loops)
    dynamic_batching = {"preferred": [], "max_queue_delay_us": 500, "pipelined": True}
    instance_kind = "KIND_GPU"
    instance_count = 2
    gpus = (0,)
    labels = ["class_%d" % i for i in range(1000)]

    C, H, W = 3, 224, 224
    OUT = 1000

    ENGINES = ("fp32", "fused", "torch")

    def __init__(self, version=1, device_id=0, buckets=BUCKETS, use_graphs=True, engine="fp32", max_batch_size=0,
                 **kw):
        super().__init__(version, device_id, **kw)
        if engine not in self.ENGINES:
            raise ServerError("unknown densenet engine %r" % engine)
        self.engine = engine
        if max_batch_size:
            # option max_batch_size: the HIP-graph buckets up to it (BUCKETS).
            # The fused engine's device throughput keeps growing with the rows
            # per forward: on MI355X (tools/engine_streams_bench.py) ~64k
            # img/s with 128-row forwards on 3-4 streams, ~70k with 256-row
            # forwards on 2 streams.
            if int(max_batch_size) not in buckets:
                raise ServerError("max_batch_size must be one of %s" % (tuple(buckets),))
            self.max_batch_size = int(max_batch_size)
        self.buckets = tuple(b for b in buckets if b <= self.max_batch_size)
        self.use_graphs = use_graphs

    # -- load ----------------------------------------------------------------------
    def load(self):
        from triton_client_amd.models import densenet

        torch, _, dev = self._gpu("densenet_onnx requires a GPU")
        torch.cuda.set_device(self.device_id)
        if self.engine == "fp32":
            from triton_client_amd.models import densenet_fp32

            self.model, _ = densenet_fp32.build(max(self.buckets), device=dev)
        elif self.engine == "fused":
            from triton_client_amd.models import densenet_fused

            self.model, _ = densenet_fused.build(max(self.buckets), device=dev)
        else:
            self.model = densenet.build(device=dev)
        self.scale = None
        # the instances' streams run concurrently: engines route small batches for that
        self.model.concurrent_streams = max(1, self.instance_count)
        for _ in range(max(1, self.instance_count)):
            self._slots.add(self._make_slot(dev))
        self._pgx = None
        if self.engine != "torch" and self.use_graphs and os.environ.get("TCAMD_NATIVE_EXEC", "1") != "0":
            self._pgx = self._make_executor()

    def _make_executor(self):
        """C++ per-batch dispatch (csrc/runtime/graph_exec.hip): pointer table,
        graph replay, output scatter and the completion wait run in the server's
        batcher thread without Python (the GIL stays out of the request path)."""
        from triton_client_amd.ops import hip

        x = hip.PtrGraphExecutor(self.device_id, len(self._slots), self.C * self.H * self.W * 4, self.OUT * 4,
                                 self.buckets)
        for i, slot in enumerate(self._slots):
            execs = [slot["graphs"][b].raw_cuda_graph_exec() for b in self.buckets]
            x.bind(i, slot["stream"].cuda_stream, execs, slot["net"].ptrs.data_ptr(), slot["stage_dev"].data_ptr(),
                   slot["out"].data_ptr(), slot["pad_ptrs"])
        return x

    def native_executor(self):
        """(tcserve_exec_fn address, user pointer) of the C++ executor, or None."""
        if self._pgx is None:
            return None
        return self._pgx.fn_address, self._pgx.handle

    @property
    def native_topk(self):
        """The C++ executor answers classification requests with device-selected
        pairs (TcBatch.class_counts); the Python execute_native does not."""
        return getattr(self, "_pgx", None) is not None

    def executor_stats(self):
        return None if self._pgx is None else self._pgx.stats()

    def _make_slot(self, dev):
        torch = self.torch
        net = self.model
        if self.engine != "torch" and len(self._slots):
            net = self.model.with_workspace()  # own activation buffers per concurrent stream
        slot = {"stream": torch.cuda.Stream(device=dev), "graphs": {}, "net": net,
                "ev": [torch.cuda.Event(enable_timing=True) for _ in range(4)]}
        maxb = max(self.buckets)
        img_bytes = self.C * self.H * self.W * 4
        fused = self.engine != "torch"  # pointer-table engines (fp32 / bf16 fused kernels)
        slot["out"] = torch.zeros(maxb, self.OUT, device=dev, dtype=torch.float32)
        self._pinned(slot, "stage_host", maxb * img_bytes)
        slot["stage_dev"] = torch.zeros(maxb * self.C * self.H * self.W, device=dev, dtype=torch.float32)
        self._pinned(slot, "out_host", maxb * self.OUT * 4)
        if fused:
            # padded rows of a bucket read (finite) staging images, never a stale request region
            pad = np.arange(maxb, dtype=np.int64) * img_bytes + slot["stage_dev"].data_ptr()
            slot["pad_ptrs"] = pad
            slot["ptrs_tbl"] = pinned_view(self._pinned(slot, "ptrs_host", maxb * 8), np.int64, maxb)
            net.ptrs.copy_(torch.from_numpy(pad))

            def run(b):
                return net.forward_ptrs(b, out=slot["out"])
        else:
            slot["inp"] = torch.zeros(maxb, self.H, self.W, self.C, device=dev, dtype=torch.bfloat16)

            def run(b):
                x = slot["inp"][:b].permute(0, 3, 1, 2)  # NCHW view of NHWC memory
                return slot["out"][:b].copy_(net(x).float())
        with torch.cuda.stream(slot["stream"]), torch.no_grad():
            for b in self.buckets:
                for _ in range(2):  # warm up library kernel selection
                    run(b)
                if self.use_graphs:
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g, stream=slot["stream"]):
                        run(b)
                    slot["graphs"][b] = g
        slot["stream"].synchronize()
        return slot

    def unload(self):
        if getattr(self, "_pgx", None) is not None:
            self._pgx.close()
            self._pgx = None
        super().unload()

    # -- execute ----------------------------------------------------------------------
    def forward_device(self, slot, srcs, rows):
        """Assemble ``rows`` images from device pointers and run the model."""
        with roctx.range("densenet_onnx.forward rows=%d" % rows):
            return self._forward_device(slot, srcs, rows)

    def _forward_device(self, slot, srcs, rows):
        torch = self.torch
        from triton_client_amd.ops import hip

        bucket = next(b for b in self.buckets if b >= rows)
        stream = slot["stream"]
        sh = stream.cuda_stream
        fused = self.engine != "torch"
        slot["ev"][0].record(stream)
        if fused:
            tbl = slot["ptrs_tbl"]
            tbl[:rows] = srcs
            tbl[rows:bucket] = slot["pad_ptrs"][rows:bucket]
            hip.memcpy_async(slot["net"].ptrs.data_ptr(), slot["ptrs_host"], bucket * 8, sh)
        else:
            hip.layout_pack(srcs, "FP32", "NCHW", slot["inp"].data_ptr(), "BF16", "NHWC",
                            self.C, self.H, self.W, rounding="rne", stream=sh)
        slot["ev"][1].record(stream)
        if self.use_graphs:
            with torch.cuda.stream(stream):
                slot["graphs"][bucket].replay()
        else:
            with torch.cuda.stream(stream), torch.no_grad():
                if fused:
                    slot["net"].forward_ptrs(bucket, out=slot["out"])
                else:
                    x = slot["inp"][:bucket].permute(0, 3, 1, 2)
                    slot["out"][:bucket].copy_(slot["net"](x).float())
        slot["ev"][2].record(stream)
        return bucket

    def execute(self, requests):
        img_bytes = self.C * self.H * self.W * 4
        out_row = self.OUT * 4
        rows = 0
        plan = []  # (request, first_row, nrows)
        for r in requests:
            t = r.input("data_0")
            n = int(t.shape[0])
            plan.append((r, rows, n))
            rows += n
        if rows > max(self.buckets):
            return [ServerError("batch of %d rows exceeds the largest bucket" % rows)] * len(requests)
        if getattr(self, "_pgx", None) is not None:
            return self._execute_pgx(plan, rows, img_bytes, out_row)
        try:
            with self._slots.slot() as (_, slot):
                return self._execute(slot, requests, plan, rows, img_bytes, out_row)
        except ServerError as e:
            return [e] * len(requests)

    def _execute(self, slot, requests, plan, rows, img_bytes, out_row):
        from triton_client_amd.ops import hip

        stream = slot["stream"]
        sh = stream.cuda_stream
        srcs = []
        host_rows = 0
        for r, first, n in plan:
            t = r.input("data_0")
            if isinstance(t.data, DeviceView):
                if t.data.nbytes < n * img_bytes:
                    raise ServerError("input region too small for data_0")
                srcs += [t.data.ptr + k * img_bytes for k in range(n)]
            else:
                a = np.ascontiguousarray(t.data, dtype=np.float32)
                np.copyto(pinned_view(slot["stage_host"] + host_rows * img_bytes, np.float32, a.size), a.reshape(-1))
                srcs += [slot["stage_dev"].data_ptr() + (host_rows + k) * img_bytes for k in range(n)]
                host_rows += n
        if host_rows:
            hip.memcpy_async(slot["stage_dev"].data_ptr(), slot["stage_host"], host_rows * img_bytes, sh)
        self.forward_device(slot, srcs, rows)
        # outputs: device-shm targets get a K7 scatter, the rest one D2H
        out_base = slot["out"].data_ptr()
        c_src, c_dst, c_n = [], [], []
        need_host = False
        results = []
        for r, first, n in plan:
            ro = next((o for o in r.outputs if o.name == "fc6_1"), None)
            target = None
            if ro is not None and ro.shm is not None and ro.class_count == 0:
                target = self._server_target(r, ro)
            if isinstance(target, DeviceView):
                if target.nbytes < n * out_row:
                    raise ServerError(
                        "shared memory size specified with the request for output 'fc6_1' "
                        "(%d bytes) should be at least %d bytes" % (target.nbytes, n * out_row)
                    )
                c_src.append(out_base + first * out_row)
                c_dst.append(target.ptr)
                c_n.append(n * out_row)
                results.append(("shm", ro))
            else:
                need_host = True
                results.append(("host", None))
        if c_src:
            hip.batched_copy(c_src, c_dst, c_n, sh)
        if need_host:
            hip.memcpy_async(slot["out_host"], out_base, rows * out_row, sh)
        slot["ev"][3].record(stream)
        stream.synchronize()
        if self._batch_stats is not None:
            ev = slot["ev"]
            ms_in, ms_inf, ms_out = (ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2]),
                                     ev[2].elapsed_time(ev[3]))
            self._batch_stats(rows, len(requests), int(ms_in * 1e6), int(ms_inf * 1e6), int(ms_out * 1e6))
        host_all = None
        if need_host:
            host_all = pinned_view(slot["out_host"], np.float32, rows * self.OUT).reshape(rows, self.OUT).copy()
        out = []
        for (r, first, n), (kind, ro) in zip(plan, results):
            if kind == "shm":
                o = OutputTensor("fc6_1", "FP32", [n, self.OUT], None, shm=ro.shm)
            else:
                o = OutputTensor("fc6_1", "FP32", [n, self.OUT], host_all[first : first + n])
            out.append([o])
        return out

    def _execute_pgx(self, plan, rows, img_bytes, out_row):
        """Python-scheduled batch through the same C++ executor tcserve uses."""
        from .native_frontend import TcBatch, TcRef

        n = len(plan)
        ins = (TcRef * n)()
        outs = (TcRef * n)()
        keep, results = [], []
        try:
            for j, (r, first, k) in enumerate(plan):
                t = r.input("data_0")
                if isinstance(t.data, DeviceView):
                    if t.data.nbytes < k * img_bytes:
                        raise ServerError("input region too small for data_0")
                    ins[j] = TcRef(1, self.device_id, t.data.ptr, t.data.nbytes)
                else:
                    a = np.ascontiguousarray(t.data, dtype=np.float32)
                    keep.append(a)
                    ins[j] = TcRef(0, 0, a.ctypes.data, a.nbytes)
                ro = next((o for o in r.outputs if o.name == "fc6_1"), None)
                target = None
                if ro is not None and ro.shm is not None and ro.class_count == 0:
                    target = self._server_target(r, ro)
                if isinstance(target, DeviceView):
                    if target.nbytes < k * out_row:
                        raise ServerError(
                            "shared memory size specified with the request for output 'fc6_1' "
                            "(%d bytes) should be at least %d bytes" % (target.nbytes, k * out_row)
                        )
                    outs[j] = TcRef(1, self.device_id, target.ptr, target.nbytes)
                    results.append(("shm", ro, None))
                else:
                    host = np.empty((k, self.OUT), dtype=np.float32)
                    outs[j] = TcRef(0, 0, host.ctypes.data, host.nbytes)
                    results.append(("host", None, host))
            nrows = (ctypes.c_int32 * n)(*[k for _, _, k in plan])
            timing = (ctypes.c_uint64 * 3)()
            b = TcBatch(n, rows, nrows, 1, ins, 1, outs, timing)
            with self._slots.slot() as (i, _):
                try:
                    self._pgx.execute(i, ctypes.addressof(b))
                except RuntimeError as e:
                    raise ServerError(str(e)) from e
        except ServerError as e:
            return [e] * n
        if self._batch_stats is not None:
            self._batch_stats(rows, n, int(timing[0]), int(timing[1]), int(timing[2]))
        out = []
        for (r, first, k), (kind, ro, host) in zip(plan, results):
            if kind == "shm":
                out.append([OutputTensor("fc6_1", "FP32", [k, self.OUT], None, shm=ro.shm)])
            else:
                out.append([OutputTensor("fc6_1", "FP32", [k, self.OUT], host)])
        return out

    # -- native fast path (tcserve, csrc/cpp/server) ------------------------------------
    supports_native = True

    def execute_native(self, instance, b):
        """One dynamic batch assembled by the C++ front end: raw device / host
        pointers in, outputs written straight to their targets."""
        from triton_client_amd.ops import hip

        img_bytes = self.C * self.H * self.W * 4
        out_row = self.OUT * 4
        total = int(b.total_rows)
        if total > max(self.buckets):
            raise ServerError("batch of %d rows exceeds the largest bucket" % total)
        i = self._slots.acquire()
        slot = self._slots[i]
        try:
            stream = slot["stream"]
            sh = stream.cuda_stream
            srcs, plan = [], []
            host_rows = first = 0
            stage_dev = slot["stage_dev"].data_ptr()
            for r in range(b.n_requests):
                rows = int(b.rows[r])
                ref = b.inputs[r * b.n_inputs]
                if ref.kind == 1:
                    srcs += [ref.ptr + k * img_bytes for k in range(rows)]
                else:  # in-band tensor or system shm: stage through pinned memory
                    ctypes.memmove(slot["stage_host"] + host_rows * img_bytes, ref.ptr, rows * img_bytes)
                    srcs += [stage_dev + (host_rows + k) * img_bytes for k in range(rows)]
                    host_rows += rows
                plan.append((first, rows))
                first += rows
            if host_rows:
                hip.memcpy_async(stage_dev, slot["stage_host"], host_rows * img_bytes, sh)
            self.forward_device(slot, srcs, total)
            out_base = slot["out"].data_ptr()
            c_src, c_dst, c_n, host_outs = [], [], [], []
            for r, (f, rows) in enumerate(plan):
                ref = b.outputs[r * b.n_outputs]
                if not ref.ptr:
                    continue
                if ref.kind == 1:
                    c_src.append(out_base + f * out_row)
                    c_dst.append(ref.ptr)
                    c_n.append(rows * out_row)
                else:
                    host_outs.append((ref.ptr, f, rows))
            if c_src:
                hip.batched_copy(c_src, c_dst, c_n, sh)
            if host_outs:
                hip.memcpy_async(slot["out_host"], out_base, total * out_row, sh)
            ev = slot["ev"]
            ev[3].record(stream)
            hip.stream_synchronize(sh)  # ctypes call: the GIL is released while the GPU runs
            for ptr, f, rows in host_outs:
                ctypes.memmove(ptr, slot["out_host"] + f * out_row, rows * out_row)
            b.timing_ns[0] = int(ev[0].elapsed_time(ev[1]) * 1e6)
            b.timing_ns[1] = int(ev[1].elapsed_time(ev[2]) * 1e6)
            b.timing_ns[2] = int(ev[2].elapsed_time(ev[3]) * 1e6)
        finally:
            self._slots.release(i)

    _server = None
    # set by the scheduler: (rows, n_requests, compute_input_ns, compute_infer_ns, compute_output_ns)
    _batch_stats = None
    reports_batch_stats = True

    def _server_target(self, r, ro):
        region, nbytes, offset = ro.shm
        return self._server.shm_target(region, nbytes, offset)


class PreprocessInception(DeviceModel):
    """``preprocess_inception`` on the GPU: the same I/O contract as the CPU
    model of that name (BYTES PPM / PGM / TCIMG / JPEG / PNG blobs in, INCEPTION-scaled
    FP32 NCHW [3,224,224] out), which it replaces on a ``--gpu`` server.

    Per batch the host only parses each blob's header and copies its uint8
    pixels into a pinned staging area; one H2D copy and one K20 ``resize_pack``
    launch per 64 images (csrc/kernels/resize.hip) resample, scale and pack
    them into a device fp32 [rows, 3, 224, 224] tensor.  A request that the
    server marked as an ensemble step (``accepts_device_outputs`` on the
    internal request, core._infer_ensemble) gets its rows back as a
    ``DeviceView`` with the owning tensor attached, so ``densenet_onnx`` puts
    them straight into its pointer table; a direct request gets them copied to
    the host.  Blobs that do not fit the staging area or exceed K20's size
    limit take the numpy routine.  ``TCAMD_DEVICE_PREPROCESS=0`` (read at
    load) runs the numpy step for everything.

    A baseline JPEG blob is routed by ``utils.jpeg_stage``, which defines the
    routes, their order and the layout of the staging area: by default the host
    Huffman-decodes it straight into the pinned staging area;
    ``TCAMD_DEVICE_HUFFMAN=1`` and ``TCAMD_DEVICE_HUFFMAN_WIDE=N`` (both read
    at load) have the host only pack the scan, and K23 ``jpeg_huffman`` or the
    K24 ``jpeg_huffman_wide`` kernels decode it on the device.  K22
    ``jpeg_decode`` turns the coefficients of every route into pixels, which
    K20 / K21 read like any staged image; all of it runs on the slot's stream,
    K23, K24, K22 and then the resize.  What this model adds to that module's
    contract: a JPEG that fits no route is decoded on the host and goes on as
    raw pixels; a request that raises takes everything it staged back out of
    the plan; an image whose status word K23 or K24 left non-zero (read after
    the stream synchronise) is decoded by the host, which fills its row or
    fails its request, and that request alone, with the host decoder's message.

    A PNG blob that is not interlaced takes the same module's PNG route
    (``TCAMD_DEVICE_PNG``, read at load; 1 by default): the host parses its
    headers and inflates its IDAT stream straight into the pinned staging area,
    the filtered scanlines go up in the batch's one copy, and K25
    ``png_unfilter`` writes the pixels where K20 / K21 read them, after the JPEG
    kernels and before the resize on the slot's stream.  An interlaced PNG, one
    that does not fit, or any PNG with the knob at 0 is decoded by the host and
    goes on as raw pixels; the rows are the same bit for bit.  A PNG that does
    not decode fails its own request with the host decoder's message.

    The custom request parameter ``antialias`` (bool, default false) selects
    the antialiased resize for that request's images: the batch's device jobs
    are split by the flag into at most one K20 and one K21 ``resize_pack``
    call, both on the slot's stream, and the host fallbacks use
    ``utils.image.resize_area``.

    The custom request parameter ``jpeg_scale`` (int64: 1, 2, 4 or 8, or 0 for
    ``utils.image.jpeg_auto_scale`` against the model's H x W; without it a
    request is served at full size, as before) decodes that request's JPEG
    blobs at 1/2, 1/4 or 1/8 size in the DCT domain: the host's entropy
    decoder stores only the coefficients the reduced transform uses, the
    staging-area fit test counts the compact coefficient buffer and the reduced
    pixels (a 12-megapixel 4:2:0 photo needs about 1.7 MB at 1/8 instead of
    72 MB), and K22 decodes the images of all scales of a batch in the same
    ``jpeg_decode`` call.  The host fallbacks decode at the same scale, so
    every route gives the same rows.  PPM / PGM / TCIMG / PNG blobs ignore the parameter;
    any other value fails that request alone."""

    name = "preprocess_inception"
    max_batch_size = 8
    inputs = (TensorSpec("INPUT", "BYTES", [1]),)
    outputs = (TensorSpec("OUTPUT", "FP32", [3, 224, 224]),)
    dynamic_batching = {"preferred": [], "max_queue_delay_us": 100}
    instance_kind = "KIND_GPU"
    instance_count = 2
    gpus = (0,)

    C, H, W = 3, 224, 224
    STAGE_BYTES = 32 << 20  # pinned + device uint8 staging per instance (8 images of 1280x1024x3)

    def load(self):
        self.device_huffman = jpeg_stage.device_huffman_knob()
        self.device_huffman_wide = jpeg_stage.device_huffman_wide_knob()
        self.device_png = jpeg_stage.device_png_knob()
        if not self._load_twin(_cpu.PreprocessInception, os.environ.get("TCAMD_DEVICE_PREPROCESS", "1") != "0"):
            return
        from triton_client_amd.ops import host_codec

        self._codec = host_codec.load()  # the JPEG entropy decoder and the PNG inflate
        torch, _, dev = self._gpu()
        for _ in range(max(1, self.instance_count)):
            slot = {"stream": torch.cuda.Stream(device=dev),
                    "stage_dev": torch.empty(self.STAGE_BYTES, device=dev, dtype=torch.uint8)}
            slot["stage_np"] = pinned_view(self._pinned(slot, "stage_host", self.STAGE_BYTES), np.uint8,
                                           self.STAGE_BYTES)
            self._slots.add(slot)

    def unload(self):
        for s in self._slots:
            s.pop("stage_np", None)  # the view goes before the memory under it
        super().unload()

    def _host_one(self, r):
        try:
            return self._host.execute([r])[0]
        except Exception as e:  # noqa: BLE001 - per-request failure, the CPU model's own error
            return e

    def _open(self, blob, scale=1):
        """A decoded image, or (blob, parse) of a JPEG or a non-interlaced PNG whose decode is
        still to be routed; ``scale`` is the request's ``jpeg_scale``, 0 for automatic."""
        from triton_client_amd.utils.image import PNG_SIGNATURE, decode_image

        blob = bytes(blob)
        if blob[:2] == b"\xff\xd8":
            return blob, jpeg_stage.parse_at_scale(self._codec, blob, scale, self.H, self.W)
        if self.device_png and blob[:8] == PNG_SIGNATURE:
            info = self._codec.png_parse(blob)
            if not info.interlace:
                return blob, info
        return decode_image(blob)

    def _read_status(self, status):
        """The status words K23 or K24 left for a batch, after the stream synchronise."""
        return status.cpu().numpy()

    def execute(self, requests):
        if not self.device_path:
            return [self._host_one(r) for r in requests]
        # before the plan: JPEG coefficients are decoded straight into the slot's staging area
        with self._slots.slot() as (_, slot):
            return self._execute(slot, requests)

    def _execute(self, slot, requests):
        from triton_client_amd.ops import hip, host_codec
        from triton_client_amd.utils.image import inception_preprocess

        img_bytes = self.C * self.H * self.W * 4
        stage = jpeg_stage.StagePlan(slot["stage_np"][:self.STAGE_BYTES], self._codec, self.device_huffman,
                                     self.device_huffman_wide, hip.RESIZE_MAX_DIM)
        plan = []  # per request: (first_row, n_rows), or its exception
        for r in requests:
            mark = stage.mark()
            try:
                aa = self._host.wants_antialias(r)
                scale = self._host.jpeg_scale_of(r)
                for item in [self._open(b, scale) for b in r.input("INPUT").numpy().reshape(-1)]:
                    if isinstance(item, tuple):
                        blob, info = item
                        if isinstance(info, host_codec.PngInfo):
                            if stage.add_png(blob, info, aa, len(plan)) is not None:
                                continue
                            item = self._codec.png_decode(blob)
                        else:
                            if stage.add_jpeg(blob, info, aa, len(plan)) is not None:
                                continue
                            item = self._codec.jpeg_decode(blob, info.scale)
                    stage.add_raw(item, aa)
            except Exception as e:  # noqa: BLE001 - an undecodable blob fails its own request
                stage.rollback(mark)
                plan.append(e)
                continue
            plan.append((mark[0], stage.rows - mark[0]))
        rows = stage.rows
        if rows == 0:
            return plan
        torch = self.torch
        stream = slot["stream"]
        sh = stream.cuda_stream
        with roctx.range("preprocess_inception rows=%d" % rows), torch.cuda.stream(stream):
            out = torch.empty((rows, self.C, self.H, self.W), device=stream.device, dtype=torch.float32)
            base = out.data_ptr()
            src = slot["stage_dev"].data_ptr()
            if stage.used:
                hip.memcpy_async(src, slot["stage_host"], stage.used, sh)
            ran = jpeg_stage.launch_decode(
                hip, stage.jpegs, src, src, src + stage.workspace, stage.ws_need - 16,
                lambda n: torch.empty(n, device=stream.device, dtype=torch.int32), sh, pngs=stage.pngs)
            staged = sorted(stage.jpegs + stage.pngs + [j for j in stage.raws if j.pix is not None],
                            key=lambda j: j.row)
            for aa in (False, True):
                jobs = [j for j in staged if j.antialias == aa]
                if jobs:
                    hip.resize_pack([src + j.pix for j in jobs], [j.shape for j in jobs],
                                    [base + j.row * img_bytes for j in jobs], "FP32", "NCHW",
                                    self.C, self.H, self.W, scale=[1.0 / 127.5] * 3, bias=[-1.0] * 3,
                                    stream=sh, antialias=aa)
            for j in stage.raws:
                if j.pix is None:
                    out[j.row].copy_(torch.from_numpy(inception_preprocess(j.image, self.H, self.W, "NCHW",
                                                                           antialias=j.antialias)))
            want_host = any(not isinstance(p, Exception) and not getattr(r, "accepts_device_outputs", False)
                            for r, p in zip(requests, plan))
            host_all = out.cpu().numpy() if want_host else None  # synchronises the stream
            hip.stream_synchronize(sh)
            # an image K23 or K24 gave up on: the host decodes it into its row, or its request fails
            redo = [j for jobs, status in ran for j, st in zip(jobs, self._read_status(status)) if st]
            for j in redo:
                if isinstance(plan[j.request], Exception):
                    continue
                try:
                    img = inception_preprocess(self._codec.jpeg_decode(j.blob, j.info.scale), self.H, self.W, "NCHW",
                                               antialias=j.antialias)
                except Exception as e:  # noqa: BLE001 - the host decoder's error fails this request alone
                    plan[j.request] = e
                    continue
                out[j.row].copy_(torch.from_numpy(img))
                if host_all is not None:
                    host_all[j.row] = img
            if redo:
                hip.stream_synchronize(sh)
        res = []
        for r, p in zip(requests, plan):
            if isinstance(p, Exception):
                res.append(p)
                continue
            first, n = p
            shape = [n, self.C, self.H, self.W]
            if getattr(r, "accepts_device_outputs", False):
                o = OutputTensor("OUTPUT", "FP32", shape, DeviceView(base + first * img_bytes, n * img_bytes,
                                                                     self.device_id))
                o.owner = out  # keeps the device memory alive while the ensemble holds the tensor
            else:
                o = OutputTensor("OUTPUT", "FP32", shape, host_all[first:first + n])
            res.append([o])
        return res


class PreprocessInceptionEnsemble(Ensemble):
    """Ensemble: raw image bytes -> preprocess_inception -> densenet_onnx
    (the model the reference's ensemble_image_client drives,
    src/python/examples/ensemble_image_client.py)."""

    name = "preprocess_inception_ensemble"
    max_batch_size = 8
    inputs = (TensorSpec("INPUT", "BYTES", [1]),)
    outputs = (TensorSpec("OUTPUT", "FP32", [1000], label_filename="densenet_labels.txt"),)
    ensemble_steps = [
        ("preprocess_inception", {"INPUT": "INPUT"}, {"OUTPUT": "preprocessed_image"}),
        ("densenet_onnx", {"data_0": "preprocessed_image"}, {"fc6_1": "OUTPUT"}),
    ]
    labels = DensenetOnnx.labels


class BertLarge(DeviceModel):
    """``bert_large`` — BERT-large SQuAD-style QA (models/bert.py), the model of
    BASELINE.json's concurrency-sweep config.  INT32 [384] input_ids /
    attention_mask / token_type_ids in, FP32 [384] start/end logits out;
    dynamic batching into HIP-graph buckets.  Inputs from device shm are
    gathered with K7 batched_copy (one launch per input tensor), outputs are
    scattered the same way; both the Python scheduler and the native front end
    (execute_native) use it.

    ``TCAMD_BERT_PACKED=1`` (read at load; 0 by default) adds the padding-free
    route: per row bucket ``b`` and fill ``f`` of ``PACKED_FILL`` a second kind
    of graph that runs ``BertLargeQA.forward_packed`` over ``t_cap = b * f``
    token slots (K30 plan over the bucket's rows of the slot's mask buffer --
    the bucket's padding rows are zeroed, hence empty -- the packed embedding,
    the layers with K12v attention, the unpack).  A batch counts its tokens
    (mask >= 1: on the host for host-staged parts, one device reduction and
    ``.item()`` on the slot's stream if a part came from device memory, in
    place of ``_mask_all_ones``'s own) and ``packed_bucket`` picks the smallest
    fill that holds them; a batch no fill holds runs the masked or dense padded
    graph, chosen as without the knob.  On a packed batch the positions with
    mask below 1 hold ``PAD_LOGIT`` (-10000); no consumer reads them (K27, K29
    and utils/qa.py all go by the mask).  ``route_counts`` counts the batches
    per route.  The fp32-parity ``bert_large_fp32`` takes the same route with
    the fp32 form of ``forward_packed`` (K12xv attention)."""

    name = "bert_large"
    platform = "pytorch_libtorch"
    backend = "pytorch"
    # 128: a bs128 HIP-graph forward runs 4,292 seq/s against 4,095 at bs64
    # (tools/bert_probe.py --graphs, profiles/r6_bert_batching/)
    max_batch_size = 128
    SEQ = 384
    inputs = (TensorSpec("input_ids", "INT32", [384]), TensorSpec("attention_mask", "INT32", [384]),
              TensorSpec("token_type_ids", "INT32", [384]))
    outputs = (TensorSpec("start_logits", "FP32", [384]), TensorSpec("end_logits", "FP32", [384]))
    dynamic_batching = {"preferred": [], "max_queue_delay_us": 1000}
    instance_kind = "KIND_GPU"
    instance_count = 1
    supports_native = True
    # HIP-graph buckets: a batch runs the smallest one that holds it.  Steps of
    # 4 rows from 8 to 32 (where c64's batches land), 8 above: closed-loop loads
    # batch anything from 1 to 64 rows, and
    # with power-of-two buckets a 33-row batch paid for 64 (served c64: 33 rows
    # per batch at 11.5 ms vs 7.9 ms for a 32-row forward)
    BUCKETS = (1, 2, 4, 8, 12, 16, 20, 24, 28, 32, 40, 48, 56, 64, 80, 96, 112, 128)
    # a second, unmasked ("dense") graph for the buckets from DENSE_FROM rows,
    # picked per batch when no real row is padded.  Below that every batch
    # runs the masked graph: K12 classifies its key chunks, so an all-ones
    # mask runs the unmasked math (bs1 9.8 vs 9.7-10.8 us), while picking the
    # dense graph costs a device reduction and a host sync per batch on
    # HIP-shm inputs (~40 us of compute_input at c1).  At 64 rows the
    # unmasked kernel is still 4-8 % faster (78-80 vs 82-87 us,
    # profiles/r6_k12/k12_allones.log), worth the sync.
    DENSE_FROM = 32
    # the packed route's graphs: t_cap = bucket * fill token slots (a question
    # plus a paragraph is typically 100-250 of the 384 tokens)
    PACKED_FILL = (128, 256)
    supports_packed = True

    def __init__(self, version=1, device_id=0, use_graphs=True, layers=24, **kw):
        super().__init__(version, device_id, **kw)
        self.use_graphs = use_graphs
        self.layers = int(layers)
        self.packed = False
        self.route_counts = {"packed": 0, "padded": 0}

    @classmethod
    def packed_bucket(cls, total_rows, tokens):
        """(row bucket, fill) of the packed graph that serves ``total_rows`` rows
        holding ``tokens`` valid tokens: the rows' bucket and the smallest fill
        of PACKED_FILL with tokens <= bucket * fill; None when no fill holds
        them (the padded graph serves the batch).  Host only."""
        bucket = next((b for b in cls.BUCKETS if b >= total_rows), None)
        if bucket is None or total_rows < 1:
            return None
        for f in cls.PACKED_FILL:
            if tokens <= bucket * f:
                return bucket, f
        return None

    def load(self):
        from triton_client_amd.models import bert

        torch, _, dev = self._gpu("bert_large requires a GPU")
        torch.cuda.set_device(self.device_id)
        self.model = self._build_model(bert, dev)
        self.packed = self.supports_packed and os.environ.get("TCAMD_BERT_PACKED", "0") == "1"
        self.route_counts = {"packed": 0, "padded": 0}
        # before the warm-up runs and graph captures below pick their GEMM solutions
        self.tuned_gemms = bert.use_tuned_gemms()
        for _ in range(max(1, self.instance_count)):
            self._slots.add(self._make_slot(dev))

    def _build_model(self, bert, dev):
        return bert.build(device=dev, layers=self.layers)

    def _make_slot(self, dev):
        torch = self.torch
        n, s = self.max_batch_size, self.SEQ
        slot = {"stream": torch.cuda.Stream(device=dev), "graphs": {},
                "ins": [torch.zeros(n, s, device=dev, dtype=torch.int32) for _ in range(3)],
                "outs": [torch.zeros(n, s, device=dev, dtype=torch.float32) for _ in range(2)],
                "ev": [torch.cuda.Event(enable_timing=True) for _ in range(4)]}
        slot["ins"][1].fill_(1)
        self._pinned(slot, "stage_host", 3 * n * s * 4)
        self._pinned(slot, "out_host", 2 * n * s * 4)

        def run(b, dense=False):
            ids, mask, tt = (t[:b] for t in slot["ins"])
            # synthetic load generators send arbitrary INT32: keep indices in range
            # (an out-of-range embedding index is a device fault, not an error)
            st, en = self.model(ids.long().remainder(30522), mask.clamp(0, 1), tt.long().clamp(0, 1), dense=dense)
            slot["outs"][0][:b].copy_(st)
            slot["outs"][1][:b].copy_(en)

        def run_packed(b, fill):
            ids, mask, tt = (t[:b] for t in slot["ins"])
            # the kernels wrap the ids and clamp the types themselves; valid = mask >= 1
            st, en = self.model.forward_packed(ids, mask, tt, b * fill)
            slot["outs"][0][:b].copy_(st)
            slot["outs"][1][:b].copy_(en)

        slot["run"] = run
        slot["run_packed"] = run_packed
        # one graph per bucket with the key-padding mask, plus a "dense" one
        # without it from DENSE_FROM rows (no padding in any real row)
        with torch.cuda.stream(slot["stream"]), torch.no_grad():
            for b in self.BUCKETS:
                for dense in ((False, True) if b >= self.DENSE_FROM else (False,)):
                    run(b, dense)
                    if self.use_graphs:
                        g = torch.cuda.CUDAGraph()
                        with torch.cuda.graph(g, stream=slot["stream"]):
                            run(b, dense)
                        slot["graphs"][(b, dense)] = g
            if self.packed:
                # captured with an all-empty mask (no row has a token): the
                # warm-up run and the capture then touch no token at all
                slot["ins"][1].zero_()
                for b in self.BUCKETS:
                    for fill in self.PACKED_FILL:
                        run_packed(b, fill)
                        if self.use_graphs:
                            g = torch.cuda.CUDAGraph()
                            with torch.cuda.graph(g, stream=slot["stream"]):
                                run_packed(b, fill)
                            slot["graphs"][(b, "packed", fill)] = g
                slot["ins"][1].fill_(1)
        slot["stream"].synchronize()
        return slot

    def _mask_all_ones(self, slot, parts, total):
        """True when every real row's attention_mask is >= 1 everywhere (the
        model clamps it to [0, 1]).  Host-staged parts are scanned in place;
        if any part came from device memory (HIP shm) the staged device rows
        are checked on the slot stream (one small reduction + sync)."""
        on_device = False
        for kind, ptr, rows in parts:
            if kind == 1:
                on_device = True
                continue
            if pinned_view(ptr, np.int32, rows * self.SEQ).min() < 1:
                return False
        if not on_device:
            return True
        torch = self.torch
        with torch.cuda.stream(slot["stream"]):
            return not bool((slot["ins"][1][:total] < 1).any().item())

    def _count_tokens(self, slot, parts, total):
        """The batch's valid tokens (attention_mask >= 1) over its real rows:
        counted on the host for host-staged parts; if any part came from device
        memory, one reduction over the staged rows and ``.item()`` on the slot's
        stream (the sync ``_mask_all_ones`` would otherwise take)."""
        if any(kind == 1 for kind, _, _ in parts):
            torch = self.torch
            with torch.cuda.stream(slot["stream"]):
                return int((slot["ins"][1][:total] >= 1).sum().item())
        return sum(int((pinned_view(ptr, np.int32, rows * self.SEQ) >= 1).sum()) for _, ptr, rows in parts)

    def _run_batch(self, slot, srcs, outs, total):
        """srcs: per input a list of (kind, ptr, rows) in row order; outs: per
        output a list of (kind, ptr, first_row, rows).  Returns timings (ns)."""
        from triton_client_amd.ops import hip

        row = self.SEQ * 4
        bucket = next(b for b in self.BUCKETS if b >= total)
        stream = slot["stream"]
        sh = stream.cuda_stream
        ev = slot["ev"]
        ev[0].record(stream)
        for k, parts in enumerate(srcs):
            base = slot["ins"][k].data_ptr()
            c_src, c_dst, c_n = [], [], []
            host_off = 0
            first = 0
            stage = slot["stage_host"] + k * self.max_batch_size * row
            for kind, ptr, rows in parts:
                if kind == 1:
                    c_src.append(ptr)
                    c_dst.append(base + first * row)
                    c_n.append(rows * row)
                else:
                    ctypes.memmove(stage + host_off, ptr, rows * row)
                    hip.memcpy_async(base + first * row, stage + host_off, rows * row, sh)
                    host_off += rows * row
                first += rows
            if c_src:
                hip.batched_copy(c_src, c_dst, c_n, sh)
            if bucket > total:  # padding rows: keep them deterministic (mask 1, ids 0)
                hip.memset_async(base + total * row, 0, (bucket - total) * row, sh)
        pick = None
        if self.packed:
            tokens = self._count_tokens(slot, srcs[1], total)
            pick = self.packed_bucket(total, tokens)
            # all ones <=> every position of every real row counted: no second scan or sync
            dense = pick is None and bucket >= self.DENSE_FROM and tokens == total * self.SEQ
        else:
            dense = bucket >= self.DENSE_FROM and self._mask_all_ones(slot, srcs[1], total)
        self.route_counts["padded" if pick is None else "packed"] += 1
        ev[1].record(stream)
        with self.torch.cuda.stream(stream), self.torch.no_grad():
            if pick is not None:
                if self.use_graphs:
                    slot["graphs"][(bucket, "packed", pick[1])].replay()
                else:
                    slot["run_packed"](bucket, pick[1])
            elif self.use_graphs:
                slot["graphs"][(bucket, dense)].replay()
            else:
                slot["run"](bucket, dense)
        ev[2].record(stream)
        host_outs = []
        for k, parts in enumerate(outs):
            base = slot["outs"][k].data_ptr()
            c_src, c_dst, c_n = [], [], []
            for kind, ptr, first, rows in parts:
                if not ptr:
                    continue
                if kind == 1:
                    c_src.append(base + first * row)
                    c_dst.append(ptr)
                    c_n.append(rows * row)
                else:
                    host_outs.append((k, ptr, first, rows))
            if c_src:
                hip.batched_copy(c_src, c_dst, c_n, sh)
        if host_outs:
            for k in range(2):
                hip.memcpy_async(slot["out_host"] + k * self.max_batch_size * row, slot["outs"][k].data_ptr(),
                                 total * row, sh)
        ev[3].record(stream)
        hip.stream_synchronize(sh)
        for k, ptr, first, rows in host_outs:
            ctypes.memmove(ptr, slot["out_host"] + k * self.max_batch_size * row + first * row, rows * row)
        return [int(ev[0].elapsed_time(ev[1]) * 1e6), int(ev[1].elapsed_time(ev[2]) * 1e6),
                int(ev[2].elapsed_time(ev[3]) * 1e6)]

    def execute_native(self, instance, b):
        total = int(b.total_rows)
        if total > self.max_batch_size:
            raise ServerError("batch of %d rows exceeds max_batch_size" % total)
        srcs = [[] for _ in range(3)]
        outs = [[] for _ in range(2)]
        first = 0
        for r in range(b.n_requests):
            rows = int(b.rows[r])
            for k in range(3):
                ref = b.inputs[r * b.n_inputs + k]
                srcs[k].append((ref.kind, ref.ptr, rows))
            for k in range(2):
                ref = b.outputs[r * b.n_outputs + k]
                outs[k].append((ref.kind, ref.ptr, first, rows))
            first += rows
        with self._slots.slot() as (_, slot):
            t = self._run_batch(slot, srcs, outs, total)
        for k in range(3):
            b.timing_ns[k] = t[k]

    def execute(self, requests):
        total = 0
        plan = []
        for r in requests:
            n = int(r.input("input_ids").shape[0])
            plan.append((r, total, n))
            total += n
        if total > self.max_batch_size:
            return [ServerError("batch of %d rows exceeds max_batch_size" % total)] * len(requests)
        names = [s.name for s in self.inputs]
        srcs = [[] for _ in range(3)]
        keep = []
        for r, first, n in plan:
            for k, nm in enumerate(names):
                t = r.input(nm)
                if isinstance(t.data, DeviceView):
                    srcs[k].append((1, t.data.ptr, n))
                else:
                    a = np.ascontiguousarray(t.data, dtype=np.int32)
                    keep.append(a)
                    srcs[k].append((0, a.ctypes.data, n))
        if all(getattr(r, "accepts_device_outputs", False) for r in requests):
            return self._execute_device_outputs(requests, plan, srcs, total)
        # outputs come back to host; shm targets are filled by the server (deliver_to_shm)
        res = np.empty((2, total, self.SEQ), dtype=np.float32)
        outs = [[(0, res[k].ctypes.data, 0, total)] for k in range(2)]
        with self._slots.slot() as (_, slot):
            t = self._run_batch(slot, srcs, outs, total)
        if self._batch_stats is not None:
            self._batch_stats(total, len(requests), *t)
        return [[OutputTensor("start_logits", "FP32", [n, self.SEQ], res[0, f:f + n]),
                 OutputTensor("end_logits", "FP32", [n, self.SEQ], res[1, f:f + n])] for _, f, n in plan]

    def _execute_device_outputs(self, requests, plan, srcs, total):
        """A batch of ensemble steps (``accepts_device_outputs`` on every request,
        core._infer_ensemble): the logits stay on the device.  The rows go from
        the slot's output buffers, which the next batch overwrites, into a tensor
        of this batch's own (K7 batched_copy on the slot's stream, inside
        _run_batch), and each request gets its rows of it as ``DeviceView`` with
        the tensor as ``owner``."""
        torch = self.torch
        row = self.SEQ * 4
        with self._slots.slot() as (_, slot):
            with torch.cuda.stream(slot["stream"]):
                res = torch.empty((2, total, self.SEQ), device=slot["stream"].device, dtype=torch.float32)
            outs = [[(1, res[k].data_ptr(), 0, total)] for k in range(2)]
            t = self._run_batch(slot, srcs, outs, total)  # ends with a stream synchronise
        if self._batch_stats is not None:
            self._batch_stats(total, len(requests), *t)
        out = []
        for _, f, n in plan:
            tensors = []
            for k, nm in enumerate(("start_logits", "end_logits")):
                o = OutputTensor(nm, "FP32", [n, self.SEQ],
                                 DeviceView(res[k].data_ptr() + f * row, n * row, self.device_id))
                o.owner = res  # keeps the device memory alive while the ensemble holds the tensor
                tensors.append(o)
            out.append(tensors)
        return out

    _batch_stats = None
    reports_batch_stats = True


class BertLargeFP32(BertLarge):
    """``bert_large_fp32`` — the same BERT-large QA model (same seed, same
    inputs and outputs) with fp32-parity compute, the way densenet_onnx has
    one: fp32 weights and activations, every projection one bf16x3 GEMM on
    the bf16 MFMA (models/bert.py prepare_x3: x_hi W_hi + x_hi W_lo + x_lo W_hi,
    fp32 accumulate), LayerNorm / GELU / softmax attention in fp32.  Served
    logits match an fp32 forward of the fp32 weights to ~1e-5
    (tests/test_bert_accuracy_gpu.py); ~3x the bf16 model's GEMM work.  The
    bf16 ``bert_large`` stays the config-4 serving default.  With
    ``TCAMD_BERT_PACKED=1`` it takes the padding-free route of the base class:
    packed graphs per (bucket <= 64, fill 128 / 256) that run the fp32 form of
    ``BertLargeQA.forward_packed`` -- the fp32 packed embedding LayerNorm, the
    bf16x3 projections and K11p over ``t_cap`` tokens, K12xv (K12x over packed
    rows, csrc/kernels/bert.hip); ``packed_bucket`` and ``route_counts`` as in
    the base class.  Without the knob every batch runs the padded graphs."""

    name = "bert_large_fp32"
    # 64 rows, as before bert_large went to 128: a bs128 fp32-parity forward
    # (~110 ms) outlasts the sweep's queue delay, so c256 ran partial 88-row
    # batches at 1,142 infer/s against 1,200 with 64-row ones
    # (profiles/r6_bert_batching/)
    max_batch_size = 64
    BUCKETS = tuple(b for b in BertLarge.BUCKETS if b <= 64)
    # the packed route of the base class, in fp32: K12xv is K12x's counterpart of K12v
    supports_packed = True

    def _build_model(self, bert, dev):
        import torch

        return bert.prepare_x3(bert.build(device=dev, dtype=torch.float32, layers=self.layers))


class QaSpans(DeviceModel):
    """``qa_spans`` on the GPU: the same I/O contract, request parameters and
    rule as the CPU model of that name (server/cpu_models.py QaSpans), which it
    replaces on a ``--gpu`` server and whose parameter checks it uses.

    Per batch, K27 ``qa_spans`` (csrc/kernels/qa_spans.hip) picks every row's
    spans on the slot's stream; requests of different ``n_best`` and
    ``max_answer_length`` share the launch through the kernel's per-row
    ``k_row`` / ``len_row`` arrays.  An input that arrives as ``DeviceView`` (a
    HIP shm region, or the logits ``bert_large`` left on the device for the
    ensemble) is read in place; a host input goes up through the slot's pinned
    staging buffer, one copy per tensor.  The kernel reads rows at one stride
    from one base, so a batch is launched once per run of requests whose four
    tensors each follow the previous request's in memory: once when everything
    is staged or comes from one ``bert_large`` batch in order.  The outputs of
    the batch come back in one copy of ``rows * (kmax * 12 + 4)`` bytes.
    ``TCAMD_DEVICE_QA_SPANS=0`` (read at load) runs the host twin instead."""

    name = "qa_spans"
    max_batch_size = 128
    SEQ = 384
    inputs = (TensorSpec("start_logits", "FP32", [384]), TensorSpec("end_logits", "FP32", [384]),
              TensorSpec("attention_mask", "INT32", [384]), TensorSpec("token_type_ids", "INT32", [384]))
    outputs = (TensorSpec("spans", "INT32", [-1, 2]), TensorSpec("scores", "FP32", [-1]),
               TensorSpec("null_score", "FP32", [1]))
    dynamic_batching = {"preferred": [], "max_queue_delay_us": 100}
    instance_kind = "KIND_GPU"
    instance_count = 2
    gpus = (0,)

    def load(self):
        if not self._load_twin(_cpu.QaSpans, os.environ.get("TCAMD_DEVICE_QA_SPANS", "1") != "0"):
            return
        _, hip, dev = self._gpu()
        n, row = self.max_batch_size, self.SEQ * 4
        self.in_bytes = 4 * n * row + 2 * n * 4  # the four tensors, then k_row and len_row
        self.out_bytes = n * (hip.QA_SPANS_KMAX * 12 + 4)
        self._add_stage_slots(dev, self.in_bytes, self.out_bytes)

    def execute(self, requests):
        plan, total = self._host.plan(requests)
        if total == 0:
            return plan
        if total > self.max_batch_size:
            return [ServerError("batch of %d rows exceeds max_batch_size" % total)] * len(requests)
        if not self.device_path:
            return self._host.results(plan, *self._host.run_host(requests, plan, total))
        from triton_client_amd.ops import hip

        try:
            with self._slots.slot() as (_, slot):
                return self._host.results(plan, *self._execute(slot, requests, plan, total))
        except (ServerError, hip.HipError) as e:
            return plan_errors(plan, "qa_spans", e)

    def _execute(self, slot, requests, plan, total):
        from triton_client_amd.ops import hip

        n_max, row = self.max_batch_size, self.SEQ * 4
        sh = slot["stream"].cuda_stream
        in_host, in_dev = slot["in_host"], slot["in_dev"].data_ptr()
        k_row, len_row, kmax = self._host.row_params(plan, total)
        par = 4 * n_max * row  # k_row and len_row: one copy
        pars = pinned_view(in_host + par, np.int32, 2 * n_max)
        pars[:total] = k_row
        pars[n_max:n_max + total] = len_row
        hip.memcpy_async(in_dev + par, in_host + par, 2 * n_max * 4, sh)
        good = [(r, p) for r, p in zip(requests, plan) if not isinstance(p, Exception)]
        at = []  # per tensor: where each good request's rows are on the device
        for c, spec in enumerate(self.inputs):
            base = c * n_max * row
            dt = np.float32 if spec.datatype == "FP32" else np.int32
            lo, hi, where = None, 0, []
            for r, (first, n, _, _) in good:
                ptr, staged = place_input(slot, r.input(spec.name), spec.name, dt, n * row, base + first * row)
                if staged:  # the staged rows of a tensor go up in one copy
                    lo, hi = first if lo is None else lo, first + n
                where.append(ptr)
            if lo is not None:
                hip.memcpy_async(in_dev + base + lo * row, in_host + base + lo * row, (hi - lo) * row, sh)
            at.append(where)
        out_dev = slot["out_dev"].data_ptr()
        o_scores, o_null = total * kmax * 8, total * kmax * 12
        # one launch per run of requests that follow each other in memory, tensor by tensor
        g = 0
        while g < len(good):
            first = good[g][1][0]
            h, rows = g + 1, good[g][1][1]
            while h < len(good) and all(w[h] == w[g] + (good[h][1][0] - first) * row for w in at):
                rows += good[h][1][1]
                h += 1
            hip.qa_spans(at[0][g], at[1][g], row, at[2][g], at[3][g], row, rows, self.SEQ,
                         in_dev + par + first * 4, in_dev + par + (n_max + first) * 4, kmax,
                         out_dev + first * kmax * 8, out_dev + o_scores + first * kmax * 4,
                         out_dev + o_null + first * 4, stream=sh)
            g = h
        raw = download(hip, slot, total * (kmax * 12 + 4), sh)
        return (raw[:o_scores].view(np.int32).reshape(total, kmax, 2),
                raw[o_scores:o_null].view(np.float32).reshape(total, kmax),
                raw[o_null:].view(np.float32))


class BertQaEnsemble(Ensemble):
    """Ensemble: token ids -> ``bert_large`` -> ``qa_spans``.  The logits stay
    on the device between the steps (``bert_large`` hands them over as
    ``DeviceView``, K27 reads them in place); the second step takes the
    request's own ``attention_mask`` and ``token_type_ids``.  ``n_best`` and
    ``max_answer_length`` reach ``qa_spans`` as the ensemble's custom request
    parameters.  ``start_logits`` / ``end_logits`` are outputs too, so a client
    can see the logits its spans were picked from; a request that does not ask
    for them does not pay for their copy."""

    name = "bert_qa_ensemble"
    max_batch_size = 128
    inputs = BertLarge.inputs
    outputs = QaSpans.outputs + BertLarge.outputs
    ensemble_steps = [
        ("bert_large", {"input_ids": "input_ids", "attention_mask": "attention_mask",
                        "token_type_ids": "token_type_ids"},
         {"start_logits": "start_logits", "end_logits": "end_logits"}),
        ("qa_spans", {"start_logits": "start_logits", "end_logits": "end_logits", "attention_mask": "attention_mask",
                      "token_type_ids": "token_type_ids"},
         {"spans": "spans", "scores": "scores", "null_score": "null_score"}),
    ]


class BertTokenizer(DeviceModel):
    """``bert_tokenizer`` on the GPU: the same I/O contract, request parameter,
    vocabulary and rule as the CPU model of that name (server/cpu_models.py
    BertTokenizer), which it replaces on a ``--gpu`` server and whose checks it
    uses.

    Per batch, the host copies each request's strings end to end into the
    slot's pinned staging area behind the per-row table (``{question_off,
    question_len, context_off, context_len}`` and ``max_query_length``), one
    upload takes table and texts to the device, K28 ``wordpiece_tokenize``
    (csrc/kernels/wordpiece.hip) decodes, folds, matches and assembles the rows
    on the slot's stream against the vocabulary image uploaded at load, and one
    download brings the outputs back.  A batch whose texts exceed the staging
    budget (``TEXT_BUDGET``) runs in several launches, each over as many rows as
    fit.  For a batch of ensemble steps (``accepts_device_outputs``) the three
    id tensors are written into a tensor of the batch's own and handed on as
    ``DeviceView`` with ``owner`` set, as ``BertLarge._execute_device_outputs``
    does with its logits; ``offsets`` and ``overflow`` always go to the host.
    ``TCAMD_DEVICE_TOKENIZER=0`` (read at load) runs the host twin instead."""

    name = "bert_tokenizer"
    max_batch_size = 128
    SEQ = 384
    TEXT_BUDGET = 1 << 20  # bytes of text per launch; one row needs at most 2 * 65,536
    inputs = (TensorSpec("question", "BYTES", [1]), TensorSpec("context", "BYTES", [1]))
    outputs = (TensorSpec("input_ids", "INT32", [384]), TensorSpec("attention_mask", "INT32", [384]),
               TensorSpec("token_type_ids", "INT32", [384]), TensorSpec("offsets", "INT32", [384, 2]),
               TensorSpec("overflow", "INT32", [1]))
    dynamic_batching = {"preferred": [], "max_queue_delay_us": 100}
    instance_kind = "KIND_GPU"
    instance_count = 2
    gpus = (0,)

    def load(self):
        device_path = self._load_twin(_cpu.BertTokenizer, os.environ.get("TCAMD_DEVICE_TOKENIZER", "1") != "0")
        self.vocab = self._host.vocab
        if not device_path:
            return
        torch, hip, dev = self._gpu()
        n = self.max_batch_size
        self.head_bytes = n * 16 + n * 4  # the row table, then max_query_length per row
        self.in_bytes = self.head_bytes + self.TEXT_BUDGET
        self.ws_bytes = hip.wordpiece_workspace(n, self.TEXT_BUDGET)
        self.out_bytes = n * (self.SEQ * 5 + 2) * 4
        self.vocab_dev = torch.from_numpy(self.vocab.image.view(np.int32).copy()).to(dev)
        self._add_stage_slots(dev, self.in_bytes, self.out_bytes, ws=self.ws_bytes)

    def execute(self, requests):
        plan, total = self._host.plan(requests)
        if total == 0:
            return plan
        if total > self.max_batch_size:
            return [ServerError("batch of %d rows exceeds max_batch_size" % total)] * len(requests)
        if not self.device_path:
            return self._host.results(plan, *self._host.run_host(plan))
        from triton_client_amd.ops import hip

        on_device = all(getattr(r, "accepts_device_outputs", False) for r in requests)
        try:
            with self._slots.slot() as (_, slot):
                return self._execute(slot, plan, total, on_device)
        except (ServerError, hip.HipError) as e:
            return plan_errors(plan, "bert_tokenizer", e)

    @classmethod
    def launches(cls, lens):
        """The rows of a batch dealt into launches: ``[(first_row, rows)]``, each
        launch's texts within ``TEXT_BUDGET``; ``lens[r]`` = the bytes of row r."""
        out, first, used = [], 0, 0
        for r, n in enumerate(lens):
            if r > first and used + n > cls.TEXT_BUDGET:
                out.append((first, r - first))
                first, used = r, 0
            used += n
        out.append((first, len(lens) - first))
        return out

    def _execute(self, slot, plan, total, on_device):
        from triton_client_amd.ops import hip

        torch, S, n_max = self.torch, self.SEQ, self.max_batch_size
        sh = slot["stream"].cuda_stream
        qs, cs, mq = self._host.batch_texts(plan)
        in_host, in_dev = slot["in_host"], slot["in_dev"].data_ptr()
        out_dev = slot["out_dev"].data_ptr()
        # the outputs of the batch, compact: offsets, overflow, status; then ids, mask, type ids
        o_over, o_stat, o_ids = total * S * 8, total * S * 8 + total * 4, total * S * 8 + total * 8
        res = None
        if on_device:
            with torch.cuda.stream(slot["stream"]):
                res = torch.empty((3, total, S), device=slot["stream"].device, dtype=torch.int32)
            id_ptrs = [res[k].data_ptr() for k in range(3)]
        else:
            id_ptrs = [out_dev + o_ids + k * total * S * 4 for k in range(3)]
        table = pinned_view(in_host, np.uint32, n_max * 4).reshape(n_max, 4)
        maxq = pinned_view(in_host + n_max * 16, np.int32, n_max)
        lens = [len(q) + len(c) for q, c in zip(qs, cs)]
        groups = self.launches(lens)
        for g, (first, rows) in enumerate(groups):
            if g:
                hip.stream_synchronize(sh)  # the staging area is about to be rewritten
            at = stage_texts(slot, table, zip(qs[first:first + rows], cs[first:first + rows]), self.head_bytes)
            maxq[:rows] = mq[first:first + rows]
            hip.memcpy_async(in_dev, in_host, self.head_bytes + at, sh)
            hip.wordpiece_tokenize(in_dev + self.head_bytes, at, in_dev, in_dev + n_max * 16, rows, S,
                                   self.vocab_dev.data_ptr(), self.vocab.image.size, slot["ws"].data_ptr(),
                                   self.ws_bytes, id_ptrs[0] + first * S * 4, id_ptrs[1] + first * S * 4,
                                   id_ptrs[2] + first * S * 4, out_dev + first * S * 8, out_dev + o_over + first * 4,
                                   out_dev + o_stat + first * 4, stream=sh)
        raw = download(hip, slot, o_ids if on_device else o_ids + 3 * total * S * 4, sh)
        offsets = raw[:o_over].view(np.int32).reshape(total, S, 2)
        overflow, status = raw[o_over:o_stat].view(np.int32), raw[o_stat:o_ids].view(np.uint32)
        if on_device:
            return self._host.results(plan, None, None, None, offsets, overflow, status, device=(res, self.device_id))
        ids, mask, tt = (raw[o_ids + k * total * S * 4:o_ids + (k + 1) * total * S * 4].view(np.int32).reshape(total, S)
                         for k in range(3))
        return self._host.results(plan, ids, mask, tt, offsets, overflow, status)


class BertQaTextEnsemble(Ensemble):
    """Ensemble: UTF-8 text -> ``bert_tokenizer`` -> ``bert_large`` ->
    ``qa_spans``.  The ids stay on the device between the first two steps and
    the logits between the last two (each step hands its outputs on as
    ``DeviceView``); ``offsets`` and ``overflow`` come from the first step, so
    ``utils.qa.answer_text`` can turn a span back into the context's bytes.
    ``max_query_length``, ``n_best`` and ``max_answer_length`` travel as the
    ensemble's custom request parameters to the steps that read them.  The ids
    and the logits are outputs too; a request that does not ask for them does
    not pay for their copy.  A context longer than the row is cut
    (``overflow``); ``bert_qa_doc_ensemble`` answers over the whole of it with
    doc-stride windows."""

    name = "bert_qa_text_ensemble"
    max_batch_size = 128
    inputs = BertTokenizer.inputs
    outputs = QaSpans.outputs + BertTokenizer.outputs[3:] + BertTokenizer.outputs[:3] + BertLarge.outputs
    ensemble_steps = [
        ("bert_tokenizer", {"question": "question", "context": "context"},
         {"input_ids": "input_ids", "attention_mask": "attention_mask", "token_type_ids": "token_type_ids",
          "offsets": "offsets", "overflow": "overflow"}),
        ("bert_large", {"input_ids": "input_ids", "attention_mask": "attention_mask",
                        "token_type_ids": "token_type_ids"},
         {"start_logits": "start_logits", "end_logits": "end_logits"}),
        ("qa_spans", {"start_logits": "start_logits", "end_logits": "end_logits", "attention_mask": "attention_mask",
                      "token_type_ids": "token_type_ids"},
         {"spans": "spans", "scores": "scores", "null_score": "null_score"}),
    ]


class BertWindowTokenizer(DeviceModel):
    """``bert_window_tokenizer`` on the GPU: the same I/O contract, request
    parameters, vocabulary and rule as the CPU model of that name
    (server/cpu_models.py BertWindowTokenizer), which it replaces on a ``--gpu``
    server and whose checks and messages it uses.

    Per request, the host copies the documents' strings end to end into the
    slot's pinned staging area behind the per-document table and parameters, one
    upload takes them to the device, and K28w ``wordpiece_windows``
    (csrc/kernels/wordpiece.hip) tokenizes and lays out the windows of all
    documents on the slot's stream against the vocabulary image uploaded at
    load.  ``doc_info``, the row count and ``window_info`` come back first (4
    KB): they say whether a document was refused and how many rows there are;
    then exactly those rows of ``offsets``.  For an ensemble step
    (``accepts_device_outputs``) the four id tensors are written into a tensor
    of the request's own and handed on as ``DeviceView`` with ``owner`` set;
    otherwise their rows are downloaded too.  The texts of a request are limited
    to ``TEXT_BUDGET`` bytes.  ``TCAMD_DEVICE_TOKENIZER=0`` (read at load) runs
    the host twin instead."""

    name = "bert_window_tokenizer"
    max_batch_size = 0
    SEQ = 384
    MAX_ROWS = 128
    TEXT_BUDGET = 1 << 20
    inputs, outputs = _cpu.BertWindowTokenizer.inputs, _cpu.BertWindowTokenizer.outputs
    instance_kind = "KIND_GPU"
    instance_count = 2
    gpus = (0,)

    def load(self):
        device_path = self._load_twin(_cpu.BertWindowTokenizer, os.environ.get("TCAMD_DEVICE_TOKENIZER", "1") != "0")
        self.vocab = self._host.vocab
        if not device_path:
            return
        torch, hip, dev = self._gpu()
        n, S = self.MAX_ROWS, self.SEQ
        self.head_bytes = n * 16 + 3 * n * 4  # the table, then max_query_length, doc_stride, max_windows per document
        self.in_bytes = self.head_bytes + self.TEXT_BUDGET
        self.ws_bytes = hip.wordpiece_windows_workspace(n, self.TEXT_BUDGET)
        # doc_info, n_rows (16 bytes), window_info; offsets; ids, mask, type ids, start mask
        self.o_nrows, self.o_winfo, self.o_offsets = n * 16, n * 16 + 16, 2 * n * 16 + 16
        self.o_ids = self.o_offsets + n * S * 8
        self.out_bytes = self.o_ids + 4 * n * S * 4
        self.vocab_dev = torch.from_numpy(self.vocab.image.view(np.int32).copy()).to(dev)
        self._add_stage_slots(dev, self.in_bytes, self.out_bytes, ws=self.ws_bytes)

    def execute(self, requests):
        return self._per_request(requests, self._one)

    def _one(self, r):
        p = self._host.plan_one(r)
        if not self.device_path:
            return self._host.run_host_one(p)
        with self._slots.slot() as (_, slot):
            return self._execute(slot, p, bool(getattr(r, "accepts_device_outputs", False)))

    def _execute(self, slot, p, on_device):
        from triton_client_amd.ops import hip

        qs, cs, mq, ds, mw = p
        torch, S, n = self.torch, self.SEQ, self.MAX_ROWS
        docs = len(qs)
        total = sum(len(q) + len(c) for q, c in zip(qs, cs))
        if total > self.TEXT_BUDGET:
            raise ServerError("%s: the texts of a request have %d bytes, at most %d" % (self.name, total, self.TEXT_BUDGET))
        sh = slot["stream"].cuda_stream
        in_host, in_dev, out_host = slot["in_host"], slot["in_dev"].data_ptr(), slot["out_host"]
        out_dev = slot["out_dev"].data_ptr()
        table = pinned_view(in_host, np.uint32, n * 4).reshape(n, 4)
        pars = pinned_view(in_host + n * 16, np.int32, 3 * n).reshape(3, n)
        at = stage_texts(slot, table, zip(qs, cs), self.head_bytes)
        pars[0, :docs], pars[1, :docs], pars[2, :docs] = mq, ds, mw
        res = None
        if on_device:
            with torch.cuda.stream(slot["stream"]):
                res = torch.empty((4, n, S), device=slot["stream"].device, dtype=torch.int32)
            id_ptrs = [res[k].data_ptr() for k in range(4)]
        else:
            id_ptrs = [out_dev + self.o_ids + k * n * S * 4 for k in range(4)]
        hip.memcpy_async(in_dev, in_host, self.head_bytes + at, sh)
        hip.wordpiece_windows(in_dev + self.head_bytes, at, in_dev, in_dev + n * 16, in_dev + n * 20, in_dev + n * 24,
                              docs, S, self.vocab_dev.data_ptr(), self.vocab.image.size, slot["ws"].data_ptr(),
                              self.ws_bytes, n, id_ptrs[0], id_ptrs[1], id_ptrs[2], id_ptrs[3],
                              out_dev + self.o_offsets, out_dev + self.o_winfo, out_dev, out_dev + self.o_nrows,
                              stream=sh)
        head = download(hip, slot, self.o_offsets, sh)
        dinfo = head[:docs * 16].view(np.uint32).reshape(docs, 4)
        n_rows = int(head[self.o_nrows:self.o_nrows + 4].view(np.int32)[0])
        err = self._host.doc_error(dinfo, mw)
        if err:
            raise ServerError(err)
        host = {"window_info": head[self.o_winfo:self.o_winfo + n_rows * 16].view(np.int32).reshape(n_rows, 4)}
        hip.memcpy_async(out_host + self.o_offsets, out_dev + self.o_offsets, n_rows * S * 8, sh)
        if not on_device:
            for k in range(4):
                o = self.o_ids + k * n * S * 4
                hip.memcpy_async(out_host + o, out_dev + o, n_rows * S * 4, sh)
        hip.stream_synchronize(sh)

        def rows_at(o, width):
            return pinned_view(out_host + o, np.int32, n_rows * S * width).copy()

        host["offsets"] = rows_at(self.o_offsets, 2).reshape(n_rows, S, 2)
        if on_device:
            return self._host.window_results(dinfo, n_rows, host, device=(res, self.device_id))
        for k, nm in enumerate(("input_ids", "attention_mask", "token_type_ids", "start_mask")):
            host[nm] = rows_at(self.o_ids + k * n * S * 4, 1).reshape(n_rows, S)
        return self._host.window_results(dinfo, n_rows, host)


class QaDocSpans(DeviceModel):
    """``qa_doc_spans`` on the GPU: the same I/O contract, request parameters
    and rule as the CPU model of that name (server/cpu_models.py QaDocSpans),
    which it replaces on a ``--gpu`` server and whose checks it uses.

    Per request, an input that arrives as ``DeviceView`` (the logits
    ``bert_large`` and the id tensors ``bert_window_tokenizer`` left on the
    device for the ensemble) is read in place, a host input goes up through the
    slot's pinned staging buffer; K27 with the start mask
    (``qa_spans_masked``) leaves every window's list in the slot's scratch and
    K29 ``qa_merge`` (csrc/kernels/qa_merge.hip) merges them per document, back
    to back on the slot's stream; the document-level result alone comes back, in
    one copy of ``D * (n_best * 16 + 4)`` bytes.  ``TCAMD_DEVICE_QA_SPANS=0``
    (read at load) runs the host twins instead."""

    name = "qa_doc_spans"
    max_batch_size = 0
    SEQ = 384
    MAX_ROWS = 128
    inputs, outputs = _cpu.QaDocSpans.inputs, _cpu.QaDocSpans.outputs
    instance_kind = "KIND_GPU"
    instance_count = 2
    gpus = (0,)

    def load(self):
        if not self._load_twin(_cpu.QaDocSpans, os.environ.get("TCAMD_DEVICE_QA_SPANS", "1") != "0"):
            return
        _, hip, dev = self._gpu()
        n, row, kmax = self.MAX_ROWS, self.SEQ * 4, hip.QA_SPANS_KMAX
        # the five row tensors, window_info, doc_info, then k_row, len_row and k_doc
        self.o_winfo = 5 * n * row
        self.o_dinfo, self.o_par = self.o_winfo + n * 16, self.o_winfo + 2 * n * 16
        self.in_bytes = self.o_par + 3 * n * 4
        self.list_bytes = n * (kmax * 12 + 4)  # K27's lists: spans, scores, null
        self.out_bytes = n * (kmax * 16 + 4)   # K29's: spans, windows, scores, null
        self._add_stage_slots(dev, self.in_bytes, self.out_bytes, lists=self.list_bytes)

    def execute(self, requests):
        return self._per_request(requests, self._one, wrapped=(ValueError,))

    def _one(self, r):
        p = self._host.plan_one(r)
        if not self.device_path:
            return self._host.run_host_one(r, p)
        with self._slots.slot() as (_, slot):
            return self._host.doc_results(p[2], *self._execute(slot, r, p))

    def _execute(self, slot, r, p):
        from triton_client_amd.ops import hip

        W, D, k, ln = p
        n, row = self.MAX_ROWS, self.SEQ * 4
        sh = slot["stream"].cuda_stream
        in_host, in_dev = slot["in_host"], slot["in_dev"].data_ptr()
        pars = pinned_view(in_host + self.o_par, np.int32, 3 * n).reshape(3, n)
        pars[0, :W], pars[1, :W], pars[2, :D] = k, ln, k
        hip.memcpy_async(in_dev + self.o_par, in_host + self.o_par, 3 * n * 4, sh)
        specs = [(nm, dt, W * row, c * n * row) for c, (nm, dt) in enumerate(self._host.ROW_INPUTS)]
        specs += [("window_info", np.int32, W * 16, self.o_winfo), ("doc_info", np.int32, D * 16, self.o_dinfo)]
        at = [stage_input(hip, slot, r.input(nm), nm, dt, nbytes, base, sh) for nm, dt, nbytes, base in specs]
        lists, out_dev = slot["lists"].data_ptr(), slot["out_dev"].data_ptr()
        l_scores, l_null = W * k * 8, W * k * 12
        hip.qa_spans_masked(at[0], at[1], row, at[2], at[3], at[4], row, W, self.SEQ, in_dev + self.o_par,
                            in_dev + self.o_par + n * 4, k, lists, lists + l_scores, lists + l_null, stream=sh)
        o_windows, o_scores, o_null = D * k * 8, D * k * 12, D * k * 16
        hip.qa_merge(lists, lists + l_scores, lists + l_null, W, at[5], at[6], D, in_dev + self.o_par + 2 * n * 4, k,
                     out_dev, out_dev + o_windows, out_dev + o_scores, out_dev + o_null, stream=sh)
        raw = download(hip, slot, D * (k * 16 + 4), sh)
        return (raw[:o_windows].view(np.int32).reshape(D, k, 2), raw[o_windows:o_scores].view(np.int32).reshape(D, k),
                raw[o_scores:o_null].view(np.float32).reshape(D, k), raw[o_null:].view(np.float32))


class BertQaDocEnsemble(Ensemble):
    """Ensemble: UTF-8 documents -> ``bert_window_tokenizer`` -> ``bert_large``
    -> ``qa_doc_spans``: question answering over contexts longer than the
    384-token row, by overlapping doc-stride windows, the max-context rule and a
    merge of the windows' answers per document.  The W rows of a request's
    documents are one ``bert_large`` batch; ids, masks and logits stay on the
    device between the steps.  ``max_query_length``, ``doc_stride``,
    ``max_windows``, ``n_best`` and ``max_answer_length`` travel as the
    ensemble's custom request parameters to the steps that read them.
    ``offsets`` (``utils.qa.answer_text_doc`` turns a span and its window back
    into the context's bytes), ``window_info``, ``doc_info``, the ids and the
    logits are outputs too; a request that does not ask for them does not pay
    for their copy."""

    name = "bert_qa_doc_ensemble"
    max_batch_size = 0
    inputs = BertWindowTokenizer.inputs
    outputs = (QaDocSpans.outputs + BertWindowTokenizer.outputs[4:] + BertWindowTokenizer.outputs[:4] +
               (TensorSpec("start_logits", "FP32", [-1, 384]), TensorSpec("end_logits", "FP32", [-1, 384])))
    ensemble_steps = [
        ("bert_window_tokenizer", {"question": "question", "context": "context"},
         {"input_ids": "input_ids", "attention_mask": "attention_mask", "token_type_ids": "token_type_ids",
          "start_mask": "start_mask", "offsets": "offsets", "window_info": "window_info", "doc_info": "doc_info"}),
        ("bert_large", {"input_ids": "input_ids", "attention_mask": "attention_mask",
                        "token_type_ids": "token_type_ids"},
         {"start_logits": "start_logits", "end_logits": "end_logits"}),
        ("qa_doc_spans", {"start_logits": "start_logits", "end_logits": "end_logits",
                          "attention_mask": "attention_mask", "token_type_ids": "token_type_ids",
                          "start_mask": "start_mask", "window_info": "window_info", "doc_info": "doc_info"},
         {"spans": "spans", "windows": "windows", "scores": "scores", "null_score": "null_score"}),
    ]


GPU_MODELS = [DensenetOnnx, PreprocessInception, PreprocessInceptionEnsemble, BertLarge, QaSpans, BertQaEnsemble,
              BertTokenizer, BertQaTextEnsemble, BertWindowTokenizer, QaDocSpans, BertQaDocEnsemble]
# loaded only when --models names them: bert_large_fp32 adds ~2 GB of bf16x3
# weights and 28 captured HIP graphs per instance (round-5 advisor finding)
OPT_IN_GPU_MODELS = [BertLargeFP32]

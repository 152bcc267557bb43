"""CPU model zoo used by the examples and the test-suite.

Behaviour is pinned by the reference's example/test expectations:

* ``simple`` / ``simple_string`` — add/sub of two [1,16] tensors
  (reference src/python/examples/simple_http_infer_client.py:207-290,
  simple_http_string_infer_client.py:41-105).
* ``simple_identity`` — BYTES identity (simple_http_string_infer_client.py:110-141).
* ``onnx_int32_int32_int32`` v1..3 — add/sub; v2,v3 swap the outputs
  (reference src/c++/tests/cc_client_test.cc:435-470).
* ``custom_identity_int32`` — identity with an execution delay, for timeout tests
  (reference src/c++/tests/client_timeout_test.cc:421).
* ``simple_sequence`` / ``simple_dyna_sequence`` / ``simple_string_dyna_sequence``
  — stateful models (simple_grpc_sequence_sync_infer_client.py:186-205).
* ``repeat_int32`` — decoupled: one response per IN element after DELAY[i] ms
  (simple_grpc_custom_repeat.py:78-152).
* ``preprocess_inception`` + ``preprocess_inception_ensemble`` — BYTES image ->
  tensor -> classifier ensemble (ensemble_image_client.py).

Not from the reference: ``qa_spans``, the answer-span step behind ``bert_large``
(examples/python/bert_qa_client.py), here on the host twin of K27, and
``bert_tokenizer``, the step in front of it (examples/python/bert_qa_text_client.py),
here on the host twin of K28; and their doc-stride forms for contexts longer
than a row, ``bert_window_tokenizer`` and ``qa_doc_spans``
(examples/python/bert_qa_doc_client.py), on the host twins of K28w, of K27 with
a start mask and of K29.
"""

import threading
import time

import numpy as np

from .model_base import Model, TensorSpec
from .types import OutputTensor, ServerError


class SimpleAddSub(Model):
    name = "simple"
    max_batch_size = 8
    inputs = (TensorSpec("INPUT0", "INT32", [16]), TensorSpec("INPUT1", "INT32", [16]))
    outputs = (TensorSpec("OUTPUT0", "INT32", [16]), TensorSpec("OUTPUT1", "INT32", [16]))
    swap_versions = ()

    def execute(self, requests):
        out = []
        for r in requests:
            try:
                a = r.input("INPUT0").numpy()
                b = r.input("INPUT1").numpy()
                s, d = np.add(a, b, dtype=a.dtype), np.subtract(a, b, dtype=a.dtype)
                if self.version in self.swap_versions:
                    s, d = d, s
                out.append([self.out("OUTPUT0", s), self.out("OUTPUT1", d)])
            except Exception as e:  # per-request failure
                out.append(e)
        return out


class OnnxInt32(SimpleAddSub):
    name = "onnx_int32_int32_int32"
    platform = "onnxruntime_onnx"
    backend = "onnxruntime"
    versions = (1, 2, 3)
    swap_versions = (2, 3)


class SimpleString(Model):
    name = "simple_string"
    max_batch_size = 8
    inputs = (TensorSpec("INPUT0", "BYTES", [16]), TensorSpec("INPUT1", "BYTES", [16]))
    outputs = (TensorSpec("OUTPUT0", "BYTES", [16]), TensorSpec("OUTPUT1", "BYTES", [16]))

    def execute(self, requests):
        res = []
        for r in requests:
            try:
                a = r.input("INPUT0").numpy()
                b = r.input("INPUT1").numpy()
                ai = np.vectorize(lambda x: int(x))(a).astype(np.int64)
                bi = np.vectorize(lambda x: int(x))(b).astype(np.int64)
                s = np.array([str(x).encode() for x in (ai + bi).ravel()], dtype=np.object_)
                d = np.array([str(x).encode() for x in (ai - bi).ravel()], dtype=np.object_)
                res.append([self.out("OUTPUT0", s.reshape(a.shape)), self.out("OUTPUT1", d.reshape(a.shape))])
            except Exception as e:
                res.append(ServerError("simple_string: %s" % e))
        return res


class Identity(Model):
    """Generic identity over one input (datatype set per instance)."""

    name = "simple_identity"
    max_batch_size = 8
    datatype = "BYTES"

    def __init__(self, version=1, **kw):
        super().__init__(version, **kw)
        self.inputs = (TensorSpec("INPUT0", self.datatype, [-1]),)
        self.outputs = (TensorSpec("OUTPUT0", self.datatype, [-1]),)

    def execute(self, requests):
        delay_ms = float(self.options.get("delay_ms", 0))
        if delay_ms:
            time.sleep(delay_ms / 1000.0)
        return [[self.out("OUTPUT0", r.input("INPUT0").numpy())] for r in requests]


class CustomIdentityInt32(Identity):
    name = "custom_identity_int32"
    datatype = "INT32"

    def __init__(self, version=1, **kw):
        kw.setdefault("delay_ms", 500)
        super().__init__(version, **kw)


class IdentityInt32(Identity):
    """custom_identity_int32 without the delay (soak tests)."""

    name = "identity_int32"
    datatype = "INT32"


class IdentityFP32(Identity):
    name = "identity_fp32"
    datatype = "FP32"
    max_batch_size = 0


class IdentityInt8(Identity):
    name = "identity_int8"
    datatype = "INT8"


class IdentityBF16(Identity):
    name = "identity_bf16"
    datatype = "BF16"
    max_batch_size = 0


class SimpleSequence(Model):
    """out = in + 1 on the START request, else out = in (int or string corrid)."""

    name = "simple_sequence"
    max_batch_size = 8
    sequence_batching = True
    inputs = (TensorSpec("INPUT", "INT32", [1]),)
    outputs = (TensorSpec("OUTPUT", "INT32", [1]),)

    def __init__(self, version=1, **kw):
        super().__init__(version, **kw)
        self._state = {}
        self._lock = threading.Lock()

    def _step(self, r, x):
        return x + (1 if r.sequence_start else 0)

    def execute(self, requests):
        res = []
        for r in requests:
            if r.sequence_id in (0, ""):
                res.append(ServerError(
                    "inference request to model '%s' must specify a non-zero or non-empty correlation ID"
                    % self.name))
                continue
            x = r.input("INPUT").numpy()
            with self._lock:
                y = self._step(r, x)
                if r.sequence_end:
                    self._state.pop(r.sequence_id, None)
            res.append([self.out("OUTPUT", np.asarray(y, dtype=np.int32))])
        return res


class SimpleDynaSequence(SimpleSequence):
    """Like simple_sequence, plus the correlation id on the END request."""

    name = "simple_dyna_sequence"

    def _step(self, r, x):
        y = x + (1 if r.sequence_start else 0)
        if r.sequence_end:
            y = y + int(r.sequence_id)
        return y


class SimpleStringDynaSequence(SimpleSequence):
    """Accumulator keyed by a string correlation id that must decode to int."""

    name = "simple_string_dyna_sequence"

    def _step(self, r, x):
        try:
            corr = int(r.sequence_id)
        except (TypeError, ValueError):
            raise ServerError("simple_string_dyna_sequence requires an integer-decodable sequence id")
        if r.sequence_start:
            acc = x.copy()
        else:
            acc = self._state.get(r.sequence_id, np.zeros_like(x)) + x
        self._state[r.sequence_id] = acc
        y = acc
        if r.sequence_end:
            y = acc + corr
        return y


class RepeatInt32(Model):
    """Decoupled: for each element i of IN, sleep DELAY[i] ms then emit OUT=[IN[i]]
    and IDX=[i]; WAIT ms are slept before releasing the request."""

    name = "repeat_int32"
    decoupled = True
    inputs = (
        TensorSpec("IN", "INT32", [-1]),
        TensorSpec("DELAY", "UINT32", [-1]),
        TensorSpec("WAIT", "UINT32", [1]),
    )
    outputs = (TensorSpec("OUT", "INT32", [1]), TensorSpec("IDX", "UINT32", [1]))

    def execute_decoupled(self, request, emit):
        vals = request.input("IN").numpy().ravel()
        d = request.input("DELAY")
        delays = d.numpy().ravel() if d is not None else np.zeros(len(vals), np.uint32)
        w = request.input("WAIT")
        wait = int(w.numpy().ravel()[0]) if w is not None else 0
        if len(delays) != len(vals):
            raise ServerError("repeat_int32: IN and DELAY must have the same length")
        for i, v in enumerate(vals):
            if delays[i]:
                time.sleep(delays[i] / 1000.0)
            emit([
                self.out("OUT", np.array([v], dtype=np.int32)),
                self.out("IDX", np.array([i], dtype=np.uint32)),
            ])
        if wait:
            time.sleep(wait / 1000.0)


class PreprocessInception(Model):
    """Decode an image (BYTES: PPM/PGM, raw HxWx3 uint8 with a header, or a
    baseline JPEG file, decoded by csrc/host/jpeg.cc through
    ``utils.image.decode_image``) and
    produce INCEPTION-scaled FP32 NCHW [3,224,224].  The custom request
    parameter ``antialias`` (bool, default false) resizes with
    ``utils.image.resize_area`` instead of ``resize_bilinear``.  The custom
    request parameter ``jpeg_scale`` (int64: 1, 2, 4 or 8, or 0 for
    ``utils.image.jpeg_auto_scale`` against 224 x 224; default: full size)
    decodes the request's JPEG blobs at that fraction of their size in the DCT
    domain before the resize; the other encodings ignore it, and any other
    value fails the request."""

    name = "preprocess_inception"
    max_batch_size = 8
    inputs = (TensorSpec("INPUT", "BYTES", [1]),)
    outputs = (TensorSpec("OUTPUT", "FP32", [3, 224, 224]),)

    @staticmethod
    def wants_antialias(request):
        return bool(request.parameters.get("antialias", False))

    @staticmethod
    def jpeg_scale_of(request):
        """The request's ``jpeg_scale``: 0 (automatic), 1, 2, 4 or 8; 1 without the parameter."""
        from triton_client_amd.utils.image import check_jpeg_scale

        if "jpeg_scale" not in request.parameters:
            return 1
        try:
            return check_jpeg_scale(request.parameters["jpeg_scale"])
        except ValueError as e:
            raise ValueError("request parameter %s" % e) from None

    def execute(self, requests):
        from triton_client_amd.utils.image import JPEG_SOI, _jpeg_codec, decode_image, inception_preprocess
        from triton_client_amd.utils.jpeg_stage import parse_at_scale

        res = []
        for r in requests:
            blobs = r.input("INPUT").numpy().reshape(-1)
            aa = self.wants_antialias(r)
            scale = self.jpeg_scale_of(r)
            outs = []
            for b in blobs:
                if scale != 1 and bytes(b[:2]) == JPEG_SOI:
                    b = bytes(b)
                    img = decode_image(b, parse_at_scale(_jpeg_codec(), b, scale, 224, 224).scale)
                else:
                    img = decode_image(b)
                outs.append(inception_preprocess(img, 224, 224, "NCHW", antialias=aa))
            res.append([self.out("OUTPUT", np.stack(outs).astype(np.float32))])
        return res


class AddSubBatched(Model):
    """INT32 add/sub with dynamic batching; also served on the native fast path.

    ``execute_native`` receives one batch from tcserve (csrc/cpp/server) with
    host pointers (in-band tensors or system shared memory) and writes the
    outputs in place.
    """

    name = "add_sub_batched"
    max_batch_size = 8
    inputs = (TensorSpec("INPUT0", "INT32", [16]), TensorSpec("INPUT1", "INT32", [16]))
    outputs = (TensorSpec("OUTPUT0", "INT32", [16]), TensorSpec("OUTPUT1", "INT32", [16]))
    dynamic_batching = {"preferred": [], "max_queue_delay_us": 200}
    instance_count = 2
    supports_native = True
    native_delay_s = 0.0  # tests: hold each native batch this long (region-lifetime checks)

    def execute(self, requests):
        out = []
        for r in requests:
            try:
                a = r.input("INPUT0").numpy()
                b = r.input("INPUT1").numpy()
                out.append([self.out("OUTPUT0", a + b), self.out("OUTPUT1", a - b)])
            except Exception as e:  # per-request failure
                out.append(e)
        return out

    def execute_native(self, instance, b):
        import ctypes
        import time

        t0 = time.monotonic_ns()
        if self.native_delay_s:
            time.sleep(self.native_delay_s)
        ni, no = b.n_inputs, b.n_outputs
        for r in range(b.n_requests):
            rows = b.rows[r]
            arrs = []
            for k in range(ni):
                ref = b.inputs[r * ni + k]
                if ref.kind != 0:
                    raise ServerError("add_sub_batched runs on host memory only")
                arrs.append(np.ctypeslib.as_array((ctypes.c_int32 * (rows * 16)).from_address(ref.ptr)))
            res = (arrs[0] + arrs[1], arrs[0] - arrs[1])
            for k in range(no):
                ref = b.outputs[r * no + k]
                if ref.ptr:
                    if ref.kind != 0:
                        raise ServerError("add_sub_batched runs on host memory only")
                    np.ctypeslib.as_array((ctypes.c_int32 * (rows * 16)).from_address(ref.ptr))[:] = res[k]
        t1 = time.monotonic_ns()
        b.timing_ns[0] = 0
        b.timing_ns[1] = t1 - t0
        b.timing_ns[2] = 0


class AddSubPipelined(AddSubBatched):
    """add_sub_batched with every tcserve batcher rule engaged: 2 instances,
    a preferred batch of 8 rows (full batches -> staggered starts), idle-aware
    and pipelined dispatch of partial batches.  Exists so the threaded
    batcher's rules run under the sanitizers (tools/sanitize_tcserve.py) and
    the CPU tests; the rules themselves are unit-tested on scripted arrivals
    (tests/test_batch_policy.py)."""

    name = "add_sub_pipelined"
    dynamic_batching = {"preferred": [8], "max_queue_delay_us": 300, "pipelined": True}
    instance_count = 2
    native_delay_s = 0.0002  # each batch holds its instance ~0.2 ms: queues build, rules fire


class FrontendSink(Model):
    """densenet_onnx-shaped model that does no compute: FP32 [3,224,224] in,
    FP32 [1000] out (first input value broadcast).  Served natively, it
    measures what the tcserve front end and the transport alone sustain for
    the headline request shape, with no GPU involved."""

    name = "frontend_sink"
    max_batch_size = 8
    inputs = (TensorSpec("data_0", "FP32", [3, 224, 224]),)
    outputs = (TensorSpec("fc6_1", "FP32", [1000]),)
    dynamic_batching = {"preferred": [], "max_queue_delay_us": 100}
    instance_count = 2
    supports_native = True

    def execute(self, requests):
        out = []
        for r in requests:
            x = r.input("data_0").numpy()
            out.append([self.out("fc6_1", np.repeat(x.reshape(x.shape[0], -1)[:, :1], 1000, axis=1))])
        return out

    def execute_native(self, instance, b):
        import ctypes

        for r in range(b.n_requests):
            rows = b.rows[r]
            src, dst = b.inputs[r], b.outputs[r]
            if src.kind != 0 or (dst.ptr and dst.kind != 0):
                raise ServerError("frontend_sink runs on host memory only")
            if not dst.ptr:
                continue
            x = np.ctypeslib.as_array((ctypes.c_float * (rows * 3 * 224 * 224)).from_address(src.ptr))
            y = np.ctypeslib.as_array((ctypes.c_float * (rows * 1000)).from_address(dst.ptr)).reshape(rows, 1000)
            y[:] = x.reshape(rows, -1)[:, :1]
        b.timing_ns[0] = b.timing_ns[1] = b.timing_ns[2] = 0


class BertSink(Model):
    """bert_large-shaped model that does no compute: INT32 [384] input_ids /
    attention_mask / token_type_ids in, FP32 [384] start/end logits out (the
    mask as float).  The CPU stand-in of bench.py's bert_large sweep, so the
    multi-rank launch + fan-out + sweep aggregation path runs without a GPU."""

    name = "bert_sink"
    max_batch_size = 64
    SEQ = 384
    inputs = (TensorSpec("input_ids", "INT32", [384]), TensorSpec("attention_mask", "INT32", [384]),
              TensorSpec("token_type_ids", "INT32", [384]))
    outputs = (TensorSpec("start_logits", "FP32", [384]), TensorSpec("end_logits", "FP32", [384]))
    dynamic_batching = {"preferred": [], "max_queue_delay_us": 100}
    instance_count = 2
    supports_native = True

    def execute(self, requests):
        out = []
        for r in requests:
            m = r.input("attention_mask").numpy().astype(np.float32)
            out.append([self.out("start_logits", m), self.out("end_logits", -m)])
        return out

    def execute_native(self, instance, b):
        import ctypes

        n = self.SEQ
        for r in range(b.n_requests):
            rows = b.rows[r]
            src = b.inputs[r * 3 + 1]
            if src.kind != 0:
                raise ServerError("bert_sink runs on host memory only")
            m = np.ctypeslib.as_array((ctypes.c_int32 * (rows * n)).from_address(src.ptr)).astype(np.float32)
            for k, sign in ((0, 1.0), (1, -1.0)):
                dst = b.outputs[r * 2 + k]
                if not dst.ptr:
                    continue
                if dst.kind != 0:
                    raise ServerError("bert_sink runs on host memory only")
                np.ctypeslib.as_array((ctypes.c_float * (rows * n)).from_address(dst.ptr))[:] = sign * m
        b.timing_ns[0] = b.timing_ns[1] = b.timing_ns[2] = 0


class QaSpans(Model):
    """``qa_spans`` — the n best answer spans of question-answering logits, the
    step after ``bert_large``: FP32 [384] ``start_logits`` / ``end_logits`` and
    INT32 [384] ``attention_mask`` / ``token_type_ids`` in; per row INT32
    ``spans`` [n_best, 2] (first and last token), FP32 ``scores`` [n_best] and
    FP32 ``null_score`` [1] (``start[0] + end[0]``, the SQuAD-v2 no-answer
    score) out.  The rule is csrc/kernels/qa_span_math.h: both ends on context
    tokens (``attention_mask >= 1`` and ``token_type_ids == 1``), at most
    ``max_answer_length`` tokens, scores descending, ties to the lower start
    and then the lower end; ranks past the candidates hold ``(-1, -1)`` and
    ``-FLT_MAX``.  This class runs the host twin of K27 (``HostCodec.qa_spans``),
    one call per batch; server/gpu_models.py QaSpans runs the kernel.

    Custom request parameters: ``n_best`` (int64, 1..64, default 20) and
    ``max_answer_length`` (int64, 1..384, default 30).  Requests of different
    ``n_best`` share a batch.  A value out of range or of another type fails
    its own request."""

    name = "qa_spans"
    max_batch_size = 128
    SEQ = 384
    N_BEST, N_BEST_MAX = 20, 64
    MAX_ANSWER, MAX_ANSWER_MAX = 30, 384
    inputs = (TensorSpec("start_logits", "FP32", [384]), TensorSpec("end_logits", "FP32", [384]),
              TensorSpec("attention_mask", "INT32", [384]), TensorSpec("token_type_ids", "INT32", [384]))
    outputs = (TensorSpec("spans", "INT32", [-1, 2]), TensorSpec("scores", "FP32", [-1]),
               TensorSpec("null_score", "FP32", [1]))
    dynamic_batching = {"preferred": [], "max_queue_delay_us": 100}
    INPUT_DTYPES = (np.float32, np.float32, np.int32, np.int32)

    @staticmethod
    def _int_param(request, name, default, lo, hi):
        v = request.parameters.get(name, default)
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
            raise ServerError("request parameter %s must be an int64 in [%d, %d], not %r" % (name, lo, hi, v))
        return int(v)

    @classmethod
    def plan(cls, requests):
        """Per request ``(first_row, rows, n_best, max_answer_length)``, or the
        ServerError of its parameters; and the rows of the batch."""
        out, total = [], 0
        for r in requests:
            try:
                k = cls._int_param(r, "n_best", cls.N_BEST, 1, cls.N_BEST_MAX)
                ln = cls._int_param(r, "max_answer_length", cls.MAX_ANSWER, 1, cls.MAX_ANSWER_MAX)
            except ServerError as e:
                out.append(e)
                continue
            n = int(r.input("start_logits").shape[0])
            out.append((total, n, k, ln))
            total += n
        return out, total

    @staticmethod
    def row_params(plan, total):
        """(k_row, len_row, kmax) of a batch's plan."""
        k_row, len_row = np.zeros(total, dtype=np.int32), np.zeros(total, dtype=np.int32)
        for p in plan:
            if not isinstance(p, Exception):
                first, n, k, ln = p
                k_row[first:first + n] = k
                len_row[first:first + n] = ln
        return k_row, len_row, int(k_row.max()) if total else 1

    def results(self, plan, spans, scores, null):
        """The per-request outputs from the batch's [rows, kmax(, 2)] arrays."""
        res = []
        for p in plan:
            if isinstance(p, Exception):
                res.append(p)
                continue
            first, n, k, _ = p
            res.append([self.out("spans", np.ascontiguousarray(spans[first:first + n, :k])),
                        self.out("scores", np.ascontiguousarray(scores[first:first + n, :k])),
                        self.out("null_score", np.ascontiguousarray(null[first:first + n]).reshape(n, 1))])
        return res

    def load(self):
        from triton_client_amd.ops import host_codec

        self._codec = host_codec.load()

    def run_host(self, requests, plan, total):
        names = [s.name for s in self.inputs]
        good = [r for r, p in zip(requests, plan) if not isinstance(p, Exception)]
        cols = [np.concatenate([np.asarray(r.input(nm).numpy(), dtype=dt).reshape(-1, self.SEQ) for r in good])
                for nm, dt in zip(names, self.INPUT_DTYPES)]
        k_row, len_row, kmax = self.row_params(plan, total)
        return self._codec.qa_spans(*cols, k_row, len_row, kmax)

    def execute(self, requests):
        plan, total = self.plan(requests)
        if total == 0:
            return plan
        return self.results(plan, *self.run_host(requests, plan, total))


class BertTokenizer(Model):
    """``bert_tokenizer`` — UTF-8 text to the three inputs of ``bert_large``, the
    step in front of it: BYTES [1] ``question`` and ``context`` in; per row INT32
    [384] ``input_ids`` / ``attention_mask`` / ``token_type_ids``, INT32 [384, 2]
    ``offsets`` (the bytes of the context each context piece covers, (0, 0)
    elsewhere; ``utils.qa.answer_text`` turns a span back into text) and INT32 [1]
    ``overflow`` (context pieces that did not fit; ``bert_window_tokenizer`` is the
    doc-stride form) out.
    The rule is csrc/kernels/wordpiece_core.h: BERT's uncased WordPiece, a row
    ``[CLS] question[:max_query_length] [SEP] context [SEP]``, ``token_type_ids``
    1 on the context pieces only, so that ``qa_spans`` never answers with the
    last ``[SEP]``.  This class runs the host twin of K28
    (``HostCodec.wordpiece_tokenize``), one call per batch;
    server/gpu_models.py BertTokenizer runs the kernel.

    The vocabulary is ``TCAMD_BERT_VOCAB`` (the server's ``--bert-vocab``), else
    the demonstration vocabulary that ships with the package; it is read at
    load.  Custom request parameter: ``max_query_length`` (int64, 1..381,
    default 64); requests of different values share a batch.  A text that is
    not valid UTF-8 or longer than 65,536 bytes fails its own request."""

    name = "bert_tokenizer"
    max_batch_size = 128
    SEQ = 384
    MAX_QUERY = 64
    inputs = (TensorSpec("question", "BYTES", [1]), TensorSpec("context", "BYTES", [1]))
    outputs = (TensorSpec("input_ids", "INT32", [384]), TensorSpec("attention_mask", "INT32", [384]),
               TensorSpec("token_type_ids", "INT32", [384]), TensorSpec("offsets", "INT32", [384, 2]),
               TensorSpec("overflow", "INT32", [1]))
    dynamic_batching = {"preferred": [], "max_queue_delay_us": 100}

    @classmethod
    def plan(cls, requests):
        """Per request ``(first_row, questions, contexts, max_query_length)``, or
        the ServerError of its parameters, shapes or lengths; and the rows of the
        batch."""
        from triton_client_amd.utils.wordpiece import MAX_TEXT_BYTES

        out, total = [], 0
        for r in requests:
            try:
                mq = QaSpans._int_param(r, "max_query_length", cls.MAX_QUERY, 1, cls.SEQ - 3)
                texts = []
                for nm in ("question", "context"):
                    col = [bytes(x) if not isinstance(x, str) else x.encode("utf-8")
                           for x in np.asarray(r.input(nm).numpy(), dtype=object).reshape(-1)]
                    if any(len(x) > MAX_TEXT_BYTES for x in col):
                        raise ServerError("bert_tokenizer: %s too long" % nm)
                    texts.append(col)
                if len(texts[0]) != len(texts[1]):
                    raise ServerError("bert_tokenizer: question and context must have one element per row")
            except ServerError as e:
                out.append(e)
                continue
            out.append((total, texts[0], texts[1], mq))
            total += len(texts[0])
        return out, total

    @staticmethod
    def batch_texts(plan):
        """(questions, contexts, max_query_length per row) of the plan's good requests."""
        qs, cs, mq = [], [], []
        for p in plan:
            if not isinstance(p, Exception):
                qs += p[1]
                cs += p[2]
                mq += [p[3]] * len(p[1])
        return qs, cs, np.asarray(mq, dtype=np.int32)

    def results(self, plan, ids, mask, tt, offsets, overflow, status, device=None):
        """The per-request outputs from the batch's arrays; a request with a row
        whose status is not 0 gets that row's error.  ``device`` = (tensor, device
        id): ids / mask / type ids ``[3, rows, S]`` left on the device, handed out
        as ``DeviceView`` with the tensor as ``owner``."""
        from triton_client_amd.utils.wordpiece import status_error

        from .types import DeviceView

        res = []
        for p in plan:
            if isinstance(p, Exception):
                res.append(p)
                continue
            first, n = p[0], len(p[1])
            bad = [status_error(s) for s in status[first:first + n] if s]
            if bad:
                res.append(ServerError(bad[0]))
                continue
            outs = []
            for k, (nm, a) in enumerate((("input_ids", ids), ("attention_mask", mask), ("token_type_ids", tt))):
                if device is None:
                    outs.append(self.out(nm, np.ascontiguousarray(a[first:first + n])))
                else:
                    t, dev_id = device
                    row = self.SEQ * 4
                    o = OutputTensor(nm, "INT32", [n, self.SEQ],
                                     DeviceView(t[k].data_ptr() + first * row, n * row, dev_id))
                    o.owner = t  # keeps the device memory alive while the ensemble holds the tensor
                    outs.append(o)
            outs.append(self.out("offsets", np.ascontiguousarray(offsets[first:first + n])))
            outs.append(self.out("overflow", np.ascontiguousarray(overflow[first:first + n]).reshape(n, 1)))
            res.append(outs)
        return res

    def load(self):
        from triton_client_amd.ops import host_codec
        from triton_client_amd.utils import wordpiece

        self._codec = host_codec.load()
        self.vocab_path = wordpiece.default_vocab_path()
        try:
            self.vocab = wordpiece.Vocab.load(self.vocab_path)
        except (OSError, ValueError) as e:
            raise ServerError("bert_tokenizer: cannot load the vocabulary %s: %s" % (self.vocab_path, e))

    def run_host(self, plan):
        qs, cs, mq = self.batch_texts(plan)
        return self._codec.wordpiece_tokenize(qs, cs, self.vocab, mq, self.SEQ)

    def execute(self, requests):
        plan, total = self.plan(requests)
        if total == 0:
            return plan
        if total > self.max_batch_size:
            return [ServerError("batch of %d rows exceeds max_batch_size" % total)] * len(requests)
        return self.results(plan, *self.run_host(plan))


class BertWindowTokenizer(BertTokenizer):
    """``bert_window_tokenizer`` — ``bert_tokenizer`` for contexts longer than a
    row: BYTES [D] ``question`` and ``context`` in (D documents, at most 128);
    the doc-stride windows of all of them out, W rows in document order: INT32
    [W, 384] ``input_ids`` / ``attention_mask`` / ``token_type_ids`` /
    ``start_mask``, INT32 [W, 384, 2] ``offsets`` (bytes of the whole context),
    INT32 [W, 4] ``window_info`` (document, first context piece, context pieces,
    token of the first context piece) and INT32 [D, 4] ``doc_info`` (first row,
    windows, context pieces, 0).  The rule is rule 8 of
    csrc/kernels/wordpiece_core.h: window ``w`` starts at context piece ``w *
    doc_stride``, the last one is the first that reaches the end, a context
    without a piece still owns one row, and ``start_mask`` is 1 where the window
    is the max-context window of the piece (run_squad's rule), which
    ``qa_doc_spans`` needs to start each answer in one window only.  This class
    runs the host twin of K28w (``HostCodec.wordpiece_windows``);
    server/gpu_models.py BertWindowTokenizer runs the kernel.

    Not batched (``max_batch_size`` 0): a request is a set of documents, and
    its rows are a batch for ``bert_large``.  Custom request parameters:
    ``max_query_length`` (int64, 1..381, default 64), ``doc_stride`` (int64,
    1..381, default 128) and ``max_windows`` (int64, 1..128, default 128, per
    document).  A document that is not valid UTF-8, longer than 65,536 bytes,
    needs more than ``max_windows`` windows or does not fit the 128 rows of a
    request fails the request, with a message that names the document."""

    name = "bert_window_tokenizer"
    max_batch_size = 0
    MAX_DOCS = MAX_ROWS = 128
    DOC_STRIDE, MAX_WINDOWS = 128, 128
    inputs = (TensorSpec("question", "BYTES", [-1]), TensorSpec("context", "BYTES", [-1]))
    outputs = (TensorSpec("input_ids", "INT32", [-1, 384]), TensorSpec("attention_mask", "INT32", [-1, 384]),
               TensorSpec("token_type_ids", "INT32", [-1, 384]), TensorSpec("start_mask", "INT32", [-1, 384]),
               TensorSpec("offsets", "INT32", [-1, 384, 2]), TensorSpec("window_info", "INT32", [-1, 4]),
               TensorSpec("doc_info", "INT32", [-1, 4]))
    dynamic_batching = None

    @classmethod
    def plan_one(cls, r):
        """``(questions, contexts, max_query_length, doc_stride, max_windows)`` of
        a request; ServerError for its parameters, shapes or lengths."""
        from triton_client_amd.utils.wordpiece import MAX_TEXT_BYTES

        mq = QaSpans._int_param(r, "max_query_length", cls.MAX_QUERY, 1, cls.SEQ - 3)
        ds = QaSpans._int_param(r, "doc_stride", cls.DOC_STRIDE, 1, cls.SEQ - 3)
        mw = QaSpans._int_param(r, "max_windows", cls.MAX_WINDOWS, 1, cls.MAX_ROWS)
        texts = []
        for nm in ("question", "context"):
            col = [bytes(x) if not isinstance(x, str) else x.encode("utf-8")
                   for x in np.asarray(r.input(nm).numpy(), dtype=object).reshape(-1)]
            for d, x in enumerate(col):
                if len(x) > MAX_TEXT_BYTES:
                    raise ServerError("%s: document %d: %s too long" % (cls.name, d, nm))
            texts.append(col)
        if len(texts[0]) != len(texts[1]):
            raise ServerError("%s: question and context must have one element per document" % cls.name)
        if not 1 <= len(texts[0]) <= cls.MAX_DOCS:
            raise ServerError("%s: a request holds 1 to %d documents, not %d" % (cls.name, cls.MAX_DOCS, len(texts[0])))
        return texts[0], texts[1], mq, ds, mw

    @classmethod
    def doc_error(cls, doc_info, max_windows):
        """The message of the first document whose status is not 0, or None."""
        from triton_client_amd.utils.wordpiece import status_error

        for d, (_, W, _, st) in enumerate(np.asarray(doc_info).tolist()):
            if st == 0:
                continue
            if st & 0xFF == 6:
                if W > max_windows:
                    return "%s: document %d: context needs %d windows, max_windows %d" % (cls.name, d, W, max_windows)
                return "%s: document %d: context needs %d windows, exceeds %d rows" % (cls.name, d, W, cls.MAX_ROWS)
            return status_error(st, "%s: document %d" % (cls.name, d))
        return None

    def window_results(self, doc_info, n_rows, host, device=None):
        """The outputs of a request: ``host`` = name -> array of the capacity's
        rows; ``device`` = (tensor ``[4, rows, S]``, device id) hands the four id
        tensors on as ``DeviceView`` with the tensor as ``owner``."""
        from .types import DeviceView

        outs = []
        for k, nm in enumerate(("input_ids", "attention_mask", "token_type_ids", "start_mask")):
            if device is None:
                outs.append(self.out(nm, np.ascontiguousarray(host[nm][:n_rows])))
            else:
                t, dev_id = device
                o = OutputTensor(nm, "INT32", [n_rows, self.SEQ],
                                 DeviceView(t[k].data_ptr(), n_rows * self.SEQ * 4, dev_id))
                o.owner = t
                outs.append(o)
        outs.append(self.out("offsets", np.ascontiguousarray(host["offsets"][:n_rows])))
        outs.append(self.out("window_info", np.ascontiguousarray(host["window_info"][:n_rows])))
        outs.append(self.out("doc_info", np.ascontiguousarray(doc_info).view(np.int32)))
        return outs

    def run_host_one(self, p):
        qs, cs, mq, ds, mw = p
        ids, mask, tt, sm, offsets, winfo, dinfo, n_rows = self._codec.wordpiece_windows(
            qs, cs, self.vocab, mq, ds, mw, self.SEQ, self.MAX_ROWS)
        err = self.doc_error(dinfo, mw)
        if err:
            return ServerError(err)
        host = {"input_ids": ids, "attention_mask": mask, "token_type_ids": tt, "start_mask": sm, "offsets": offsets,
                "window_info": winfo}
        return self.window_results(dinfo, n_rows, host)

    def execute(self, requests):
        out = []
        for r in requests:
            try:
                out.append(self.run_host_one(self.plan_one(r)))
            except ServerError as e:
                out.append(e)
        return out


class QaDocSpans(Model):
    """``qa_doc_spans`` — the n best answers of each document from the logits of
    its doc-stride windows, the step after ``bert_large`` behind
    ``bert_window_tokenizer``: FP32 [W, 384] ``start_logits`` / ``end_logits``,
    INT32 [W, 384] ``attention_mask`` / ``token_type_ids`` / ``start_mask``,
    INT32 [W, 4] ``window_info`` and INT32 [D, 4] ``doc_info`` in; per document
    INT32 ``spans`` [n_best, 2] (first and last token of row ``windows``), INT32
    ``windows`` [n_best], FP32 ``scores`` [n_best] and FP32 ``null_score`` (the
    lowest ``start[0] + end[0]`` of its windows) out.  The rule is
    csrc/kernels/qa_span_math.h: per window the spans of ``qa_spans`` that start
    where ``start_mask`` is 1, then per document the best of the union by score,
    the lower document start piece, the shorter span; ranks past the candidates
    hold ``(-1, -1)``, ``-1`` and ``-FLT_MAX``.  This class runs the host twins
    of K27 with a start mask and of K29; server/gpu_models.py QaDocSpans runs
    the kernels.

    Not batched.  Custom request parameters: ``n_best`` (int64, 1..64, default
    20) and ``max_answer_length`` (int64, 1..384, default 30)."""

    name = "qa_doc_spans"
    max_batch_size = 0
    SEQ = 384
    MAX_ROWS = MAX_DOCS = 128
    inputs = (TensorSpec("start_logits", "FP32", [-1, 384]), TensorSpec("end_logits", "FP32", [-1, 384]),
              TensorSpec("attention_mask", "INT32", [-1, 384]), TensorSpec("token_type_ids", "INT32", [-1, 384]),
              TensorSpec("start_mask", "INT32", [-1, 384]), TensorSpec("window_info", "INT32", [-1, 4]),
              TensorSpec("doc_info", "INT32", [-1, 4]))
    outputs = (TensorSpec("spans", "INT32", [-1, -1, 2]), TensorSpec("windows", "INT32", [-1, -1]),
               TensorSpec("scores", "FP32", [-1, -1]), TensorSpec("null_score", "FP32", [-1]))
    ROW_INPUTS = (("start_logits", np.float32), ("end_logits", np.float32), ("attention_mask", np.int32),
                  ("token_type_ids", np.int32), ("start_mask", np.int32))

    @classmethod
    def plan_one(cls, r):
        """``(rows, documents, n_best, max_answer_length)`` of a request; ServerError
        for its parameters or shapes."""
        k = QaSpans._int_param(r, "n_best", QaSpans.N_BEST, 1, QaSpans.N_BEST_MAX)
        ln = QaSpans._int_param(r, "max_answer_length", QaSpans.MAX_ANSWER, 1, QaSpans.MAX_ANSWER_MAX)
        W = int(r.input("start_logits").shape[0])
        D = int(r.input("doc_info").shape[0])
        for nm, _ in cls.ROW_INPUTS:
            if list(r.input(nm).shape) != [W, cls.SEQ]:
                raise ServerError("%s: %s must be [%d, %d]" % (cls.name, nm, W, cls.SEQ))
        if list(r.input("window_info").shape) != [W, 4] or list(r.input("doc_info").shape) != [D, 4]:
            raise ServerError("%s: window_info must be [%d, 4] and doc_info [D, 4]" % (cls.name, W))
        if not (1 <= W <= cls.MAX_ROWS and 1 <= D <= cls.MAX_DOCS):
            raise ServerError("%s: a request holds 1 to %d rows and documents" % (cls.name, cls.MAX_ROWS))
        return W, D, k, ln

    def doc_results(self, k, spans, windows, scores, null):
        return [self.out("spans", np.ascontiguousarray(spans[:, :k])),
                self.out("windows", np.ascontiguousarray(windows[:, :k])),
                self.out("scores", np.ascontiguousarray(scores[:, :k])), self.out("null_score", np.ascontiguousarray(null))]

    def load(self):
        from triton_client_amd.ops import host_codec

        self._codec = host_codec.load()

    def run_host_one(self, r, p):
        W, D, k, ln = p
        cols = [np.asarray(r.input(nm).numpy(), dtype=dt).reshape(W, self.SEQ) for nm, dt in self.ROW_INPUTS]
        winfo = np.asarray(r.input("window_info").numpy(), dtype=np.int32).reshape(W, 4)
        dinfo = np.asarray(r.input("doc_info").numpy(), dtype=np.int32).reshape(D, 4).view(np.uint32)
        lists = self._codec.qa_spans_masked(*cols, np.full(W, k, np.int32), np.full(W, ln, np.int32), k)
        return self.doc_results(k, *self._codec.qa_merge(*lists, winfo, dinfo, np.full(D, k, np.int32), k))

    def execute(self, requests):
        out = []
        for r in requests:
            try:
                out.append(self.run_host_one(r, self.plan_one(r)))
            except (ServerError, ValueError) as e:
                out.append(e if isinstance(e, ServerError) else ServerError("%s: %s" % (self.name, e)))
        return out


CPU_MODELS = [
    BertTokenizer,
    QaSpans,
    BertWindowTokenizer,
    QaDocSpans,
    FrontendSink,
    BertSink,
    SimpleAddSub,
    OnnxInt32,
    SimpleString,
    Identity,
    CustomIdentityInt32,
    IdentityInt32,
    IdentityFP32,
    IdentityBF16,
    IdentityInt8,
    SimpleSequence,
    SimpleDynaSequence,
    SimpleStringDynaSequence,
    RepeatInt32,
    PreprocessInception,
    AddSubBatched,
    AddSubPipelined,
]

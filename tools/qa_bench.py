#!/usr/bin/env python3
"""Answer spans served against answer spans computed by the client, and K27
``qa_spans`` alone.

Served (default): one server with ``bert_large``, ``qa_spans`` and
``bert_qa_ensemble``; a closed loop over gRPC at each ``--concurrency``, in two
modes on that same server, alternating ``--reps`` times:

  ensemble  ``bert_qa_ensemble``, asking only for ``spans``, ``scores`` and
            ``null_score``: the logits never leave the device
  client    ``bert_large`` raw, then the numpy routine of utils/qa.py on every
            row of the response, inside the loop: what a user has to do
            without the ``qa_spans`` model

One JSON line per (mode, concurrency, rep): answered requests per second and
latency percentiles, the latency including the client's span computation.

``--kernel``: K27 alone on random logits, timed with HIP events around each
launch after a warm-up, at (rows, n_best, max_answer_length) = (128, 20, 30),
(128, 64, 384) and (1, 20, 30); next to it the host twin on the same rows.

``--text``: the same two for the text route.  Served: one server with
``bert_tokenizer``, ``bert_large``, ``qa_spans`` and both ensembles, in two modes:

  text      ``bert_qa_text_ensemble`` on a question of 40 bytes and a context of
            1.5 KB per row, asking for ``spans``, ``scores``, ``null_score``,
            ``offsets`` and ``overflow``: ids and logits never leave the device
  client    the Python twin of the tokenizer (tests/wordpiece_cases.py) on the
            client, inside the loop, then ``bert_qa_ensemble`` on its ids: what a
            user had to do before there was a text route

``--device-tokenizer 0|1`` starts that server with ``TCAMD_DEVICE_TOKENIZER`` set,
to hold K28 against the host twin behind the same ensemble.  ``--text --kernel``:
K28 ``wordpiece_tokenize`` alone (its ten launches between two events) at 1, 8
and 128 rows of such texts and at 128 rows of 64 KB contexts, next to the host
twin on one core and, where it is installed, ``tokenizers``' ``encode_batch``.

``--text --bert-packed``: ``bert_qa_text_ensemble`` against a server started
with ``TCAMD_BERT_PACKED=0`` and one with ``=1`` (the padding-free bert_large
route), loaded in turn ``--reps`` times, contexts of each of ``--packed-contexts`` bytes.

``--doc-stride N``: the same two for contexts longer than a row.  Served: one
server with the doc-stride models and ``bert_qa_ensemble``, one document of 40
and ``--context-bytes`` bytes per request (default 3000: the client's route below
is bound to the 1021 pieces a 1024-token row of the host twin holds), in two modes:

  doc       ``bert_qa_doc_ensemble`` asking for ``spans``, ``windows``,
            ``scores``, ``null_score``, ``offsets`` and ``doc_info``: ids and
            logits never leave the device
  client    what a user had to do before: the host twin of the tokenizer on a
            row of 1024 tokens, the windows sliced out of it in numpy
            (``utils.qa.doc_windows``), one ``bert_qa_ensemble`` request of W
            rows for the logits, and ``utils.qa.merge_windows``, all inside the
            measured latency

``--doc-stride N --kernel``: K28w ``wordpiece_windows`` (its launches between two
events) and K27 masked + K29 ``qa_merge`` at 1 and 16 documents of
``--context-bytes`` (default 4096), and K28w
against K28 on 1, 8 and 128 contexts of 1000 bytes, which fit one window (the cost
of the extra launch).
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

SEQ = 384
KERNEL_POINTS = ((128, 20, 30), (128, 64, 384), (1, 20, 30))


def make_inputs(rows, seed):
    import numpy as np

    rng = np.random.default_rng(seed)
    ids = rng.integers(1000, 30000, size=(rows, SEQ), dtype=np.int32)
    mask = np.ones((rows, SEQ), dtype=np.int32)
    tt = np.zeros((rows, SEQ), dtype=np.int32)
    for i in range(rows):
        n = SEQ if i % 3 == 0 else int(rng.integers(32, SEQ))
        q = int(rng.integers(8, max(9, n // 3)))
        mask[i, n:] = 0
        ids[i, n:] = 0
        tt[i, q:n] = 1
    return ids, mask, tt


def kernel_time(iters):
    import numpy as np
    import torch

    from triton_client_amd.ops import hip, host_codec

    torch.cuda.set_device(0)
    hc = host_codec.load()
    s = torch.cuda.current_stream().cuda_stream
    for rows, k, L in KERNEL_POINTS:
        rng = np.random.default_rng(rows + k)
        _, mask, tt = make_inputs(rows, 1)
        st = rng.standard_normal((rows, SEQ)).astype(np.float32)
        en = rng.standard_normal((rows, SEQ)).astype(np.float32)
        d = [torch.from_numpy(a).cuda() for a in (st, en, mask, tt)]
        k_row = torch.full((rows,), k, dtype=torch.int32, device="cuda")
        len_row = torch.full((rows,), L, dtype=torch.int32, device="cuda")
        spans = torch.zeros(rows, k, 2, dtype=torch.int32, device="cuda")
        scores = torch.zeros(rows, k, dtype=torch.float32, device="cuda")
        null = torch.zeros(rows, dtype=torch.float32, device="cuda")

        def launch():
            hip.qa_spans(d[0].data_ptr(), d[1].data_ptr(), SEQ * 4, d[2].data_ptr(), d[3].data_ptr(), SEQ * 4, rows,
                         SEQ, k_row.data_ptr(), len_row.data_ptr(), k, spans.data_ptr(), scores.data_ptr(),
                         null.data_ptr(), stream=s)

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
        host = []
        for _ in range(5):
            t0 = time.perf_counter()
            w_spans, w_scores, w_null = hc.qa_spans(st, en, mask, tt, [k] * rows, [L] * rows, k)
            host.append((time.perf_counter() - t0) * 1e3)
        same = (np.array_equal(spans.cpu().numpy(), w_spans)
                and np.array_equal(scores.cpu().numpy().view(np.uint32), w_scores.view(np.uint32))
                and np.array_equal(null.cpu().numpy().view(np.uint32), w_null.view(np.uint32)))
        ok = (mask >= 1) & (tt == 1)
        cands = sum(int(ok[r, i:i + L].sum()) for r in range(rows) for i in range(SEQ) if ok[r, i])
        print(json.dumps({"kernel": "K27 qa_spans", "rows": rows, "n_best": k, "max_answer_length": L, "S": SEQ,
                          "candidates": cands, "launches": iters, "mean_us": round(float(np.mean(times)), 2),
                          "min_us": round(float(np.min(times)), 2), "max_us": round(float(np.max(times)), 2),
                          "host_twin_ms_min": round(float(np.min(host)), 3), "equals_host_twin": bool(same)}),
              flush=True)


_WORDS = ("the kernel folds every code point through one table and matches pieces greedily from the left while "
          "the host twin walks each text front to back and both agree on every id and every byte offset of a "
          "context piece so a span of tokens becomes an answer again").split()
TEXT_POINTS = ((1, 1500), (8, 1500), (128, 1500), (128, 65536))


def make_texts(rows, context_bytes, seed=0):
    """``rows`` questions of 40 bytes and contexts of ``context_bytes`` bytes: English words and punctuation."""
    import random

    rng = random.Random(seed)

    def text(n, end):
        out = []
        while sum(len(w) + 1 for w in out) < n:
            out.append(rng.choice(_WORDS) + (rng.choice([",", ".", ""]) if rng.random() < 0.15 else ""))
        return (" ".join(out)[:n - 1] + end).encode()

    return [text(40, "?") for _ in range(rows)], [text(context_bytes, ".") for _ in range(rows)]


def text_kernel_time(iters):
    import numpy as np
    import torch

    from triton_client_amd.ops import hip, host_codec
    from triton_client_amd.utils import wordpiece

    torch.cuda.set_device(0)
    hc = host_codec.load()
    vocab = wordpiece.Vocab.load(wordpiece.default_vocab_path())
    vocab_dev = torch.from_numpy(vocab.image.view(np.int32).copy()).cuda()
    s = torch.cuda.current_stream().cuda_stream
    try:
        from tests import wordpiece_cases as wc

        lib = wc.library_tokenizer(wordpiece.default_vocab_path())
    except ImportError:
        lib = None
    for rows, ctx_bytes in TEXT_POINTS:
        qs, cs = make_texts(rows, ctx_bytes, rows)
        buf, table = wordpiece.pack_texts(qs, cs)
        text = torch.from_numpy(np.array(buf)).cuda()
        tab = torch.from_numpy(table.view(np.int32).copy()).cuda()
        mq = torch.full((rows,), 64, dtype=torch.int32, device="cuda")
        ws_bytes = hip.wordpiece_workspace(rows, buf.size)
        ws = torch.zeros(ws_bytes, dtype=torch.uint8, device="cuda")
        ids, mask, tt = (torch.zeros(rows, SEQ, dtype=torch.int32, device="cuda") for _ in range(3))
        offsets = torch.zeros(rows, SEQ, 2, dtype=torch.int32, device="cuda")
        overflow, status = (torch.zeros(rows, dtype=torch.int32, device="cuda") for _ in range(2))

        def launch():
            hip.wordpiece_tokenize(text.data_ptr(), buf.size, tab.data_ptr(), mq.data_ptr(), rows, SEQ,
                                   vocab_dev.data_ptr(), vocab.image.size, ws.data_ptr(), ws_bytes, ids.data_ptr(),
                                   mask.data_ptr(), tt.data_ptr(), offsets.data_ptr(), overflow.data_ptr(),
                                   status.data_ptr(), stream=s)

        n_iter = iters if ctx_bytes < 65536 else max(10, iters // 10)
        for _ in range(5):
            launch()
        torch.cuda.synchronize()
        times = []
        for _ in range(n_iter):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            launch()
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b) * 1e3)
        host = []
        for _ in range(3):
            t0 = time.perf_counter()
            want = hc.wordpiece_tokenize(qs, cs, vocab, 64)
            host.append((time.perf_counter() - t0) * 1e3)
        got = (ids, mask, tt, offsets, overflow, status)
        same = all(np.array_equal(g.cpu().numpy().view(np.uint32), np.asarray(w).view(np.uint32))
                   for g, w in zip(got, want))
        res = {"kernel": "K28 wordpiece_tokenize", "rows": rows, "question_bytes": 40, "context_bytes": ctx_bytes,
               "text_bytes": int(buf.size), "launches": n_iter, "mean_us": round(float(np.mean(times)), 2),
               "min_us": round(float(np.min(times)), 2), "max_us": round(float(np.max(times)), 2),
               "host_twin_ms_min": round(float(np.min(host)), 3), "equals_host_twin": bool(same),
               "overflow_rows": int((want[4] > 0).sum())}
        if lib is not None:
            pairs = [(q.decode(), c.decode()) for q, c in zip(qs, cs)]
            enc = []
            for _ in range(3):
                t0 = time.perf_counter()
                lib.encode_batch(pairs, add_special_tokens=False)
                enc.append((time.perf_counter() - t0) * 1e3)
            res["tokenizers_encode_batch_ms_min"] = round(float(np.min(enc)), 3)
        print(json.dumps(res), flush=True)


def text_served(args):
    import numpy as np

    import tritonclient.grpc as grpcclient
    from tests import wordpiece_cases as wc
    from triton_client_amd.perf.harness import ServerProcess
    from triton_client_amd.utils import wordpiece

    log = os.path.abspath(args.server_log) if args.server_log else None
    if log:
        os.makedirs(os.path.dirname(log), exist_ok=True)
    env = {"TCAMD_DEVICE_TOKENIZER": str(args.device_tokenizer)} if args.device_tokenizer is not None else {}
    srv = ServerProcess(device=0, models="bert_tokenizer,bert_large,qa_spans,bert_qa_ensemble,bert_qa_text_ensemble",
                        log_path=log, extra_args=["--native-grpc", args.native_grpc], env=env)
    try:
        srv.wait_ready(timeout=900, model="bert_qa_text_ensemble")
        qs, cs = make_texts(args.rows, 1500, 0)
        twin_vocab = wc.TwinVocab(wordpiece.default_vocab_path())
        c = grpcclient.InferenceServerClient(srv.grpc_url)
        text_ins = []
        for name, col in (("question", qs), ("context", cs)):
            x = grpcclient.InferInput(name, [args.rows, 1], "BYTES")
            x.set_data_from_numpy(np.array(col, dtype=object).reshape(-1, 1))
            text_ins.append(x)

        def id_inputs():
            ids, mask, tt, _, _, _ = wc.tokenize_rows(qs, cs, twin_vocab, 64)
            ins = []
            for name, a in (("input_ids", ids), ("attention_mask", mask), ("token_type_ids", tt)):
                x = grpcclient.InferInput(name, list(a.shape), "INT32")
                x.set_data_from_numpy(a)
                ins.append(x)
            return ins

        r = c.infer("bert_qa_text_ensemble", text_ins)
        ref = c.infer("bert_qa_ensemble", id_inputs())
        agree = all(np.array_equal(r.as_numpy(n).view(np.uint32), ref.as_numpy(n).view(np.uint32))
                    for n in ("spans", "scores", "null_score"))
        t0 = time.perf_counter()
        for _ in range(3):
            id_inputs()
        twin_ms = (time.perf_counter() - t0) / 3 * 1e3
        text_out = ["spans", "scores", "null_score", "offsets", "overflow"]
        for rep in range(args.reps):
            for conc in args.concurrency:
                res = closed_loop(c, grpcclient, "bert_qa_text_ensemble", text_ins, text_out, conc, args.warmup,
                                  args.seconds, lambda result: None)
                res.update(mode="text")
                # the client tokenizes every request anew, before it is sent: inside the measured latency
                res2 = closed_loop(c, grpcclient, "bert_qa_ensemble", id_inputs, ["spans", "scores", "null_score"],
                                   conc, args.warmup, args.seconds, lambda result: None)
                res2.update(mode="client", python_twin_ms_per_request=round(twin_ms, 3))
                for x in (res, res2):
                    x.update(rep=rep, rows_per_request=args.rows, context_bytes=1500,
                             text_equals_id_ensemble=bool(agree), native_grpc=args.native_grpc,
                             device_tokenizer=args.device_tokenizer)
                    print(json.dumps(x), flush=True)
        c.close()
    finally:
        srv.stop()


def text_packed_served(args):
    """``--text --bert-packed``: ``bert_qa_text_ensemble`` against a server with
    ``TCAMD_BERT_PACKED=0`` and one with ``=1``, loaded in turn ``--reps`` times;
    the same closed loops against each.  Every request carries the same rows, so
    the route of a batch follows from the rule alone (``BertLarge.packed_bucket``
    on the twin tokenizer's mask) and is printed with each line; bert_large's
    own statistics give its batches, rows and the mean compute_input (where the
    token count and its sync land) and compute_infer per batch."""
    import numpy as np

    import tritonclient.grpc as grpcclient
    from tests import wordpiece_cases as wc
    from triton_client_amd.perf.harness import ServerProcess
    from triton_client_amd.server.gpu_models import BertLarge
    from triton_client_amd.utils import wordpiece

    twin_vocab = wc.TwinVocab(wordpiece.default_vocab_path())
    text_out = ["spans", "scores", "null_score", "offsets", "overflow"]
    points = []  # per context size: (bytes, tokens per request, route per requests in a batch, inputs)
    for ctx in args.packed_contexts:
        qs, cs = make_texts(args.rows, ctx, 0)
        _, mask, _, _, _, _ = wc.tokenize_rows(qs, cs, twin_vocab, 64)
        tokens = int((np.asarray(mask) >= 1).sum())
        # a batch of n such requests: the route its token count picks
        routes = {n: BertLarge.packed_bucket(n * args.rows, n * tokens) for n in (1, 2, 4, 8)
                  if n * args.rows <= BertLarge.max_batch_size}
        ins = []
        for name, col in (("question", qs), ("context", cs)):
            x = grpcclient.InferInput(name, [args.rows, 1], "BYTES")
            x.set_data_from_numpy(np.array(col, dtype=object).reshape(-1, 1))
            ins.append(x)
        points.append((ctx, tokens, {k: ("padded" if v is None else "packed-%d" % v[1]) for k, v in routes.items()},
                       ins))

    def bert_stats(c):
        st = c.get_inference_statistics("bert_large", as_json=True)["model_stats"][0]
        inf = {k: st.get("inference_stats", {}).get(k, {}) for k in ("compute_input", "compute_infer")}
        return {"executions": int(st.get("execution_count", 0)), "rows": int(st.get("inference_count", 0)),
                "compute_input_ns": int(inf["compute_input"].get("ns", 0)),
                "compute_infer_ns": int(inf["compute_infer"].get("ns", 0))}

    for rep in range(args.reps):
        for knob in (0, 1):
            log = os.path.abspath(args.server_log) + ".packed%d" % knob if args.server_log else None
            if log:
                os.makedirs(os.path.dirname(log), exist_ok=True)
            srv = ServerProcess(device=0, log_path=log, extra_args=["--native-grpc", args.native_grpc],
                                models="bert_tokenizer,bert_large,qa_spans,bert_qa_ensemble,bert_qa_text_ensemble",
                                env={"TCAMD_BERT_PACKED": str(knob)})
            try:
                srv.wait_ready(timeout=900, model="bert_qa_text_ensemble")
                c = grpcclient.InferenceServerClient(srv.grpc_url)
                for (ctx, tokens, routes, text_ins), conc in ((p, k) for p in points for k in args.concurrency):
                    s0 = bert_stats(c)
                    res = closed_loop(c, grpcclient, "bert_qa_text_ensemble", text_ins, text_out, conc, args.warmup,
                                      args.seconds, lambda result: None)
                    s1 = bert_stats(c)
                    ex = max(1, s1["executions"] - s0["executions"])  # the ns sums grow once per batch
                    res.update(mode="text", bert_packed=knob, rep=rep, rows_per_request=args.rows, context_bytes=ctx,
                               tokens_per_request=tokens, route_by_requests_per_batch=routes,
                               bert_batches=s1["executions"] - s0["executions"],
                               bert_rows_per_batch=round((s1["rows"] - s0["rows"]) / ex, 2),
                               bert_compute_input_us=round((s1["compute_input_ns"] - s0["compute_input_ns"]) / ex / 1e3, 1),
                               bert_compute_infer_us=round((s1["compute_infer_ns"] - s0["compute_infer_ns"]) / ex / 1e3, 1),
                               native_grpc=args.native_grpc)
                    print(json.dumps(res), flush=True)
                c.close()
            finally:
                srv.stop()


def _event_times(torch, launch, iters, warm=5):
    for _ in range(warm):
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
    return times


def doc_kernel_time(iters, doc_stride, context_bytes):
    import numpy as np
    import torch

    from triton_client_amd.ops import hip, host_codec
    from triton_client_amd.utils import wordpiece

    torch.cuda.set_device(0)
    hc = host_codec.load()
    vocab = wordpiece.Vocab.load(wordpiece.default_vocab_path())
    vocab_dev = torch.from_numpy(vocab.image.view(np.int32).copy()).cuda()
    s = torch.cuda.current_stream().cuda_stream
    stat = lambda t: {"mean_us": round(float(np.mean(t)), 2), "min_us": round(float(np.min(t)), 2),  # noqa: E731
                      "max_us": round(float(np.max(t)), 2)}

    def windows_call(qs, cs, out_rows=128):
        buf, table = wordpiece.pack_texts(qs, cs)
        docs = len(qs)
        text = torch.from_numpy(np.array(buf)).cuda()
        tab = torch.from_numpy(table.view(np.int32).copy()).cuda()
        par = torch.tensor([[64] * docs, [doc_stride] * docs, [128] * docs], dtype=torch.int32, device="cuda")
        ws_bytes = hip.wordpiece_windows_workspace(docs, buf.size)
        ws = torch.zeros(ws_bytes, dtype=torch.uint8, device="cuda")
        o = {n: torch.zeros(out_rows, SEQ, dtype=torch.int32, device="cuda") for n in ("ids", "mask", "tt", "sm")}
        o["offsets"] = torch.zeros(out_rows, SEQ, 2, dtype=torch.int32, device="cuda")
        o["winfo"] = torch.zeros(out_rows, 4, dtype=torch.int32, device="cuda")
        o["dinfo"] = torch.zeros(docs, 4, dtype=torch.int32, device="cuda")
        o["n_rows"] = torch.zeros(1, dtype=torch.int32, device="cuda")

        def launch():
            hip.wordpiece_windows(text.data_ptr(), buf.size, tab.data_ptr(), par[0].data_ptr(), par[1].data_ptr(),
                                  par[2].data_ptr(), docs, SEQ, vocab_dev.data_ptr(), vocab.image.size, ws.data_ptr(),
                                  ws_bytes, out_rows, o["ids"].data_ptr(), o["mask"].data_ptr(), o["tt"].data_ptr(),
                                  o["sm"].data_ptr(), o["offsets"].data_ptr(), o["winfo"].data_ptr(),
                                  o["dinfo"].data_ptr(), o["n_rows"].data_ptr(), stream=s)

        return launch, o, (buf, table, text, tab, ws_bytes, ws)

    for docs in (1, 16):
        qs, cs = make_texts(docs, context_bytes, docs)
        launch, o, _ = windows_call(qs, cs)
        times = _event_times(torch, launch, iters)
        t0 = time.perf_counter()
        want = hc.wordpiece_windows(qs, cs, vocab, 64, doc_stride, 128)
        host_ms = (time.perf_counter() - t0) * 1e3
        got = [o[n].cpu().numpy() for n in ("ids", "mask", "tt", "sm", "offsets", "winfo")]
        n_rows = int(o["n_rows"].cpu()[0])
        same = n_rows == want[7] and all(np.array_equal(g, w) for g, w in zip(got, want[:6])) and \
            np.array_equal(o["dinfo"].cpu().numpy(), want[6].view(np.int32))
        res = {"kernel": "K28w wordpiece_windows", "documents": docs, "context_bytes": context_bytes,
               "doc_stride": doc_stride, "rows": n_rows, "launches": iters, "host_twin_ms": round(host_ms, 3),
               "equals_host_twin": bool(same)}
        res.update(stat(times))
        print(json.dumps(res), flush=True)
        # K27 with the start mask, then K29, on random logits over those windows
        rng = np.random.default_rng(docs)
        st, en = (torch.from_numpy(rng.standard_normal((128, SEQ)).astype(np.float32)).cuda() for _ in range(2))
        k = 20
        k_row = torch.full((128,), k, dtype=torch.int32, device="cuda")
        len_row = torch.full((128,), 30, dtype=torch.int32, device="cuda")
        l_spans = torch.zeros(128, k, 2, dtype=torch.int32, device="cuda")
        l_scores, l_null = torch.zeros(128, k, device="cuda"), torch.zeros(128, device="cuda")
        d_spans = torch.zeros(docs, k, 2, dtype=torch.int32, device="cuda")
        d_win = torch.zeros(docs, k, dtype=torch.int32, device="cuda")
        d_scores, d_null = torch.zeros(docs, k, device="cuda"), torch.zeros(docs, device="cuda")

        def spans():
            hip.qa_spans_masked(st.data_ptr(), en.data_ptr(), SEQ * 4, o["mask"].data_ptr(), o["tt"].data_ptr(),
                                o["sm"].data_ptr(), SEQ * 4, n_rows, SEQ, k_row.data_ptr(), len_row.data_ptr(), k,
                                l_spans.data_ptr(), l_scores.data_ptr(), l_null.data_ptr(), stream=s)

        def merge():
            hip.qa_merge(l_spans.data_ptr(), l_scores.data_ptr(), l_null.data_ptr(), n_rows, o["winfo"].data_ptr(),
                         o["dinfo"].data_ptr(), docs, k_row.data_ptr(), k, d_spans.data_ptr(), d_win.data_ptr(),
                         d_scores.data_ptr(), d_null.data_ptr(), stream=s)

        t27 = _event_times(torch, spans, iters)
        t29 = _event_times(torch, merge, iters)
        lists = hc.qa_spans_masked(st.cpu().numpy()[:n_rows], en.cpu().numpy()[:n_rows], want[1][:n_rows],
                                   want[2][:n_rows], want[3][:n_rows], [k] * n_rows, [30] * n_rows, k)
        w29 = hc.qa_merge(*lists, want[5][:n_rows], want[6], [k] * docs, k)
        same = all(g.cpu().numpy().tobytes() == w.tobytes() for g, w in zip((d_spans, d_win, d_scores, d_null), w29))
        res = {"kernel": "K29 qa_merge", "documents": docs, "rows": n_rows, "n_best": k, "launches": iters,
               "equals_host_twin": bool(same), "k27_masked_mean_us": round(float(np.mean(t27)), 2),
               "k27_masked_min_us": round(float(np.min(t27)), 2)}
        res.update(stat(t29))
        print(json.dumps(res), flush=True)
    # contexts that fit one window: K28w against K28 on the same texts
    for rows in (1, 8, 128):
        qs, cs = make_texts(rows, 1000, rows)
        launch_w, o, (buf, table, text, tab, ws_bytes, ws) = windows_call(qs, cs)
        mq = torch.full((rows,), 64, dtype=torch.int32, device="cuda")
        ids, mask, tt = (torch.zeros(rows, SEQ, dtype=torch.int32, device="cuda") for _ in range(3))
        offsets = torch.zeros(rows, SEQ, 2, dtype=torch.int32, device="cuda")
        overflow, status = (torch.zeros(rows, dtype=torch.int32, device="cuda") for _ in range(2))

        def launch_k28():
            hip.wordpiece_tokenize(text.data_ptr(), buf.size, tab.data_ptr(), mq.data_ptr(), rows, SEQ,
                                   vocab_dev.data_ptr(), vocab.image.size, ws.data_ptr(), ws_bytes, ids.data_ptr(),
                                   mask.data_ptr(), tt.data_ptr(), offsets.data_ptr(), overflow.data_ptr(),
                                   status.data_ptr(), stream=s)

        tw, t28 = [], []
        for _ in range(3):  # alternate, so that drift hits both alike
            t28 += _event_times(torch, launch_k28, iters // 3 + 1)
            tw += _event_times(torch, launch_w, iters // 3 + 1)
        same = int(o["n_rows"].cpu()[0]) == rows and torch.equal(o["ids"][:rows], ids) and \
            torch.equal(o["offsets"][:rows], offsets) and not bool(overflow.any())
        print(json.dumps({"kernel": "K28w against K28, one window", "rows": rows, "context_bytes": 1000,
                          "k28_mean_us": round(float(np.mean(t28)), 2), "k28_min_us": round(float(np.min(t28)), 2),
                          "k28w_mean_us": round(float(np.mean(tw)), 2), "k28w_min_us": round(float(np.min(tw)), 2),
                          "ratio_of_means": round(float(np.mean(tw) / np.mean(t28)), 3),
                          "ratio_of_mins": round(float(np.min(tw) / np.min(t28)), 3), "same_rows": bool(same)}),
              flush=True)


def doc_served(args):
    import numpy as np

    import tritonclient.grpc as grpcclient
    from triton_client_amd.ops import host_codec
    from triton_client_amd.perf.harness import ServerProcess
    from triton_client_amd.utils import qa, wordpiece

    log = os.path.abspath(args.server_log) if args.server_log else None
    if log:
        os.makedirs(os.path.dirname(log), exist_ok=True)
    srv = ServerProcess(device=0, models="bert_window_tokenizer,bert_large,qa_doc_spans,bert_qa_doc_ensemble,qa_spans,"
                                         "bert_qa_ensemble", log_path=log,
                        extra_args=["--native-grpc", args.native_grpc])
    try:
        srv.wait_ready(timeout=900, model="bert_qa_doc_ensemble")
        qs, cs = make_texts(1, args.context_bytes, 0)
        hc = host_codec.load()
        vocab = wordpiece.Vocab.load(wordpiece.default_vocab_path())
        c = grpcclient.InferenceServerClient(srv.grpc_url)
        doc_ins = []
        for name, col in (("question", qs), ("context", cs)):
            x = grpcclient.InferInput(name, [1], "BYTES")
            x.set_data_from_numpy(np.array(col, dtype=object))
            doc_ins.append(x)
        keep = {}

        def client_windows():
            """The rows a client cuts by hand: one row of 1024 tokens from the host twin, sliced."""
            ids, mask, tt, offsets, overflow, status = hc.wordpiece_tokenize(qs, cs, vocab, 64, 1024)
            if status[0] or overflow[0]:
                raise SystemExit("the client-side route needs a context of at most 1021 pieces")
            first = int(tt[0].argmax()) if tt[0].any() else 2
            qn, P = first - 2, int(tt[0].sum())
            starts, lens, best = qa.doc_windows(P, qn, args.doc_stride, SEQ)
            W = len(starts)
            w_ids, w_mask, w_tt, w_sm = (np.zeros((W, SEQ), np.int32) for _ in range(4))
            w_off = np.zeros((W, SEQ, 2), np.int32)
            for w in range(W):
                a, n = int(starts[w]), int(lens[w])
                w_ids[w, :first] = ids[0, :first]
                w_ids[w, first:first + n] = ids[0, first + a:first + a + n]
                w_ids[w, first + n] = vocab.sep
                w_mask[w, :first + n + 1] = 1
                w_tt[w, first:first + n] = 1
                w_sm[w, first:first + n] = best[a:a + n] == w
                w_off[w, first:first + n] = offsets[0, first + a:first + a + n]
            winfo = np.stack([np.zeros(W, np.int64), starts, lens, np.full(W, first)], axis=1).astype(np.int32)
            keep.update(ids=w_ids, mask=w_mask, tt=w_tt, sm=w_sm, winfo=winfo, dinfo=np.array([[0, W, P, 0]], np.int32),
                        offsets=w_off)
            ins = []
            for name, a in (("input_ids", w_ids), ("attention_mask", w_mask), ("token_type_ids", w_tt)):
                x = grpcclient.InferInput(name, list(a.shape), "INT32")
                x.set_data_from_numpy(a)
                ins.append(x)
            return ins

        def client_merge(result):
            return qa.merge_windows(result.as_numpy("start_logits"), result.as_numpy("end_logits"), keep["mask"],
                                    keep["tt"], keep["sm"], keep["winfo"], keep["dinfo"], 20, 30)

        params = {"doc_stride": args.doc_stride}
        r = c.infer("bert_qa_doc_ensemble", doc_ins, parameters=params)
        mine = client_merge(c.infer("bert_qa_ensemble", client_windows()))
        same_rows = all(np.array_equal(r.as_numpy(n), keep[k]) for n, k in (
            ("input_ids", "ids"), ("attention_mask", "mask"), ("token_type_ids", "tt"), ("start_mask", "sm"),
            ("offsets", "offsets"), ("window_info", "winfo"), ("doc_info", "dinfo")))
        agree = all(np.array_equal(r.as_numpy(n).view(np.uint32), m.view(np.uint32))
                    for n, m in zip(("spans", "windows", "scores", "null_score"), mine))
        t0 = time.perf_counter()
        for _ in range(3):
            client_windows()
        cut_ms = (time.perf_counter() - t0) / 3 * 1e3
        doc_out = ["spans", "windows", "scores", "null_score", "offsets", "doc_info"]
        for rep in range(args.reps):
            for conc in args.concurrency:
                res = closed_loop(c, grpcclient, "bert_qa_doc_ensemble", doc_ins, doc_out, conc, args.warmup,
                                  args.seconds, lambda result: None, parameters=params)
                res.update(mode="doc")
                res2 = closed_loop(c, grpcclient, "bert_qa_ensemble", client_windows, ["start_logits", "end_logits"],
                                   conc, args.warmup, args.seconds, client_merge)
                res2.update(mode="client", client_tokenize_and_slice_ms=round(cut_ms, 3))
                for x in (res, res2):
                    x.update(rep=rep, documents_per_request=1, context_bytes=args.context_bytes,
                             doc_stride=args.doc_stride, windows=int(keep["dinfo"][0, 1]),
                             same_windows=bool(same_rows), doc_equals_client_route=bool(agree),
                             native_grpc=args.native_grpc)
                    print(json.dumps(x), flush=True)
        c.close()
    finally:
        srv.stop()


def closed_loop(c, mod, model, ins, outputs, conc, warmup, seconds, post, parameters=None):
    """``conc`` requests in flight; ``post(result)`` runs in the callback, inside the measured latency;
    ``ins`` may be a function that makes a request's inputs, called inside it too."""
    lock = threading.Lock()
    done = threading.Event()
    state = {"lat": [], "errors": 0, "stop": False, "inflight": conc, "measure": False}
    outs = [mod.InferRequestedOutput(n) for n in outputs]

    def send():
        t0 = time.perf_counter()

        def cb(result, error):
            if error is None:
                post(result)
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

        c.async_infer(model, ins() if callable(ins) else ins, callback=cb, outputs=outs, parameters=parameters)

    for _ in range(conc):
        send()
    time.sleep(warmup)
    with lock:
        state["measure"] = True
        state["lat"] = []
    t0 = time.perf_counter()
    time.sleep(seconds)
    with lock:
        lat = sorted(state["lat"])
        state["measure"] = False
    dt = time.perf_counter() - t0
    with lock:
        state["stop"] = True
    done.wait(60)
    n = len(lat)
    return {"model": model, "concurrency": conc, "seconds": round(dt, 2), "requests": n, "errors": state["errors"],
            "infer_per_s": round(n / dt, 1), "p50_ms": round(lat[n // 2] * 1e3, 3) if n else None,
            "p99_ms": round(lat[min(n - 1, int(n * 0.99))] * 1e3, 3) if n else None}


def served(args):
    import numpy as np

    import tritonclient.grpc as grpcclient
    from triton_client_amd.perf.harness import ServerProcess
    from triton_client_amd.utils import qa

    log = os.path.abspath(args.server_log) if args.server_log else None
    if log:
        os.makedirs(os.path.dirname(log), exist_ok=True)
    srv = ServerProcess(device=0, models="bert_large,qa_spans,bert_qa_ensemble", log_path=log,
                        extra_args=["--native-grpc", args.native_grpc])
    try:
        srv.wait_ready(timeout=900, model="bert_qa_ensemble")
        ids, mask, tt = make_inputs(args.rows, 0)
        c = grpcclient.InferenceServerClient(srv.grpc_url)
        ins = []
        for name, a in (("input_ids", ids), ("attention_mask", mask), ("token_type_ids", tt)):
            x = grpcclient.InferInput(name, list(a.shape), "INT32")
            x.set_data_from_numpy(a)
            ins.append(x)

        def client_spans(result):
            st, en = result.as_numpy("start_logits"), result.as_numpy("end_logits")
            return [qa.n_best_spans(st[i], en[i], mask[i], tt[i], 20, 30) for i in range(args.rows)]

        # the two modes answer alike: the ensemble's spans are the client's routine on the ensemble's own logits
        r = c.infer("bert_qa_ensemble", ins)
        mine = client_spans(r)
        agree = all(np.array_equal(r.as_numpy("spans")[i], mine[i][0])
                    and np.array_equal(r.as_numpy("scores")[i].view(np.uint32), mine[i][1].view(np.uint32))
                    for i in range(args.rows))
        modes = {"ensemble": ("bert_qa_ensemble", ["spans", "scores", "null_score"], lambda result: None),
                 "client": ("bert_large", ["start_logits", "end_logits"], client_spans)}
        for rep in range(args.reps):
            for conc in args.concurrency:
                for mode, (model, outputs, post) in modes.items():
                    res = closed_loop(c, grpcclient, model, ins, outputs, conc, args.warmup, args.seconds, post)
                    res.update(mode=mode, rep=rep, rows_per_request=args.rows, n_best=20, max_answer_length=30,
                               ensemble_equals_client_routine=bool(agree), native_grpc=args.native_grpc,
                               device_qa_spans=os.environ.get("TCAMD_DEVICE_QA_SPANS", "1") != "0")
                    print(json.dumps(res), flush=True)
        c.close()
    finally:
        srv.stop()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--kernel", action="store_true", help="time K27 alone instead of the served loops")
    ap.add_argument("--text", action="store_true", help="the text route: K28 / bert_qa_text_ensemble (see above)")
    ap.add_argument("--device-tokenizer", type=int, default=None, choices=[0, 1],
                    help="--text: TCAMD_DEVICE_TOKENIZER of the server (default: the knob's default)")
    ap.add_argument("--doc-stride", type=int, default=None, metavar="N",
                    help="the doc-stride route: K28w, K29 / bert_qa_doc_ensemble at this stride (see above)")
    ap.add_argument("--context-bytes", type=int, default=None,
                    help="--doc-stride: bytes of the context (default 4096 with --kernel, else 3000)")
    ap.add_argument("--packed-contexts", type=int, nargs="+", default=[300, 600, 1500], metavar="BYTES",
                    help="--text --bert-packed: the context sizes, each looped at every concurrency on every server "
                         "(with the demonstration vocabulary 105, 205 and 384 tokens a row: fill 128, fill 256, padded)")
    ap.add_argument("--bert-packed", action="store_true",
                    help="--text: the text ensemble against a TCAMD_BERT_PACKED=0 and a =1 server, loaded in turn")
    ap.add_argument("--iters", type=int, default=200, help="--kernel: timed launches per point (after 10 warm-up)")
    ap.add_argument("--concurrency", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--rows", type=int, default=1, help="rows per request")
    ap.add_argument("--reps", type=int, default=2, help="rounds over the concurrencies and modes")
    ap.add_argument("--seconds", type=float, default=8.0)
    ap.add_argument("--warmup", type=float, default=2.0)
    ap.add_argument("--native-grpc", default="auto", choices=["auto", "on", "off"],
                    help="the server's gRPC front end: the native one answers bert_large itself and relays an "
                         "ensemble to the Python one; off = the Python front end answers both modes")
    ap.add_argument("--server-log", default="", metavar="PATH", help="keep the server's log in this file")
    args = ap.parse_args()
    if args.doc_stride is not None:
        if args.context_bytes is None:
            args.context_bytes = 4096 if args.kernel else 3000
        doc_kernel_time(args.iters, args.doc_stride, args.context_bytes) if args.kernel else doc_served(args)
    elif args.text and args.bert_packed:
        text_packed_served(args)
    elif args.text:
        text_kernel_time(args.iters) if args.kernel else text_served(args)
    elif args.kernel:
        kernel_time(args.iters)
    else:
        served(args)


if __name__ == "__main__":
    main()

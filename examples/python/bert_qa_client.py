#!/usr/bin/env python3
"""Token ids through the `bert_qa_ensemble` ensemble (`bert_large`, then the
`qa_spans` answer-span step on the device): prints the n best answer spans of
every row.  There is no tokenizer here: the ids are seeded random tokens laid
out like a SQuAD feature (question, context, padding).  `--check` also asks for
the logits, recomputes the spans from them with numpy (utils/qa.py) and
compares spans and scores exactly."""
import argparse
import sys

import numpy as np

import tritonclient.grpc as grpcclient
import tritonclient.http as httpclient

SEQ = 384


def make_inputs(rows, seed):
    """Seeded ids / attention_mask / token_type_ids [rows, 384]: a question of 8
    or more tokens (segment 0), a context (segment 1), zero padding."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-v", "--verbose", action="store_true")
    ap.add_argument("-m", "--model-name", default="bert_qa_ensemble")
    ap.add_argument("-u", "--url", default=None)
    ap.add_argument("-i", "--protocol", default="HTTP", choices=["HTTP", "gRPC", "http", "grpc"])
    ap.add_argument("-b", "--rows", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--n-best", type=int, default=None, help="answers per row (server default 20, at most 64)")
    ap.add_argument("--max-answer-length", type=int, default=None, help="tokens (server default 30)")
    ap.add_argument("--show", type=int, default=5, help="ranks printed per row")
    ap.add_argument("--check", action="store_true", help="recompute the spans from the returned logits with numpy")
    a = ap.parse_args()
    protocol = a.protocol.lower()
    mod = grpcclient if protocol == "grpc" else httpclient
    client = mod.InferenceServerClient(a.url or ("localhost:8001" if protocol == "grpc" else "localhost:8000"),
                                       verbose=a.verbose)
    ids, mask, tt = make_inputs(a.rows, a.seed)
    ins = []
    for name, arr in (("input_ids", ids), ("attention_mask", mask), ("token_type_ids", tt)):
        x = mod.InferInput(name, list(arr.shape), "INT32")
        x.set_data_from_numpy(arr)
        ins.append(x)
    params = {}
    if a.n_best is not None:
        params["n_best"] = a.n_best
    if a.max_answer_length is not None:
        params["max_answer_length"] = a.max_answer_length
    names = ["spans", "scores", "null_score"] + (["start_logits", "end_logits"] if a.check else [])
    r = client.infer(a.model_name, ins, outputs=[mod.InferRequestedOutput(n) for n in names],
                     parameters=params or None)
    spans, scores, null = r.as_numpy("spans"), r.as_numpy("scores"), r.as_numpy("null_score")
    for i in range(a.rows):
        context = int(((mask[i] >= 1) & (tt[i] == 1)).sum())
        print("row %d: null_score %.6f, context tokens %d" % (i, null[i, 0], context))
        print("    rank  start  end  score")
        for j in range(min(a.show, spans.shape[1])):
            print("    %4d  %5d  %3d  %.6f" % (j, spans[i, j, 0], spans[i, j, 1], scores[i, j]))
    if a.check:
        from triton_client_amd.utils import qa

        st, en = r.as_numpy("start_logits"), r.as_numpy("end_logits")
        k = spans.shape[1]
        for i in range(a.rows):
            w_spans, w_scores, w_null = qa.n_best_spans(st[i], en[i], mask[i], tt[i], k,
                                                        30 if a.max_answer_length is None else a.max_answer_length)
            same = (np.array_equal(spans[i], w_spans)
                    and np.array_equal(scores[i].view(np.uint32), w_scores.view(np.uint32))
                    and np.array_equal(null[i].view(np.uint32), np.array([w_null], np.float32).view(np.uint32)))
            if not same:
                print("error: row %d differs from the numpy recomputation" % i)
                sys.exit(1)
    print("PASS")


if __name__ == "__main__":
    main()

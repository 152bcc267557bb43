#!/usr/bin/env python3
"""A question and a context, as text, through the `bert_qa_text_ensemble`
ensemble (`bert_tokenizer` -> `bert_large` -> `qa_spans`, ids and logits staying
on the device): prints the n best answers as text, cut out of the context by
the byte offsets the tokenizer returned.  `bert_large` is served with synthetic
weights, so the answers show the plumbing, not reading comprehension.
`--check` also asks for the ids, recomputes ids and offsets with the Python
twin of the tokenizer (tests/wordpiece_cases.py) from the same vocabulary file
and compares exactly."""
import argparse
import os
import sys

import numpy as np

import tritonclient.grpc as grpcclient
import tritonclient.http as httpclient

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
QUESTION = "What does the tokenizer return for every context piece?"
CONTEXT = ("The tokenizer folds the text, splits it into words and matches pieces greedily. For every context "
           "piece it returns byte offsets into the original text, so that a span of tokens becomes an answer again.")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-v", "--verbose", action="store_true")
    ap.add_argument("-m", "--model-name", default="bert_qa_text_ensemble")
    ap.add_argument("-u", "--url", default=None)
    ap.add_argument("-i", "--protocol", default="HTTP", choices=["HTTP", "gRPC", "http", "grpc"])
    ap.add_argument("-q", "--question", action="append", help="repeat for several rows (with as many --context)")
    ap.add_argument("-c", "--context", action="append")
    ap.add_argument("--n-best", type=int, default=None, help="answers per row (server default 20, at most 64)")
    ap.add_argument("--max-answer-length", type=int, default=None, help="tokens (server default 30)")
    ap.add_argument("--max-query-length", type=int, default=None, help="question pieces kept (server default 64)")
    ap.add_argument("--show", type=int, default=5, help="ranks printed per row")
    ap.add_argument("--vocab", default=None, help="the server's vocab.txt, for --check (default: the demonstration one)")
    ap.add_argument("--check", action="store_true", help="recompute ids and offsets with the Python twin")
    a = ap.parse_args()
    questions = [q.encode("utf-8") for q in (a.question or [QUESTION])]
    contexts = [c.encode("utf-8") for c in (a.context or [CONTEXT])]
    if len(questions) != len(contexts):
        sys.exit("error: one --context per --question")
    protocol = a.protocol.lower()
    mod = grpcclient if protocol == "grpc" else httpclient
    client = mod.InferenceServerClient(a.url or ("localhost:8001" if protocol == "grpc" else "localhost:8000"),
                                       verbose=a.verbose)
    ins = []
    for name, col in (("question", questions), ("context", contexts)):
        x = mod.InferInput(name, [len(col), 1], "BYTES")
        x.set_data_from_numpy(np.array(col, dtype=object).reshape(-1, 1))
        ins.append(x)
    params = {k: v for k, v in (("n_best", a.n_best), ("max_answer_length", a.max_answer_length),
                                ("max_query_length", a.max_query_length)) if v is not None}
    names = ["spans", "scores", "null_score", "offsets", "overflow"]
    names += ["input_ids", "attention_mask", "token_type_ids"] if a.check else []
    r = client.infer(a.model_name, ins, outputs=[mod.InferRequestedOutput(n) for n in names], parameters=params or None)
    from triton_client_amd.utils.qa import answer_text

    spans, scores, null = r.as_numpy("spans"), r.as_numpy("scores"), r.as_numpy("null_score")
    offsets, overflow = r.as_numpy("offsets"), r.as_numpy("overflow")
    for i, ctx in enumerate(contexts):
        print("row %d: null_score %.6f, context pieces cut off %d" % (i, null[i, 0], overflow[i, 0]))
        print("    rank  start  end  score      answer")
        for j in range(min(a.show, spans.shape[1])):
            text = answer_text(ctx, spans[i, j], offsets[i]).decode("utf-8", "replace")
            print("    %4d  %5d  %3d  %9.6f  %s" % (j, spans[i, j, 0], spans[i, j, 1], scores[i, j], text))
    if a.check:
        sys.path.insert(0, REPO)
        from tests import wordpiece_cases as wc
        from triton_client_amd.utils import wordpiece

        vocab = wc.TwinVocab(a.vocab or wordpiece.DEMO_VOCAB)
        want = wc.tokenize_rows(questions, contexts, vocab, a.max_query_length or 64)
        got = [r.as_numpy(n) for n in ("input_ids", "attention_mask", "token_type_ids")] + [offsets, overflow.reshape(-1)]
        for name, g, w in zip(wc.NAMES, got, want):
            if not np.array_equal(g, w):
                print("error: %s differs from the Python twin's" % name)
                sys.exit(1)
    print("PASS")


if __name__ == "__main__":
    main()

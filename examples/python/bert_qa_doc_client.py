#!/usr/bin/env python3
"""A question and a context longer than BERT's 384-token row, as text, through
the `bert_qa_doc_ensemble` ensemble (`bert_window_tokenizer` -> `bert_large` ->
`qa_doc_spans`; ids and logits stay on the device): the context is cut into
overlapping doc-stride windows, every window is one row of a single `bert_large`
batch, and the n best answers of the whole document come back, each with the
window it was found in.  Prints them as text, cut out of the context by the byte
offsets the tokenizer returned.  `bert_large` is served with synthetic weights,
so the answers show the plumbing, not reading comprehension.  `--check` also
asks for the ids and the logits, recomputes the windows with the host twin of
the tokenizer from the same vocabulary file and the answers with the client-side
route (`utils.qa.merge_windows`) over the returned logits, and compares exactly."""
import argparse
import sys

import numpy as np

import tritonclient.grpc as grpcclient
import tritonclient.http as httpclient

QUESTION = "What does the window tokenizer return for every window?"
SENTENCES = ("The tokenizer folds the text, splits it into words and matches pieces greedily. ",
             "A context that does not fit one row is cut into overlapping windows a doc stride apart. ",
             "For every window it returns the ids, a start mask and byte offsets into the whole context. ",
             "A piece that lies in several windows may start an answer only in the window where it has most context. ",
             "The answers of all windows are merged by score, then by where they start in the document. ")
CONTEXT = "".join(SENTENCES[i % len(SENTENCES)] for i in range(60))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-v", "--verbose", action="store_true")
    ap.add_argument("-m", "--model-name", default="bert_qa_doc_ensemble")
    ap.add_argument("-u", "--url", default=None)
    ap.add_argument("-i", "--protocol", default="HTTP", choices=["HTTP", "gRPC", "http", "grpc"])
    ap.add_argument("-q", "--question", action="append", help="repeat for several documents (with as many --context)")
    ap.add_argument("-c", "--context", action="append")
    ap.add_argument("--n-best", type=int, default=None, help="answers per document (server default 20, at most 64)")
    ap.add_argument("--max-answer-length", type=int, default=None, help="tokens (server default 30)")
    ap.add_argument("--max-query-length", type=int, default=None, help="question pieces kept (server default 64)")
    ap.add_argument("--doc-stride", type=int, default=None, help="context pieces between windows (server default 128)")
    ap.add_argument("--max-windows", type=int, default=None, help="windows per document (server default 128)")
    ap.add_argument("--show", type=int, default=5, help="ranks printed per document")
    ap.add_argument("--vocab", default=None, help="the server's vocab.txt, for --check (default: the demonstration one)")
    ap.add_argument("--check", action="store_true", help="recompute windows and answers on the client")
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
        x = mod.InferInput(name, [len(col)], "BYTES")
        x.set_data_from_numpy(np.array(col, dtype=object))
        ins.append(x)
    params = {k: v for k, v in (("n_best", a.n_best), ("max_answer_length", a.max_answer_length),
                                ("max_query_length", a.max_query_length), ("doc_stride", a.doc_stride),
                                ("max_windows", a.max_windows)) if v is not None}
    names = ["spans", "windows", "scores", "null_score", "offsets", "window_info", "doc_info"]
    names += ["input_ids", "attention_mask", "token_type_ids", "start_mask", "start_logits", "end_logits"] if a.check \
        else []
    r = client.infer(a.model_name, ins, outputs=[mod.InferRequestedOutput(n) for n in names], parameters=params or None)
    from triton_client_amd.utils.qa import answer_text_doc, merge_windows

    spans, windows, scores, null = (r.as_numpy(n) for n in ("spans", "windows", "scores", "null_score"))
    offsets, winfo, dinfo = r.as_numpy("offsets"), r.as_numpy("window_info"), r.as_numpy("doc_info")
    for d, ctx in enumerate(contexts):
        print("document %d: %d context pieces in %d windows, null_score %.6f" % (d, dinfo[d, 2], dinfo[d, 1], null[d]))
        print("    rank  window  start  end  score      answer")
        for j in range(min(a.show, spans.shape[1])):
            text = answer_text_doc(ctx, spans[d, j], windows[d, j], offsets).decode("utf-8", "replace")
            print("    %4d  %6d  %5d  %3d  %9.6f  %s" % (j, windows[d, j] - dinfo[d, 0] if windows[d, j] >= 0 else -1,
                                                        spans[d, j, 0], spans[d, j, 1], scores[d, j], text))
    if a.check:
        from triton_client_amd.ops import host_codec
        from triton_client_amd.utils import wordpiece

        vocab = wordpiece.Vocab.load(a.vocab or wordpiece.DEMO_VOCAB)
        want = host_codec.load().wordpiece_windows(questions, contexts, vocab, a.max_query_length or 64,
                                                   a.doc_stride or 128, a.max_windows or 128)
        n = want[7]
        got = [r.as_numpy(x) for x in ("input_ids", "attention_mask", "token_type_ids", "start_mask")] + [offsets, winfo]
        for name, g, w in zip(("input_ids", "attention_mask", "token_type_ids", "start_mask", "offsets", "window_info"),
                              got, want):
            if not np.array_equal(g, w[:n]):
                sys.exit("error: %s differs from the host twin's" % name)
        if not np.array_equal(dinfo, want[6].view(np.int32)):
            sys.exit("error: doc_info differs from the host twin's")
        mine = merge_windows(r.as_numpy("start_logits"), r.as_numpy("end_logits"), got[1], got[2], got[3], winfo, dinfo,
                             a.n_best or 20, a.max_answer_length or 30)
        for name, g, w in zip(("spans", "windows", "scores", "null_score"), (spans, windows, scores, null), mine):
            if g.tobytes() != w.tobytes():
                sys.exit("error: %s differs from the client-side route's" % name)
    print("PASS")


if __name__ == "__main__":
    main()

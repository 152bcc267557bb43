#!/usr/bin/env python3
"""A few texts through the `bert_search_text_ensemble` ensemble (`bert_tokenizer`
-> `bert_large_embed` -> `embed_search`, the ids and the embedding staying on
the device): prints each text's nearest corpus rows and their scores.  Only
`indices` and `scores` are asked for, so the embeddings never leave the server.
Each text goes as `context` with an empty `question` (`[CLS] [SEP] text
[SEP]`).  The server has to be started with the ensemble and its three steps
named in `--models`; the weights and (unless `TCAMD_SEARCH_CORPUS` names one)
the corpus are synthetic, so the numbers show the plumbing, not meaning."""
import argparse

import numpy as np

import tritonclient.grpc as grpcclient
import tritonclient.http as httpclient

TEXTS = ["The tokenizer folds the text and matches pieces greedily.",
         "Pieces are matched greedily after the text is folded.",
         "A HIP graph is captured per batch bucket."]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-v", "--verbose", action="store_true")
    ap.add_argument("-m", "--model-name", default="bert_search_text_ensemble")
    ap.add_argument("-u", "--url", default=None)
    ap.add_argument("-i", "--protocol", default="HTTP", choices=["HTTP", "gRPC", "http", "grpc"])
    ap.add_argument("-t", "--text", action="append", help="repeat for several rows")
    ap.add_argument("-k", "--top-k", type=int, default=None, help="1..64; server default: 10")
    ap.add_argument("--pooling", default=None, choices=["mean", "cls"], help="server default: mean")
    a = ap.parse_args()
    texts = [t.encode("utf-8") for t in (a.text or TEXTS)]
    protocol = a.protocol.lower()
    mod = grpcclient if protocol == "grpc" else httpclient
    client = mod.InferenceServerClient(a.url or ("localhost:8001" if protocol == "grpc" else "localhost:8000"),
                                       verbose=a.verbose)
    ins = []
    for name, col in (("question", [b""] * len(texts)), ("context", texts)):
        x = mod.InferInput(name, [len(col), 1], "BYTES")
        x.set_data_from_numpy(np.array(col, dtype=object).reshape(-1, 1))
        ins.append(x)
    params = {}
    if a.top_k is not None:
        params["top_k"] = a.top_k
    if a.pooling:
        params["pooling"] = a.pooling
    res = client.infer(a.model_name, ins, outputs=[mod.InferRequestedOutput("indices"),
                                                   mod.InferRequestedOutput("scores")], parameters=params or None)
    indices, scores = res.as_numpy("indices"), res.as_numpy("scores")
    if indices.shape != scores.shape or indices.shape[0] != len(texts) or (np.diff(scores, axis=1) > 0).any():
        raise SystemExit("error: unexpected result %s %s" % (indices.shape, scores.shape))
    for text, i, s in zip(texts, indices, scores):
        print(text.decode("utf-8"))
        print("    " + "  ".join("%d:%.5f" % (j, v) for j, v in zip(i, s) if j >= 0))
    print("PASS")


if __name__ == "__main__":
    main()

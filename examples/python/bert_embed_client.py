#!/usr/bin/env python3
"""A few texts through the `bert_embed_text_ensemble` ensemble (`bert_tokenizer`
-> `bert_large_embed`, the ids staying on the device): prints the cosine matrix
of their embeddings.  Each text goes as `context` with an empty `question`
(`[CLS] [SEP] text [SEP]`).  The server has to be started with both models
named in `--models`; `bert_large_embed` is served with synthetic weights, so
the numbers show the plumbing, not meaning."""
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
    ap.add_argument("-m", "--model-name", default="bert_embed_text_ensemble")
    ap.add_argument("-u", "--url", default=None)
    ap.add_argument("-i", "--protocol", default="HTTP", choices=["HTTP", "gRPC", "http", "grpc"])
    ap.add_argument("-t", "--text", action="append", help="repeat for several rows")
    ap.add_argument("--pooling", default=None, choices=["mean", "cls"], help="server default: mean")
    ap.add_argument("--no-normalize", action="store_true", help="the pooled vector as it is, not divided by its norm")
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
    if a.pooling:
        params["pooling"] = a.pooling
    if a.no_normalize:
        params["normalize"] = False
    e = client.infer(a.model_name, ins, parameters=params or None).as_numpy("embedding").astype(np.float64)
    if e.shape != (len(texts), 1024) or not np.isfinite(e).all():
        raise SystemExit("error: unexpected embedding %s" % (e.shape,))
    unit = e / np.maximum(np.linalg.norm(e, axis=1, keepdims=True), 1e-30)
    print("norms  " + "  ".join("%.6f" % n for n in np.linalg.norm(e, axis=1)))
    print("cosine matrix")
    for row in unit @ unit.T:
        print("    " + "  ".join("%8.5f" % c for c in row))
    print("PASS")


if __name__ == "__main__":
    main()

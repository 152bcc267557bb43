#!/usr/bin/env python3
"""Record tests/golden/wordpiece/cases.json: seeded random texts (as hex) and
the ids and byte offsets the ``tokenizers`` library gives them, so that a
machine without the library still checks the tokenizers against its results.

    python tools/make_wordpiece_golden.py [--texts 40] [--seed 2028]

The library side is a ``tokenizers.Tokenizer`` assembled locally from
tests/golden/wordpiece/vocab_small.txt (WordPiece + BertNormalizer +
BertPreTokenizer, nothing downloaded).  A text is written only where the Python
twin of tests/wordpiece_cases.py agrees with the library; the tool reports how
many it left out and fails if that is not zero, since the texts draw from the
blocks on which the two are known to agree.
"""
import argparse
import json
import os
import random
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tests import wordpiece_cases as wc  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--texts", type=int, default=40)
    ap.add_argument("--seed", type=int, default=2028)
    args = ap.parse_args()
    import tokenizers

    tok = wc.library_tokenizer()
    vocab = wc.TwinVocab()
    rng = random.Random(args.seed)
    cases, left_out = [], 0
    for _ in range(args.texts):
        text = wc.random_text(rng, max_items=16)
        lib = wc.library_pieces(tok, text)
        mine, err = wc.tokenize_text(text.encode("utf-8"), vocab)
        if err is not None or [list(p) for p in mine] != lib:
            left_out += 1
            continue
        cases.append({"text": text.encode("utf-8").hex(), "ids": [p[0] for p in lib],
                      "offsets": [[p[1], p[2]] for p in lib]})
    doc = {"tokenizers": tokenizers.__version__, "unicode": wc.table().unicode_version, "seed": args.seed,
           "vocab": "vocab_small.txt", "cases": cases}
    with open(wc.GOLDEN, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print("wrote %s: %d texts, %d left out" % (os.path.relpath(wc.GOLDEN, REPO), len(cases), left_out))
    return 1 if left_out else 0


if __name__ == "__main__":
    sys.exit(main())

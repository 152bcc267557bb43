#!/usr/bin/env python3
"""Build triton_client_amd/data/bert_demo_vocab.txt, the demonstration
vocabulary the ``bert_tokenizer`` model loads when no ``--bert-vocab`` is given.

    python tools/make_wordpiece_vocab.py [--words 1600] [--suffixes 200]

``bert_large`` is served with synthetic weights, so this vocabulary is as
meaningful as any: it exists so that a question and a paragraph in English
become mostly whole-word pieces and nothing becomes ``[UNK]`` for want of a
letter.  It holds the four special pieces, every printable ASCII character as a
first and as a ``##`` piece, and the most frequent lower-cased words and word
endings of this repository's README.md (used three times or more), ties broken
by spelling, so a run over the same file gives the same bytes.  Every id is far below 30522, the
rows of ``bert_large``'s embedding table.  A user with real weights brings the
``vocab.txt`` that belongs to them.
"""
import argparse
import collections
import os
import re
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "triton_client_amd", "data", "bert_demo_vocab.txt")


def markdown_files():
    """The files the words come from: the README, which describes every component in prose."""
    return [os.path.join(REPO, "README.md")]


def build(n_words, n_suffixes):
    words = collections.Counter()
    for path in markdown_files():
        with open(path, encoding="utf-8", errors="replace") as f:
            words.update(re.findall(r"[a-z]+|[0-9]+", f.read().lower()))
    top = [w for w, c in sorted(words.items(), key=lambda kv: (-kv[1], kv[0])) if c >= 3 and 2 <= len(w) <= 24]
    top = top[:n_words]
    known = set(top)
    # endings of the words that stay without a piece of their own, weighted by use
    tails = collections.Counter()
    for w, c in words.items():
        if w in known:
            continue
        for k in (2, 3, 4, 5):
            if len(w) > k + 1:
                tails[w[-k:]] += c
    suffixes = [t for t, c in sorted(tails.items(), key=lambda kv: (-kv[1], kv[0])) if len(t) >= 2 and c >= 3]
    suffixes = suffixes[:n_suffixes]
    ascii_chars = [chr(c) for c in range(33, 127)]
    pieces = ["[PAD]", "[UNK]", "[CLS]", "[SEP]"] + ascii_chars + ["##" + c for c in ascii_chars]
    pieces += top + ["##" + s for s in suffixes]
    seen, out = set(), []
    for p in pieces:
        if p not in seen:
            seen.add(p)
            out.append(p)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--words", type=int, default=1600)
    ap.add_argument("--suffixes", type=int, default=200)
    args = ap.parse_args()
    pieces = build(args.words, args.suffixes)
    text = "\n".join(pieces) + "\n"
    if len(text.encode()) >= 64 * 1024 or len(pieces) >= 30522:
        sys.exit("the demonstration vocabulary must stay under 64 KB and 30522 pieces")
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w", encoding="utf-8") as f:
        f.write(text)
    print("wrote %s: %d pieces, %d bytes" % (os.path.relpath(OUT, REPO), len(pieces), len(text.encode())))
    return 0


if __name__ == "__main__":
    sys.exit(main())

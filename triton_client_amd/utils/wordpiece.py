"""The vocabulary image of the BERT tokenizer and the text staging both
tokenizers share (K28 ``ops.hip.wordpiece_tokenize`` and its host twin
``HostCodec.wordpiece_tokenize``).  The rule and the image's layout are
csrc/kernels/wordpiece_core.h.

``Vocab.load(path)`` reads a ``vocab.txt`` (one piece per line, the id is the
line number) and builds one flat array of 32-bit words: a header, an
open-addressing table keyed on a piece's code points and its continuation bit,
the code points for the confirming compare, the ids of ``[PAD] [UNK] [CLS]
[SEP]`` and the longest piece.  The kernel reads those words after one upload,
the host twin reads them where they are."""

import os

import numpy as np

MAGIC = 0x31565057  # "WPV1"
HEADER_WORDS = 16
EMPTY = 0xFFFFFFFF
HASH_FIRST, HASH_CONT, HASH_PRIME = 2166136261, 0x9E3779B9 ^ 2166136261, 16777619
MAX_PIECES = 1 << 20
MAX_TEXT_BYTES = 65536
SPECIALS = ("[PAD]", "[UNK]", "[CLS]", "[SEP]")
SEQ = 384
MAX_QUERY_LENGTH = 64

# status words (csrc/kernels/wordpiece_core.h): code | field << 8 | byte << 12
ST_OK, ST_INVALID, ST_TOO_LONG, ST_RANGE, ST_PARAM, ST_VOCAB = range(6)
FIELDS = ("question", "context")

DEMO_VOCAB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "data", "bert_demo_vocab.txt")


def piece_hash(cps, cont):
    h = HASH_CONT if cont else HASH_FIRST
    for c in cps:
        h = ((h ^ c) * HASH_PRIME) & 0xFFFFFFFF
    return h


def slot_of(h, slots):
    return (h ^ (h >> 15)) & (slots - 1)


def status_error(status, model="bert_tokenizer"):
    """The message of a non-zero status word, ``None`` for 0."""
    status = int(status)
    code, field, byte = status & 0xFF, FIELDS[(status >> 8) & 1], status >> 12
    if code == ST_OK:
        return None
    if code == ST_INVALID:
        return "%s: %s is not valid UTF-8 at byte %d" % (model, field, byte)
    if code == ST_TOO_LONG:
        return "%s: %s too long" % (model, field)
    if code == ST_PARAM:
        return "%s: max_query_length out of range" % model
    if code == ST_VOCAB:
        return "%s: the vocabulary image is broken" % model
    return "%s: %s lies outside the staged texts or the workspace" % (model, field)


class Vocab:
    """A WordPiece vocabulary: ``pieces`` (the lines), ``image`` (uint32, what
    the tokenizers read), ``pad`` / ``unk`` / ``cls`` / ``sep``, ``longest``
    (code points of the longest piece, without ``##``) and what the loader
    noticed without failing: ``duplicates`` (lines whose piece an earlier line
    has too; the later id wins, as in a dict), ``empty`` (empty lines; they
    keep their ids and never match) and ``unreachable`` (pieces the fold would
    change, an upper-case letter say: no folded text can ever spell them)."""

    def __init__(self, pieces, check_fold=True):
        pieces = list(pieces)
        if not 0 < len(pieces) <= MAX_PIECES:
            raise ValueError("a vocabulary holds 1 to 2^20 pieces, not %d" % len(pieces))
        self.pieces = pieces
        keys, self.duplicates, self.empty = {}, 0, 0
        for i, p in enumerate(pieces):
            cont = p.startswith("##") and len(p) > 2
            cps = tuple(ord(c) for c in (p[2:] if cont else p))
            if not cps:
                self.empty += 1
                continue
            if (cont, cps) in keys:
                self.duplicates += 1
            keys[(cont, cps)] = i
        names = {p: i for i, p in enumerate(pieces)}
        missing = [s for s in SPECIALS if s not in names]
        if missing:
            raise ValueError("the vocabulary lacks %s" % " ".join(missing))
        self.pad, self.unk, self.cls, self.sep = (names[s] for s in SPECIALS)
        self.keys = keys
        self.longest = max((len(k[1]) for k in keys), default=0)
        self.unreachable = self._count_unreachable() if check_fold else None
        self.image = self._build()

    @classmethod
    def load(cls, path, check_fold=True):
        with open(path, "rb") as f:
            raw = f.read()
        try:
            text = raw.decode("utf-8")
        except UnicodeDecodeError as e:
            raise ValueError("%s is not valid UTF-8: %s" % (path, e))
        lines = text.split("\n")
        if lines and lines[-1] == "":
            lines.pop()
        return cls([ln.rstrip("\r") for ln in lines], check_fold=check_fold)

    def _count_unreachable(self):
        from triton_client_amd.ops import host_codec

        codec, memo, n = host_codec.load(), {}, 0
        specials = {(False, tuple(ord(c) for c in s)) for s in SPECIALS}
        for key in self.keys:
            if key in specials:
                continue
            for c in key[1]:
                if c not in memo:
                    f = codec.wordpiece_fold(c) if c <= 0x10FFFF else []
                    memo[c] = len(f) == 1 and not f[0] >> 31 and f[0] & 0x1FFFFF == c
                if not memo[c]:
                    n += 1
                    break
        return n

    def _build(self):
        n = len(self.pieces)
        slots = 16
        while slots < 2 * n:
            slots *= 2
        table = np.full((slots, 4), 0, dtype=np.uint32)
        table[:, 3] = EMPTY
        cps_all, at = [], 0
        for (cont, cps), pid in self.keys.items():
            h = piece_hash(cps, cont)
            i = slot_of(h, slots)
            while table[i, 3] != EMPTY:
                i = (i + 1) & (slots - 1)
            table[i] = (h, at, len(cps) | (0x80000000 if cont else 0), pid)
            cps_all.extend(cps)
            at += len(cps)
        off_slots = HEADER_WORDS
        off_cps = off_slots + slots * 4
        words = off_cps + at
        head = np.zeros(HEADER_WORDS, dtype=np.uint32)
        head[:12] = (MAGIC, n, slots, off_slots, off_cps, at, words, self.pad, self.unk, self.cls, self.sep, self.longest)
        return np.ascontiguousarray(np.concatenate([head, table.reshape(-1), np.asarray(cps_all, dtype=np.uint32)]))

    def describe(self):
        return ("%d pieces, longest %d; %d duplicate, %d empty, %s unreachable by folded text" %
                (len(self.pieces), self.longest, self.duplicates, self.empty,
                 "?" if self.unreachable is None else self.unreachable))


def default_vocab_path():
    """``TCAMD_BERT_VOCAB`` (the server's ``--bert-vocab``), else the
    demonstration vocabulary that ships with the package."""
    return os.environ.get("TCAMD_BERT_VOCAB") or DEMO_VOCAB


def pack_texts(questions, contexts):
    """The texts of a call end to end: ``(buffer uint8, row_table uint32 [rows,
    4])`` with ``{question_off, question_len, context_off, context_len}`` per
    row.  Nothing is checked or decoded here; that is the tokenizer's work."""
    if len(questions) != len(contexts):
        raise ValueError("one context per question")
    table = np.zeros((len(questions), 4), dtype=np.uint32)
    at, parts = 0, []
    for r, (q, c) in enumerate(zip(questions, contexts)):
        for f, s in enumerate((q, c)):
            s = bytes(s)
            table[r, 2 * f], table[r, 2 * f + 1] = at, len(s)
            parts.append(s)
            at += len(s)
    buf = np.frombuffer(b"".join(parts), dtype=np.uint8) if at else np.zeros(0, dtype=np.uint8)
    return buf, table

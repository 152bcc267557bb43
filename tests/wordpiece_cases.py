"""The BERT tokenizer's rule a third time, in plain Python over the generated
fold table (csrc/kernels/wordpiece_table.h), and the cases the host and GPU
tests share.  Nothing here calls the host library or the device: the table is
parsed from the header's text, UTF-8 is decoded by hand, the vocabulary is a
dict.  The rule is written down in csrc/kernels/wordpiece_core.h."""

import os
import random
import re

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE_H = os.path.join(REPO, "csrc", "kernels", "wordpiece_table.h")
VOCAB_SMALL = os.path.join(REPO, "tests", "golden", "wordpiece", "vocab_small.txt")
GOLDEN = os.path.join(REPO, "tests", "golden", "wordpiece", "cases.json")

SEQ = 384
MAX_TEXT = 65536
MAX_WORD = 100
ST_INVALID, ST_TOO_LONG, ST_RANGE, ST_PARAM = 1, 2, 3, 4
SPACE = "space"

# the blocks on which the installed `tokenizers` and the table agree on every assigned code point
LIBRARY_BLOCKS = ((0x0000, 0x024F), (0x0300, 0x036F), (0x0370, 0x03FF), (0x0400, 0x04FF), (0x1E00, 0x1EFF),
                  (0x2000, 0x206F), (0x3000, 0x30FF), (0x4E00, 0x9FFF), (0xAC00, 0xD7A3), (0xFF00, 0xFFEF),
                  (0x1F600, 0x1F64F),
                  (0xF900, 0xFAFF))  # swept too: the ideograph is folded before it is spaced, as the library does


class FoldTable:
    """The four arrays of the header and the Unicode version it records."""

    def __init__(self, path=TABLE_H):
        text = open(path).read()
        self.unicode_version = re.search(r"Unicode version: (\S+)", text).group(1)
        arrays = {}
        for name, body in re.findall(r"(?:const|constexpr) uint\d+_t (\w+)\[\d+\] = \{(.*?)\};", text, re.S):
            arrays[name] = [int(x, 0) for x in body.replace("\n", " ").split(",") if x.strip()]

        def expand(runs):  # (value, count) pairs
            return [v for v, n in zip(runs[::2], runs[1::2]) for _ in range(n)]

        self.stage1, self.stage2 = expand(arrays["kWpStage1Runs"]), expand(arrays["kWpStage2Runs"])
        self.entries, self.ext = arrays["kWpEntries"], arrays["kWpExt"]

    def entry(self, cp):
        return self.entries[self.stage2[self.stage1[cp >> 7] * 128 + (cp & 127)]]

    def fold(self, cp):
        """``SPACE``, or the list of ``(folded code point, word of its own)``; ``[]`` = dropped."""
        e = self.entry(cp)
        if e & (1 << 23):
            return SPACE
        n = (e >> 21) & 3
        if n == 0:
            return []
        if e & (1 << 26):
            s = cp - 0xAC00
            jamo = [0x1100 + s // 588, 0x1161 + (s % 588) // 28, 0x11A7 + s % 28]
            return [(j, False) for j in jamo[:3 if s % 28 else 2]]
        if n == 1:
            return [((cp + (e & 0x1FFFFF)) & 0x1FFFFF, bool(e & (3 << 24)))]
        at = e & 0x1FFFFF
        return [(x & 0x1FFFFF, bool(x & (1 << 24))) for x in self.ext[at:at + n]]

    def classes(self, cp):
        """(is_space, is_cjk, punct bits of the folded code points) for the table tests."""
        e = self.entry(cp)
        f = self.fold(cp)
        if f == SPACE:
            return True, False, []
        n = (e >> 21) & 3
        if n == 1:
            return False, bool(e & (1 << 25)), [bool(e & (1 << 24))]
        return False, False, [iso for _, iso in f]


_TABLE = None


def table():
    global _TABLE
    if _TABLE is None:
        _TABLE = FoldTable()
    return _TABLE


class TwinVocab:
    """vocab.txt as a dict: (continuation, code points) -> id, the later line winning."""

    def __init__(self, path=VOCAB_SMALL):
        lines = open(path, "rb").read().decode("utf-8").split("\n")
        if lines and lines[-1] == "":
            lines.pop()
        self.pieces = [ln.rstrip("\r") for ln in lines]
        self.keys = {}
        for i, p in enumerate(self.pieces):
            cont = p.startswith("##") and len(p) > 2
            cps = tuple(ord(c) for c in (p[2:] if cont else p))
            if cps:
                self.keys[(cont, cps)] = i
        self.longest = max(len(k[1]) for k in self.keys)
        self.pad, self.unk, self.cls, self.sep = (self.pieces.index(s) for s in ("[PAD]", "[UNK]", "[CLS]", "[SEP]"))


def decode_utf8(data):
    """[(code point, first byte, length)], and the byte at which the text stops decoding (or None)."""
    out, i, n = [], 0, len(data)
    while i < n:
        b = data[i]
        if b < 0x80:
            out.append((b, i, 1))
            i += 1
            continue
        if b < 0xC0 or b >= 0xF8:
            return out, i
        ln = 2 if b < 0xE0 else 3 if b < 0xF0 else 4
        if i + ln > n:
            return out, i
        c = b & (0x1F if ln == 2 else 0x0F if ln == 3 else 0x07)
        for k in range(1, ln):
            if data[i + k] & 0xC0 != 0x80:
                return out, i
            c = (c << 6) | (data[i + k] & 0x3F)
        if c < (0x80, 0x800, 0x10000)[ln - 2] or 0xD800 <= c <= 0xDFFF or c > 0x10FFFF:
            return out, i
        out.append((c, i, ln))
        i += ln
    return out, None


def tokenize_text(data, vocab):
    """One text: ``([(id, begin, end)], None)`` or ``(None, invalid byte)``."""
    cps, err = decode_utf8(bytes(data))
    if err is not None:
        return None, err
    tab = table()
    words, cur = [], []  # a word: [(code point, begin, end)]
    for c, at, ln in cps:
        f = tab.fold(c)
        if f == SPACE:
            if cur:
                words.append(cur)
                cur = []
            continue
        for x, own in f:
            if own:
                if cur:
                    words.append(cur)
                    cur = []
                words.append([(x, at, at + ln)])
            else:
                cur.append((x, at, at + ln))
    if cur:
        words.append(cur)
    pieces = []
    for w in words:
        whole = [(vocab.unk, w[0][1], w[-1][2])]
        if len(w) > MAX_WORD:
            pieces += whole
            continue
        got, p = [], 0
        while p < len(w):
            for k in range(min(len(w) - p, vocab.longest), 0, -1):
                pid = vocab.keys.get((p > 0, tuple(x[0] for x in w[p:p + k])))
                if pid is not None:
                    got.append((pid, w[p][1], w[p + k - 1][2]))
                    p += k
                    break
            else:
                got = None
                break
        pieces += got if got is not None else whole
    return pieces, None


def status_word(code, field=0, byte=0):
    return code | (field << 8) | (byte << 12)


def tokenize_rows(questions, contexts, vocab, max_query_length=64, S=SEQ):
    """``(ids, mask, type_ids, offsets, overflow, status)`` as the tokenizers return them."""
    rows = len(questions)
    mq = np.broadcast_to(np.asarray(max_query_length, dtype=np.int64), (rows,))
    ids, mask, tt = (np.zeros((rows, S), dtype=np.int32) for _ in range(3))
    offsets = np.zeros((rows, S, 2), dtype=np.int32)
    overflow, status = np.zeros(rows, dtype=np.int32), np.zeros(rows, dtype=np.uint32)
    for r, (q, c) in enumerate(zip(questions, contexts)):
        if not 1 <= mq[r] <= S - 3:
            status[r] = status_word(ST_PARAM)
            continue
        long = [f for f, s in enumerate((q, c)) if len(s) > MAX_TEXT]
        if long:
            status[r] = status_word(ST_TOO_LONG, long[0])
            continue
        qp, err = tokenize_text(q, vocab)
        if err is not None:
            status[r] = status_word(ST_INVALID, 0, err)
            continue
        cp, err = tokenize_text(c, vocab)
        if err is not None:
            status[r] = status_word(ST_INVALID, 1, err)
            continue
        qp = qp[:mq[r]]
        room = S - 3 - len(qp)
        overflow[r] = max(0, len(cp) - room)
        cp = cp[:room]
        row = [vocab.cls] + [p[0] for p in qp] + [vocab.sep] + [p[0] for p in cp] + [vocab.sep]
        ids[r, :len(row)] = row
        mask[r, :len(row)] = 1
        first = 2 + len(qp)
        tt[r, first:first + len(cp)] = 1  # the last [SEP] is no answer candidate (qa_span_math.h)
        for k, p in enumerate(cp):
            offsets[r, first + k] = p[1:]
    return ids, mask, tt, offsets, overflow, status


# ---- cases ---------------------------------------------------------------------------
def _u(s):
    return s.encode("utf-8")


def fixed_cases(S=SEQ):
    """``[(name, question bytes, context bytes, max_query_length)]``: every branch
    of the rule that does not depend on the kernel's chunking."""
    room = S - 3
    cases = [
        ("plain", _u("What is the answer?"), _u("The quick brown fox jumps over the lazy dog."), 64),
        ("empty both", b"", b"", 64),
        ("empty question", b"", _u("token tokens tokenization"), 64),
        ("all space", _u(" \t\r\n    　"), _u("   "), 64),
        ("dropped only", _u("\u0000�\u0001​‍­\U000f0000͸"), _u("\u007f\u0085"), 64),
        ("word of 100", _u("x" * 100), _u("a " + "x" * 100 + " b " + "y" * 99 + " xy" + "y" * 98), 64),
        ("word of 101", _u("x" * 101), _u("a " + "x" * 101 + " b x" + "y" * 100 + " " + "zz" * 52), 64),
        ("fold to 0 2 3", _u("á̀b"), _u("é 한글 하 가 क़ שּׁ café naïve"), 64),
        ("unknown tail", _u("αβγδ"), _u("αβγσ αβγδ Σσς λόγος"), 64),
        ("cjk run", _u("中国日本語"), _u("abc中国def 豈更一 あかなカタ \U00020000x"), 64),
        ("punct runs", _u("?!...--"), _u("a.b,c;;d 。、「」 [SEP] [CLS] ## ##s #s ¡hola! —… ;·"), 64),
        ("cyrillic emoji", _u("Привет мир"), _u("приветет Ёж \U0001f600\U0001f600\U0001f601 x\U0001f600"), 64),
        ("latin folds", _u("İstanbul ı Ångström"), _u("Straße Ææ Łódź Øø Ǆ ẞ Ａｂ！"), 64),
        ("question exactly max", _u("a " * 5), _u("b"), 5),
        ("question one more", _u("a " * 6), _u("b"), 5),
        ("context fills the row", _u("a a"), _u("b " * (room - 2)), 64),
        ("context overflows by one", _u("a a"), _u("b " * (room - 1)), 64),
        ("context overflows by many", _u("a"), _u("b. " * 500), 64),
        ("max_query_length 1", _u("what is it"), _u("it is the answer"), 1),
        ("max_query_length S-3", _u("a " * (room + 4)), _u("b c"), room),
        ("max_query_length S-3 short", _u("a b"), _u("b " * 400), room),
        ("text of 65536", _u("q"), b"ab " * 21845 + b"c", 64),
        ("text of 65537", _u("q"), b"ab " * 21845 + b"cd", 64),
        ("question of 65537", b"a" * 65537, b"b", 64),
        ("max_query_length 0", b"a", b"b", 0),
        ("max_query_length S-2", b"a", b"b", room + 1),
    ]
    bad = {
        "overlong 2": b"\xc0\xaf", "overlong 3": b"\xe0\x80\xaf", "overlong 4": b"\xf0\x80\x80\xaf",
        "surrogate": b"\xed\xa0\x80", "above 10ffff": b"\xf4\x90\x80\x80", "lead f8": b"\xf8\x88\x80\x80\x80",
        "stray continuation": b"\x80", "truncated 2": b"\xc3", "truncated 3": b"\xe2\x82", "truncated 4": b"\xf0\x9f\x98",
        "lead then ascii": b"\xe2\x82A", "c1": b"\xc1\xbf", "f5": b"\xf5\x80\x80\x80",
    }
    for name, seq in bad.items():
        cases.append(("invalid %s first" % name, b"ok", seq + b" tail", 64))
        cases.append(("invalid %s last" % name, b"ok", _u("head é") + seq, 64))
        cases.append(("invalid %s mid" % name, b"ok", _u("head é中") + seq + _u("é tail"), 64))
        cases.append(("invalid %s question" % name, _u("é") + seq + b"x", seq, 64))
    return cases


_WORDS = ["the", "quick", "tokenization", "jumps", "unaffable", "walked", "reading", "kernel", "devices", "2024",
          "αβγ", "λόγος", "Σσ", "привет", "Мир",
          "한글", "하", "かな", "カタ", "中国", "\U0001f600", "café", "naïve",
          "Straße", "x" * 100, "x" * 101, "Hello", "?", "...", "。"]


def assigned(cp):
    """Assigned in the table's Unicode version: what the table drops is drawn
    only if it is a control, format or private-use character here too, so a
    Python with a later Unicode adds nothing the table calls unassigned."""
    import unicodedata

    cat = unicodedata.category(chr(cp))
    if cat in ("Cn", "Cs"):
        return False
    return table().fold(cp) != [] or cat in ("Cc", "Cf", "Co")


def random_text(rng, blocks=LIBRARY_BLOCKS, max_items=40):
    """Words of the vocabulary's languages, separators and single code points
    drawn from ``blocks``, joined without a plan."""
    out = []
    for _ in range(rng.randrange(max_items + 1)):
        k = rng.random()
        if k < 0.35:
            out.append(rng.choice(_WORDS))
        elif k < 0.6:
            out.append(rng.choice([" ", " ", "  ", "\t", "\n", " ", "　", ""]))
        elif k < 0.75:
            out.append(chr(rng.randrange(0x20, 0x7F)))
        else:
            lo, hi = rng.choice(blocks)
            cp = rng.randrange(lo, hi + 1)
            if assigned(cp):
                out.append(chr(cp))
    return "".join(out)


def random_rows(seed, rows, invalid=0.03, max_items=40):
    """``(questions, contexts, max_query_length per row)``, seeded; a few rows invalid."""
    rng = random.Random(seed)
    qs, cs, mq = [], [], []
    for _ in range(rows):
        q = _u(random_text(rng, max_items=12))
        c = _u(random_text(rng, max_items=max_items))
        if rng.random() < invalid:
            at = rng.randrange(len(c) + 1)
            c = c[:at] + rng.choice([b"\x80", b"\xc3", b"\xed\xa0\x80", b"\xf4\x90\x80\x80", b"\xe2\x82"]) + c[at:]
        qs.append(q)
        cs.append(c)
        mq.append(rng.choice([64, 64, 64, 1, 3, 10, 381]))
    return qs, cs, np.asarray(mq, dtype=np.int32)


NAMES = ("ids", "mask", "type_ids", "offsets", "overflow", "status")


def assert_same(got, want, what=""):
    for name, g, w in zip(NAMES, got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)[0]
            raise AssertionError("%s: %s differs first at %s: got %s, expected %s" %
                                 (what, name, tuple(bad), g[tuple(bad)], w[tuple(bad)]))


# ---- the `tokenizers` library, where it is installed ---------------------------------------
def library_tokenizer(path=VOCAB_SMALL):
    """A ``tokenizers.Tokenizer`` by the rule's own recipe, assembled from the vocabulary file."""
    from tokenizers import Tokenizer, models, normalizers, pre_tokenizers

    pieces = TwinVocab(path).pieces
    tok = Tokenizer(models.WordPiece({p: i for i, p in enumerate(pieces)}, unk_token="[UNK]",
                                     continuing_subword_prefix="##", max_input_chars_per_word=MAX_WORD))
    tok.normalizer = normalizers.BertNormalizer(clean_text=True, handle_chinese_chars=True, strip_accents=True,
                                                lowercase=True)
    tok.pre_tokenizer = pre_tokenizers.BertPreTokenizer()
    return tok


def library_pieces(tok, text):
    """``[[id, begin byte, end byte]]`` of a str, the library's character offsets converted to bytes."""
    enc = tok.encode(text, add_special_tokens=False)
    at = [0]
    for ch in text:
        at.append(at[-1] + len(ch.encode("utf-8")))
    return [[i, at[a], at[b]] for i, (a, b) in zip(enc.ids, enc.offsets)]

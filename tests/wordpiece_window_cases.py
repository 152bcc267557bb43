"""The doc-stride window rule (rule 8 of csrc/kernels/wordpiece_core.h) a third
time, in plain Python and numpy on ``wordpiece_cases.tokenize_text``, and the
cases the host and GPU tests of K28w share.  Nothing here calls the host library
or the device.  Windows are laid out one after the other, and the max-context
window of a piece is found by scoring every window of the document, in exact
integers; wherever the integer scores do not tie, ``windows_of`` asserts that
run_squad's float64 form ``min(l, r) + 0.01 * len`` picks the same window."""

import numpy as np

from tests import wordpiece_cases as wc

ST_WINDOWS = 6
MAX_WINDOWS = 128
NEVER = 0x7FFFFFFF
NAMES = ("ids", "mask", "type_ids", "start_mask", "offsets", "window_info", "doc_info", "n_rows")


def windows_of(P, cap, doc_stride):
    """``(starts, lens, best)``: the windows of ``P`` context pieces in rows
    that hold ``cap`` of them, and per piece its max-context window; ``None``
    when no window can advance (``cap == 0`` and ``P > 0``)."""
    if cap == 0 and P > 0:
        return None
    stride = min(doc_stride, cap)
    starts, lens, at = [], [], 0
    while True:
        ln = min(cap, P - at)
        starts.append(at)
        lens.append(ln)
        if at + ln >= P:
            break
        at += stride
    best = []
    for k in range(P):
        holding = [w for w in range(len(starts)) if starts[w] <= k < starts[w] + lens[w]]
        exact = [100 * min(k - starts[w], starts[w] + lens[w] - 1 - k) + lens[w] for w in holding]
        pick = holding[exact.index(max(exact))]  # ties to the lowest window
        if exact.count(max(exact)) == 1:
            flt = [min(k - starts[w], starts[w] + lens[w] - 1 - k) + 0.01 * lens[w] for w in holding]
            assert holding[flt.index(max(flt))] == pick, (P, cap, doc_stride, k)
        best.append(pick)
    return starts, lens, best


def window_rows(questions, contexts, vocab, max_query_length=64, doc_stride=128, max_windows=128, S=wc.SEQ,
                out_rows=128):
    """What ``HostCodec.wordpiece_windows`` returns, and per good document its
    untruncated context pieces (for the slice checks)."""
    docs = len(questions)
    per = lambda v: np.broadcast_to(np.asarray(v, dtype=np.int64), (docs,))  # noqa: E731
    mq, ds, mw = per(max_query_length), per(doc_stride), per(max_windows)
    ids, mask, tt, sm = (np.zeros((out_rows, S), dtype=np.int32) for _ in range(4))
    offsets = np.zeros((out_rows, S, 2), dtype=np.int32)
    winfo = np.zeros((out_rows, 4), dtype=np.int32)
    dinfo = np.zeros((docs, 4), dtype=np.uint32)
    pieces_of = {}
    asked = 0
    for d, (q, c) in enumerate(zip(questions, contexts)):
        if not 1 <= mq[d] <= S - 3:
            dinfo[d, 3] = wc.status_word(wc.ST_PARAM)
            continue
        long = [f for f, s in enumerate((q, c)) if len(s) > wc.MAX_TEXT]
        if long:
            dinfo[d, 3] = wc.status_word(wc.ST_TOO_LONG, long[0])
            continue
        qp, err = wc.tokenize_text(q, vocab)
        if err is not None:
            dinfo[d, 3] = wc.status_word(wc.ST_INVALID, 0, err)
            continue
        cp, err = wc.tokenize_text(c, vocab)
        if err is not None:
            dinfo[d, 3] = wc.status_word(wc.ST_INVALID, 1, err)
            continue
        if not (1 <= ds[d] <= S - 3 and 1 <= mw[d] <= MAX_WINDOWS):
            dinfo[d, 3] = wc.status_word(wc.ST_PARAM, 2)
            continue
        qp = qp[:mq[d]]
        cap, P = S - 3 - len(qp), len(cp)
        win = windows_of(P, cap, int(ds[d]))
        W = NEVER if win is None else len(win[0])
        dinfo[d, 1], dinfo[d, 2] = W, P
        if W > mw[d]:
            dinfo[d, 3] = ST_WINDOWS
            continue
        base = asked
        asked += W
        if base + W > out_rows:
            dinfo[d, 3] = ST_WINDOWS
            continue
        dinfo[d, 0] = base
        pieces_of[d] = cp
        starts, lens, best = win
        first = 2 + len(qp)
        for w in range(W):
            r = base + w
            part = cp[starts[w]:starts[w] + lens[w]]
            row = [vocab.cls] + [p[0] for p in qp] + [vocab.sep] + [p[0] for p in part] + [vocab.sep]
            ids[r, :len(row)] = row
            mask[r, :len(row)] = 1
            tt[r, first:first + len(part)] = 1
            for j, p in enumerate(part):
                offsets[r, first + j] = p[1:]
                sm[r, first + j] = 1 if best[starts[w] + j] == w else 0
            winfo[r] = (d, starts[w], lens[w], first)
    good = dinfo[:, 3] == 0
    n_rows = int((dinfo[good, 0] + dinfo[good, 1]).max()) if good.any() else 0
    return (ids, mask, tt, sm, offsets, winfo, dinfo, n_rows), pieces_of


def assert_same(got, want, what=""):
    for name, g, w in zip(NAMES, got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape and g.dtype.kind == w.dtype.kind, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)[0]
            raise AssertionError("%s: %s differs first at %s: got %s, expected %s" %
                                 (what, name, tuple(bad), g[tuple(bad)], w[tuple(bad)]))


def assert_properties(out, pieces_of, S):
    """What holds of any output of the rule: rows past n_rows are zero, each
    window's pieces are the matching slice of the untruncated list, and every
    context piece has its start mask set in exactly one window."""
    ids, mask, tt, sm, offsets, winfo, dinfo, n_rows = out
    for a in (ids, mask, tt, sm, offsets, winfo):
        assert not np.asarray(a)[n_rows:].any()
    assert ((sm == 0) | (tt == 1)).all()
    for d, cp in pieces_of.items():
        base, W, P, st = (int(x) for x in dinfo[d])
        assert st == 0 and P == len(cp) and W >= 1
        owners = np.zeros(P, dtype=np.int64)
        covered = np.zeros(P, dtype=bool)
        for r in range(base, base + W):
            doc, start, ln, first = (int(x) for x in winfo[r])
            assert doc == d and tt[r].sum() == ln
            assert [int(x) for x in ids[r, first:first + ln]] == [p[0] for p in cp[start:start + ln]]
            assert [tuple(int(v) for v in x) for x in offsets[r, first:first + ln]] == \
                [p[1:] for p in cp[start:start + ln]]
            owners[start:start + ln] += sm[r, first:first + ln]
            covered[start:start + ln] = True
        assert covered.all() and (owners == 1).all()


# ---- cases ---------------------------------------------------------------------------
def words(n, salt=0):
    """A context of exactly ``n`` pieces of the small vocabulary: single letters
    and digits that are pieces of their own, of varying byte width between."""
    seps = [" ", "  ", "\t", " \n"]
    return "".join("ab"[(i + salt) % 2] + seps[(i * 7 + salt) % 4] for i in range(n)).encode()


def small_cases():
    """``[(name, questions, contexts, mq, doc_stride, max_windows, out_rows)]`` at
    S = 12 with a question of two pieces (cap = 7): every P and stride the rule
    branches on, and the row-capacity and max_windows refusals."""
    q = b"a b"
    cases = []
    for P in (0, 1, 7, 8, 10, 11, 50):
        for stride in (1, 3, 7, 9):
            cases.append(("P %d stride %d" % (P, stride), [q], [words(P)], 9, stride, 128, 128))
    cases.append(("two documents", [q, b"b"], [words(10), words(20, 1)], 9, 3, 128, 128))
    cases.append(("per document parameters", [q, q, q], [words(10), words(10), words(30)], [9, 1, 2], [3, 7, 9],
                  [128, 2, 4], 128))
    # W of words(n) at stride 3, cap 7: 1 for n <= 7, else ceil((n - 7) / 3) + 1
    cases.append(("one below max_windows", [q, q], [words(20), words(5)], 9, 3, [5, 1], 128))   # W = 6 > 5
    cases.append(("exactly max_windows", [q], [words(20)], 9, 3, 6, 128))
    cases.append(("invalid between", [q, q, q], [words(9), b"a \xed\xa0\x80", words(12, 1)], 9, 3, 128, 128))
    cases.append(("bad doc_stride", [q, q], [words(9), words(9)], 9, [0, 10], 128, 128))
    cases.append(("bad max_windows", [q, q, q], [words(9), words(9), words(9)], 9, 3, [0, 129, 128], 128))
    cases.append(("cap 0", [b"a " * 12, b"a " * 12], [words(3), b""], 9, 3, 128, 128))
    cases.append(("small capacity", [q, q, q], [words(10), words(10), words(3)], 9, 3, 128, 3))  # 2 + 2 + 1 rows
    return cases


def capacity_case(total):
    """128 documents whose windows add up to ``total`` rows (128 or 129) at
    S = 12, stride 7: the last document has one window more when ``total`` is 129."""
    q = b"a b"
    cs = [words(3, d) for d in range(127)] + [words(3 if total == 128 else 10)]
    return [q] * 128, cs, 9, 7, 128, 128


def long_context(nbytes, seed):
    """A context of about ``nbytes`` bytes with multi-byte characters, so that
    words and windows cross the kernel's chunk edges (1024 bytes)."""
    import random

    rng = random.Random(seed)
    out, size = [], 0
    while size < nbytes:
        w = rng.choice(["the", "quick", "tokenization", "café", "Straße", "привет", "中国", "한글", "unaffable", "?",
                        "x" * 100])
        out.append(w)
        size += len(w.encode()) + 1
    return " ".join(out).encode()

"""The cross-window merge of K29 ``qa_merge`` in numpy, K27's start mask in
numpy, and the cases the kernels and their host twins are checked on
(tests/test_qa_merge_host.py, tests/test_qa_merge_gpu.py).

The rule (csrc/kernels/qa_span_math.h): document ``d`` owns rows ``first ..
first + W - 1`` (``doc_info[d] = {first, W, P, status}``, no rows unless the
status is 0); rank ``(s, e)`` of row ``r`` starts at document piece
``window_info[r][1] + s - window_info[r][3]``; the document's ``k`` best are the
``k`` largest of the union of its rows' first ``k`` ranks by
``monotone_u32(score) << 32 | (0xFFFFFFFF - (doc_start * 1024 + (e - s)))``, equal
keys to the lower row; a filler rank ends a row's list.  :func:`reference` sorts
the union, which is the contract itself.  ``null_score`` is the row null with
the lowest image (the lowest row among equals), NaN canonical.

A call's outputs live in one int32 buffer, :func:`out_layout`, between guard
words; :func:`expected_buffer` is that buffer as a correct call leaves it when
every word started as ``CANARY``."""

import functools

import numpy as np

from tests import qa_span_cases as qc

CANARY, GUARD = qc.CANARY, qc.GUARD
SPAN = 1024

_SCORE_BITS = np.array([
    0x7FC00000, 0xFFC12345,              # NaNs: canonical, negative with a payload
    0x7F800000, 0xFF800000,              # +inf, -inf
    0x80000000, 0x00000000,              # -0.0, +0.0 tie
    0x3F800000, 0x3F800000, 0x3F800000,  # many equal scores
    0x40000000, 0xBF800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x00000001,
], dtype=np.uint32)


def merge_keys(spans, bits, winfo_row):
    """uint64 keys of one row's ranks, 0 where the rank is a filler."""
    s, e = spans[:, 0].astype(np.int64), spans[:, 1].astype(np.int64)
    doc_start = int(winfo_row[1]) + s - int(winfo_row[3])
    ok = (s >= 0) & (e >= s) & (e - s < SPAN) & (doc_start >= 0) & (doc_start < 65536)
    idx = np.where(ok, doc_start * SPAN + (e - s), 0).astype(np.uint64)
    key = (qc.monotone_u32(bits).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - idx)
    return np.where(ok, key, np.uint64(0))


def make_case(name, seed, S, docs, kmax, scores="random"):
    """``docs`` = [(W, k, fill)]: the windows of each document (0: a document
    refused with a status), its ``k_doc`` and how many of each row's ``k`` ranks
    hold a candidate (``"full"``, ``"some"``, ``"none"``)."""
    rng = np.random.default_rng(seed)
    rows = sum(W for W, _, _ in docs)
    qn = min(2, S - 4)
    first_tok, cap = 2 + qn, S - 3 - qn
    case = {"name": name, "S": S, "rows": rows, "docs": len(docs), "kmax": kmax,
            "spans": np.zeros((max(rows, 1), kmax, 2), np.int32), "scores": np.zeros((max(rows, 1), kmax), np.uint32),
            "null": np.zeros(max(rows, 1), np.uint32), "window_info": np.zeros((max(rows, 1), 4), np.int32),
            "doc_info": np.zeros((len(docs), 4), np.uint32),
            "k_doc": np.array([k for _, k, _ in docs], dtype=np.int32)}
    # what the kernel must not read: ranks past k and rows outside the documents hold a pattern
    case["spans"][:] = 7
    case["scores"][:] = 0x7F800000
    r = 0
    stride = max(1, cap // 2)
    for d, (W, k, fill) in enumerate(docs):
        if W == 0:
            case["doc_info"][d] = (0, 3, 40, 6)  # refused: too many windows
            continue
        case["doc_info"][d] = (r, W, (W - 1) * stride + cap, 0)
        kk = min(max(k, 0), kmax)
        for w in range(W):
            case["window_info"][r] = (d, w * stride, cap, first_tok)
            case["null"][r] = rng.choice(_SCORE_BITS) if scores != "normal" else \
                np.float32(rng.standard_normal()).view(np.uint32)
            n = {"full": kk, "none": 0, "some": int(rng.integers(0, kk + 1))}[fill]
            s0 = rng.integers(first_tok, first_tok + cap, size=3 * n + 8)
            e0 = np.minimum(s0 + rng.integers(0, 30, size=s0.size), first_tok + cap - 1)
            pairs = rng.permutation(np.unique(np.stack([s0, e0], axis=1), axis=0))
            n = min(n, len(pairs))
            sp = pairs[:n].astype(np.int32).reshape(n, 2)
            if scores == "normal":
                bits = rng.standard_normal(n).astype(np.float32).view(np.uint32)
            elif scores == "equal":
                bits = np.full(n, 0x3F800000, np.uint32)
            else:
                bits = rng.choice(_SCORE_BITS, size=n)
            order = np.argsort(merge_keys(sp, bits, case["window_info"][r]), kind="stable")[::-1] if n else []
            case["spans"][r, :kk], case["scores"][r, :kk] = -1, qc.FILLER_BITS
            case["spans"][r, :n], case["scores"][r, :n] = sp[order], bits[order]
            r += 1
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


def reference(case):
    """``(spans, windows, score bits, null bits, written)``: the outputs per
    document and which documents are written at all."""
    D, kmax = case["docs"], case["kmax"]
    spans = np.zeros((D, kmax, 2), np.int32)
    windows = np.zeros((D, kmax), np.int32)
    bits = np.zeros((D, kmax), np.uint32)
    null = np.zeros(D, np.uint32)
    written = np.zeros(D, bool)
    for d in range(D):
        k = min(int(case["k_doc"][d]), kmax)
        if k < 1:
            continue
        written[d] = True
        first, W, _, status = (int(x) for x in case["doc_info"][d])
        if status != 0:
            W = 0
        cand = []
        null[d], best = qc.FILLER_BITS, None
        for r in range(first, first + W):
            img = int(qc.monotone_u32(case["null"][r:r + 1])[0])
            if best is None or img < best:
                best, nb = img, int(case["null"][r])
                null[d] = qc.CANON_NAN if (nb & 0x7FFFFFFF) > 0x7F800000 else nb
            keys = merge_keys(case["spans"][r, :k], case["scores"][r, :k], case["window_info"][r])
            for h in range(k):
                if keys[h] == 0:
                    break
                cand.append((int(keys[h]), -r, h))
        cand.sort(reverse=True)  # the largest key first, equal keys to the lower row
        spans[d, :k], windows[d, :k], bits[d, :k] = -1, -1, qc.FILLER_BITS
        for j, (_, nr, h) in enumerate(cand[:k]):
            b = int(case["scores"][-nr, h])
            spans[d, j], windows[d, j] = case["spans"][-nr, h], -nr
            bits[d, j] = qc.CANON_NAN if (b & 0x7FFFFFFF) > 0x7F800000 else b
    return spans, windows, bits, null, written


def out_layout(docs, kmax):
    """Word offsets of (spans, windows, scores, null_score) in the output buffer and its length."""
    o_spans = GUARD
    o_windows = o_spans + docs * kmax * 2 + GUARD
    o_scores = o_windows + docs * kmax + GUARD
    o_null = o_scores + docs * kmax + GUARD
    return o_spans, o_windows, o_scores, o_null, o_null + docs + GUARD


def expected_buffer(case):
    D, kmax = case["docs"], case["kmax"]
    o_spans, o_windows, o_scores, o_null, total = out_layout(D, kmax)
    buf = np.full(total, CANARY, dtype=np.uint32)
    spans, windows, bits, null, written = reference(case)
    for d in range(D):
        if not written[d]:
            continue
        k = min(int(case["k_doc"][d]), kmax)
        buf[o_spans + d * kmax * 2:o_spans + d * kmax * 2 + 2 * k] = spans[d, :k].reshape(-1).view(np.uint32)
        buf[o_windows + d * kmax:o_windows + d * kmax + k] = windows[d, :k].view(np.uint32)
        buf[o_scores + d * kmax:o_scores + d * kmax + k] = bits[d, :k]
        buf[o_null + d] = null[d]
    return buf.view(np.int32)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> case.  Built once per process; nothing may change a case."""
    out = []
    for S in (8, 384):
        for k in (1, 20, 64):
            docs = [(W, k, fill) for W in (1, 2, 64, 128) for fill in ("full", "some")]
            docs += [(3, k, "none"), (0, k, "full"), (2, 0, "full"), (2, -5, "full")]
            out.append(make_case("S%d_k%d" % (S, k), 2900 + S + k, S, docs, 64 if k > 20 else max(k, 7)))
    out.append(make_case("equal_scores", 2990, 8, [(5, 20, "full"), (128, 64, "full"), (2, 1, "full")], 64,
                         scores="equal"))
    out.append(make_case("normal_scores", 2991, 384, [(4, 20, "full"), (1, 20, "some"), (9, 64, "some")], 64,
                         scores="normal"))
    out.append(make_case("mixed_k", 2992, 8, [(3, 1, "full"), (3, 7, "some"), (3, 100, "full")], 64))
    return {c["name"]: c for c in out}


@functools.lru_cache(maxsize=None)
def expected(name):
    buf = expected_buffer(cases()[name])
    buf.setflags(write=False)
    return buf


# ---- K27 with a start mask ------------------------------------------------------------
MASKED_CASES = ("S1", "S2", "S65", "S257", "S384", "eligible_none", "eligible_holes", "logits_specials", "rows5_kmax7",
                "served_default")


def start_mask_of(case, seed=27):
    """A random start mask for a case of tests/qa_span_cases.py: 0, 1, values above 1 (which count
    as 1) and negative ones (which do not), seeded."""
    rng = np.random.default_rng(seed + case["S"] + case["rows"])
    return rng.choice(np.array([0, 0, 1, 1, 2, -1], dtype=np.int32), size=case["mask"].shape)


def masked_reference(case, ok):
    """``(spans [rows, kmax, 2], score bits [rows, kmax], null bits [rows])`` by a sort of every
    candidate's key; ``fill`` (default 0) where the rule writes nothing."""
    return _masked_reference(case, ok, 0)


def _masked_reference(case, ok, fill):
    rows, kmax, S = case["rows"], case["kmax"], case["S"]
    spans = np.full((rows, kmax, 2), fill, np.uint32).view(np.int32)
    bits = np.full((rows, kmax), fill, np.uint32)
    null = np.full(rows, fill, np.uint32)
    for r in range(rows):
        k = min(int(case["k_row"][r]), kmax)
        if k < 1:
            continue
        start, end = case["start"][r], case["end"][r]
        el = (case["mask"][r] >= 1) & (case["ttype"][r] == 1)
        L = min(max(int(case["len_row"][r]), 0), S)
        s_i, e_i = np.arange(S)[:, None], np.arange(S)[None, :]
        cand = (el & (ok[r] >= 1))[:, None] & el[None, :] & (e_i >= s_i) & (e_i - s_i < L)
        s, e = np.nonzero(cand)
        b = qc.score_bits(start[s], end[e]) if s.size else np.zeros(0, np.uint32)
        key = (qc.monotone_u32(b).astype(np.uint64) << np.uint64(32)) | (
            np.uint64(0xFFFFFFFF) - (s.astype(np.uint64) * np.uint64(S) + e.astype(np.uint64)))
        order = np.argsort(key)[::-1][:k]
        spans[r, :k], bits[r, :k] = -1, qc.FILLER_BITS
        spans[r, :order.size, 0], spans[r, :order.size, 1], bits[r, :order.size] = s[order], e[order], b[order]
        null[r] = qc.score_bits(start[:1], end[:1])[0]
    return spans, bits, null


def masked_expected_buffer(case, ok):
    """The output buffer of tests/qa_span_cases.py ``out_layout`` as a correct masked call leaves it."""
    rows, kmax = case["rows"], case["kmax"]
    o_spans, o_scores, o_null, total = qc.out_layout(rows, kmax)
    buf = np.full(total, CANARY, dtype=np.uint32)
    spans, bits, null = _masked_reference(case, ok, CANARY)
    buf[o_spans:o_spans + rows * kmax * 2] = spans.reshape(-1).view(np.uint32)
    buf[o_scores:o_scores + rows * kmax] = bits.reshape(-1)
    buf[o_null:o_null + rows] = null
    return buf.view(np.int32)

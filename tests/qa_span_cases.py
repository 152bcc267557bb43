"""The answer-span rule of K27 ``qa_spans`` in numpy, and the cases that the
kernel and its host twin are checked on (tests/test_qa_spans_host.py,
tests/test_qa_spans_gpu.py).

The rule (csrc/kernels/qa_span_math.h): token ``t`` of a row is eligible when
``attention_mask[t] >= 1 and token_type_ids[t] == 1``; a candidate is a pair
``(s, e)`` of eligible tokens with ``s <= e`` and ``e - s < L``; its score is
``start[s] + end[e]`` in fp32, a NaN made the canonical 0x7fc00000; candidates
go by their 64-bit key ``monotone_u32(score) << 32 | (0xFFFFFFFF - (s * S + e))``,
largest first, where ``monotone_u32`` maps NaN to 0, folds -0.0 into +0.0 and
otherwise orders the bits as the values.  :func:`row_reference` sorts every key
of a row, which is the contract itself, not an algorithm for it.

A call's outputs live in one int32 buffer, :func:`out_layout`: guard words,
``spans[rows][kmax][2]``, guard words, ``scores[rows][kmax]`` (as bits), guard
words, ``null_score[rows]``, guard words.  :func:`expected_buffer` is that
buffer as a correct call leaves it when every word started as ``CANARY``: the
comparison of the whole buffer checks the answers and that nothing else was
written (ranks past ``k_row[r]``, skipped rows, the guards).
"""

import functools

import numpy as np

CANARY = 0x5A5A5A5A
GUARD = 8  # int32 words
CANON_NAN = 0x7FC00000
FILLER_BITS = 0xFF7FFFFF  # -FLT_MAX
KMAX = 64
MAX_SEQ = 1024


def score_bits(a, b):
    """uint32 bits of the fp32 sum of two fp32 arrays, NaN canonical."""
    with np.errstate(all="ignore"):
        s = np.asarray(a, dtype=np.float32) + np.asarray(b, dtype=np.float32)
    bits = np.atleast_1d(s).view(np.uint32).copy()
    bits[(bits & 0x7FFFFFFF) > 0x7F800000] = CANON_NAN
    return bits


def monotone_u32(bits):
    bits = np.asarray(bits, dtype=np.uint32).copy()
    nan = (bits & 0x7FFFFFFF) > 0x7F800000
    bits[bits == 0x80000000] = 0
    neg = (bits & 0x80000000) != 0
    m = np.where(neg, ~bits, bits | np.uint32(0x80000000)).astype(np.uint32)
    m[nan] = 0
    return m


def row_reference(start, end, mask, ttype, k, L):
    """One row: (spans int32 [k, 2], score bits uint32 [k], null bits) for
    ``k >= 1``; ranks past the candidates are ``(-1, -1)`` / ``FILLER_BITS``."""
    S = start.shape[0]
    ok = (mask >= 1) & (ttype == 1)
    L = min(max(int(L), 0), S)
    s_i, e_i = np.arange(S)[:, None], np.arange(S)[None, :]
    cand = ok[:, None] & ok[None, :] & (e_i >= s_i) & (e_i - s_i < L)
    s, e = np.nonzero(cand)
    bits = score_bits(start[s], end[e]) if s.size else np.zeros(0, np.uint32)
    key = (monotone_u32(bits).astype(np.uint64) << np.uint64(32)) | (
        np.uint64(0xFFFFFFFF) - (s.astype(np.uint64) * np.uint64(S) + e.astype(np.uint64)))
    order = np.argsort(key)[::-1][:k]  # the keys are unique
    spans = np.full((k, 2), -1, dtype=np.int32)
    out_bits = np.full(k, FILLER_BITS, dtype=np.uint32)
    spans[:order.size, 0] = s[order]
    spans[:order.size, 1] = e[order]
    out_bits[:order.size] = bits[order]
    return spans, out_bits, int(score_bits(start[:1], end[:1])[0])


def out_layout(rows, kmax):
    """Word offsets of (spans, scores, null_score) in the output buffer and its length."""
    o_spans = GUARD
    o_scores = o_spans + rows * kmax * 2 + GUARD
    o_null = o_scores + rows * kmax + GUARD
    return o_spans, o_scores, o_null, o_null + rows + GUARD


def expected_buffer(case):
    rows, kmax = case["rows"], case["kmax"]
    o_spans, o_scores, o_null, total = out_layout(rows, kmax)
    buf = np.full(total, CANARY, dtype=np.uint32)
    for r in range(rows):
        k = min(int(case["k_row"][r]), kmax)
        if k < 1:
            continue
        spans, bits, null = row_reference(case["start"][r], case["end"][r], case["mask"][r], case["ttype"][r], k,
                                          case["len_row"][r])
        buf[o_spans + r * kmax * 2:o_spans + r * kmax * 2 + 2 * k] = spans.reshape(-1).view(np.uint32)
        buf[o_scores + r * kmax:o_scores + r * kmax + k] = bits
        buf[o_null + r] = null
    return buf.view(np.int32)


# ---------------------------------------------------------------------------------------------
# rows
# ---------------------------------------------------------------------------------------------
_SPECIAL_BITS = np.array([
    0x7FC00000, 0xFFC12345, 0x7FA00001,  # NaNs: canonical, negative with a payload, signalling
    0x7F800000, 0xFF800000,              # +inf, -inf (their sum is a NaN)
    0x80000000, 0x00000000,              # -0.0, +0.0
    0x00000001, 0x80000001, 0x007FFFFF,  # denormals
    0x7F7FFFFF, 0xFF7FFFFF,              # +-FLT_MAX (the filler's score among them)
    0x3F800000, 0xBF800000,
], dtype=np.uint32)

LOGITS = ("normal", "integers", "equal", "specials")
ELIGIBLE = ("context", "all", "none", "one", "holes", "mask2")


def _logits(rng, S, kind, L):
    if kind == "normal":
        return rng.standard_normal((2, S)).astype(np.float32) * 4
    if kind == "integers":  # many ties
        return rng.integers(-2, 3, size=(2, S)).astype(np.float32)
    if kind == "equal":  # the order is purely (s, e)
        return np.full((2, S), 1.5, dtype=np.float32)
    x = rng.integers(-2, 3, size=(2, S)).astype(np.float32)
    hit = rng.random((2, S)) < 0.3
    x.view(np.uint32)[hit] = rng.choice(_SPECIAL_BITS, size=int(hit.sum()))
    # the edges of a window: its first token, its last one and the first one outside
    Lc = min(max(int(L), 1), S)
    s0 = int(rng.integers(0, S))
    for e, bits in ((s0, 0x80000000), (s0 + Lc - 1, 0x7FC00000), (s0 + Lc, 0x7F800000)):
        if e < S:
            x[1].view(np.uint32)[e] = bits
    x[0].view(np.uint32)[s0] = 0xFF800000 if rng.random() < 0.5 else 0x7F800000
    return x


def _eligibility(rng, S, kind):
    mask, ttype = np.ones(S, dtype=np.int32), np.ones(S, dtype=np.int32)
    if kind == "context":  # question, context, padding
        q = int(rng.integers(0, S // 3 + 1))
        pad = int(rng.integers(0, S // 4 + 1))
        ttype[:q] = 0
        if pad:
            mask[S - pad:] = 0
            ttype[S - pad:] = 0
    elif kind == "none":
        ttype[:] = rng.integers(-1, 3, size=S)
        mask[ttype == 1] = rng.integers(-2, 1, size=int((ttype == 1).sum()))
    elif kind == "one":
        ttype[:] = 0
        ttype[int(rng.integers(0, S))] = 1
    elif kind == "holes":
        mask[:] = rng.integers(0, 2, size=S)
        ttype[:] = rng.integers(0, 3, size=S)
    elif kind == "mask2":  # a mask above 1 counts as 1, a token type above 1 is not the context
        mask[:] = rng.integers(0, 3, size=S)
        ttype[:] = rng.choice(np.array([0, 1, 1, 1, 2], dtype=np.int32), size=S)
    return mask, ttype


def make_case(name, seed, S, rows, ks, lens, logits=LOGITS, eligible=ELIGIBLE, kmax=None):
    """``rows`` rows of ``S`` tokens; row ``r`` takes ``ks[r % len]``, ``lens[r % len]`` and cycles
    through ``logits`` and ``eligible`` (with different periods, so the kinds mix)."""
    rng = np.random.default_rng(seed)
    case = {"name": name, "S": S, "rows": rows,
            "start": np.zeros((rows, S), np.float32), "end": np.zeros((rows, S), np.float32),
            "mask": np.zeros((rows, S), np.int32), "ttype": np.zeros((rows, S), np.int32),
            "k_row": np.array([ks[r % len(ks)] for r in range(rows)], dtype=np.int32),
            "len_row": np.array([lens[r % len(lens)] for r in range(rows)], dtype=np.int32)}
    for r in range(rows):
        x = _logits(rng, S, logits[r % len(logits)], case["len_row"][r])
        case["start"][r], case["end"][r] = x[0], x[1]
        case["mask"][r], case["ttype"][r] = _eligibility(rng, S, eligible[(r // 2) % len(eligible)])
    case["kmax"] = int(kmax) if kmax else max(1, min(KMAX, int(case["k_row"].max())))
    return case


def _size_case(S):
    # every (L, k) of the list in one call: L in 1, 2, S - 1, S and above S; k in 1, 20, 64
    lens = [1, 2, S - 1, S, S + 5]
    combos = [(L, k) for L in lens for k in (1, 20, 64)]
    return make_case("S%d" % S, 1000 + S, S, len(combos), [k for _, k in combos], [L for L, _ in combos],
                     eligible=("context", "all", "holes", "mask2"))


@functools.lru_cache(maxsize=None)
def cases():
    """name -> case.  Built once per process; nothing may change a case."""
    out = [_size_case(S) for S in (1, 2, 63, 64, 65, 255, 256, 257, 384, 1024)]
    # each kind of eligibility against each kind of logits, k above the candidate count
    for i, el in enumerate(ELIGIBLE):
        out.append(make_case("eligible_" + el, 2000 + i, 65, 8, [64, 20, 1], [30, 65, 3, 1], eligible=(el,)))
    for i, lg in enumerate(LOGITS):
        out.append(make_case("logits_" + lg, 2100 + i, 257, 6, [64, 20], [30, 256, 2], logits=(lg,)))
    # 1, 5 and 129 rows: mixed k_row (0 and negative skip the row, above kmax is kmax), mixed len_row
    ks, lens = [20, 0, 64, 3, -1, 100, 1], [30, 39, 0, 1, 100, -4, 7, 38]
    for rows in (1, 5, 129):
        out.append(make_case("rows%d" % rows, 2200 + rows, 39, rows, ks, lens, kmax=64))
    out.append(make_case("rows5_kmax7", 2300, 39, 5, [7, 0, 9, 2, 5], lens, kmax=7))
    out.append(make_case("served_default", 2400, 384, 4, [20], [30], logits=("normal", "integers"),
                         eligible=("context",)))
    for c in out:
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return {c["name"]: c for c in out}


@functools.lru_cache(maxsize=None)
def expected(name):
    buf = expected_buffer(cases()[name])
    buf.setflags(write=False)
    return buf


# (first element's offset in elements, extra elements per row): a packed 16-byte aligned base,
# and a base that is 4-byte but not 16-byte aligned with row strides above S * 4
LAYOUTS = {"packed": (0, 0), "offset_strided": (1, 3)}


def pack(a, layout):
    """``a`` [rows, S] -> (flat array, first element's offset, stride in elements) under a layout;
    the words of the flat array outside the rows hold a pattern nothing should read as data."""
    off, extra = LAYOUTS[layout]
    rows, S = a.shape
    stride = S + extra
    flat = np.full(off + max(rows, 1) * stride + 4, 0x7FC00000 if a.dtype == np.float32 else 1, dtype=np.uint32)
    flat = flat.view(a.dtype)
    for r in range(rows):
        flat[off + r * stride:off + r * stride + S] = a[r]
    return flat, off, stride


def describe_mismatch(case, got):
    """The first differing word of an output buffer, in words of the layout."""
    want = expected(case["name"])
    bad = np.nonzero(np.asarray(got) != want)[0]
    if bad.size == 0:
        return None
    o_spans, o_scores, o_null, total = out_layout(case["rows"], case["kmax"])
    w = int(bad[0])
    where = "guard"
    if o_spans <= w < o_scores - GUARD:
        r, j = divmod((w - o_spans) // 2, case["kmax"])
        where = "spans[row %d][rank %d][%d]" % (r, j, (w - o_spans) % 2)
    elif o_scores <= w < o_null - GUARD:
        r, j = divmod(w - o_scores, case["kmax"])
        where = "scores[row %d][rank %d]" % (r, j)
    elif o_null <= w < total - GUARD:
        where = "null_score[row %d]" % (w - o_null)
    return "%s: %d words differ, first at %s: got 0x%08x, want 0x%08x" % (
        case["name"], bad.size, where, int(got[w]) & 0xFFFFFFFF, int(want[w]) & 0xFFFFFFFF)

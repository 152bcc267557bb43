"""Answer spans from question-answering logits on the client, in numpy: what
a user of ``bert_large`` does with the raw ``start_logits`` / ``end_logits``,
and what ``examples/python/bert_qa_client.py --check`` and ``tools/qa_bench.py``
hold the served ``qa_spans`` answers against.  The rule is the served one
(csrc/kernels/qa_span_math.h): context tokens only, at most
``max_answer_length`` tokens, scores descending, ties to the lower start and
then the lower end, NaN below every number.

For contexts longer than a row, the doc-stride rule of the served
``bert_window_tokenizer`` / ``qa_doc_spans`` (rule 8 of
csrc/kernels/wordpiece_core.h, the merge of csrc/kernels/qa_span_math.h) is here
too: :func:`doc_windows`, :func:`merge_windows` and :func:`answer_text_doc`,
what a client had to do by hand before ``bert_qa_doc_ensemble`` and what
``examples/python/bert_qa_doc_client.py --check`` and ``tools/qa_bench.py
--doc-stride`` hold the served answers against."""

import numpy as np

FILLER_SCORE = np.float32(-3.4028234663852886e38)  # -FLT_MAX


def answer_text(context_bytes, span, offsets):
    """The bytes of the context a span ``(first token, last token)`` covers, by
    the ``offsets`` ``[S, 2]`` that ``bert_tokenizer`` returned for the row:
    ``context[offsets[s, 0]:offsets[e, 1]]``; ``b""`` for the filler span
    ``(-1, -1)``."""
    s, e = int(span[0]), int(span[1])
    if s < 0 or e < 0:
        return b""
    offsets = np.asarray(offsets)
    return bytes(context_bytes)[int(offsets[s, 0]):int(offsets[e, 1])]


def n_best_spans(start, end, attention_mask, token_type_ids, n_best=20, max_answer_length=30, start_mask=None):
    """One row: ``(spans int32 [n_best, 2], scores fp32 [n_best], null_score)``.
    Ranks past the candidates hold ``(-1, -1)`` and ``-FLT_MAX``.  With
    ``start_mask`` a span may start only where it is at least 1."""
    start = np.asarray(start, dtype=np.float32).reshape(-1)
    end = np.asarray(end, dtype=np.float32).reshape(-1)
    S = start.size
    ok = (np.asarray(attention_mask).reshape(-1) >= 1) & (np.asarray(token_type_ids).reshape(-1) == 1)
    ok_start = ok if start_mask is None else ok & (np.asarray(start_mask).reshape(-1) >= 1)
    L = min(max(int(max_answer_length), 0), S)
    s_all, e_all, v_all = [], [], []
    with np.errstate(all="ignore"):
        for d in range(L):  # candidates by length: e = s + d
            s = np.nonzero(ok_start[:S - d] & ok[d:])[0]
            s_all.append(s)
            e_all.append(s + d)
            v_all.append(start[s] + end[s + d])
    s = np.concatenate(s_all) if s_all else np.zeros(0, np.int64)
    e = np.concatenate(e_all) if e_all else np.zeros(0, np.int64)
    v = np.concatenate(v_all) if v_all else np.zeros(0, np.float32)
    nan = np.isnan(v)
    # descending score (-0.0 == +0.0 as values), NaN last, then the lower s * S + e
    order = np.lexsort((s * S + e, np.where(nan, np.float32(0), -v), nan))[:n_best]
    spans = np.full((n_best, 2), -1, dtype=np.int32)
    scores = np.full(n_best, FILLER_SCORE, dtype=np.float32)
    spans[:order.size, 0], spans[:order.size, 1] = s[order], e[order]
    scores[:order.size] = np.where(nan[order], np.float32(np.nan), v[order])
    with np.errstate(all="ignore"):
        null = np.float32(start[0] + end[0])
    return spans, scores, null if not np.isnan(null) else np.float32(np.nan)


def doc_windows(P, qn, doc_stride, S=384):
    """The doc-stride windows of a context of ``P`` pieces behind a question of
    ``qn`` kept pieces, in rows of ``S`` tokens: ``(starts, lens, best)``, the
    first context piece and the pieces of each window, and per piece its
    max-context window, the one in which a span may start there (run_squad's
    ``_check_is_max_context`` in exact integers: the largest ``100 * min(left,
    right) + len``, ties to the lowest window).  ``P == 0`` is one empty window."""
    cap = S - 3 - int(qn)
    if P > cap and cap < 1:
        raise ValueError("doc_windows: the question leaves no room for the context")
    stride = min(int(doc_stride), cap)
    if P > cap and stride < 1:
        raise ValueError("doc_windows: doc_stride must be at least 1")
    W = 1 if P <= cap else -(-(P - cap) // stride) + 1
    starts = np.arange(W, dtype=np.int64) * (stride if W > 1 else 0)
    lens = np.minimum(cap, P - starts)
    k = np.arange(P, dtype=np.int64)[:, None]
    left, right = k - starts[None, :], starts[None, :] + lens[None, :] - 1 - k
    score = np.where((left >= 0) & (right >= 0), 100 * np.minimum(left, right) + lens[None, :], -1)
    best = score.argmax(axis=1) if P else np.zeros(0, dtype=np.int64)  # argmax takes the first of equals
    return starts, lens, best


def answer_text_doc(context_bytes, span, window, offsets):
    """The bytes of the context a document-level answer covers: ``span`` =
    (first token, last token) of row ``window`` of the ``offsets`` ``[W, S, 2]``
    that ``bert_window_tokenizer`` returned (bytes of the whole context);
    ``b""`` for the filler."""
    if int(window) < 0:
        return b""
    return answer_text(context_bytes, span, np.asarray(offsets)[int(window)])


def merge_windows(start, end, attention_mask, token_type_ids, start_mask, window_info, doc_info, n_best=20,
                  max_answer_length=30):
    """The served ``qa_doc_spans`` on the client: per window the ``n_best``
    spans that start on a piece the window owns (``start_mask``), merged per
    document by score, then the lower document start piece, then the shorter
    span.  ``start`` / ``end`` fp32 ``[W, S]``, the three int arrays ``[W, S]``,
    ``window_info`` ``[W, 4]`` and ``doc_info`` ``[D, 4]`` as
    ``bert_window_tokenizer`` returns them.  Returns ``(spans [D, n_best, 2],
    windows [D, n_best], scores [D, n_best], null_score [D])``; ranks past the
    candidates hold ``(-1, -1)``, ``-1`` and ``-FLT_MAX``; ``null_score`` is the
    lowest of the document's windows (NaN if any is)."""
    start, end = np.asarray(start, dtype=np.float32), np.asarray(end, dtype=np.float32)
    window_info, doc_info = np.asarray(window_info), np.asarray(doc_info)
    D = doc_info.shape[0]
    spans = np.full((D, n_best, 2), -1, dtype=np.int32)
    windows = np.full((D, n_best), -1, dtype=np.int32)
    scores = np.full((D, n_best), FILLER_SCORE, dtype=np.float32)
    null = np.full(D, FILLER_SCORE, dtype=np.float32)
    for d in range(D):
        first, W, _, status = (int(x) for x in doc_info[d])
        if status != 0 or W < 1:
            continue
        cand, nulls = [], []
        for r in range(first, first + W):
            sp, sc, nu = n_best_spans(start[r], end[r], attention_mask[r], token_type_ids[r], n_best,
                                      max_answer_length, start_mask[r])
            nulls.append(nu)
            for (s, e), v in zip(sp, sc):
                if s >= 0:
                    cand.append((int(window_info[r, 1]) + int(s) - int(window_info[r, 3]), int(e - s), r, int(s),
                                 int(e), v))
        nulls = np.asarray(nulls, dtype=np.float32)
        null[d] = np.float32(np.nan) if np.isnan(nulls).any() else nulls.min()
        v = np.asarray([c[5] for c in cand], dtype=np.float32)
        nan = np.isnan(v)
        order = np.lexsort(([c[2] for c in cand], [c[1] for c in cand], [c[0] for c in cand],
                            np.where(nan, np.float32(0), -v), nan))[:n_best] if cand else []
        for j, i in enumerate(order):
            spans[d, j], windows[d, j], scores[d, j] = cand[i][3:5], cand[i][2], cand[i][5]
    return spans, windows, scores, null

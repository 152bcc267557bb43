"""Answer spans from question-answering logits on the client, in numpy: what
a user of ``bert_large`` does with the raw ``start_logits`` / ``end_logits``,
and what ``examples/python/bert_qa_client.py --check`` and ``tools/qa_bench.py``
hold the served ``qa_spans`` answers against.  The rule is the served one
(csrc/kernels/qa_span_math.h): context tokens only, at most
``max_answer_length`` tokens, scores descending, ties to the lower start and
then the lower end, NaN below every number."""

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


def n_best_spans(start, end, attention_mask, token_type_ids, n_best=20, max_answer_length=30):
    """One row: ``(spans int32 [n_best, 2], scores fp32 [n_best], null_score)``.
    Ranks past the candidates hold ``(-1, -1)`` and ``-FLT_MAX``."""
    start = np.asarray(start, dtype=np.float32).reshape(-1)
    end = np.asarray(end, dtype=np.float32).reshape(-1)
    S = start.size
    ok = (np.asarray(attention_mask).reshape(-1) >= 1) & (np.asarray(token_type_ids).reshape(-1) == 1)
    L = min(max(int(max_answer_length), 0), S)
    s_all, e_all, v_all = [], [], []
    with np.errstate(all="ignore"):
        for d in range(L):  # candidates by length: e = s + d
            s = np.nonzero(ok[:S - d] & ok[d:])[0]
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

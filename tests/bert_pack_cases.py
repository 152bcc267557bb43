"""The pack plan of the padding-free bert_large forward as a numpy twin of K30
``bert_pack_plan`` (csrc/kernels/bert_pack.hip), and the masks that
tests/test_bert_pack_cases.py and tests/test_bert_pack_gpu.py share.

The rule: a position is valid when its mask is >= 1; the valid positions of a
``[rows, S]`` batch are numbered in row order, positions ascending within a
row (a stable compaction).  ``row_len[r]`` counts row r's valid positions,
``cu`` is their exclusive scan with ``cu[rows] = T``, ``tok_src[t] = r * S + p``
for packed token t (``-1`` for ``T <= t < t_cap``), ``tok_of[r * S + p] = t``
or ``-1``.  With ``T > t_cap`` only the tokens below ``t_cap`` exist in
``tok_src`` and ``tok_of`` while ``row_len`` and ``cu`` keep the true counts."""

import numpy as np

S = 384
# one 12-row batch: every length at which K12v takes another path (empty row,
# one key, a wave's 32 queries -1 / 0 / +1, a 64-key chunk -1 / 0 / +1, two
# chunks -1 / 0 / +1, the full row)
LENGTHS = (0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 384)


def plan_twin(mask, t_cap):
    """(row_len [rows], cu [rows + 1], tok_src [t_cap], tok_of [rows * S]) int32 of an int mask [rows, S]."""
    mask = np.asarray(mask)
    rows, s = mask.shape
    valid = mask >= 1
    row_len = valid.sum(1).astype(np.int32)
    cu = np.concatenate([[0], np.cumsum(row_len)]).astype(np.int32)
    src = np.flatnonzero(valid.reshape(-1)).astype(np.int32)  # ascending: the stable order
    tok_src = np.full(t_cap, -1, np.int32)
    keep = src[:t_cap]
    tok_src[:keep.size] = keep
    tok_of = np.full(rows * s, -1, np.int32)
    tok_of[keep] = np.arange(keep.size, dtype=np.int32)
    return row_len, cu, tok_src, tok_of


def prefix_mask(lengths, s=S):
    m = np.zeros((len(lengths), s), np.int32)
    for r, n in enumerate(lengths):
        m[r, :n] = 1
    return m


def lengths_mask():
    return prefix_mask(LENGTHS)


def holes_mask():
    """Row 0: holes at 0, 63, 64 and S - 1; row 1: a leading pad over the first
    chunk and part of the second; row 2: mask values other than 0 and 1 (2 and
    7 are valid, -3 is not); row 3: one valid position, the last."""
    m = np.ones((4, S), np.int32)
    m[0, [0, 63, 64, S - 1]] = 0
    m[1, :64 + 23] = 0
    m[2, ::3] = 2
    m[2, 1::3] = -3
    m[2, 2::3] = 7
    m[3] = 0
    m[3, S - 1] = 1
    return m


def empty_mask(rows=5):
    return np.zeros((rows, S), np.int32)


def plan_cases():
    """(name, mask, t_cap) of every plan case."""
    lens = lengths_mask()
    total = int((lens >= 1).sum())
    holes = holes_mask()
    return [
        ("lengths", lens, 12 * 128),
        ("holes", holes, 4 * S),
        ("empty", empty_mask(), 5 * 128),
        ("exact", lens, total),           # T == t_cap
        ("overflow", lens, total - 1),    # T == t_cap + 1
        ("one-row", prefix_mask([77]), 128),
        ("s-not-64", prefix_mask([5, 0, 100, 37], s=100), 256),
        ("128-rows", prefix_mask([(7 * r) % 130 for r in range(128)]), 128 * 128),
    ]

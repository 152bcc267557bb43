"""The row sets that tests/test_bert_pack_fp32_gpu.py shares: the padding-free
route of the fp32-parity ``bert_large_fp32`` (K12xv ``attention_f32_packed``,
the fp32 packed embedding LayerNorm, ``BertLargeQA.forward_packed`` in fp32).

K12xv's block is (row, head, 16 * NW queries) with NW = 4 or 8 waves of 16
queries, and it runs ``ceil(len / 64)`` key chunks, so the lengths are every
one at which it takes another path."""

from tests.bert_pack_cases import S, prefix_mask

HEADS = 16
HIDDEN = 1024
# the empty row, one key, a wave's 16 queries -1 / 0 / +1, a chunk and the
# 4-wave block -1 / 0 / +1, the 8-wave block -1 / 0 / +1, an odd tail, the full row
LENGTHS_F32 = (0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 257, 384)
FIVE_F32 = (1, 17, 65, 129, 384)
# (lengths, t_cap, waves of K12xv's plan): rows * heads * 3 >= 256 picks 8 waves
ROW_SETS = {
    "14-rows": (LENGTHS_F32, 14 * 128, 8),
    "5-rows": (FIVE_F32, 5 * 128, 4),
}

assert sum(LENGTHS_F32) == 1521 and sum(FIVE_F32) == 596
assert all(sum(lens) <= t_cap for lens, t_cap, _ in ROW_SETS.values())
assert S == 384


def cu_of(lengths):
    cu = [0]
    for n in lengths:
        cu.append(cu[-1] + n)
    return cu


def lengths_mask_f32():
    return prefix_mask(LENGTHS_F32)

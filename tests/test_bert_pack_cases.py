"""The padding-free bert_large route without a GPU: the invariants of the pack
plan's numpy twin (tests/bert_pack_cases.py), the served model's host-only
graph choice ``BertLarge.packed_bucket``, and ``BertLargeQA.forward_packed`` on
the CPU in fp32 against the padded ``forward``."""

import numpy as np
import pytest

from tests import bert_pack_cases as cases

torch = pytest.importorskip("torch")


@pytest.mark.parametrize("name,mask,t_cap", cases.plan_cases(), ids=[c[0] for c in cases.plan_cases()])
def test_twin_invariants(name, mask, t_cap):
    """tok_src and tok_of are inverse, cu is monotone and ends at T, the order is stable."""
    rows, s = mask.shape
    row_len, cu, tok_src, tok_of = cases.plan_twin(mask, t_cap)
    T = int((mask >= 1).sum())
    assert row_len.tolist() == [(mask[r] >= 1).sum() for r in range(rows)]
    assert cu[0] == 0 and cu[rows] == T and (np.diff(cu) == row_len).all() and (np.diff(cu) >= 0).all()
    n = min(T, t_cap)
    assert (tok_src[:n] >= 0).all() and (tok_src[n:] == -1).all()
    assert (np.diff(tok_src[:n]) > 0).all(), "rows in order, positions ascending"
    assert (tok_of[tok_src[:n]] == np.arange(n)).all()
    placed = np.flatnonzero(tok_of >= 0)
    assert placed.size == n and (tok_src[tok_of[placed]] == placed).all()
    assert (mask.reshape(-1)[placed] >= 1).all()
    for r in range(rows):  # row r's tokens are cu[r] .. cu[r] + row_len[r] - 1
        t = tok_of[r * s:(r + 1) * s]
        t = t[t >= 0]
        assert t.tolist() == list(range(cu[r], min(cu[r] + row_len[r], max(n, cu[r]))))[:t.size]
    if name == "overflow":
        assert T == t_cap + 1 and (tok_of >= 0).sum() == t_cap


def test_packed_bucket_is_monotone_and_never_too_small():
    from triton_client_amd.server.gpu_models import BertLarge

    assert BertLarge.PACKED_FILL == (128, 256)
    for rows in (1, 2, 3, 5, 8, 9, 31, 33, 64, 65, 127, 128):
        b = next(x for x in BertLarge.BUCKETS if x >= rows)
        last = 0
        for tokens in sorted({0, 1, rows, 100 * rows, b * 128 - 1, b * 128, b * 128 + 1, b * 256 - 1, b * 256,
                              min(rows * 384, b * 256)}):
            if tokens > rows * 384:
                continue
            pick = BertLarge.packed_bucket(rows, tokens)
            assert pick is not None, (rows, tokens)
            assert pick[0] == b and pick[1] in BertLarge.PACKED_FILL
            t_cap = pick[0] * pick[1]
            assert t_cap >= tokens and t_cap >= last
            if pick[1] != BertLarge.PACKED_FILL[0]:
                assert tokens > b * BertLarge.PACKED_FILL[0], "a smaller fill would have held them"
            last = t_cap
        if rows * 384 > b * 256:
            assert BertLarge.packed_bucket(rows, b * 256 + 1) is None
            assert BertLarge.packed_bucket(rows, rows * 384) is None
    assert BertLarge.packed_bucket(129, 10) is None  # no bucket holds the rows
    assert BertLarge.packed_bucket(0, 0) is None


@pytest.fixture(scope="module")
def cpu_model():
    from triton_client_amd.models import bert

    m = bert.build(device="cpu", dtype=torch.float32, layers=2)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():  # non-zero biases and LayerNorm parameters
        for p in m.parameters():
            if p.dim() == 1:
                p.add_(torch.randn(p.shape, generator=g) * 0.05)
    return m


@pytest.mark.parametrize("which", ["lengths", "holes", "empty"])
def test_forward_packed_cpu_equals_padded_forward(cpu_model, which):
    """fp32 torch ops on both sides, differing only in the summation order over
    at most 384 keys: 1e-4 relative at the valid positions (the largest
    difference against the largest logit, and rel-L2); PAD_LOGIT at every other
    one.  Ids and types out of range, as a load generator sends them."""
    from triton_client_amd.models import bert

    mask = {"lengths": cases.lengths_mask(), "holes": cases.holes_mask(), "empty": cases.empty_mask(3)}[which]
    rows = mask.shape[0]
    g = torch.Generator().manual_seed(rows)
    ids = torch.randint(-50, 2 * bert.VOCAB, (rows, cases.S), generator=g, dtype=torch.int32)
    tt = torch.randint(-1, 4, (rows, cases.S), generator=g, dtype=torch.int32)
    m = torch.from_numpy(mask)
    T = int((mask >= 1).sum())
    with torch.no_grad():
        want = cpu_model(ids.long().remainder(bert.VOCAB), m.clamp(0, 1), tt.long().clamp(0, 1))
        got = cpu_model.forward_packed(ids, m, tt, T + 5)
        exact = cpu_model.forward_packed(ids, m, tt, T) if T else got
    valid = m >= 1
    for g_, e_, w_ in zip(got, exact, want):
        assert g_.dtype == torch.float32 and g_.shape == (rows, cases.S)
        assert (g_[~valid] == bert.PAD_LOGIT).all()
        assert torch.equal(g_, e_), "t_cap changes nothing"
        if T:
            d, w = g_[valid] - w_[valid], w_[valid]
            rel_max, rel_l2 = (d.abs().max() / w.abs().max()).item(), (d.norm() / w.norm()).item()
            print("[bert-pack] cpu %s: max|diff|/max|ref|=%.3g rel-L2=%.3g" % (which, rel_max, rel_l2))
            assert rel_max < 1e-4 and rel_l2 < 1e-4, (rel_max, rel_l2)
    if T:
        with pytest.raises(ValueError):
            cpu_model.forward_packed(ids, m, tt, T - 1)


def test_pad_logit_is_one_constant():
    from triton_client_amd.models import bert
    from triton_client_amd.ops import hip

    assert bert.PAD_LOGIT == hip.BERT_PAD_LOGIT == hip.lib().tcamd_bert_pad_logit() == -10000.0

"""The host twins of K29 ``qa_merge`` (csrc/host/qa_merge.cc) and of K27 with a
start mask (csrc/host/qa_spans.cc tcamd_host_qa_spans_masked) against the numpy
rule of tests/qa_merge_cases.py, bit for bit, and the client's
``utils.qa.merge_windows`` against the two chained."""

import numpy as np
import pytest

from tests import qa_merge_cases as mc
from tests import qa_span_cases as qc


@pytest.fixture(scope="module")
def codec():
    from triton_client_amd.ops import host_codec

    return host_codec.load()


@pytest.mark.parametrize("name", sorted(mc.cases()))
def test_qa_merge_is_a_sort_of_the_union(codec, name):
    c = mc.cases()[name]
    rows = c["rows"]
    got = codec.qa_merge(c["spans"][:rows], c["scores"][:rows].view(np.float32), c["null"][:rows].view(np.float32),
                         c["window_info"][:rows], c["doc_info"], c["k_doc"], c["kmax"])
    spans, windows, bits, null, written = mc.reference(c)
    np.testing.assert_array_equal(got[0], spans)
    np.testing.assert_array_equal(got[1], windows)
    np.testing.assert_array_equal(got[2].view(np.uint32), bits)
    np.testing.assert_array_equal(got[3].view(np.uint32), null)
    assert written.sum() == (c["k_doc"] >= 1).sum()


def test_the_cases_cover_what_they_should():
    c = mc.cases()["equal_scores"]
    spans, windows, bits, _, _ = mc.reference(c)
    assert len(set(windows[1, :64].tolist())) > 2  # one score everywhere: the ranks come from many windows
    c = mc.cases()["S8_k20"]
    spans, windows, bits, null, written = mc.reference(c)
    assert (bits == qc.CANON_NAN).any() and (bits == 0x7F800000).any() and (null == qc.CANON_NAN).any()
    assert (windows[8, :20] == -1).all() and not written[10] and (windows[9, :20] == -1).all()
    assert ((windows[:8, :20] == -1).sum(axis=1) > 0).any()  # lists with fewer than k candidates


def test_what_the_entry_refuses(codec):
    c = mc.cases()["mixed_k"]
    rows = c["rows"]
    args = [c["spans"][:rows], c["scores"][:rows].view(np.float32), c["null"][:rows].view(np.float32),
            c["window_info"][:rows], c["doc_info"], c["k_doc"]]
    with pytest.raises(ValueError):
        codec.qa_merge(*args, kmax=65)
    with pytest.raises(ValueError):
        codec.qa_merge(*args[:4], c["doc_info"][:, :3], c["k_doc"])
    # rows that lie outside the lists are no rows: the document is all filler
    far = c["doc_info"].copy()
    far[0, 0] = rows - 1
    got = codec.qa_merge(*args[:4], far, c["k_doc"], c["kmax"])
    assert (got[1][0, :1] == -1).all() and got[3].view(np.uint32)[0] == qc.FILLER_BITS


# ---- K27 with a start mask ------------------------------------------------------------
@pytest.mark.parametrize("name", mc.MASKED_CASES)
def test_qa_spans_masked_with_all_ones_is_qa_spans(codec, name):
    c = qc.cases()[name]
    args = (c["start"], c["end"], c["mask"], c["ttype"])
    want = codec.qa_spans(*args, c["k_row"], c["len_row"], c["kmax"])
    got = codec.qa_spans_masked(*args, np.ones_like(c["mask"]), c["k_row"], c["len_row"], c["kmax"])
    for g, w in zip(got, want):
        assert g.tobytes() == w.tobytes()


@pytest.mark.parametrize("name", mc.MASKED_CASES)
def test_qa_spans_masked_is_the_rule(codec, name):
    c = qc.cases()[name]
    ok = mc.start_mask_of(c)
    spans, scores, null = codec.qa_spans_masked(c["start"], c["end"], c["mask"], c["ttype"], ok, c["k_row"],
                                                c["len_row"], c["kmax"])
    w_spans, w_bits, w_null = mc.masked_reference(c, ok)
    np.testing.assert_array_equal(spans, w_spans)
    np.testing.assert_array_equal(scores.view(np.uint32), w_bits)
    np.testing.assert_array_equal(null.view(np.uint32), w_null)


# ---- the client's route ---------------------------------------------------------------
def test_merge_windows_of_the_client_is_the_two_twins_chained(codec):
    from triton_client_amd.utils.qa import doc_windows, merge_windows

    rng = np.random.default_rng(29)
    S, qn, stride, n_best, L = 24, 3, 5, 20, 6
    rows, winfo, dinfo, sm = [], [], [], []
    for d, P in enumerate((40, 9, 0, 18)):
        starts, lens, best = doc_windows(P, qn, stride, S)
        dinfo.append((len(rows), len(starts), P, 0))
        for w, (st, ln) in enumerate(zip(starts, lens)):
            m = np.zeros(S, np.int32)
            m[2 + qn:2 + qn + ln] = best[st:st + ln] == w
            sm.append(m)
            winfo.append((d, st, ln, 2 + qn))
            rows.append(ln)
    dinfo.append((0, 0, 0, 6))  # a refused document
    W = len(rows)
    tt = np.zeros((W, S), np.int32)
    for r, ln in enumerate(rows):
        tt[r, 2 + qn:2 + qn + ln] = 1
    mask = (np.arange(S)[None, :] < (np.asarray(rows)[:, None] + 3 + qn)).astype(np.int32)
    start = rng.integers(-3, 4, size=(W, S)).astype(np.float32)  # many ties, within and across windows
    end = rng.integers(-3, 4, size=(W, S)).astype(np.float32)
    start[1, 7] = np.nan
    sm, winfo, dinfo = np.asarray(sm), np.asarray(winfo, np.int32), np.asarray(dinfo, np.uint32)
    k_row = np.full(W, n_best, np.int32)
    lists = codec.qa_spans_masked(start, end, mask, tt, sm, k_row, np.full(W, L, np.int32), n_best)
    want = codec.qa_merge(*lists, winfo, dinfo, np.full(len(dinfo), n_best, np.int32), n_best)
    got = merge_windows(start, end, mask, tt, sm, winfo, dinfo, n_best, L)
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    assert got[2].tobytes() == want[2].tobytes() and got[3].tobytes() == want[3].tobytes()
    assert (want[1][2] == -1).all() and (want[1][4] == -1).all()  # P == 0 and the refused document: no answer

"""The answer-span rule on the CPU: the host twin of K27 (csrc/host/qa_spans.cc,
``HostCodec.qa_spans``) and the client-side numpy routine (utils/qa.py) against
the numpy twin of tests/qa_span_cases.py, exact equality of every span and every
score bit; what the entry refuses; and the CPU ``qa_spans`` model in the
in-process server over HTTP and gRPC."""

import numpy as np
import pytest

from tests import qa_span_cases as qc
from triton_client_amd.ops import host_codec


@pytest.fixture(scope="module")
def hc():
    return host_codec.load()


def _call(case, layout, fn, **change):
    """One raw call on host memory; ``change`` replaces arguments by name.  Returns the output buffer."""
    st, off, stride = qc.pack(case["start"], layout)
    en, _, _ = qc.pack(case["end"], layout)
    mk, ioff, istride = qc.pack(case["mask"], layout)
    tt, _, _ = qc.pack(case["ttype"], layout)
    rows, kmax = case["rows"], case["kmax"]
    o_spans, o_scores, o_null, total = qc.out_layout(rows, kmax)
    out = np.full(total, qc.CANARY, dtype=np.uint32).view(np.int32)
    k_row, len_row = case["k_row"].copy(), case["len_row"].copy()
    args = dict(start=st.ctypes.data + 4 * off, end=en.ctypes.data + 4 * off, logit_stride=stride * 4,
                mask=mk.ctypes.data + 4 * ioff, ttype=tt.ctypes.data + 4 * ioff, ids_stride=istride * 4, rows=rows,
                S=case["S"], k_row=k_row.ctypes.data, len_row=len_row.ctypes.data, kmax=kmax,
                spans=out.ctypes.data + 4 * o_spans, scores=out.ctypes.data + 4 * o_scores,
                null_score=out.ctypes.data + 4 * o_null)
    for name, v in change.items():
        args[name] = v(args[name]) if callable(v) else v
    fn(*args.values())
    return out


@pytest.mark.parametrize("layout", sorted(qc.LAYOUTS))
@pytest.mark.parametrize("name", sorted(qc.cases()))
def test_host_twin_equals_the_numpy_twin(hc, name, layout):
    case = qc.cases()[name]
    got = _call(case, layout, hc.qa_spans_raw)
    assert qc.describe_mismatch(case, got) is None


def test_the_cases_cover_what_they_claim():
    cs = qc.cases()
    assert {c["S"] for c in cs.values()} >= {1, 2, 63, 64, 65, 255, 256, 257, 384, 1024}
    assert {c["rows"] for c in cs.values()} >= {1, 5, 129}
    c = cs["S65"]
    assert set(c["len_row"]) == {1, 2, 64, 65, 70} and set(c["k_row"]) == {1, 20, 64}
    ok = (cs["eligible_none"]["mask"] >= 1) & (cs["eligible_none"]["ttype"] == 1)
    assert not ok.any()
    ok = (cs["eligible_one"]["mask"] >= 1) & (cs["eligible_one"]["ttype"] == 1)
    assert (ok.sum(axis=1) == 1).all()
    assert (cs["eligible_mask2"]["mask"] == 2).any() and (cs["eligible_mask2"]["ttype"] == 2).any()
    assert np.isnan(cs["logits_specials"]["end"]).any() and np.isinf(cs["logits_specials"]["start"]).any()
    # filler: a row with fewer candidates than answers; skipped rows: k_row 0 and below
    want = qc.expected("eligible_one")
    o_spans, _, _, _ = qc.out_layout(8, 64)
    assert (want[o_spans:o_spans + 4] == [want[o_spans], want[o_spans], -1, -1]).all()
    assert (cs["rows129"]["k_row"] <= 0).any() and (cs["rows129"]["k_row"] > 64).any()
    assert (cs["rows129"]["len_row"] <= 0).any() and (cs["rows129"]["len_row"] > 39).any()


def test_inf_minus_inf_is_a_canonical_nan_below_every_number():
    S = 4
    start = np.array([[np.inf, 1.0, -np.inf, 0.0]], np.float32)
    end = np.array([[-np.inf, 2.0, np.inf, -0.0]], np.float32)
    one = np.ones((1, S), np.int32)
    spans, bits, null = qc.row_reference(start[0], end[0], one[0], one[0], 10, 1)
    # L = 1: (1,1) = 3.0, (3,3) = 0.0, then the NaNs (0,0) and (2,2) in index order
    assert spans[:4].tolist() == [[1, 1], [3, 3], [0, 0], [2, 2]] and spans[4:].tolist() == [[-1, -1]] * 6
    assert bits[2] == bits[3] == null == qc.CANON_NAN and bits[4] == qc.FILLER_BITS


def test_binding_returns_the_same_arrays(hc):
    case = qc.cases()["rows5_kmax7"]
    spans, scores, null = hc.qa_spans(case["start"], case["end"], case["mask"], case["ttype"], case["k_row"],
                                      case["len_row"], kmax=7)
    o_spans, o_scores, o_null, _ = qc.out_layout(5, 7)
    want = qc.expected("rows5_kmax7").copy()
    want[want == np.int32(qc.CANARY)] = 0  # the binding hands out zeroed arrays: unwritten slots are 0
    np.testing.assert_array_equal(spans.reshape(-1), want[o_spans:o_spans + 70])
    np.testing.assert_array_equal(scores.view(np.int32).reshape(-1), want[o_scores:o_scores + 35])
    np.testing.assert_array_equal(null.view(np.int32), want[o_null:o_null + 5])
    empty = hc.qa_spans(np.zeros((0, 9), np.float32), np.zeros((0, 9), np.float32), np.zeros((0, 9), np.int32),
                        np.zeros((0, 9), np.int32), [], [])
    assert [a.shape for a in empty] == [(0, 1, 2), (0, 1), (0,)]
    with pytest.raises(ValueError, match="one shape"):
        hc.qa_spans(case["start"], case["end"][:, :5], case["mask"], case["ttype"], case["k_row"], case["len_row"])


BAD = {
    "S_zero": dict(S=0), "S_above_1024": dict(S=1025), "kmax_zero": dict(kmax=0), "kmax_above_64": dict(kmax=65),
    "rows_negative": dict(rows=-1),
    "logit_stride_odd": dict(logit_stride=lambda v: v + 2), "logit_stride_short": dict(logit_stride=4 * 38),
    "ids_stride_odd": dict(ids_stride=lambda v: v + 1), "ids_stride_short": dict(ids_stride=0),
}
for _p in ("start", "end", "mask", "ttype", "k_row", "len_row", "spans", "scores", "null_score"):
    BAD[_p + "_null"] = {_p: None}
    BAD[_p + "_misaligned"] = {_p: lambda v: v + 2}


@pytest.mark.parametrize("what", sorted(BAD))
def test_host_entry_refuses(hc, what):
    with pytest.raises(ValueError, match="refuses"):
        _call(qc.cases()["rows5_kmax7"], "packed", hc.qa_spans_raw, **BAD[what])


def test_refused_calls_leave_the_canaries(hc):
    case = qc.cases()["rows5_kmax7"]
    for what, change in sorted(BAD.items()):
        if any(k in change for k in ("spans", "scores", "null_score")):
            continue  # the buffer's address itself is the bad argument
        refused = []

        def fn(*a):
            try:
                hc.qa_spans_raw(*a)
            except ValueError:
                refused.append(what)

        out = _call(case, "packed", fn, **change)
        assert refused, what
        assert (out == np.int32(qc.CANARY)).all(), what


def test_zero_rows_is_success_and_writes_nothing(hc):
    out = _call(qc.cases()["rows5_kmax7"], "packed", hc.qa_spans_raw, rows=0)
    assert (out == np.int32(qc.CANARY)).all()


@pytest.mark.parametrize("name", ["S65", "logits_specials", "logits_integers", "logits_equal", "eligible_holes",
                                  "rows5_kmax7", "served_default"])
def test_client_side_numpy_routine_equals_the_twin(name):
    from triton_client_amd.utils import qa

    case = qc.cases()[name]
    for r in range(case["rows"]):
        k = min(int(case["k_row"][r]), case["kmax"])
        if k < 1:
            continue
        want = qc.row_reference(case["start"][r], case["end"][r], case["mask"][r], case["ttype"][r], k,
                                case["len_row"][r])
        spans, scores, null = qa.n_best_spans(case["start"][r], case["end"][r], case["mask"][r], case["ttype"][r], k,
                                              case["len_row"][r])
        np.testing.assert_array_equal(spans, want[0])
        np.testing.assert_array_equal(scores.view(np.uint32), want[1])
        assert np.array([null], np.float32).view(np.uint32)[0] == want[2]


# ---------------------------------------------------------------------------------------------
# the CPU model, served
# ---------------------------------------------------------------------------------------------
def _served_rows(n, seed):
    case = qc.make_case("served", seed, 384, n, [1], [1], logits=("integers", "normal"), eligible=("context",))
    return [case[k] for k in ("start", "end", "mask", "ttype")]


def _want(rows, k, L):
    per = [qc.row_reference(*(a[r] for a in rows), k, L) for r in range(rows[0].shape[0])]
    return (np.stack([p[0] for p in per]), np.stack([p[1] for p in per]),
            np.array([p[2] for p in per], np.uint32).reshape(-1, 1))


def _client(cpu_server, kind):
    if kind == "http":
        import tritonclient.http as mod

        return mod, mod.InferenceServerClient(cpu_server.http_url)
    import tritonclient.grpc as mod

    return mod, mod.InferenceServerClient(cpu_server.grpc_url)


def _inputs(mod, rows):
    names = ("start_logits", "end_logits", "attention_mask", "token_type_ids")
    ins = []
    for nm, a in zip(names, rows):
        i = mod.InferInput(nm, list(a.shape), "FP32" if a.dtype == np.float32 else "INT32")
        i.set_data_from_numpy(np.ascontiguousarray(a))
        ins.append(i)
    return ins


def _check_response(r, rows, k, L):
    spans, bits, null = _want(rows, k, L)
    np.testing.assert_array_equal(r.as_numpy("spans"), spans)
    np.testing.assert_array_equal(r.as_numpy("scores").view(np.uint32), bits)
    np.testing.assert_array_equal(r.as_numpy("null_score").view(np.uint32), null)


@pytest.mark.parametrize("kind", ["http", "grpc"])
def test_cpu_model_served_with_defaults_and_both_parameters(cpu_server, kind):
    mod, c = _client(cpu_server, kind)
    rows = _served_rows(3, 11)
    _check_response(c.infer("qa_spans", _inputs(mod, rows)), rows, 20, 30)
    _check_response(c.infer("qa_spans", _inputs(mod, rows), parameters={"n_best": 64}), rows, 64, 30)
    _check_response(c.infer("qa_spans", _inputs(mod, rows), parameters={"max_answer_length": 1}), rows, 20, 1)
    _check_response(c.infer("qa_spans", _inputs(mod, rows), parameters={"n_best": 3, "max_answer_length": 384}),
                    rows, 3, 384)
    r = c.infer("qa_spans", _inputs(mod, rows), outputs=[mod.InferRequestedOutput("spans")])
    assert r.as_numpy("scores") is None and r.as_numpy("spans").shape == (3, 20, 2)
    md = c.get_model_metadata("qa_spans") if kind == "http" else c.get_model_metadata("qa_spans", as_json=True)
    assert [o["name"] for o in md["outputs"]] == ["spans", "scores", "null_score"]


@pytest.mark.parametrize("kind", ["http", "grpc"])
@pytest.mark.parametrize("params,message", [
    ({"n_best": 0}, "request parameter n_best must be an int64 in [1, 64], not 0"),
    ({"n_best": 65}, "request parameter n_best must be an int64 in [1, 64], not 65"),
    ({"n_best": "20"}, "request parameter n_best must be an int64 in [1, 64], not '20'"),
    ({"n_best": True}, "request parameter n_best must be an int64 in [1, 64], not True"),
    ({"max_answer_length": 0}, "request parameter max_answer_length must be an int64 in [1, 384], not 0"),
    ({"max_answer_length": 385}, "request parameter max_answer_length must be an int64 in [1, 384], not 385"),
    ({"max_answer_length": "x"}, "request parameter max_answer_length must be an int64 in [1, 384], not 'x'"),
], ids=lambda v: "-".join("%s=%r" % kv for kv in v.items()) if isinstance(v, dict) else None)
def test_cpu_model_parameter_errors_name_the_parameter_and_the_range(cpu_server, kind, params, message):
    from tritonclient.utils import InferenceServerException

    mod, c = _client(cpu_server, kind)
    with pytest.raises(InferenceServerException) as e:
        c.infer("qa_spans", _inputs(mod, _served_rows(1, 12)), parameters=params)
    assert message in str(e.value)


def test_mixed_n_best_share_a_batch_and_one_call_and_an_error_fails_alone(hc, monkeypatch):
    from triton_client_amd.server.cpu_models import QaSpans
    from triton_client_amd.server.types import InferRequest, InputTensor, ServerError

    m = QaSpans()
    m.load()
    calls = []
    real = hc.qa_spans_raw
    monkeypatch.setattr(hc, "qa_spans_raw", lambda *a: (calls.append(a[6]), real(*a))[1])
    names = ("start_logits", "end_logits", "attention_mask", "token_type_ids")
    reqs, rowsets, params = [], [], [{"n_best": 1}, {}, {"n_best": 65}, {"n_best": 64, "max_answer_length": 5}]
    for i, p in enumerate(params):
        rows = _served_rows(i + 1, 20 + i)
        rowsets.append(rows)
        reqs.append(InferRequest(model_name="qa_spans", parameters=p, inputs=[
            InputTensor(nm, "FP32" if a.dtype == np.float32 else "INT32", list(a.shape), a)
            for nm, a in zip(names, rows)]))
    res = m.execute(reqs)
    assert calls == [1 + 2 + 4]  # the three good requests' rows, one call
    assert isinstance(res[2], ServerError) and "n_best" in res[2].msg
    for i, (k, L) in {0: (1, 30), 1: (20, 30), 3: (64, 5)}.items():
        spans, bits, null = _want(rowsets[i], k, L)
        got = {o.name: o.data for o in res[i]}
        np.testing.assert_array_equal(got["spans"], spans)
        np.testing.assert_array_equal(got["scores"].view(np.uint32), bits)
        np.testing.assert_array_equal(got["null_score"].view(np.uint32), null)

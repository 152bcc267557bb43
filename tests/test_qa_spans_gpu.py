"""K27 qa_spans (csrc/kernels/qa_spans.hip) against the numpy twin of
tests/qa_span_cases.py, exact equality of every span and every score bit, with
canaries around, between and behind everything it writes; what the entry
refuses; the GPU ``qa_spans`` model against the CPU one; and
``bert_qa_ensemble`` served in process on a 2-layer ``bert_large``."""

import numpy as np
import pytest

from tests import qa_span_cases as qc
from tests.test_examples import run_example

pytestmark = pytest.mark.gpu

NAMES = ("start_logits", "end_logits", "attention_mask", "token_type_ids")


@pytest.fixture(scope="module")
def torch():
    import torch

    torch.cuda.set_device(0)
    return torch


def _call(torch, case, layout, **change):
    """One ``hip.qa_spans`` call on the null stream; ``change`` replaces arguments by name.
    Returns the output buffer, guards included, as int32."""
    from triton_client_amd.ops import hip

    keep = []

    def up(a):
        t = torch.from_numpy(np.array(a)).cuda()
        keep.append(t)
        return t.data_ptr()

    st, off, stride = qc.pack(case["start"], layout)
    en, _, _ = qc.pack(case["end"], layout)
    mk, ioff, istride = qc.pack(case["mask"], layout)
    tt, _, _ = qc.pack(case["ttype"], layout)
    rows, kmax = case["rows"], case["kmax"]
    o_spans, o_scores, o_null, total = qc.out_layout(rows, kmax)
    out = torch.from_numpy(np.full(total, qc.CANARY, dtype=np.uint32).view(np.int32)).cuda()
    args = dict(start=up(st) + 4 * off, end=up(en) + 4 * off, logit_stride=stride * 4, mask=up(mk) + 4 * ioff,
                ttype=up(tt) + 4 * ioff, ids_stride=istride * 4, rows=rows, S=case["S"], k_row=up(case["k_row"]),
                len_row=up(case["len_row"]), kmax=kmax, spans=out.data_ptr() + 4 * o_spans,
                scores=out.data_ptr() + 4 * o_scores, null_score=out.data_ptr() + 4 * o_null)
    if layout == "offset_strided":
        assert args["start"] % 16 == 4 and args["mask"] % 16 == 4 and args["logit_stride"] > case["S"] * 4
    for name, v in change.items():
        args[name] = v(args[name]) if callable(v) else v
    try:
        hip.qa_spans(*args.values())
    finally:
        torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("layout", sorted(qc.LAYOUTS))
@pytest.mark.parametrize("name", sorted(qc.cases()))
def test_kernel_equals_the_numpy_twin(torch, name, layout):
    case = qc.cases()[name]
    got = _call(torch, case, layout)
    assert qc.describe_mismatch(case, got) is None


def test_limits_come_from_the_header():
    from triton_client_amd.ops import hip

    assert (hip.QA_SPANS_KMAX, hip.QA_SPANS_MAX_SEQ) == (qc.KMAX, qc.MAX_SEQ) == (64, 1024)


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
def test_entry_refuses_before_any_launch(torch, what):
    from triton_client_amd.ops import hip

    with pytest.raises(hip.HipError) as e:
        _call(torch, qc.cases()["rows5_kmax7"], "packed", **BAD[what])
    assert e.value.code == 1  # hipErrorInvalidValue


def test_refused_calls_leave_the_canaries(torch):
    from triton_client_amd.ops import hip

    case = qc.cases()["rows5_kmax7"]
    real = hip.qa_spans
    refused = []

    def fn(*a):
        try:
            real(*a)
        except hip.HipError:
            refused.append(1)

    mp = pytest.MonkeyPatch()
    mp.setattr(hip, "qa_spans", fn)
    try:
        for what, change in sorted(BAD.items()):
            n = len(refused)
            out = _call(torch, case, "packed", **change)
            assert len(refused) == n + 1, what
            assert (out == np.int32(qc.CANARY)).all(), what
    finally:
        mp.undo()


def test_zero_rows_is_success_and_writes_nothing(torch):
    out = _call(torch, qc.cases()["rows5_kmax7"], "packed", rows=0)
    assert (out == np.int32(qc.CANARY)).all()


# ---------------------------------------------------------------------------------------------
# the model classes
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def models(torch):
    """The CPU ``qa_spans`` and the GPU one loaded with TCAMD_DEVICE_QA_SPANS=1 and =0."""
    from triton_client_amd.server import cpu_models, gpu_models

    mp = pytest.MonkeyPatch()
    out = {"cpu": cpu_models.QaSpans()}
    out["cpu"].load()
    for knob in ("1", "0"):
        mp.setenv("TCAMD_DEVICE_QA_SPANS", knob)
        out[knob] = gpu_models.QaSpans()
        out[knob].load()
    mp.undo()
    assert out["1"].device_path and not out["0"].device_path
    yield out
    for m in out.values():
        m.unload()


def _rows(n, seed):
    case = qc.make_case("served", seed, 384, n, [1], [1], logits=("integers", "normal"), eligible=("context", "holes"))
    return [case[k] for k in ("start", "end", "mask", "ttype")]


def _request(rows, device=None, **parameters):
    """A ``qa_spans`` request; ``device`` = a list that keeps the tensors of DeviceView inputs alive."""
    import torch

    from triton_client_amd.server.types import DeviceView, InferRequest, InputTensor

    ins = []
    for nm, a in zip(NAMES, rows):
        data = a
        if device is not None:
            # a tensor of its own with room in front: no two requests' rows ever follow each other
            t = torch.zeros(a.size + 32, dtype=torch.float32 if a.dtype == np.float32 else torch.int32, device="cuda")
            t[32:].copy_(torch.from_numpy(np.array(a)).reshape(-1))
            device.append(t)
            data = DeviceView(t.data_ptr() + 128, a.size * 4, 0)
        ins.append(InputTensor(nm, "FP32" if a.dtype == np.float32 else "INT32", list(a.shape), data))
    return InferRequest(model_name="qa_spans", parameters=parameters, inputs=ins)


BATCH = [(1, {}), (3, {"n_best": 64}), (2, {"n_best": 1, "max_answer_length": 384}), (1, {"n_best": 65}),
         (4, {"max_answer_length": 1})]


def _batch(device=None, mixed=False):
    return [_request(_rows(n, 40 + i), device if not mixed or i % 2 else None, **p) for i, (n, p) in enumerate(BATCH)]


def _assert_same(got, want):
    from triton_client_amd.server.types import ServerError

    assert len(got) == len(want)
    for g, w in zip(got, want):
        if isinstance(w, Exception):
            assert isinstance(g, ServerError) and g.msg == w.msg
            continue
        assert [o.name for o in g] == [o.name for o in w] == ["spans", "scores", "null_score"]
        for a, b in zip(g, w):
            assert a.shape == b.shape and a.datatype == b.datatype
            np.testing.assert_array_equal(np.asarray(a.data).view(np.int32), np.asarray(b.data).view(np.int32))


def _count(mp):
    from triton_client_amd.ops import hip

    real, calls = hip.qa_spans, []

    def counted(*a, **kw):
        calls.append(a[6])  # rows
        return real(*a, **kw)

    mp.setattr(hip, "qa_spans", counted)
    return calls


@pytest.mark.parametrize("inputs", ["host", "device", "mixed"])
def test_gpu_class_equals_the_cpu_class(models, inputs, monkeypatch):
    want = models["cpu"].execute(_batch())
    assert isinstance(want[3], Exception) and "n_best" in want[3].msg
    # and the CPU class equals the numpy twin, so all three agree
    rows = _rows(3, 41)
    spans = np.stack([qc.row_reference(*(a[r] for a in rows), 64, 30)[0] for r in range(3)])
    np.testing.assert_array_equal(want[1][0].data, spans)
    keep = []
    k27 = _count(monkeypatch)
    got = models["1"].execute(_batch(None if inputs == "host" else keep, mixed=inputs == "mixed"))
    # host inputs are staged back to back: the ten rows of the four good requests share one launch;
    # DeviceViews of separate tensors are read in place, request by request; mixed: the second request
    # alone is on the device, and the two staged requests behind it follow each other again
    assert k27 == {"host": [10], "device": [1, 3, 2, 4], "mixed": [1, 3, 6]}[inputs]
    _assert_same(got, want)


def test_device_views_that_follow_each_other_share_a_launch(models, torch, monkeypatch):
    """What ``bert_large`` hands the ensemble: every request's rows in one tensor of the batch."""
    from triton_client_amd.server.types import DeviceView, InferRequest, InputTensor

    rows = _rows(6, 50)
    dev = [torch.from_numpy(np.array(a)).cuda() for a in rows]
    reqs, want_reqs = [], []
    for first, n, p in ((0, 2, {"n_best": 3}), (2, 1, {}), (3, 3, {"n_best": 64, "max_answer_length": 7})):
        ins = [InputTensor(nm, "FP32" if a.dtype == np.float32 else "INT32", [n, 384],
                           DeviceView(t.data_ptr() + first * 1536, n * 1536, 0) if k < 2 else a[first:first + n])
               for k, (nm, a, t) in enumerate(zip(NAMES, rows, dev))]
        reqs.append(InferRequest(model_name="qa_spans", parameters=p, inputs=ins))
        want_reqs.append(_request([a[first:first + n] for a in rows], **p))
    k27 = _count(monkeypatch)
    got = models["1"].execute(reqs)
    assert k27 == [6]
    _assert_same(got, models["cpu"].execute(want_reqs))


def test_the_knob_changes_the_route_and_not_one_bit_of_the_spans(models, monkeypatch):
    res = {}
    for knob in ("1", "0"):
        k27 = _count(monkeypatch)
        res[knob] = models[knob].execute(_batch())
        assert k27 == ([10] if knob == "1" else [])
        monkeypatch.undo()
    _assert_same(res["1"], res["0"])


# ---------------------------------------------------------------------------------------------
# the ensemble, served in process
# ---------------------------------------------------------------------------------------------
def _inputs(b, seed):
    rng = np.random.default_rng(seed)
    ids = rng.integers(1000, 30000, size=(b, 384), dtype=np.int32)
    mask = np.ones((b, 384), dtype=np.int32)
    tt = np.zeros((b, 384), dtype=np.int32)
    for i in range(b):
        n = 384 if i % 3 == 0 else int(rng.integers(32, 384))
        q = int(rng.integers(8, max(9, n // 3)))
        mask[i, n:] = 0
        ids[i, n:] = 0
        tt[i, q:n] = 1  # question | context segments
    return ids, mask, tt


@pytest.fixture(scope="module")
def served(torch):
    """(server handle, per bert_large batch: how many of its outputs were DeviceViews / host arrays)."""
    from triton_client_amd.server import ServerHandle
    from triton_client_amd.server.gpu_models import BertLarge, BertQaEnsemble, QaSpans
    from triton_client_amd.server.types import DeviceView

    h = ServerHandle(models=[BertLarge, QaSpans, BertQaEnsemble], model_options={"bert_large": {"layers": 2}},
                     native_grpc=False).start()
    _, _, inst = h.server.get_instance("bert_large", "")
    seen = []
    real = inst.execute

    def execute(requests):
        res = real(requests)
        outs = [o for r in res if not isinstance(r, Exception) for o in r]
        views = [o for o in outs if isinstance(o.data, DeviceView)]
        assert all(o.owner.is_cuda and o.owner.data_ptr() <= o.data.ptr for o in views)
        seen.append((len(views), len(outs) - len(views)))
        return res

    inst.execute = execute
    yield h, seen
    h.stop()


def _infer(mod, client, model, ids, mask, tt, outputs=None, **parameters):
    ins = []
    for name, a in (("input_ids", ids), ("attention_mask", mask), ("token_type_ids", tt)):
        x = mod.InferInput(name, list(a.shape), "INT32")
        x.set_data_from_numpy(a)
        ins.append(x)
    return client.infer(model, ins, outputs=[mod.InferRequestedOutput(n) for n in outputs] if outputs else None,
                        parameters=parameters or None)


@pytest.mark.parametrize("kind", ["http", "grpc"])
@pytest.mark.parametrize("b,parameters", [(1, {}), (3, {}), (3, {"n_best": 64, "max_answer_length": 5})],
                         ids=["1row", "3rows", "3rows_n64_len5"])
def test_ensemble_spans_are_the_twin_of_its_own_logits(served, kind, b, parameters):
    import tritonclient.grpc as grpcclient
    import tritonclient.http as httpclient

    h, seen = served
    mod = httpclient if kind == "http" else grpcclient
    c = mod.InferenceServerClient(h.http_url if kind == "http" else h.grpc_url)
    ids, mask, tt = _inputs(b, 7 + b)
    del seen[:]
    r = _infer(mod, c, "bert_qa_ensemble", ids, mask, tt, **parameters)
    assert seen == [(2, 0)]  # one bert_large batch: both outputs stayed on the device
    st, en = r.as_numpy("start_logits"), r.as_numpy("end_logits")
    assert st.shape == en.shape == (b, 384) and np.isfinite(st).all() and np.isfinite(en).all()
    k, L = parameters.get("n_best", 20), parameters.get("max_answer_length", 30)
    assert r.as_numpy("spans").shape == (b, k, 2) and r.as_numpy("scores").shape == (b, k)
    for i in range(b):
        spans, bits, null = qc.row_reference(st[i], en[i], mask[i], tt[i], k, L)
        np.testing.assert_array_equal(r.as_numpy("spans")[i], spans)
        np.testing.assert_array_equal(r.as_numpy("scores")[i].view(np.uint32), bits)
        assert r.as_numpy("null_score")[i].view(np.uint32)[0] == null
        ok = (mask[i] >= 1) & (tt[i] == 1)
        assert ok[spans[:, 0]].all() and ok[spans[:, 1]].all()  # 30 answers at least: no filler here
    # a direct bert_large request still gets host arrays (its logits are not compared: random-weight
    # logits are nearly flat, and a span picked from one forward says nothing about another)
    del seen[:]
    raw = _infer(mod, c, "bert_large", ids, mask, tt)
    assert seen == [(0, 2)]
    assert raw.as_numpy("start_logits").shape == (b, 384)
    c.close()


def test_a_request_that_selects_only_spans_gets_only_spans(served):
    import tritonclient.http as httpclient

    h, _ = served
    c = httpclient.InferenceServerClient(h.http_url)
    ids, mask, tt = _inputs(2, 3)
    r = _infer(httpclient, c, "bert_qa_ensemble", ids, mask, tt, outputs=["spans"])
    assert [o["name"] for o in r.get_response()["outputs"]] == ["spans"]
    full = _infer(httpclient, c, "bert_qa_ensemble", ids, mask, tt)
    np.testing.assert_array_equal(r.as_numpy("spans"), full.as_numpy("spans"))
    assert [o["name"] for o in full.get_response()["outputs"]] == ["spans", "scores", "null_score", "start_logits",
                                                                  "end_logits"]
    c.close()


def test_ensemble_parameter_error_is_the_steps_own(served):
    import tritonclient.http as httpclient
    from tritonclient.utils import InferenceServerException

    h, _ = served
    c = httpclient.InferenceServerClient(h.http_url)
    with pytest.raises(InferenceServerException, match=r"n_best must be an int64 in \[1, 64\], not 0"):
        _infer(httpclient, c, "bert_qa_ensemble", *_inputs(1, 4), n_best=0)
    c.close()


@pytest.mark.parametrize("proto", ["http", "grpc"])
def test_example_check_passes(served, proto):
    h, _ = served
    r = run_example("bert_qa_client.py", h.http_url if proto == "http" else h.grpc_url,
                    ["-i", proto, "-b", "3", "--n-best", "25", "--check"])
    assert r.returncode == 0 and r.stdout.rstrip().endswith("PASS"), r.stdout[-1500:] + r.stderr[-1500:]
    assert r.stdout.count("rank  start  end  score") == 3

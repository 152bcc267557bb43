"""K29 qa_merge (csrc/kernels/qa_merge.hip) and K27 with a start mask
(tcamd_qa_spans_masked) against the numpy rule of tests/qa_merge_cases.py,
exact equality of every span, row and score bit, with canaries around, between
and behind everything they write; what the entries refuse; and the GPU
``qa_doc_spans`` model against the CPU one, knob on and off, host and device
inputs."""

import numpy as np
import pytest

from tests import qa_merge_cases as mc
from tests import qa_span_cases as qc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch

    torch.cuda.set_device(0)
    return torch


def _merge(torch, case, **change):
    """One ``hip.qa_merge`` call on the null stream; ``change`` replaces arguments by name.
    Returns the output buffer, guards included, as int32."""
    from triton_client_amd.ops import hip

    keep = []

    def up(a):
        t = torch.from_numpy(np.array(a)).cuda()
        keep.append(t)
        return t.data_ptr()

    D, kmax = case["docs"], case["kmax"]
    o_spans, o_windows, o_scores, o_null, total = mc.out_layout(D, kmax)
    out = torch.from_numpy(np.full(total, mc.CANARY, dtype=np.uint32).view(np.int32)).cuda()
    p = out.data_ptr()
    args = dict(spans=up(case["spans"]), scores=up(case["scores"].view(np.int32)), null=up(case["null"].view(np.int32)),
                rows=case["rows"], window_info=up(case["window_info"]), doc_info=up(case["doc_info"].view(np.int32)),
                docs=D, k_doc=up(case["k_doc"]), kmax=kmax, out_spans=p + 4 * o_spans, out_windows=p + 4 * o_windows,
                out_scores=p + 4 * o_scores, out_null=p + 4 * o_null)
    for name, v in change.items():
        args[name] = v(args[name]) if callable(v) else v
    try:
        hip.qa_merge(*args.values())
    finally:
        torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("name", sorted(mc.cases()))
def test_kernel_equals_the_numpy_twin(torch, name):
    got = _merge(torch, mc.cases()[name])
    want = mc.expected(name)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "%s: %d words differ, first at word %d: got 0x%08x, want 0x%08x" % (
        name, bad.size, bad[0], int(got[bad[0]]) & 0xFFFFFFFF, int(want[bad[0]]) & 0xFFFFFFFF)


BAD = {"kmax_zero": dict(kmax=0), "kmax_above_64": dict(kmax=65), "rows_negative": dict(rows=-1),
       "docs_negative": dict(docs=-1)}
for _p in ("spans", "scores", "null", "window_info", "doc_info", "k_doc", "out_spans", "out_windows", "out_scores",
           "out_null"):
    BAD[_p + "_null"] = {_p: None}
    BAD[_p + "_misaligned"] = {_p: lambda v: v + 2}


def test_entry_refuses_before_any_launch_and_leaves_the_canaries(torch):
    from triton_client_amd.ops import hip

    case = mc.cases()["mixed_k"]
    for what, change in sorted(BAD.items()):
        with pytest.raises(hip.HipError) as e:
            _merge(torch, case, **change)
        assert e.value.code == 1, what  # hipErrorInvalidValue
    assert (_merge(torch, case, docs=0) == np.int32(mc.CANARY)).all()
    # rows == 0: every document's rows lie outside, all are filler
    out = _merge(torch, case, rows=0)
    o_spans, o_windows, _, o_null, _ = mc.out_layout(case["docs"], case["kmax"])
    assert out[o_windows] == -1 and out[o_null].view(np.uint32) == qc.FILLER_BITS


# ---- K27 with a start mask ------------------------------------------------------------
def _masked(torch, case, ok, layout):
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
    so, _, _ = qc.pack(ok, layout)
    rows, kmax = case["rows"], case["kmax"]
    o_spans, o_scores, o_null, total = qc.out_layout(rows, kmax)
    out = torch.from_numpy(np.full(total, qc.CANARY, dtype=np.uint32).view(np.int32)).cuda()
    hip.qa_spans_masked(up(st) + 4 * off, up(en) + 4 * off, stride * 4, up(mk) + 4 * ioff, up(tt) + 4 * ioff,
                        up(so) + 4 * ioff, istride * 4, rows, case["S"], up(case["k_row"]), up(case["len_row"]), kmax,
                        out.data_ptr() + 4 * o_spans, out.data_ptr() + 4 * o_scores, out.data_ptr() + 4 * o_null)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("layout", sorted(qc.LAYOUTS))
@pytest.mark.parametrize("name", mc.MASKED_CASES + ("S1024", "rows129"))
def test_masked_kernel_equals_the_numpy_rule(torch, name, layout):
    case = qc.cases()[name]
    ok = mc.start_mask_of(case)
    got = _masked(torch, case, ok, layout)
    want = mc.masked_expected_buffer(case, ok)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "%s: %d words differ, first at word %d" % (name, bad.size, bad[0])
    # and with every start allowed it is K27 as before
    assert qc.describe_mismatch(case, _masked(torch, case, np.ones_like(case["mask"]), layout)) is None


def test_masked_entry_refuses_a_null_mask(torch):
    from triton_client_amd.ops import hip

    t = torch.zeros(1024, dtype=torch.int32, device="cuda")
    p = t.data_ptr()
    for bad in (0, p + 2):
        with pytest.raises(hip.HipError) as e:
            hip.qa_spans_masked(p, p, 32, p, p, bad, 32, 1, 8, p, p, 1, p, p, p)
        assert e.value.code == 1
    torch.cuda.synchronize()
    assert (t.cpu().numpy() == 0).all()


# ---------------------------------------------------------------------------------------------
# the model classes
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def models(torch):
    """The CPU ``qa_doc_spans`` and the GPU one loaded with TCAMD_DEVICE_QA_SPANS=1 and =0."""
    from triton_client_amd.server import cpu_models, gpu_models

    mp = pytest.MonkeyPatch()
    out = {"cpu": cpu_models.QaDocSpans()}
    out["cpu"].load()
    for knob in ("1", "0"):
        mp.setenv("TCAMD_DEVICE_QA_SPANS", knob)
        out[knob] = gpu_models.QaDocSpans()
        out[knob].load()
    mp.undo()
    assert out["1"].device_path and not out["0"].device_path
    yield out
    for m in out.values():
        m.unload()


NAMES = ("start_logits", "end_logits", "attention_mask", "token_type_ids", "start_mask", "window_info", "doc_info")


def _doc_arrays(seed, lens=(700, 9, 0, 400), qn=3, stride=100, S=384):
    """The seven inputs of a request over documents of ``lens`` context pieces."""
    from triton_client_amd.utils.qa import doc_windows

    rng = np.random.default_rng(seed)
    sm, winfo, dinfo, n = [], [], [], []
    for d, P in enumerate(lens):
        starts, ln, best = doc_windows(P, qn, stride, S)
        dinfo.append((len(n), len(starts), P, 0))
        for w in range(len(starts)):
            m = np.zeros(S, np.int32)
            m[2 + qn:2 + qn + ln[w]] = best[starts[w]:starts[w] + ln[w]] == w
            sm.append(m)
            winfo.append((d, starts[w], ln[w], 2 + qn))
            n.append(int(ln[w]))
    W = len(n)
    tt = np.zeros((W, S), np.int32)
    for r, k in enumerate(n):
        tt[r, 2 + qn:2 + qn + k] = 1
    mask = (np.arange(S)[None, :] < (np.asarray(n)[:, None] + 3 + qn)).astype(np.int32)
    start = rng.integers(-4, 5, size=(W, S)).astype(np.float32)  # ties within and across windows
    end = rng.integers(-4, 5, size=(W, S)).astype(np.float32)
    return [start, end, mask, tt, np.asarray(sm), np.asarray(winfo, np.int32), np.asarray(dinfo, np.int32)]


def _request(arrays, device=None, **parameters):
    """A ``qa_doc_spans`` request; ``device`` = a list that keeps the tensors of DeviceView inputs
    alive: the five row tensors arrive as DeviceViews, as from the ensemble's earlier steps."""
    import torch

    from triton_client_amd.server.types import DeviceView, InferRequest, InputTensor

    ins = []
    for k, (nm, a) in enumerate(zip(NAMES, arrays)):
        data = a
        if device is not None and k < 5:
            t = torch.from_numpy(np.array(a)).cuda()
            device.append(t)
            data = DeviceView(t.data_ptr(), a.size * 4, 0)
        ins.append(InputTensor(nm, "FP32" if a.dtype == np.float32 else "INT32", list(a.shape), data))
    return InferRequest(model_name="qa_doc_spans", parameters=parameters, inputs=ins)


def _batch(device=None):
    return [_request(_doc_arrays(1), device), _request(_doc_arrays(2, lens=(50,)), device, n_best=64),
            _request(_doc_arrays(3, lens=(1200, 1200), stride=20), device, n_best=1, max_answer_length=384),
            _request(_doc_arrays(4), device, n_best=65), _request(_doc_arrays(5, lens=(0,)), device, max_answer_length=1)]


def _assert_same(got, want):
    from triton_client_amd.server.types import ServerError

    assert len(got) == len(want)
    for g, w in zip(got, want):
        if isinstance(w, Exception):
            assert isinstance(g, ServerError) and g.msg == w.msg
            continue
        assert [o.name for o in g] == [o.name for o in w] == ["spans", "windows", "scores", "null_score"]
        for a, b in zip(g, w):
            assert list(a.shape) == list(b.shape) and a.datatype == b.datatype
            np.testing.assert_array_equal(np.asarray(a.data).view(np.int32), np.asarray(b.data).view(np.int32))


@pytest.mark.parametrize("inputs", ["host", "device"])
def test_gpu_class_equals_the_cpu_class_and_the_clients_route(models, inputs):
    from triton_client_amd.utils.qa import merge_windows

    want = models["cpu"].execute(_batch())
    assert isinstance(want[3], Exception) and "n_best" in want[3].msg
    assert want[2][0].shape == [2, 1, 2] and 64 < _doc_arrays(3, lens=(1200, 1200), stride=20)[0].shape[0] <= 128
    got = merge_windows(*_doc_arrays(1), 20, 30)
    for o, a in zip(want[0], got):
        assert np.asarray(o.data).tobytes() == a.tobytes(), o.name
    keep = []
    _assert_same(models["1"].execute(_batch(None if inputs == "host" else keep)), want)


def test_the_knob_changes_the_route_and_not_one_bit_of_the_answers(models, monkeypatch):
    from triton_client_amd.ops import hip

    res = {}
    for knob in ("1", "0"):
        calls = []
        for fn in ("qa_spans_masked", "qa_merge"):
            monkeypatch.setattr(hip, fn, lambda *a, _real=getattr(hip, fn), _fn=fn, **kw: (calls.append(_fn),
                                                                                         _real(*a, **kw))[1])
        res[knob] = models[knob].execute(_batch())
        assert calls == (["qa_spans_masked", "qa_merge"] * 4 if knob == "1" else [])
        monkeypatch.undo()
    _assert_same(res["1"], res["0"])

"""K28w wordpiece_windows (csrc/kernels/wordpiece.hip) against its host twin,
exact equality of every output word with canaries behind the workspace and the
outputs: the small shapes of tests/wordpiece_window_cases.py (S = 12, cap = 7:
every P and stride the rule branches on, max_windows, an invalid document
between good ones), 128 documents of 128 and of 129 rows, contexts over one and
two chunks, two calls on one stream; the GPU ``bert_window_tokenizer`` with the
knob on and off; and ``bert_qa_doc_ensemble`` served in process on a 2-layer
``bert_large``."""

import numpy as np
import pytest

from tests import wordpiece_cases as wc
from tests import wordpiece_window_cases as ww

pytestmark = pytest.mark.gpu

CANARY = 0x5A5A5A5A


@pytest.fixture(scope="module")
def torch():
    import torch

    torch.cuda.set_device(0)
    return torch


@pytest.fixture(scope="module")
def vocab():
    from triton_client_amd.utils import wordpiece

    return wordpiece.Vocab.load(wc.VOCAB_SMALL)


@pytest.fixture(scope="module")
def vocab_dev(torch, vocab):
    return torch.from_numpy(vocab.image.view(np.int32).copy()).cuda()


def _host(qs, cs, vocab, mq, ds, mw, S, out_rows):
    from triton_client_amd.ops import host_codec

    return host_codec.load().wordpiece_windows(qs, cs, vocab, mq, ds, mw, S, out_rows)


def _device(torch, vocab, vocab_dev, qs, cs, mq, ds, mw, S, out_rows, calls=1, stream=None):
    """``calls`` ``hip.wordpiece_windows`` calls back to back on one stream, each
    into outputs of its own, all on one workspace of exactly the advertised size
    with a canary behind it.  Returns the outputs of every call."""
    from triton_client_amd.ops import hip
    from triton_client_amd.utils import wordpiece

    buf, table = wordpiece.pack_texts(qs, cs)
    docs = table.shape[0]
    par = np.stack([np.broadcast_to(np.asarray(v, dtype=np.int32), (docs,)) for v in (mq, ds, mw)]).copy()
    ws_bytes = hip.wordpiece_windows_workspace(docs, buf.size)
    assert ws_bytes % 4 == 0 and ws_bytes == hip.wordpiece_workspace(docs, buf.size)
    ws = torch.full((ws_bytes // 4 + 64,), CANARY, dtype=torch.int32, device="cuda")
    text = torch.from_numpy(np.concatenate([buf, np.zeros(4, np.uint8)])).cuda()
    tab = torch.from_numpy(table.view(np.int32).copy()).cuda()
    pard = torch.from_numpy(par).cuda()
    n = out_rows * S
    words = 6 * n + 4 * out_rows + 4 * docs + 1
    outs = [torch.full((words + 64,), CANARY, dtype=torch.int32, device="cuda") for _ in range(calls)]
    sh = None if stream is None else stream.cuda_stream
    for out in outs:
        p = out.data_ptr()
        hip.wordpiece_windows(text.data_ptr(), buf.size, tab.data_ptr(), pard[0].data_ptr(), pard[1].data_ptr(),
                              pard[2].data_ptr(), docs, S, vocab_dev.data_ptr(), vocab.image.size, ws.data_ptr(),
                              ws_bytes, out_rows, p, p + 4 * n, p + 8 * n, p + 12 * n, p + 16 * n, p + 24 * n,
                              p + 24 * n + 16 * out_rows, p + 24 * n + 16 * out_rows + 16 * docs, stream=sh)
    torch.cuda.synchronize()
    assert (ws[ws_bytes // 4:].cpu().numpy() == CANARY).all(), "the kernel wrote behind its workspace"
    res = []
    for out in outs:
        a = out.cpu().numpy()
        assert (a[words:] == CANARY).all(), "the kernel wrote behind its outputs"
        w0 = 6 * n
        res.append((a[:n].reshape(out_rows, S), a[n:2 * n].reshape(out_rows, S), a[2 * n:3 * n].reshape(out_rows, S),
                    a[3 * n:4 * n].reshape(out_rows, S), a[4 * n:6 * n].reshape(out_rows, S, 2),
                    a[w0:w0 + 4 * out_rows].reshape(out_rows, 4),
                    a[w0 + 4 * out_rows:w0 + 4 * out_rows + 4 * docs].view(np.uint32).reshape(docs, 4),
                    int(a[words - 1])))
    return res


def _check(torch, vocab, vocab_dev, qs, cs, mq, ds, mw, S, out_rows, what):
    want = _host(qs, cs, vocab, mq, ds, mw, S, out_rows)
    got = _device(torch, vocab, vocab_dev, qs, cs, mq, ds, mw, S, out_rows)[0]
    ww.assert_same(got, want, what)
    return want


def test_kernel_equals_the_host_twin_on_the_small_shapes(torch, vocab, vocab_dev):
    seen = set()
    for name, qs, cs, mq, ds, mw, out_rows in ww.small_cases():
        want = _check(torch, vocab, vocab_dev, qs, cs, mq, ds, mw, 12, out_rows, name)
        seen |= {int(s) & 0xFF for s in want[6][:, 3]}
        if name.startswith("P "):
            assert want[6][0, 3] == 0 and want[7] == want[6][0, 1]
    assert seen == {0, 1, 4, 6}  # good, invalid UTF-8, a parameter, too many windows


@pytest.mark.parametrize("total", [128, 129])
def test_128_documents_at_the_row_capacity(torch, vocab, vocab_dev, total):
    qs, cs, mq, ds, mw, out_rows = ww.capacity_case(total)
    want = _check(torch, vocab, vocab_dev, qs, cs, mq, ds, mw, 12, out_rows, "capacity %d" % total)
    assert (want[6][:127, 3] == 0).all() and want[6][127, 3] == (0 if total == 128 else ww.ST_WINDOWS)
    assert want[7] == (128 if total == 128 else 127) and want[1][126].any() and want[1][127].any() == (total == 128)


@pytest.mark.parametrize("nbytes", [1100, 2100, 4096])
def test_contexts_across_chunk_edges(torch, vocab, vocab_dev, nbytes):
    qs = [b"What is tokenization?", "Σσ привет".encode()]
    cs = [ww.long_context(nbytes, nbytes), ww.long_context(nbytes // 2, 7)]
    # at the served shape, and at S = 32 where a window is shorter than a chunk by far
    _check(torch, vocab, vocab_dev, qs, cs, [64, 3], [128, 50], 128, 384, 128, "long %d" % nbytes)
    want = _check(torch, vocab, vocab_dev, qs, cs, [5, 3], [11, 24], 128, 32, 128, "long %d, S 32" % nbytes)
    assert want[6][0, 1] > 4 and want[6][0, 3] == 0


def test_two_calls_back_to_back_on_one_stream(torch, vocab, vocab_dev):
    qs, cs, mq = wc.random_rows(78, 9, invalid=0.1, max_items=200)
    args = (np.minimum(mq, 29), 7, 128, 32, 128)
    want = _host(qs, cs, vocab, *args)
    got = _device(torch, vocab, vocab_dev, qs, cs, *args, calls=2, stream=torch.cuda.Stream())
    ww.assert_same(got[0], want, "first call")
    ww.assert_same(got[1], want, "second call")


def test_entry_refuses_before_any_launch(torch, vocab, vocab_dev):
    from triton_client_amd.ops import hip

    t = torch.zeros(8192, dtype=torch.int32, device="cuda")
    p = t.data_ptr()
    good = [p, 4, p, p, p, p, 1, 12, vocab_dev.data_ptr(), vocab.image.size, p, hip.wordpiece_windows_workspace(1, 4), 1,
            p, p, p, p, p, p, p, p]
    for at, bad in ((6, 129), (6, -1), (7, 3), (7, 1025), (2, 0), (4, 0), (5, p + 2), (8, 0), (10, 0), (11, 16), (12, 0),
                    (12, 129), (16, 0), (18, p + 1), (19, 0), (20, 0)):
        args = list(good)
        args[at] = bad
        with pytest.raises(hip.HipError) as e:
            hip.wordpiece_windows(*args)
        assert e.value.code == 1, (at, bad)  # hipErrorInvalidValue
    torch.cuda.synchronize()
    assert (t.cpu().numpy() == 0).all()


# ---------------------------------------------------------------------------------------------
# the model classes
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def models(torch):
    """The CPU ``bert_window_tokenizer`` and the GPU one loaded with TCAMD_DEVICE_TOKENIZER=1 and =0."""
    from triton_client_amd.server import cpu_models, gpu_models

    mp = pytest.MonkeyPatch()
    mp.setenv("TCAMD_BERT_VOCAB", wc.VOCAB_SMALL)
    out = {"cpu": cpu_models.BertWindowTokenizer()}
    out["cpu"].load()
    for knob in ("1", "0"):
        mp.setenv("TCAMD_DEVICE_TOKENIZER", knob)
        out[knob] = gpu_models.BertWindowTokenizer()
        out[knob].load()
    mp.undo()
    assert out["1"].device_path and not out["0"].device_path
    yield out
    for m in out.values():
        m.unload()


def _request(questions, contexts, device_outputs=False, **parameters):
    from triton_client_amd.server.types import InferRequest, InputTensor

    n = len(questions)
    ins = [InputTensor(nm, "BYTES", [n], np.array(list(col), dtype=object))
           for nm, col in (("question", questions), ("context", contexts))]
    r = InferRequest(model_name="bert_window_tokenizer", parameters=parameters, inputs=ins)
    r.accepts_device_outputs = device_outputs
    return r


LONG = (b"b " * 600 + b"unaffable kernel devices" + b" a" * 40)[:1282]


def _batch(device_outputs=False):
    qs, cs, _ = wc.random_rows(6, 5, invalid=0.0, max_items=150)
    return [_request(qs, cs, device_outputs), _request([b"a b c", b"q"], [LONG, b"x"], device_outputs, doc_stride=64),
            _request([b"ok", b"ok"], [b"fine", b"head \xc3"], device_outputs),
            _request([b"a b c"], [LONG], device_outputs, max_windows=3),
            _request([b"a b c"] * 4, [LONG] * 4, device_outputs, doc_stride=8),
            _request([b"q"], [b"c" * 65537], device_outputs), _request([b"q"], [b"c"], device_outputs, doc_stride=0)]


def _assert_same_results(got, want):
    from triton_client_amd.ops import hip
    from triton_client_amd.server.types import DeviceView, ServerError

    assert len(got) == len(want)
    for g, w in zip(got, want):
        if isinstance(w, Exception):
            assert isinstance(g, ServerError) and g.msg == w.msg
            continue
        assert [o.name for o in g] == [o.name for o in w] == ["input_ids", "attention_mask", "token_type_ids",
                                                              "start_mask", "offsets", "window_info", "doc_info"]
        for a, b in zip(g, w):
            assert list(a.shape) == list(b.shape) and a.datatype == b.datatype == "INT32"
            data = a.data
            if isinstance(data, DeviceView):
                raw = np.empty(data.nbytes, dtype=np.uint8)
                hip.memcpy_d2h(raw, data.ptr, data.nbytes)
                data = raw.view(np.int32).reshape(a.shape)
            np.testing.assert_array_equal(np.asarray(data), np.asarray(b.data))


def test_the_knob_changes_the_route_and_not_one_bit_of_the_rows(models):
    from triton_client_amd.server.types import DeviceView

    want = models["cpu"].execute(_batch())
    assert want[2].msg == "bert_window_tokenizer: document 1: context is not valid UTF-8 at byte 5"
    assert want[3].msg == "bert_window_tokenizer: document 0: context needs 4 windows, max_windows 3"
    assert want[4].msg == "bert_window_tokenizer: document 3: context needs 34 windows, exceeds 128 rows"
    assert want[5].msg == "bert_window_tokenizer: document 0: context too long" and "doc_stride" in want[6].msg
    assert want[1][0].shape[0] > 5
    _assert_same_results(models["1"].execute(_batch()), want)
    _assert_same_results(models["0"].execute(_batch()), want)
    on_device = models["1"].execute(_batch(device_outputs=True))
    assert all(isinstance(o.data, DeviceView) and o.owner.is_cuda for o in on_device[1][:4])
    assert not any(isinstance(o.data, DeviceView) for o in on_device[1][4:])
    _assert_same_results(on_device, want)


# ---------------------------------------------------------------------------------------------
# the document ensemble, served in process
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def served(torch):
    """(server handle, per bert_large batch: (rows, inputs that were DeviceViews, host inputs))."""
    from triton_client_amd.server import ServerHandle
    from triton_client_amd.server.gpu_models import BertLarge, BertQaDocEnsemble, BertWindowTokenizer, QaDocSpans
    from triton_client_amd.server.types import DeviceView

    mp = pytest.MonkeyPatch()
    mp.setenv("TCAMD_BERT_VOCAB", wc.VOCAB_SMALL)
    mp.setenv("TCAMD_DEVICE_TOKENIZER", "1")
    mp.setenv("TCAMD_DEVICE_QA_SPANS", "1")
    h = ServerHandle(models=[BertWindowTokenizer, BertLarge, QaDocSpans, BertQaDocEnsemble],
                     model_options={"bert_large": {"layers": 2}}, native_grpc=False).start()
    mp.undo()
    seen = []
    for name in ("bert_large", "qa_doc_spans"):
        _, _, inst = h.server.get_instance(name, "")

        def execute(requests, real=inst.execute, name=name):
            ins = [t for r in requests for t in r.inputs]
            views = [t for t in ins if isinstance(t.data, DeviceView)]
            seen.append((name, int(requests[0].inputs[0].shape[0]), len(views), len(ins) - len(views)))
            return real(requests)

        inst.execute = execute
    yield h, seen
    h.stop()


QUESTIONS = [b"What is tokenization?", "Who walked? Σσ".encode(), b"when"]
CONTEXTS = [LONG, "Привет мир! The model walked and talked; 中国 tokenization, café.".encode(),
            ww.long_context(3000, 11)]


def _doc_inputs(mod, questions, contexts):
    ins = []
    for name, col in (("question", questions), ("context", contexts)):
        x = mod.InferInput(name, [len(col)], "BYTES")
        x.set_data_from_numpy(np.array(list(col), dtype=object))
        ins.append(x)
    return ins


@pytest.mark.parametrize("kind", ["http", "grpc"])
def test_doc_ensemble_is_the_clients_route_over_its_own_logits(served, vocab, kind):
    import tritonclient.grpc as grpcclient
    import tritonclient.http as httpclient

    from triton_client_amd.utils.qa import answer_text_doc, merge_windows

    h, seen = served
    mod = httpclient if kind == "http" else grpcclient
    c = mod.InferenceServerClient(h.http_url if kind == "http" else h.grpc_url)
    params = {"doc_stride": 96, "n_best": 7, "max_answer_length": 12}
    want = _host(QUESTIONS, CONTEXTS, vocab, 64, 96, 128, 384, 128)
    n = want[7]
    assert n > 5 and not want[6][:, 3].any()
    del seen[:]
    r = c.infer("bert_qa_doc_ensemble", _doc_inputs(mod, QUESTIONS, CONTEXTS), parameters=params)
    # one bert_large batch of all windows, ids in place; the span step reads five tensors in place
    assert seen == [("bert_large", n, 3, 0), ("qa_doc_spans", n, 5, 2)]
    for name, a in zip(("input_ids", "attention_mask", "token_type_ids", "start_mask", "offsets", "window_info"), want[:6]):
        np.testing.assert_array_equal(r.as_numpy(name), a[:n])
    np.testing.assert_array_equal(r.as_numpy("doc_info"), want[6].view(np.int32))
    st, en = r.as_numpy("start_logits"), r.as_numpy("end_logits")
    assert st.shape == en.shape == (n, 384) and np.isfinite(st).all()
    got = merge_windows(st, en, want[1][:n], want[2][:n], want[3][:n], want[5][:n], want[6], 7, 12)
    np.testing.assert_array_equal(r.as_numpy("spans"), got[0])
    np.testing.assert_array_equal(r.as_numpy("windows"), got[1])
    assert r.as_numpy("scores").tobytes() == got[2].tobytes() and r.as_numpy("null_score").tobytes() == got[3].tobytes()
    assert r.as_numpy("spans").shape == (3, 7, 2)
    for d in range(3):
        w, (s, e) = int(r.as_numpy("windows")[d, 0]), r.as_numpy("spans")[d, 0]
        assert want[5][w, 0] == d and want[3][w, s] == 1 and want[2][w, e] == 1
        text = answer_text_doc(CONTEXTS[d], (s, e), w, r.as_numpy("offsets"))
        assert text and text == CONTEXTS[d][want[4][w, s, 0]:want[4][w, e, 1]]
    # asked for the answers alone, nothing else comes back
    del seen[:]
    few = c.infer("bert_qa_doc_ensemble", _doc_inputs(mod, QUESTIONS, CONTEXTS), parameters=params,
                  outputs=[mod.InferRequestedOutput(x) for x in ("spans", "windows")])
    np.testing.assert_array_equal(few.as_numpy("spans"), got[0])
    assert few.as_numpy("offsets") is None
    c.close()


def test_doc_ensemble_fails_a_request_with_the_documents_message(served):
    import tritonclient.http as httpclient
    from tritonclient.utils import InferenceServerException

    h, _ = served
    c = httpclient.InferenceServerClient(h.http_url)
    with pytest.raises(InferenceServerException, match="document 1: question is not valid UTF-8 at byte 2"):
        c.infer("bert_qa_doc_ensemble", _doc_inputs(httpclient, [b"a", b"ab\xff"], [b"c", b"c"]))
    with pytest.raises(InferenceServerException, match="document 0: context needs 4 windows, max_windows 2"):
        c.infer("bert_qa_doc_ensemble", _doc_inputs(httpclient, [b"a b c"], [LONG]), parameters={"max_windows": 2})
    r = c.infer("bert_qa_doc_ensemble", _doc_inputs(httpclient, [b"a"], [b"c d"]), parameters={"n_best": 2})
    assert r.as_numpy("spans").shape == (1, 2, 2) and r.as_numpy("windows").tolist() == [[0, 0]]
    c.close()


@pytest.mark.parametrize("proto", ["http", "grpc"])
def test_example_check_passes(served, proto):
    from tests.test_examples import run_example

    h, _ = served
    r = run_example("bert_qa_doc_client.py", h.http_url if proto == "http" else h.grpc_url,
                    ["-i", proto, "--n-best", "5", "--doc-stride", "64", "--vocab", wc.VOCAB_SMALL, "--check"])
    assert r.returncode == 0 and r.stdout.rstrip().endswith("PASS"), r.stdout[-1500:] + r.stderr[-1500:]

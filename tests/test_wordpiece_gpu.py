"""K28 wordpiece (csrc/kernels/wordpiece.hip) against its host twin, exact
equality of every id, offset, overflow and status word: on the fixed cases of
tests/wordpiece_cases.py, on cases aimed at the kernel's own chunk edges
(``wordpiece_geometry()``), on 1, 2 and 128 rows in one call, and twice on one
stream with a workspace of exactly the advertised size and a canary behind
it; the GPU ``bert_tokenizer`` with the knob on and off; and
``bert_qa_text_ensemble`` served in process on a 2-layer ``bert_large``."""

import numpy as np
import pytest

from tests import wordpiece_cases as wc

pytestmark = pytest.mark.gpu

CANARY = 0x5A5A5A5A
S = wc.SEQ


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


def _host(questions, contexts, vocab, mq):
    from triton_client_amd.ops import host_codec

    return host_codec.load().wordpiece_tokenize(questions, contexts, vocab, mq, S)


def _device(torch, vocab, vocab_dev, questions, contexts, mq, calls=1, stream=None):
    """``calls`` ``hip.wordpiece_tokenize`` calls back to back on one stream, each
    into outputs of its own, all on one workspace of exactly the advertised size
    with a canary behind it.  Returns the outputs of every call."""
    from triton_client_amd.ops import hip
    from triton_client_amd.utils import wordpiece

    buf, table = wordpiece.pack_texts(questions, contexts)
    rows = table.shape[0]
    mq = np.array(np.broadcast_to(np.asarray(mq, dtype=np.int32), (rows,)))  # a writable copy
    ws_bytes = hip.wordpiece_workspace(rows, buf.size)
    assert ws_bytes % 4 == 0
    ws = torch.full((ws_bytes // 4 + 64,), CANARY, dtype=torch.int32, device="cuda")
    text = torch.from_numpy(np.concatenate([buf, np.zeros(4, np.uint8)])).cuda()
    tab = torch.from_numpy(table.view(np.int32).copy()).cuda()
    mqd = torch.from_numpy(mq).cuda()
    words = rows * (S * 5 + 2)
    outs = [torch.full((words + 64,), CANARY, dtype=torch.int32, device="cuda") for _ in range(calls)]
    sh = None if stream is None else stream.cuda_stream
    for out in outs:
        p = out.data_ptr()
        hip.wordpiece_tokenize(text.data_ptr(), buf.size, tab.data_ptr(), mqd.data_ptr(), rows, S,
                               vocab_dev.data_ptr(), vocab.image.size, ws.data_ptr(), ws_bytes, p, p + rows * S * 4,
                               p + rows * S * 8, p + rows * S * 12, p + rows * S * 20, p + rows * S * 20 + rows * 4,
                               stream=sh)
    torch.cuda.synchronize()
    assert (ws[ws_bytes // 4:].cpu().numpy() == CANARY).all(), "the kernel wrote behind its workspace"
    res = []
    for out in outs:
        a = out.cpu().numpy()
        assert (a[words:] == CANARY).all(), "the kernel wrote behind its outputs"
        n = rows * S
        res.append((a[:n].reshape(rows, S), a[n:2 * n].reshape(rows, S), a[2 * n:3 * n].reshape(rows, S),
                    a[3 * n:5 * n].reshape(rows, S, 2), a[5 * n:5 * n + rows], a[5 * n + rows:words].view(np.uint32)))
    return res


def _check(torch, vocab, vocab_dev, questions, contexts, mq=64, what=""):
    want = _host(questions, contexts, vocab, mq)
    got = _device(torch, vocab, vocab_dev, questions, contexts, mq)[0]
    wc.assert_same(got, want, what)
    return want


def test_geometry_and_workspace_agree_with_the_host_library():
    from triton_client_amd.ops import hip, host_codec

    codec = host_codec.load()
    g = hip.wordpiece_geometry()
    assert g == codec.wordpiece_geometry()
    assert g["chunk"] % g["block"] == 0 and g["max_text_bytes"] == 65536 and g["max_rows"] == 128
    for rows, nbytes in ((1, 0), (1, 1), (2, 1500), (128, 128 * 65536)):
        assert hip.wordpiece_workspace(rows, nbytes) == codec.wordpiece_workspace(rows, nbytes)


def test_kernel_equals_the_host_twin_on_the_fixed_cases(torch, vocab, vocab_dev):
    cases = wc.fixed_cases()
    want = _check(torch, vocab, vocab_dev, [c[1] for c in cases], [c[2] for c in cases], [c[3] for c in cases],
                  "fixed cases")
    by = {c[0]: r for r, c in enumerate(cases)}
    assert want[4][by["context overflows by one"]] == 1 and want[4][by["context fills the row"]] == 0
    assert want[5][by["text of 65537"]] == 2 | 1 << 8 and want[5][by["text of 65536"]] == 0
    assert want[5][by["invalid surrogate mid"]] & 0xFF == 1


def _edge_cases():
    from triton_client_amd.ops import host_codec

    g = host_codec.load().wordpiece_geometry()
    C = g["chunk"]
    u = lambda s: s.encode("utf-8")  # noqa: E731
    cases = {}
    for back in (1, 2, 3):  # a 4-byte, a 3-byte and a 2-byte character over the edge
        for ch in ("\U0001f600", "한", "é"):
            n = len(u(ch))
            if back < n:
                head = "a " * ((C - back) // 2) + "a" * ((C - back) % 2)
                cases["%d-byte char %d before the edge" % (n, back)] = u(head + ch + " tail")
    # a fold that expands (3 jamo from 3 bytes) across the edge of the folded positions: dropped code
    # points in front shift the folded stream against the bytes
    cases["expanding folds across the edge"] = u("한" * (C // 3 + 5) + " 글")
    cases["dropped then expanding"] = u("​" * 7 + "한글" * (C // 6 + 3))
    cases["word across the byte edge"] = u("a " * (C // 2 - 3) + "tokenization walked")
    cases["long word across the edge"] = u("b " * (C // 2 - 20) + "x" * 100 + " " + "x" * 101 + " end")
    cases["unknown word across the edge"] = u("b " * (C // 2 - 1) + "αβγδ" + " αβγ")
    cases["exactly one chunk"] = u("ab " * (C // 3) + "c" * (C % 3))
    cases["one chunk and one byte"] = u("ab " * (C // 3) + "c" * (C % 3 + 1))
    cases["one byte"] = b"a"
    cases["one invalid byte"] = b"\x80"
    cases["invalid at the edge"] = u("a" * (C - 1)) + b"\xe2\x82"
    cases["invalid lead before the edge"] = u("a" * (C - 1)) + b"\xe2A" + u("b" * 10)
    cases["text of 65536"] = (b"ab " * 21846)[:65536]
    cases["pieces across many chunks"] = u("a b. " * 700)
    assert len(cases["exactly one chunk"]) == C and len(cases["text of 65536"]) == 65536
    return cases


def test_kernel_equals_the_host_twin_at_its_chunk_edges(torch, vocab, vocab_dev):
    cases = _edge_cases()
    names = sorted(cases)
    # as contexts (offsets are checked) and as questions, cut at every max_query_length
    want = _check(torch, vocab, vocab_dev, [b"what is it?"] * len(names), [cases[n] for n in names], 64, "edges, context")
    assert want[5][names.index("invalid at the edge")] != 0 and want[4][names.index("pieces across many chunks")] > 0
    _check(torch, vocab, vocab_dev, [cases[n] for n in names], [b"b c"] * len(names), 381, "edges, question")


@pytest.mark.parametrize("rows", [1, 2, 128])
def test_rows_of_mixed_lengths_share_a_call(torch, vocab, vocab_dev, rows):
    qs, cs, mq = wc.random_rows(1000 + rows, rows, invalid=0.0, max_items=120)
    cs = [c * (1 + (r % 5) * 7) for r, c in enumerate(cs)]  # up to a few chunks
    for r in range(3, rows, 17):
        qs[r], cs[r] = b"", b""
    if rows > 2:
        cs[rows // 2] = cs[rows // 2][:40] + b"\xed\xa0\x80" + cs[rows // 2][40:]
    want = _check(torch, vocab, vocab_dev, qs, cs, mq, "%d rows" % rows)
    if rows > 2:
        assert want[5][rows // 2] & 0xFF == 1 and np.count_nonzero(want[5]) == 1
        assert (want[0][rows // 2] == 0).all() and (want[0][rows // 2 + 1] != 0).any()


def test_two_calls_back_to_back_on_one_stream(torch, vocab, vocab_dev):
    qs, cs, mq = wc.random_rows(77, 16, invalid=0.1, max_items=200)
    want = _host(qs, cs, vocab, mq)
    stream = torch.cuda.Stream()
    got = _device(torch, vocab, vocab_dev, qs, cs, mq, calls=2, stream=stream)
    wc.assert_same(got[0], want, "first call")
    wc.assert_same(got[1], want, "second call")


def test_entry_refuses_before_any_launch(torch, vocab, vocab_dev):
    from triton_client_amd.ops import hip

    t = torch.zeros(4096, dtype=torch.int32, device="cuda")
    p = t.data_ptr()
    good = [p, 4, p, p, 1, S, vocab_dev.data_ptr(), vocab.image.size, p, hip.wordpiece_workspace(1, 4), p, p, p, p, p, p]
    for at, bad in ((4, 129), (4, -1), (5, 3), (5, 1025), (2, 0), (2, p + 2), (6, 0), (7, 3), (8, 0), (9, 16), (10, p + 1),
                    (15, 0)):
        args = list(good)
        args[at] = bad
        with pytest.raises(hip.HipError) as e:
            hip.wordpiece_tokenize(*args)
        assert e.value.code == 1, (at, bad)  # hipErrorInvalidValue
    torch.cuda.synchronize()
    assert (t.cpu().numpy() == 0).all()


# ---------------------------------------------------------------------------------------------
# the model classes
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def models(torch):
    """The CPU ``bert_tokenizer`` and the GPU one loaded with TCAMD_DEVICE_TOKENIZER=1 and =0."""
    from triton_client_amd.server import cpu_models, gpu_models

    mp = pytest.MonkeyPatch()
    mp.setenv("TCAMD_BERT_VOCAB", wc.VOCAB_SMALL)
    out = {"cpu": cpu_models.BertTokenizer()}
    out["cpu"].load()
    for knob in ("1", "0"):
        mp.setenv("TCAMD_DEVICE_TOKENIZER", knob)
        out[knob] = gpu_models.BertTokenizer()
        out[knob].load()
    mp.undo()
    assert out["1"].device_path and not out["0"].device_path
    yield out
    for m in out.values():
        m.unload()


def _request(questions, contexts, **parameters):
    from triton_client_amd.server.types import InferRequest, InputTensor

    n = len(questions)
    ins = [InputTensor(nm, "BYTES", [n, 1], np.array(list(col), dtype=object).reshape(n, 1))
           for nm, col in (("question", questions), ("context", contexts))]
    return InferRequest(model_name="bert_tokenizer", parameters=parameters, inputs=ins)


def _batch():
    qs, cs, _ = wc.random_rows(5, 9, invalid=0.0, max_items=150)
    return [_request(qs[0:1], cs[0:1]), _request(qs[1:4], cs[1:4], max_query_length=3),
            _request([b"ok"], [b"head \xc3"]), _request(qs[4:6], cs[4:6], max_query_length=0),
            _request(qs[6:9], cs[6:9], max_query_length=381), _request([b"q"], [b"c" * 65537])]


def _assert_same_results(got, want):
    from triton_client_amd.server.types import ServerError

    assert len(got) == len(want)
    for g, w in zip(got, want):
        if isinstance(w, Exception):
            assert isinstance(g, ServerError) and g.msg == w.msg
            continue
        assert [o.name for o in g] == [o.name for o in w]
        assert [o.name for o in g] == ["input_ids", "attention_mask", "token_type_ids", "offsets", "overflow"]
        for a, b in zip(g, w):
            assert a.shape == b.shape and a.datatype == b.datatype == "INT32"
            np.testing.assert_array_equal(np.asarray(a.data), np.asarray(b.data))


def _count(mp):
    from triton_client_amd.ops import hip

    real, calls = hip.wordpiece_tokenize, []

    def counted(*a, **kw):
        calls.append(a[4])  # rows
        return real(*a, **kw)

    mp.setattr(hip, "wordpiece_tokenize", counted)
    return calls


def test_the_knob_changes_the_route_and_not_one_bit_of_the_rows(models, monkeypatch):
    want = models["cpu"].execute(_batch())
    assert want[2].msg == "bert_tokenizer: context is not valid UTF-8 at byte 5"
    assert "max_query_length" in want[3].msg and want[5].msg == "bert_tokenizer: context too long"
    res = {}
    for knob in ("1", "0"):
        k28 = _count(monkeypatch)
        res[knob] = models[knob].execute(_batch())
        assert k28 == ([8] if knob == "1" else [])  # the rows of the four requests whose parameters passed
        monkeypatch.undo()
    _assert_same_results(res["1"], want)
    _assert_same_results(res["0"], want)


def test_a_batch_beyond_the_staging_budget_runs_in_several_launches(models, monkeypatch):
    m = models["1"]
    ctx = (b"the quick brown fox. " * 3200)[:65536]
    reqs = [_request([b"what is it"] * 5, [ctx[:65536 - 7 * r] for r in range(5)]) for _ in range(4)]
    assert 20 * 65536 > m.TEXT_BUDGET
    k28 = _count(monkeypatch)
    got = m.execute(reqs)
    assert len(k28) == 2 and sum(k28) == 20
    monkeypatch.undo()
    _assert_same_results(got, models["cpu"].execute(reqs))


# ---------------------------------------------------------------------------------------------
# the text ensemble, served in process
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def served(torch):
    """(server handle, per bert_large batch: how many of its inputs were DeviceViews / host arrays)."""
    from triton_client_amd.server import ServerHandle
    from triton_client_amd.server.gpu_models import (BertLarge, BertQaEnsemble, BertQaTextEnsemble, BertTokenizer,
                                                     QaSpans)
    from triton_client_amd.server.types import DeviceView

    mp = pytest.MonkeyPatch()
    mp.setenv("TCAMD_BERT_VOCAB", wc.VOCAB_SMALL)
    mp.setenv("TCAMD_DEVICE_TOKENIZER", "1")
    h = ServerHandle(models=[BertTokenizer, BertLarge, QaSpans, BertQaEnsemble, BertQaTextEnsemble],
                     model_options={"bert_large": {"layers": 2}}, native_grpc=False).start()
    mp.undo()
    _, _, inst = h.server.get_instance("bert_large", "")
    seen = []
    real = inst.execute

    def execute(requests):
        ins = [t for r in requests for t in r.inputs]
        views = [t for t in ins if isinstance(t.data, DeviceView)]
        seen.append((len(views), len(ins) - len(views)))
        return real(requests)

    inst.execute = execute
    yield h, seen
    h.stop()


QUESTIONS = [b"What jumps over the lazy dog?", "Who walked? Σσ".encode(), b"when"]
CONTEXTS = ["The quick brown fox jumps over the lazy dog. ".encode() * 3,
            "Привет мир! The model walked and talked; 中国 tokenization, café.".encode(),
            b"b. " * 600]


def _text_inputs(mod, questions, contexts):
    ins = []
    for name, col in (("question", questions), ("context", contexts)):
        x = mod.InferInput(name, [len(col), 1], "BYTES")
        x.set_data_from_numpy(np.array(list(col), dtype=object).reshape(-1, 1))
        ins.append(x)
    return ins


@pytest.mark.parametrize("kind", ["http", "grpc"])
def test_text_ensemble_equals_the_id_ensemble_on_the_twins_ids(served, vocab, kind):
    import tritonclient.grpc as grpcclient
    import tritonclient.http as httpclient

    from triton_client_amd.utils.qa import answer_text

    h, seen = served
    mod = httpclient if kind == "http" else grpcclient
    c = mod.InferenceServerClient(h.http_url if kind == "http" else h.grpc_url)
    ids, mask, tt, offsets, overflow, status = _host(QUESTIONS, CONTEXTS, vocab, 64)
    assert not status.any() and overflow[2] > 0 and overflow[0] == 0
    del seen[:]
    wanted = ["spans", "scores", "null_score", "offsets", "overflow"]
    r = c.infer("bert_qa_text_ensemble", _text_inputs(mod, QUESTIONS, CONTEXTS),
                outputs=[mod.InferRequestedOutput(n) for n in wanted])
    assert seen == [(3, 0)]  # one bert_large batch: its three inputs arrived as DeviceViews
    ins = []
    for name, a in (("input_ids", ids), ("attention_mask", mask), ("token_type_ids", tt)):
        x = mod.InferInput(name, list(a.shape), "INT32")
        x.set_data_from_numpy(a)
        ins.append(x)
    ref = c.infer("bert_qa_ensemble", ins)
    for name in ("spans", "scores", "null_score"):
        np.testing.assert_array_equal(r.as_numpy(name).view(np.int32), ref.as_numpy(name).view(np.int32))
    np.testing.assert_array_equal(r.as_numpy("offsets"), offsets)
    np.testing.assert_array_equal(r.as_numpy("overflow").reshape(-1), overflow)
    for i in range(3):
        s, e = r.as_numpy("spans")[i, 0]
        assert tt[i, s] == 1 and tt[i, e] == 1 and s <= e
        assert answer_text(CONTEXTS[i], (s, e), r.as_numpy("offsets")[i]) == CONTEXTS[i][offsets[i, s, 0]:offsets[i, e, 1]]
        assert answer_text(CONTEXTS[i], (s, e), r.as_numpy("offsets")[i]) != b""
    # asked for, the ids come down and are the twin's
    full = c.infer("bert_qa_text_ensemble", _text_inputs(mod, QUESTIONS, CONTEXTS))
    np.testing.assert_array_equal(full.as_numpy("input_ids"), ids)
    np.testing.assert_array_equal(full.as_numpy("attention_mask"), mask)
    np.testing.assert_array_equal(full.as_numpy("token_type_ids"), tt)
    c.close()


def test_text_ensemble_fails_the_invalid_request_alone(served):
    import tritonclient.http as httpclient
    from tritonclient.utils import InferenceServerException

    h, _ = served
    c = httpclient.InferenceServerClient(h.http_url)
    with pytest.raises(InferenceServerException, match="bert_tokenizer: question is not valid UTF-8 at byte 2"):
        c.infer("bert_qa_text_ensemble", _text_inputs(httpclient, [b"ab\xff"], [b"c"]))
    with pytest.raises(InferenceServerException, match=r"max_query_length must be an int64 in \[1, 381\], not 382"):
        c.infer("bert_qa_text_ensemble", _text_inputs(httpclient, [b"a"], [b"c"]), parameters={"max_query_length": 382})
    r = c.infer("bert_qa_text_ensemble", _text_inputs(httpclient, [b"a"], [b"c d"]), parameters={"n_best": 2})
    assert r.as_numpy("spans").shape == (1, 2, 2)
    c.close()


@pytest.mark.parametrize("proto", ["http", "grpc"])
def test_example_check_passes(served, proto):
    from tests.test_examples import run_example

    h, _ = served
    r = run_example("bert_qa_text_client.py", h.http_url if proto == "http" else h.grpc_url,
                    ["-i", proto, "--n-best", "7", "--max-query-length", "6", "--vocab", wc.VOCAB_SMALL, "--check",
                     "-q", "Who walked?", "-c", "The model walked and talked.", "-q", "Σσ?", "-c", "中国 café naïve."])
    assert r.returncode == 0 and r.stdout.rstrip().endswith("PASS"), r.stdout[-1500:] + r.stderr[-1500:]
    assert r.stdout.count("rank  start  end  score      answer") == 2

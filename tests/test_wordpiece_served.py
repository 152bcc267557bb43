"""The ``bert_tokenizer`` model on the in-process CPU server (the host twin of
K28 behind server/cpu_models.py BertTokenizer): over HTTP and gRPC against the
Python twin of tests/wordpiece_cases.py, requests of different
``max_query_length`` in one batch, one invalid request failing alone with its
message, the parameter checks, and where the vocabulary comes from.

The CPU zoo has no ``bert_large`` (its weights and kernels are GPU code), so
``bert_qa_text_ensemble`` is a GPU-server model: this file asserts the
``bert_tokenizer`` half, and that the ensemble is declared over it;
tests/test_wordpiece_gpu.py serves the ensemble."""

import numpy as np
import pytest

from tests import wordpiece_cases as wc

QS = [b"What is the answer?", "Σσ Привет".encode(), b"a a a a a a", b""]
CS = ["The quick brown fox jumps over the lazy dog. café".encode(), "中国 tokenization 한글".encode(), b"b. " * 200,
      b"walked"]


@pytest.fixture(scope="module")
def served():
    from triton_client_amd.server import ServerHandle
    from triton_client_amd.server.cpu_models import BertTokenizer

    mp = pytest.MonkeyPatch()
    mp.setenv("TCAMD_BERT_VOCAB", wc.VOCAB_SMALL)
    h = ServerHandle(models=[BertTokenizer], native_grpc=False).start()
    mp.undo()
    yield h
    h.stop()


@pytest.fixture(scope="module")
def twin_vocab():
    return wc.TwinVocab()


def _inputs(mod, questions, contexts):
    ins = []
    for name, col in (("question", questions), ("context", contexts)):
        x = mod.InferInput(name, [len(col), 1], "BYTES")
        x.set_data_from_numpy(np.array(list(col), dtype=object).reshape(-1, 1))
        ins.append(x)
    return ins


def _client(served, kind):
    import tritonclient.grpc as grpcclient
    import tritonclient.http as httpclient

    mod = httpclient if kind == "http" else grpcclient
    return mod, mod.InferenceServerClient(served.http_url if kind == "http" else served.grpc_url)


def _assert_rows(r, want, rows):
    ids, mask, tt, offsets, overflow, status = want
    assert not status.any()
    for name, a in (("input_ids", ids), ("attention_mask", mask), ("token_type_ids", tt), ("offsets", offsets)):
        got = r.as_numpy(name)
        assert got.dtype == np.int32 and got.shape == a[rows].shape, name
        np.testing.assert_array_equal(got, a[rows])
    assert r.as_numpy("overflow").shape == (len(ids[rows]), 1)
    np.testing.assert_array_equal(r.as_numpy("overflow").reshape(-1), overflow[rows])


@pytest.mark.parametrize("kind", ["http", "grpc"])
def test_bert_tokenizer_equals_the_python_twin(served, twin_vocab, kind):
    mod, c = _client(served, kind)
    assert c.is_model_ready("bert_tokenizer")
    want = wc.tokenize_rows(QS, CS, twin_vocab, 64)
    assert want[4][2] > 0  # the third context overflows
    _assert_rows(c.infer("bert_tokenizer", _inputs(mod, QS, CS)), want, slice(0, 4))
    _assert_rows(c.infer("bert_tokenizer", _inputs(mod, QS[1:2], CS[1:2])), want, slice(1, 2))
    want3 = wc.tokenize_rows(QS, CS, twin_vocab, 3)
    assert (want3[0] != want[0]).any()
    _assert_rows(c.infer("bert_tokenizer", _inputs(mod, QS, CS), parameters={"max_query_length": 3}), want3,
                 slice(0, 4))
    md = c.get_model_metadata("bert_tokenizer")
    names = [o["name"] for o in md["outputs"]] if kind == "http" else [o.name for o in md.outputs]
    assert names == ["input_ids", "attention_mask", "token_type_ids", "offsets", "overflow"]
    c.close()


def _request(questions, contexts, **parameters):
    from triton_client_amd.server.types import InferRequest, InputTensor

    ins = [InputTensor(nm, "BYTES", [len(col), 1], np.array(list(col), dtype=object).reshape(len(col), 1))
           for nm, col in (("question", questions), ("context", contexts))]
    return InferRequest(model_name="bert_tokenizer", parameters=parameters, inputs=ins)


def test_one_batch_of_different_parameters_and_one_invalid_request(served, twin_vocab):
    """What the dynamic batcher hands the model: requests of different
    ``max_query_length`` in one ``execute``; the invalid one fails alone."""
    from triton_client_amd.server.types import ServerError

    _, _, inst = served.server.get_instance("bert_tokenizer", "")
    reqs = [_request(QS[:2], CS[:2]), _request(QS[2:3], CS[2:3], max_query_length=2),
            _request([b"fine", b"ab\xed\xa0\x80"], [b"fine", b"fine"]), _request(QS[3:], CS[3:], max_query_length=381),
            _request([b"q"], [b"x" * 65537]), _request([b"q" * 65537], [b"x"]), _request([b"q"], [b"\xc3"])]
    res = inst.execute(reqs)
    for k, (rows, mq) in {0: (slice(0, 2), 64), 1: (slice(2, 3), 2), 3: (slice(3, 4), 381)}.items():
        want = wc.tokenize_rows(QS[rows], CS[rows], twin_vocab, mq)
        assert [o.name for o in res[k]] == ["input_ids", "attention_mask", "token_type_ids", "offsets", "overflow"]
        for o, a in zip(res[k][:4], want[:4]):
            np.testing.assert_array_equal(o.data, a)
        np.testing.assert_array_equal(np.asarray(res[k][4].data).reshape(-1), want[4])
    assert all(isinstance(res[k], ServerError) for k in (2, 4, 5, 6))
    assert res[2].msg == "bert_tokenizer: question is not valid UTF-8 at byte 2"
    assert res[4].msg == "bert_tokenizer: context too long"
    assert res[5].msg == "bert_tokenizer: question too long"
    assert res[6].msg == "bert_tokenizer: context is not valid UTF-8 at byte 0"


def test_an_invalid_request_fails_over_the_wire_with_its_message(served):
    from tritonclient.utils import InferenceServerException

    mod, c = _client(served, "http")
    with pytest.raises(InferenceServerException, match="bert_tokenizer: context is not valid UTF-8 at byte 4"):
        c.infer("bert_tokenizer", _inputs(mod, [b"ok"], [b"abc \xf4\x90\x80\x80"]))
    r = c.infer("bert_tokenizer", _inputs(mod, [b"ok"], [b"abc"]))  # the server goes on
    assert r.as_numpy("attention_mask").sum() == 8  # [CLS] o ##k [SEP] a ##b ##c [SEP]
    c.close()


@pytest.mark.parametrize("value", [0, 382, -1, "64", 1.5, True])
def test_parameter_checks(served, value):
    from tritonclient.utils import InferenceServerException

    mod, c = _client(served, "http")
    with pytest.raises(InferenceServerException, match=r"max_query_length must be an int64 in \[1, 381\]"):
        c.infer("bert_tokenizer", _inputs(mod, [b"a"], [b"b"]), parameters={"max_query_length": value})
    c.close()


def test_question_and_context_must_pair_up(served):
    from triton_client_amd.server.types import ServerError

    _, _, inst = served.server.get_instance("bert_tokenizer", "")
    res = inst.execute([_request([b"a", b"b"], [b"c"])])
    assert isinstance(res[0], ServerError) and "one element per row" in res[0].msg


def test_the_vocabulary_comes_from_the_environment(monkeypatch, tmp_path):
    from triton_client_amd.server.cpu_models import BertTokenizer
    from triton_client_amd.server.types import ServerError
    from triton_client_amd.utils import wordpiece

    monkeypatch.delenv("TCAMD_BERT_VOCAB", raising=False)
    m = BertTokenizer()
    m.load()
    assert m.vocab_path == wordpiece.DEMO_VOCAB and len(m.vocab.pieces) > 1000
    monkeypatch.setenv("TCAMD_BERT_VOCAB", wc.VOCAB_SMALL)
    m = BertTokenizer()
    m.load()
    assert m.vocab_path == wc.VOCAB_SMALL and len(m.vocab.pieces) == len(wc.TwinVocab().pieces)
    bad = tmp_path / "vocab.txt"
    bad.write_text("[PAD]\n[UNK]\n[CLS]\nword\n")
    monkeypatch.setenv("TCAMD_BERT_VOCAB", str(bad))
    with pytest.raises(ServerError, match=r"lacks \[SEP\]"):
        BertTokenizer().load()
    monkeypatch.setenv("TCAMD_BERT_VOCAB", str(tmp_path / "missing.txt"))
    with pytest.raises(ServerError, match="cannot load the vocabulary"):
        BertTokenizer().load()


def test_the_models_are_registered_and_the_ensemble_is_declared_over_the_tokenizer():
    from triton_client_amd.server.app import default_models
    from triton_client_amd.server.cpu_models import CPU_MODELS

    assert "bert_tokenizer" in [m.name for m in CPU_MODELS]
    assert "bert_large" not in [m.name for m in CPU_MODELS]  # hence no text ensemble on a CPU server
    assert "bert_tokenizer" in [m.name for m in default_models()]
    gpu_models = pytest.importorskip("triton_client_amd.server.gpu_models")
    names = [m.name for m in gpu_models.GPU_MODELS]
    assert "bert_tokenizer" in names and "bert_qa_text_ensemble" in names
    ens = gpu_models.BertQaTextEnsemble
    assert [s[0] for s in ens.ensemble_steps] == ["bert_tokenizer", "bert_large", "qa_spans"]
    assert [t.name for t in ens.inputs] == ["question", "context"]
    assert [t.name for t in ens.outputs] == ["spans", "scores", "null_score", "offsets", "overflow", "input_ids",
                                             "attention_mask", "token_type_ids", "start_logits", "end_logits"]


def test_answer_text():
    from triton_client_amd.utils.qa import answer_text

    ctx = "The café is in 中国.".encode()
    ids, mask, tt, offsets, _, _ = wc.tokenize_rows([b"where"], [ctx], wc.TwinVocab(), 64)
    first = int(tt[0].argmax())
    assert answer_text(ctx, (first, first), offsets[0]) == b"The"
    assert answer_text(ctx, (first + 1, first + 1), offsets[0]).decode() == "café"  # one piece, "cafe"
    assert answer_text(ctx, (first + 1, first + 2), offsets[0]).decode() == "café is"
    assert answer_text(ctx, (-1, -1), offsets[0]) == b""
    last = first + int(tt[0].sum()) - 1
    assert answer_text(ctx, (first, last), offsets[0]) == ctx

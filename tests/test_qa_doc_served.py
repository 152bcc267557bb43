"""``bert_window_tokenizer``, ``qa_doc_spans`` and ``bert_qa_doc_ensemble`` on
the in-process CPU server (the host twins of K28w, K27 with a start mask and
K29 behind server/cpu_models.py): against the Python twin of
tests/wordpiece_window_cases.py and ``utils.qa.merge_windows``, the parameter
checks, the per-document messages, and an answer that lies wholly behind the
first row's end.

The CPU zoo has no ``bert_large``; the ensembles here run over a stand-in of
that name whose logits are a fixed function of the token ids, so a piece scores
the same in every window that holds it and the merge has ties to break."""

import numpy as np
import pytest

from tests import wordpiece_cases as wc
from tests import wordpiece_window_cases as ww

ANSWER = b"unaffable kernel devices"
QUESTION = b"What is tokenization?"
CONTEXT = b"b " * 600 + ANSWER + b" a" * 40


def _bert_stand_in():
    from triton_client_amd.server.cpu_models import BertSink

    vocab = wc.TwinVocab()
    pieces, _ = wc.tokenize_text(ANSWER, vocab)
    first, last = pieces[0][0], pieces[-1][0]

    class BertStandIn(BertSink):
        """``bert_large``'s contract; start peaks on the answer's first piece, end on its last."""

        name = "bert_large"
        max_batch_size = 128
        supports_native = False

        def execute(self, requests):
            out = []
            for r in requests:
                ids = r.input("input_ids").numpy().astype(np.int64)
                noise = ((ids * 2654435761) % 7).astype(np.float32) * 0.125
                start = noise + np.where(ids == first, 9.0, 0.0).astype(np.float32)
                end = noise + np.where(ids == last, 9.0, 0.0).astype(np.float32)
                out.append([self.out("start_logits", start.astype(np.float32)),
                            self.out("end_logits", end.astype(np.float32))])
            return out

    return BertStandIn


@pytest.fixture(scope="module")
def served():
    from triton_client_amd.server import ServerHandle
    from triton_client_amd.server.cpu_models import BertTokenizer, BertWindowTokenizer, QaDocSpans, QaSpans

    gpu_models = pytest.importorskip("triton_client_amd.server.gpu_models")
    mp = pytest.MonkeyPatch()
    mp.setenv("TCAMD_BERT_VOCAB", wc.VOCAB_SMALL)
    h = ServerHandle(models=[BertWindowTokenizer, QaDocSpans, _bert_stand_in(), BertTokenizer, QaSpans,
                             gpu_models.BertQaDocEnsemble, gpu_models.BertQaTextEnsemble], native_grpc=False).start()
    mp.undo()
    yield h
    h.stop()


@pytest.fixture(scope="module")
def client(served):
    import tritonclient.http as httpclient

    c = httpclient.InferenceServerClient(served.http_url)
    yield httpclient, c
    c.close()


def _doc_inputs(mod, questions, contexts):
    ins = []
    for name, col in (("question", questions), ("context", contexts)):
        x = mod.InferInput(name, [len(col)], "BYTES")
        x.set_data_from_numpy(np.array(list(col), dtype=object))
        ins.append(x)
    return ins


def test_bert_window_tokenizer_equals_the_python_twin(client):
    mod, c = client
    qs = [QUESTION, "Σσ привет".encode(), b"", b"a"]
    cs = [CONTEXT, ww.long_context(3000, 5), b"walked", b""]
    for params, (mq, ds, mw) in (({}, (64, 128, 128)),
                                 ({"max_query_length": 3, "doc_stride": 50, "max_windows": 40}, (3, 50, 40))):
        want, pieces_of = ww.window_rows(qs, cs, wc.TwinVocab(), mq, ds, mw, 384, 128)
        n = want[7]
        assert not want[6][:, 3].any() and n > 6
        r = c.infer("bert_window_tokenizer", _doc_inputs(mod, qs, cs), parameters=params)
        for name, a in zip(("input_ids", "attention_mask", "token_type_ids", "start_mask", "offsets", "window_info"),
                           want[:6]):
            got = r.as_numpy(name)
            assert got.dtype == np.int32 and got.shape == a[:n].shape, name
            np.testing.assert_array_equal(got, a[:n])
        np.testing.assert_array_equal(r.as_numpy("doc_info"), want[6].view(np.int32))
    md = c.get_model_metadata("bert_window_tokenizer")
    assert [o["name"] for o in md["outputs"]] == ["input_ids", "attention_mask", "token_type_ids", "start_mask",
                                                  "offsets", "window_info", "doc_info"]
    assert c.get_model_config("bert_window_tokenizer").get("max_batch_size", 0) == 0


@pytest.mark.parametrize("name,value,lo,hi", [
    ("doc_stride", 0, 1, 381), ("doc_stride", 382, 1, 381), ("doc_stride", "128", 1, 381), ("doc_stride", True, 1, 381),
    ("max_windows", 0, 1, 128), ("max_windows", 129, 1, 128), ("max_windows", 1.5, 1, 128),
    ("max_query_length", 0, 1, 381), ("max_query_length", 382, 1, 381)])
def test_parameter_checks(client, name, value, lo, hi):
    from tritonclient.utils import InferenceServerException

    mod, c = client
    for model in ("bert_window_tokenizer", "bert_qa_doc_ensemble"):
        with pytest.raises(InferenceServerException, match=r"%s must be an int64 in \[%d, %d\]" % (name, lo, hi)):
            c.infer(model, _doc_inputs(mod, [b"a"], [b"b"]), parameters={name: value})


@pytest.mark.parametrize("name,value,lo,hi", [("n_best", 0, 1, 64), ("n_best", 65, 1, 64),
                                              ("max_answer_length", 0, 1, 384), ("max_answer_length", "30", 1, 384)])
def test_parameter_checks_of_the_span_step(client, name, value, lo, hi):
    from tritonclient.utils import InferenceServerException

    mod, c = client
    with pytest.raises(InferenceServerException, match=r"%s must be an int64 in \[%d, %d\]" % (name, lo, hi)):
        c.infer("bert_qa_doc_ensemble", _doc_inputs(mod, [b"a"], [b"b"]), parameters={name: value})


def test_per_document_messages(client):
    from tritonclient.utils import InferenceServerException

    mod, c = client

    def fails(match, qs, cs, **params):
        with pytest.raises(InferenceServerException, match=match):
            c.infer("bert_window_tokenizer", _doc_inputs(mod, qs, cs), parameters=params)

    fails("bert_window_tokenizer: document 1: context is not valid UTF-8 at byte 2", [b"a", b"a", b"a"],
          [b"fine", b"a \xed\xa0\x80", b"fine"])
    fails("bert_window_tokenizer: document 0: question is not valid UTF-8 at byte 0", [b"\xc3"], [b"fine"])
    fails("bert_window_tokenizer: document 2: context too long", [b"a"] * 3, [b"b", b"b", b"x" * 65537])
    # 641 context pieces, cap 378 (a question of 3 pieces): ceil(263 / 128) + 1 = 4 windows
    fails("bert_window_tokenizer: document 1: context needs 4 windows, max_windows 3", [b"a", b"a b c"],
          [b"b", CONTEXT[:1282]], max_windows=3)
    # at stride 8: ceil(263 / 8) + 1 = 34 windows a document; the fourth does not fit 128 rows
    fails("bert_window_tokenizer: document 3: context needs 34 windows, exceeds 128 rows", [b"a b c"] * 4,
          [CONTEXT[:1282]] * 4, doc_stride=8)
    fails("one element per document", [b"a", b"b"], [b"c"])
    fails("1 to 128 documents", [b"a"] * 129, [b"c"] * 129)
    r = c.infer("bert_window_tokenizer", _doc_inputs(mod, [b"ok"], [b"abc"]))  # the server goes on
    assert r.as_numpy("attention_mask").sum() == 8 and r.as_numpy("doc_info").tolist() == [[0, 1, 3, 0]]


def test_an_answer_behind_the_first_row_is_found(client):
    """The answer starts at context piece 600; ``bert_qa_text_ensemble`` sees
    pieces 0 .. 375 of it only."""
    from triton_client_amd.utils.qa import answer_text, answer_text_doc, merge_windows

    mod, c = client
    ins = _doc_inputs(mod, [QUESTION, b"a"], [CONTEXT, b"b a"])
    r = c.infer("bert_qa_doc_ensemble", ins, parameters={"n_best": 5})
    spans, windows, scores = r.as_numpy("spans"), r.as_numpy("windows"), r.as_numpy("scores")
    assert spans.shape == (2, 5, 2) and windows.shape == (2, 5) and scores.shape == (2, 5)
    assert r.as_numpy("null_score").shape == (2,)
    dinfo, winfo, offsets = r.as_numpy("doc_info"), r.as_numpy("window_info"), r.as_numpy("offsets")
    assert dinfo[0, 1] > 2 and dinfo[1].tolist() == [int(dinfo[0, 1]), 1, 2, 0]
    w = int(windows[0, 0])
    assert 0 <= w < dinfo[0, 1] and winfo[w, 0] == 0
    assert answer_text_doc(CONTEXT, spans[0, 0], w, offsets) == ANSWER
    assert scores[0, 0] > 18 and scores[0, 1] < scores[0, 0]
    # the client's route over the logits the ensemble returned gives the same answers
    got = merge_windows(r.as_numpy("start_logits"), r.as_numpy("end_logits"), r.as_numpy("attention_mask"),
                        r.as_numpy("token_type_ids"), r.as_numpy("start_mask"), winfo, dinfo, 5, 30)
    np.testing.assert_array_equal(got[0], spans)
    np.testing.assert_array_equal(got[1], windows)
    assert got[2].tobytes() == scores.tobytes() and got[3].tobytes() == r.as_numpy("null_score").tobytes()
    # the one-row ensemble on the same document: the context is cut, the answer out of reach
    ins1 = []
    for name, text in (("question", QUESTION), ("context", CONTEXT)):
        x = mod.InferInput(name, [1, 1], "BYTES")
        x.set_data_from_numpy(np.array([[text]], dtype=object))
        ins1.append(x)
    r1 = c.infer("bert_qa_text_ensemble", ins1, parameters={"n_best": 5})
    assert r1.as_numpy("overflow")[0, 0] > 0
    assert r1.as_numpy("offsets")[0].max() < CONTEXT.index(ANSWER)
    assert all(ANSWER not in answer_text(CONTEXT, s, r1.as_numpy("offsets")[0]) for s in r1.as_numpy("spans")[0])
    assert r1.as_numpy("scores")[0, 0] < 9


def test_only_what_was_asked_for_comes_back(client):
    mod, c = client
    outs = [mod.InferRequestedOutput("spans"), mod.InferRequestedOutput("windows")]
    r = c.infer("bert_qa_doc_ensemble", _doc_inputs(mod, [QUESTION], [CONTEXT]), outputs=outs)
    assert r.as_numpy("spans").shape == (1, 20, 2) and r.as_numpy("start_logits") is None


def test_qa_doc_spans_checks_its_shapes(served):
    from triton_client_amd.server.types import InferRequest, InputTensor, ServerError

    _, _, inst = served.server.get_instance("qa_doc_spans", "")
    W, S = 3, 384

    def request(**over):
        shapes = {"start_logits": ("FP32", [W, S]), "end_logits": ("FP32", [W, S]), "attention_mask": ("INT32", [W, S]),
                  "token_type_ids": ("INT32", [W, S]), "start_mask": ("INT32", [W, S]), "window_info": ("INT32", [W, 4]),
                  "doc_info": ("INT32", [1, 4])}
        shapes.update(over)
        ins = [InputTensor(nm, dt, sh, np.zeros(sh, np.float32 if dt == "FP32" else np.int32))
               for nm, (dt, sh) in shapes.items()]
        return InferRequest(model_name="qa_doc_spans", inputs=ins)

    res = inst.execute([request(), request(start_mask=("INT32", [W - 1, S])), request(window_info=("INT32", [W + 1, 4]))])
    assert [o.name for o in res[0]] == ["spans", "windows", "scores", "null_score"]
    assert res[0][0].data.shape == (1, 20, 2) and (res[0][1].data == -1).all()  # doc_info says no windows
    assert isinstance(res[1], ServerError) and "start_mask must be [3, 384]" in res[1].msg
    assert isinstance(res[2], ServerError) and "window_info must be [3, 4]" in res[2].msg


def test_the_models_are_registered_and_the_ensemble_is_declared():
    from triton_client_amd.server.app import default_models
    from triton_client_amd.server.cpu_models import CPU_MODELS

    names = [m.name for m in CPU_MODELS]
    assert "bert_window_tokenizer" in names and "qa_doc_spans" in names
    assert {"bert_window_tokenizer", "qa_doc_spans"} <= {m.name for m in default_models()}
    gpu_models = pytest.importorskip("triton_client_amd.server.gpu_models")
    names = [m.name for m in gpu_models.GPU_MODELS]
    assert {"bert_window_tokenizer", "qa_doc_spans", "bert_qa_doc_ensemble"} <= set(names)
    ens = gpu_models.BertQaDocEnsemble
    assert ens.max_batch_size == 0
    assert [s[0] for s in ens.ensemble_steps] == ["bert_window_tokenizer", "bert_large", "qa_doc_spans"]
    assert [t.name for t in ens.inputs] == ["question", "context"]
    assert [t.name for t in ens.outputs] == ["spans", "windows", "scores", "null_score", "offsets", "window_info",
                                             "doc_info", "input_ids", "attention_mask", "token_type_ids", "start_mask",
                                             "start_logits", "end_logits"]


@pytest.mark.parametrize("proto", ["http", "grpc"])
def test_example_check_passes(served, proto):
    from tests.test_examples import run_example

    r = run_example("bert_qa_doc_client.py", served.http_url if proto == "http" else served.grpc_url,
                    ["-i", proto, "--n-best", "5", "--doc-stride", "64", "--vocab", wc.VOCAB_SMALL, "--check"])
    assert r.returncode == 0 and r.stdout.rstrip().endswith("PASS"), r.stdout[-1500:] + r.stderr[-1500:]
    assert "in 1 windows" not in r.stdout and r.stdout.count("rank  window  start  end  score") == 1

"""``embed_search`` and ``bert_search_text_ensemble`` served in process (``bert_large_embed`` at
layers=2, a 300-row corpus).  ``DeviceView`` inputs are what a registered HIP shm region is to the model."""

import numpy as np
import pytest

from tests import wordpiece_cases as wc

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

TEXTS = ["The quick brown fox jumps over the lazy dog.".encode(), "Привет мир! 中国 tokenization, café.".encode()]


def _unit(n, seed):
    x = np.random.default_rng(seed).standard_normal((n, 1024))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


CORPUS, QUERIES = _unit(300, 11), _unit(3, 12)


@pytest.fixture(scope="module")
def served():
    from triton_client_amd.server import ServerHandle
    from triton_client_amd.server.gpu_models import BertLargeEmbed, BertSearchTextEnsemble, BertTokenizer, EmbedSearch

    mp = pytest.MonkeyPatch()
    mp.setenv("TCAMD_BERT_VOCAB", wc.VOCAB_SMALL)
    h = ServerHandle(models=[BertTokenizer, BertLargeEmbed, EmbedSearch, BertSearchTextEnsemble],
                     model_options={"bert_large_embed": {"layers": 2}, "embed_search": {"corpus": CORPUS}},
                     native_grpc=False).start()
    mp.undo()
    yield h
    h.stop()


def _request(q, device=False, **parameters):
    from triton_client_amd.server.types import DeviceView, InferRequest, InputTensor

    keep = torch.from_numpy(q).cuda() if device else None
    r = InferRequest(model_name="embed_search", parameters=parameters,
                     inputs=[InputTensor("embedding", "FP32", list(q.shape),
                                         DeviceView(keep.data_ptr(), q.nbytes, 0) if device else q)])
    r.keep = keep  # the device tensor lives as long as the request
    return r


def _direct(inst, q, k):  # K33 called directly on the model's index: (indices, scores) [rows, k]
    from triton_client_amd.ops import hip

    qd, kd = torch.from_numpy(q).cuda(), torch.full((len(q),), k, dtype=torch.int32, device="cuda")
    ws = torch.zeros(hip.search_workspace(len(q), inst.corpus_rows), dtype=torch.uint8, device="cuda")
    idx, sc = (torch.zeros((len(q), k), dtype=dt, device="cuda") for dt in (torch.int32, torch.float32))
    hip.search_topk(qd.data_ptr(), 4096, len(q), inst.index[0].data_ptr(), inst.index[1].data_ptr(), inst.corpus_rows,
                    1024, kd.data_ptr(), k, ws.data_ptr(), idx.data_ptr(), sc.data_ptr())
    torch.cuda.synchronize()
    return idx.cpu().numpy(), sc.cpu().numpy()


def _infer(served, model, cols, names, datatype, **kw):
    import tritonclient.http as httpclient

    ins = [httpclient.InferInput(nm, list(np.shape(a)), datatype) for nm, a in zip(names, cols)]
    for i, a in zip(ins, cols):
        i.set_data_from_numpy(a)
    c = httpclient.InferenceServerClient(served.http_url)
    try:
        return c.infer(model, ins, **kw)
    finally:
        c.close()


def test_host_and_device_inputs_give_the_same_rows(served):
    _, _, inst = served.server.get_instance("embed_search", "")
    host, dev = inst.execute([_request(QUERIES)])[0], inst.execute([_request(QUERIES, device=True)])[0]
    want = _direct(inst, QUERIES, 10)  # the default top_k
    for res in (host, dev):
        assert [o.name for o in res] == ["indices", "scores"] and res[0].data.dtype == np.int32
        np.testing.assert_array_equal(res[0].data, want[0])
        np.testing.assert_array_equal(res[1].data, want[1])
    np.testing.assert_array_equal(want[0][:, 0], (QUERIES.astype(np.float64) @ CORPUS.astype(np.float64).T).argmax(1))


def test_requests_of_different_top_k_share_a_launch_and_a_bad_one_fails_alone(served):
    from triton_client_amd.server.types import ServerError

    _, _, inst = served.server.get_instance("embed_search", "")
    res = inst.execute([_request(QUERIES[:1], top_k=1), _request(QUERIES[1:], top_k=64), _request(QUERIES, top_k=0)])
    assert isinstance(res[2], ServerError) and "top_k" in res[2].msg
    for got, q, k in ((res[0], QUERIES[:1], 1), (res[1], QUERIES[1:], 64)):
        want = _direct(inst, q, k)
        np.testing.assert_array_equal(got[0].data, want[0])
        np.testing.assert_array_equal(got[1].data, want[1])


def test_text_ensemble_equals_its_steps(served):
    texts = [np.array(col, dtype=object).reshape(-1, 1) for col in ([b""] * len(TEXTS), TEXTS)]
    par = {"pooling": "cls", "top_k": 7}
    ens = _infer(served, "bert_search_text_ensemble", texts, ("question", "context"), "BYTES", parameters=par)
    names = ("input_ids", "attention_mask", "token_type_ids")
    tok = _infer(served, "bert_tokenizer", texts, ("question", "context"), "BYTES")
    emb = _infer(served, "bert_large_embed", [tok.as_numpy(nm) for nm in names], names, "INT32",
                 parameters={"pooling": "cls"}).as_numpy("embedding")
    step = _infer(served, "embed_search", [emb], ("embedding",), "FP32", parameters={"top_k": 7})
    assert ens.as_numpy("indices").shape == (2, 7) and ens.as_numpy("indices").min() >= 0
    np.testing.assert_array_equal(ens.as_numpy("embedding"), emb)
    np.testing.assert_array_equal(ens.as_numpy("indices"), step.as_numpy("indices"))
    np.testing.assert_array_equal(ens.as_numpy("scores"), step.as_numpy("scores"))


def test_the_corpus_comes_from_the_environment(tmp_path, monkeypatch):
    from triton_client_amd.server.gpu_models import EmbedSearch

    np.save(tmp_path / "corpus.npy", CORPUS[:70][::-1])
    monkeypatch.setenv("TCAMD_SEARCH_CORPUS", str(tmp_path / "corpus.npy"))
    m = EmbedSearch()
    m.load()
    try:
        assert m.corpus_rows == 70
        res = m.execute([_request(CORPUS[:2], top_k=1)])[0]
        np.testing.assert_array_equal(res[0].data, [[69], [68]])
    finally:
        m.unload()


def test_a_batch_that_needs_more_workspace_than_the_largest_one():
    """112 rows over 2,100 corpus rows run 33 slices (128 rows: 17): the most key lists of any batch."""
    from triton_client_amd.server.gpu_models import EmbedSearch

    m, q = EmbedSearch(corpus=_unit(2100, 13)), _unit(112, 14)
    m.load()
    try:
        got, want = m.execute([_request(q, top_k=64)])[0], _direct(m, q, 64)
        np.testing.assert_array_equal(got[0].data, want[0])  # [112, 64]
        np.testing.assert_array_equal(got[1].data, want[1])
    finally:
        m.unload()

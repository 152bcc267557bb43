"""``bert_large_embed`` and ``bert_embed_text_ensemble`` served in process
(layers=2).  Inputs in device memory arrive as ``DeviceView``, which is what a
registered HIP shm region is to the model."""

import numpy as np
import pytest

from tests import wordpiece_cases as wc

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

NAMES = ("input_ids", "attention_mask", "token_type_ids")
TEXTS = ["The quick brown fox jumps over the lazy dog.".encode(), "Привет мир! 中国 tokenization, café.".encode()]


@pytest.fixture(scope="module")
def served():
    from triton_client_amd.server import ServerHandle
    from triton_client_amd.server.gpu_models import BertEmbedTextEnsemble, BertLargeEmbed, BertTokenizer

    mp = pytest.MonkeyPatch()
    mp.setenv("TCAMD_BERT_VOCAB", wc.VOCAB_SMALL)
    h = ServerHandle(models=[BertTokenizer, BertLargeEmbed, BertEmbedTextEnsemble],
                     model_options={"bert_large_embed": {"layers": 2}}, native_grpc=False).start()
    mp.undo()
    yield h
    h.stop()


@pytest.fixture(scope="module")
def rows():
    """(ids, mask, type ids) int32 [2, 384]: a full row and one of 100 tokens."""
    ids = np.random.default_rng(5).integers(1000, 30000, size=(2, 384), dtype=np.int32)
    mask = (np.arange(384)[None] < np.array([[384], [100]])).astype(np.int32)
    return ids, mask, np.zeros((2, 384), dtype=np.int32)


def _request(arrays, device=False, **parameters):
    from triton_client_amd.server.types import DeviceView, InferRequest, InputTensor

    keep = [torch.from_numpy(a).cuda() for a in arrays] if device else []
    ins = [InputTensor(nm, "INT32", list(a.shape), DeviceView(keep[k].data_ptr(), a.nbytes, 0) if device else a)
           for k, (nm, a) in enumerate(zip(NAMES, arrays))]
    r = InferRequest(model_name="bert_large_embed", parameters=parameters, inputs=ins)
    r.keep = keep  # the device tensors live as long as the request
    return r


def _infer(served, model, cols, **kw):
    """One HTTP request: ``cols`` = the three id arrays, or (questions, contexts)."""
    import tritonclient.http as httpclient

    ins = []
    for nm, a in zip(NAMES if len(cols) == 3 else ("question", "context"), cols):
        a = a if len(cols) == 3 else np.array(a, dtype=object).reshape(-1, 1)
        ins.append(httpclient.InferInput(nm, list(a.shape), "INT32" if len(cols) == 3 else "BYTES"))
        ins[-1].set_data_from_numpy(a)
    c = httpclient.InferenceServerClient(served.http_url)
    try:
        return c.infer(model, ins, **kw)
    finally:
        c.close()


def test_host_and_device_inputs_give_the_same_unit_vectors(served, rows):
    _, _, inst = served.server.get_instance("bert_large_embed", "")
    wire = _infer(served, "bert_large_embed", rows).as_numpy("embedding")
    dev = inst.execute([_request(rows, device=True)])[0][0]
    assert wire.shape == (2, 1024) and wire.dtype == np.float32 and dev.name == "embedding"
    np.testing.assert_array_equal(wire, np.asarray(dev.data).reshape(2, 1024))
    np.testing.assert_allclose(np.linalg.norm(wire.astype(np.float64), axis=1), 1.0, rtol=0, atol=1e-6)


def test_requests_of_different_pooling_share_a_batch_and_a_bad_one_fails_alone(served, rows):
    from triton_client_amd.server.types import ServerError

    _, _, inst = served.server.get_instance("bert_large_embed", "")
    one = [a[1:2] for a in rows]
    res = inst.execute([_request(one), _request(one, pooling="max"), _request(one, pooling="cls", normalize=False)])
    assert isinstance(res[1], ServerError) and "pooling must be" in res[1].msg
    got = np.stack([np.asarray(res[k][0].data).reshape(1024) for k in (0, 2)])
    two = [torch.from_numpy(np.concatenate([a, a])).cuda() for a in one]
    with torch.no_grad():
        want = inst.model.embed(two[0].long(), two[1], two[2].long(), flags=[0, 3]).cpu().numpy()
    np.testing.assert_array_equal(got, want)  # the same 2-row bucket, eager: each row by its own flags
    assert np.abs(got[0] - got[1]).max() > 1e-3 and abs(np.linalg.norm(got[1]) - 1) > 1e-2


def test_text_ensemble_equals_its_steps(served):
    texts = ([b""] * len(TEXTS), TEXTS)  # a single text: the context of an empty question
    ens = _infer(served, "bert_embed_text_ensemble", texts, parameters={"pooling": "cls"})
    tok = _infer(served, "bert_tokenizer", texts)
    ids = [tok.as_numpy(nm) for nm in NAMES]
    assert (ids[0][:, :2] == ids[0][0, :2]).all() and (ids[1].sum(1) > 5).all()  # [CLS] [SEP] text [SEP]
    step = _infer(served, "bert_large_embed", ids, parameters={"pooling": "cls"})
    got = ens.as_numpy("embedding")
    assert got.shape == (2, 1024) and np.isfinite(got).all()
    np.testing.assert_array_equal(got, step.as_numpy("embedding"))

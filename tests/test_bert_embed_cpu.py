"""``BertLargeQA.embed`` off the GPU (the torch path, 1 layer, fp32) against
the pooling formula in numpy over the model's own last hidden state, with the
all-zero-mask and CLS rules; and the served model's parameter check."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")


def pool_ref(h, mask, flags):
    """fp64: masked mean (zeros without a token) or token 0 (flag 1), over the L2 norm unless flag 2 or norm 0."""
    h = h.astype(np.float64)
    out = np.zeros((h.shape[0], h.shape[2]))
    for r in range(h.shape[0]):
        valid = mask[r] >= 1
        e = h[r, 0] if flags[r] & 1 else (h[r, valid].sum(0) / valid.sum() if valid.any() else out[r])
        norm = np.sqrt((e * e).sum())
        out[r] = e if flags[r] & 2 or norm == 0 else e / norm
    return out


@pytest.mark.parametrize("flags", [None, [0, 1, 2, 3, 0]])
def test_embed_cpu_matches_the_formula(flags):
    from triton_client_amd.models import bert

    m = bert.build(device="cpu", dtype=torch.float32, layers=1)
    ids = torch.randint(0, bert.VOCAB, (5, 16), generator=torch.Generator().manual_seed(1))
    mask = torch.ones(5, 16, dtype=torch.int32)
    mask[1, 10:] = 0
    mask[2, ::3] = 0
    mask[4] = 0  # no valid token: zeros, no NaN
    tt = torch.zeros(5, 16, dtype=torch.long)
    with torch.no_grad():
        x = m._embed(ids, tt)
        bias = (1.0 - mask[:, None, None, :].float()) * -10000.0
        h = m.layers[0](x, bias).numpy()
        e = m.embed(ids, mask, tt, flags=flags).numpy()
    assert e.shape == (5, 1024) and e.dtype == np.float32
    want = pool_ref(h, mask.numpy(), flags or [0] * 5)
    # an fp32 sum of <= 16 values of |h| ~ 1: 15 x 2^-24 x ~1, then a division and a scale: ~1e-6
    np.testing.assert_allclose(e, want, rtol=0, atol=2e-6)
    assert not e[4].any()


@pytest.mark.parametrize("parameters, want", [
    ({}, 0), ({"pooling": "mean", "normalize": True}, 0), ({"pooling": "cls"}, 1), ({"normalize": False}, 2),
    ({"pooling": "cls", "normalize": False, "max_query_length": 8}, 3), ({"pooling": "max"}, None), ({"pooling": 1}, None),
    ({"pooling": b"cls"}, None), ({"normalize": 1}, None), ({"normalize": "true"}, None)])
def test_request_flags(parameters, want):
    gpu_models = pytest.importorskip("triton_client_amd.server.gpu_models")
    from triton_client_amd.server.types import ServerError

    if want is not None:
        assert gpu_models.BertLargeEmbed.request_flags(parameters) == want
        return
    with pytest.raises(ServerError, match="request parameter (pooling|normalize) must be"):
        gpu_models.BertLargeEmbed.request_flags(parameters)

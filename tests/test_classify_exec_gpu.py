"""GPU test of classification in the native batch executor
(csrc/runtime/graph_exec.hip): TcBatch.class_counts makes it answer a request
with the {score, index} pairs K19 topk_rows selected on the device (k <= 64)
or the host routine selected from the full logits (k > 64), next to raw
requests of the same batch."""

import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

PAIR = np.dtype([("score", np.uint32), ("index", np.int32)])


@pytest.fixture(scope="module")
def model():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from triton_client_amd.server.gpu_models import DensenetOnnx

    m = DensenetOnnx(engine="fp32", max_batch_size=8)
    m.instance_count = 2
    m.load()
    yield m
    m.unload()


def _topk(logits, k):
    """numpy reference pairs [rows, k] of fp32 logits [rows, C]."""
    out = np.zeros((logits.shape[0], k), dtype=PAIR)
    for r, row in enumerate(logits):
        idx = np.argsort(-row, kind="stable")[:k]
        out[r]["score"] = row[idx].view(np.uint32)
        out[r]["index"] = idx
    return out


@pytest.mark.parametrize("instance", [0, 1])
def test_executor_mixed_classification_and_raw(model, instance):
    from triton_client_amd.server.native_frontend import TcBatch, TcRef

    assert model.native_topk
    dev = torch.device("cuda", 0)
    x = torch.randn(5, 3, 224, 224, generator=torch.Generator().manual_seed(21 + instance))
    xd = x[:2].to(dev).contiguous()                 # request 0: 2 rows, device input, k = 3
    xr = np.ascontiguousarray(x[2:3].numpy())       # request 1: 1 row, raw logits into a host buffer
    xh = np.ascontiguousarray(x[3:].numpy())        # request 2: 2 rows, host input, k = 70 (host fallback)
    p3 = np.full((2, 3), 0xFF, dtype=PAIR)
    raw = np.full((1, 1000), np.nan, dtype=np.float32)
    p70 = np.full((2, 70), 0xFF, dtype=PAIR)
    torch.cuda.synchronize()
    ins = (TcRef * 3)(TcRef(1, 0, xd.data_ptr(), xd.numel() * 4), TcRef(0, 0, xr.ctypes.data, xr.nbytes),
                      TcRef(0, 0, xh.ctypes.data, xh.nbytes))
    outs = (TcRef * 3)(TcRef(0, 0, p3.ctypes.data, p3.nbytes), TcRef(0, 0, raw.ctypes.data, raw.nbytes),
                       TcRef(0, 0, p70.ctypes.data, p70.nbytes))
    nrows = (ctypes.c_int32 * 3)(2, 1, 2)
    counts = (ctypes.c_int32 * 3)(3, 0, 70)
    timing = (ctypes.c_uint64 * 3)()
    b = TcBatch(3, 5, nrows, 1, ins, 1, outs, timing, counts)
    model._pgx.execute(instance, ctypes.addressof(b))
    # what the kernel saw: the instance's graph output buffer (the engine is not
    # bitwise reproducible between forwards, the buffer is)
    logits = model._slots[instance]["out"][:5].cpu().numpy()
    assert np.isfinite(logits).all()
    np.testing.assert_array_equal(p3, _topk(logits[:2], 3))
    np.testing.assert_array_equal(raw.view(np.uint32), logits[2:3].view(np.uint32))
    np.testing.assert_array_equal(p70, _topk(logits[3:], 70))
    assert timing[2] > 0


def test_executor_without_class_counts_keeps_raw_outputs(model):
    """The 8-value TcBatch constructor leaves class_counts NULL: raw outputs as before."""
    from triton_client_amd.server.native_frontend import TcBatch, TcRef

    x = torch.randn(2, 3, 224, 224, generator=torch.Generator().manual_seed(5)).cuda().contiguous()
    out = np.full((2, 1000), np.nan, dtype=np.float32)
    torch.cuda.synchronize()
    ins = (TcRef * 1)(TcRef(1, 0, x.data_ptr(), x.numel() * 4))
    outs = (TcRef * 1)(TcRef(0, 0, out.ctypes.data, out.nbytes))
    nrows = (ctypes.c_int32 * 1)(2)
    timing = (ctypes.c_uint64 * 3)()
    b = TcBatch(1, 2, nrows, 1, ins, 1, outs, timing)
    assert not b.class_counts
    model._pgx.execute(0, ctypes.addressof(b))
    logits = model._slots[0]["out"][:2].cpu().numpy()
    np.testing.assert_array_equal(out.view(np.uint32), logits.view(np.uint32))

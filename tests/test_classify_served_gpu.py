"""densenet_onnx answering the `classification` extension end to end on the
GPU server: HIP-shm input, class_count=5 over gRPC and REST (tcserve's native
path, device top-K by K19), against the raw logits of the same input."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROWS, K = 2, 5


@pytest.fixture(scope="module")
def hipshm():
    import torch

    torch.cuda.set_device(0)
    from tritonclient.utils import hip_shared_memory

    return hip_shared_memory


def test_densenet_classification_matches_raw_logits(gpu_server, hipshm):
    import tritonclient.grpc as grpcclient
    import tritonclient.http as httpclient

    x = np.random.default_rng(42).standard_normal((ROWS, 3, 224, 224)).astype(np.float32)
    hin = hipshm.create_shared_memory_region("cls_in", x.nbytes, 0)
    g = grpcclient.InferenceServerClient(gpu_server.grpc_url)
    h = httpclient.InferenceServerClient(gpu_server.http_url)
    try:
        hipshm.set_shared_memory_region(hin, [x])
        g.register_cuda_shared_memory("cls_in", hipshm.get_raw_handle(hin), 0, x.nbytes)
        gi = grpcclient.InferInput("data_0", list(x.shape), "FP32")
        gi.set_shared_memory("cls_in", x.nbytes)
        hi = httpclient.InferInput("data_0", list(x.shape), "FP32")
        hi.set_shared_memory("cls_in", x.nbytes)
        raw = g.infer("densenet_onnx", [gi], outputs=[grpcclient.InferRequestedOutput("fc6_1")]).as_numpy("fc6_1")
        assert raw.shape == (ROWS, 1000) and np.isfinite(raw).all()
        # two forwards of one input differ by float-atomic ordering only
        bound = 1e-4 * float(np.abs(raw).max())
        srt = np.sort(raw, axis=1)
        gap = srt[:, -1] - srt[:, -2]
        print("top-2 gaps", gap, "bound", bound)
        assert (gap > bound).all(), "pick another seed: top-2 gap %s within the noise bound %g" % (gap, bound)
        tops = {
            "grpc": g.infer("densenet_onnx", [gi],
                            outputs=[grpcclient.InferRequestedOutput("fc6_1", class_count=K)]).as_numpy("fc6_1"),
            "http": h.infer("densenet_onnx", [hi],
                            outputs=[httpclient.InferRequestedOutput("fc6_1", binary_data=True, class_count=K)]
                            ).as_numpy("fc6_1"),
        }
        for proto, top in tops.items():
            assert top.shape == (ROWS, K), proto
            for r in range(ROWS):
                scores = []
                for s in top[r]:
                    score, index, label = s.decode().split(":")
                    assert label == "class_%d" % int(index), (proto, s)
                    assert abs(float(score) - float(raw[r, int(index)])) <= bound, (proto, s, raw[r, int(index)])
                    scores.append(float(score))
                assert scores == sorted(scores, reverse=True), (proto, scores)
                assert int(top[r, 0].decode().split(":")[1]) == int(raw[r].argmax()), proto
    finally:
        g.unregister_cuda_shared_memory()
        hipshm.destroy_shared_memory_region(hin)
        g.close()
        h.close()

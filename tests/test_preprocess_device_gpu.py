"""The GPU ``preprocess_inception`` (server/gpu_models.py, K20 resize_pack):
in process against utils.image.preprocess in float64, and served as the first
step of ``preprocess_inception_ensemble`` against ``densenet_onnx`` fed with
host-preprocessed tensors."""

import os
import re

import numpy as np
import pytest

from triton_client_amd.utils import image

pytestmark = pytest.mark.gpu

SIZES = [(240, 320, 3), (97, 131, 3), (480, 640, 3)]


def _images(sizes=SIZES, seed=11):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, s, dtype=np.uint8) for s in sizes]


def _request(blobs, ensemble_step=False):
    from triton_client_amd.server.types import InferRequest, InputTensor

    data = np.array(list(blobs), dtype=np.object_).reshape(len(blobs), 1)
    r = InferRequest(model_name="preprocess_inception", inputs=[InputTensor("INPUT", "BYTES", [len(blobs), 1], data)])
    if ensemble_step:
        r.accepts_device_outputs = True  # what core._infer_ensemble sets on its sub-requests
    return r


def _assert_within_bound(got, imgs, what):
    """The K20 bound of tests/test_resize_gpu.py for INCEPTION scaling, FP32."""
    for k, (g, img) in enumerate(zip(got, imgs)):
        ref = image.preprocess(img, 3, 224, 224, "INCEPTION", "NCHW", np.float64)
        err = np.abs(g.astype(np.float64) - ref)
        bound = 8 * 2.0 ** -24 * 256 / 127.5 + 2.0 ** -23 * np.abs(ref)
        print("%s image %d: max err %.3g, worst err/bound %.3g" % (what, k, err.max(), (err / bound).max()))
        assert (err <= bound).all(), (what, k)


@pytest.fixture(scope="module")
def model():
    from triton_client_amd.server.gpu_models import PreprocessInception

    m = PreprocessInception()
    m.load()
    yield m
    m.unload()


def test_ensemble_step_gets_a_device_view(model):
    from triton_client_amd.server.types import DeviceView, InputTensor

    imgs = _images() + [_images([(64, 48, 1)], seed=5)[0]]
    blobs = [image.encode_ppm(imgs[0]), image.encode_raw(imgs[1]), image.encode_ppm(imgs[2]),
             image.encode_raw(imgs[3])]
    # two requests in one batch: rows 0-2 and row 3
    res = model.execute([_request(blobs[:3], True), _request(blobs[3:], True)])
    got = []
    for outs, n in zip(res, (3, 1)):
        (o,) = outs
        assert isinstance(o.data, DeviceView) and o.shape == [n, 3, 224, 224] and o.datatype == "FP32"
        assert o.data.nbytes == n * 3 * 224 * 224 * 4 and o.owner.is_cuda
        got += list(InputTensor("x", "FP32", o.shape, o.data).numpy())
    _assert_within_bound(got, imgs, "device view")


def test_direct_request_gets_a_host_array(model):
    imgs = _images()
    (outs,) = model.execute([_request([image.encode_raw(im) for im in imgs])])
    (o,) = outs
    assert isinstance(o.data, np.ndarray) and o.data.dtype == np.float32 and o.data.shape == (3, 3, 224, 224)
    _assert_within_bound(o.data, imgs, "host array")


def test_blobs_past_the_staging_area_take_the_host_routine(model, monkeypatch):
    imgs = _images()
    monkeypatch.setattr(model, "STAGE_BYTES", imgs[0].size + imgs[1].size)  # the third image does not fit
    (outs,) = model.execute([_request([image.encode_ppm(im) for im in imgs])])
    got = outs[0].data
    _assert_within_bound(got[:2], imgs[:2], "staged")
    np.testing.assert_array_equal(got[2], image.inception_preprocess(imgs[2], 224, 224, "NCHW"))


def test_knob_off_is_the_numpy_step(monkeypatch):
    from triton_client_amd.server.cpu_models import PreprocessInception as HostModel
    from triton_client_amd.server.gpu_models import PreprocessInception

    monkeypatch.setenv("TCAMD_DEVICE_PREPROCESS", "0")
    m = PreprocessInception()
    m.load()
    try:
        blobs = [image.encode_ppm(im) for im in _images(SIZES[:2])]
        (outs,) = m.execute([_request(blobs, True)])
        (ref,) = HostModel().execute([_request(blobs)])
        assert isinstance(outs[0].data, np.ndarray)
        np.testing.assert_array_equal(outs[0].data, ref[0].data)
    finally:
        m.unload()


def test_undecodable_blob_fails_its_request_with_the_cpu_models_error(model):
    from triton_client_amd.server.cpu_models import PreprocessInception as HostModel

    good = image.encode_ppm(_images(SIZES[:1])[0])
    for bad in (b"JFIF not an image", image.encode_raw(_images(SIZES[:1])[0])[:100]):
        with pytest.raises(Exception) as host_err:
            HostModel().execute([_request([bad])])
        res = model.execute([_request([bad]), _request([good])])
        assert type(res[0]) is type(host_err.value) and str(res[0]) == str(host_err.value)
        assert res[1][0].data.shape == (1, 3, 224, 224)


# -- served ---------------------------------------------------------------------------
def _client(gpu_server, proto):
    import tritonclient.grpc as grpcclient
    import tritonclient.http as httpclient

    mod = grpcclient if proto == "grpc" else httpclient
    return mod, mod.InferenceServerClient(gpu_server.grpc_url if proto == "grpc" else gpu_server.http_url)


@pytest.fixture(scope="module")
def served_reference(gpu_server):
    """densenet_onnx on the host-preprocessed tensors of the three images."""
    imgs = _images()
    mod, c = _client(gpu_server, "http")
    x = np.stack([image.inception_preprocess(im, 224, 224, "NCHW") for im in imgs]).astype(np.float32)
    inp = mod.InferInput("data_0", list(x.shape), "FP32")
    inp.set_data_from_numpy(x)
    ref = c.infer("densenet_onnx", [inp]).as_numpy("fc6_1")
    c.close()
    return imgs, ref


def _preprocess_count(gpu_server):
    mod, c = _client(gpu_server, "http")
    st = c.get_inference_statistics("preprocess_inception")
    c.close()
    return int(st["model_stats"][0]["inference_count"])


@pytest.mark.parametrize("proto", ["http", "grpc"])
@pytest.mark.parametrize("codec", ["ppm", "tcimg"])
def test_served_ensemble_matches_densenet_on_host_preprocessed_tensors(gpu_server, served_reference, codec, proto):
    imgs, ref = served_reference
    enc = image.encode_ppm if codec == "ppm" else image.encode_raw
    data = np.array([enc(im) for im in imgs], dtype=np.object_).reshape(3, 1)
    before = _preprocess_count(gpu_server)
    mod, c = _client(gpu_server, proto)
    inp = mod.InferInput("INPUT", [3, 1], "BYTES")
    inp.set_data_from_numpy(data)
    got = c.infer("preprocess_inception_ensemble", [inp]).as_numpy("OUTPUT")
    c.close()
    assert got.shape == (3, 1000)
    rel = np.linalg.norm(got - ref, axis=1) / np.linalg.norm(ref, axis=1)
    print("%s %s: per-row rel-L2 vs host-preprocessed densenet_onnx %s" % (codec, proto, rel))
    assert rel.max() < 1e-3, rel
    assert np.array_equal(got.argmax(axis=1), ref.argmax(axis=1))
    assert _preprocess_count(gpu_server) - before == 3


def test_served_preprocess_is_a_gpu_model(gpu_server):
    mod, c = _client(gpu_server, "http")
    cfg = c.get_model_config("preprocess_inception")
    c.close()
    assert cfg["instance_group"][0]["kind"] == "KIND_GPU"
    assert cfg["max_batch_size"] == 8 and "dynamic_batching" in cfg


def test_image_client_device_resize_classifies_as_the_host_path(gpu_server, tmp_path):
    from tests.test_examples import run_example

    for i, im in enumerate(_images()):
        with open(os.path.join(tmp_path, "img%d.ppm" % i), "wb") as f:
            f.write(image.encode_ppm(im))
    picks = []
    for extra in ([], ["--device-resize"]):
        r = run_example("image_client.py", gpu_server.http_url,
                        ["-m", "densenet_onnx", "-s", "INCEPTION", "-c", "1", "-b", "3"] + extra + [str(tmp_path)],
                        timeout=300)
        assert r.returncode == 0 and "PASS" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]
        picks.append(re.findall(r"\((\d+)\) = ", r.stdout))
    assert len(picks[0]) == 3 and picks[0] == picks[1], picks

"""K26 compare_expected on the device against the numpy rule of
tests/compare_cases.py, every record field exactly; then the two served paths:
``compare_shared_memory_region`` of the HIP shm module, and perf_analyzer
validating outputs in HIP shared memory against the GPU bench server."""

import json
import subprocess

import numpy as np
import pytest

from tests import compare_cases as cc

pytestmark = pytest.mark.gpu

RECORD = np.dtype([("mismatches", "<u8"), ("first_index", "<u8"), ("max_abs_diff", "<f8"), ("got_bits", "<u8"),
                   ("expected_bits", "<u8")])


@pytest.fixture(scope="module")
def hip():
    import torch

    torch.cuda.set_device(0)
    from triton_client_amd.ops import hip

    assert hip.COMPARE_RECORD_BYTES == RECORD.itemsize
    assert hip.compare_geometry()[0] == cc.UNIT
    return hip


def _launch(hip, cases, atol=0.0, rtol=0.0):
    """One K26 call over ``cases`` (at most 64), each array at its own offset
    past a 64-byte boundary of one device buffer; returns the records."""
    import torch

    spans, total = [], 0
    for c in cases:
        for key in ("got", "exp"):
            a = c[key]
            start = total + c[key + "_off"] * a.dtype.itemsize
            spans.append((start, a))
            total = (start + a.nbytes + 63) & ~63
        total += 64
    host = np.zeros(total + 64, dtype=np.uint8)
    for start, a in spans:
        host[start:start + a.nbytes] = a.view(np.uint8)
    buf = torch.from_numpy(host).cuda()
    assert buf.data_ptr() % 64 == 0
    # stale bytes for the kernel to overwrite
    rec = torch.full((len(cases) * RECORD.itemsize,), 0xa5, dtype=torch.uint8, device="cuda")
    pairs = [(buf.data_ptr() + spans[2 * i][0], buf.data_ptr() + spans[2 * i + 1][0], c["got"].size, c["datatype"])
             for i, c in enumerate(cases)]
    hip.compare_expected(pairs, rec.data_ptr(), atol, rtol, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rec.cpu().numpy().view(RECORD)


def _check(hip, cases, atol=0.0, rtol=0.0):
    for at in range(0, len(cases), hip.COMPARE_MAX_PAIRS):
        chunk = cases[at:at + hip.COMPARE_MAX_PAIRS]
        recs = _launch(hip, chunk, atol, rtol)
        for c, r in zip(chunk, recs):
            want = cc.reference(c["got"], c["exp"], c["datatype"], atol, rtol)
            assert tuple(r.tolist()) == want, (c["name"], atol, rtol)


def test_sizes_alignments_and_edge_positions(hip):
    """Widths 1, 2, 4, 8 at counts 0 .. 4099, got and expected misaligned alike,
    differently and not at all; a clean pair and one flipped bit at the first,
    the last, the body's last and the tail's first element."""
    cases = cc.layout_cases()
    assert {c["got"].dtype.itemsize for c in cases} == {1, 2, 4, 8}
    _check(hip, cases)


def test_several_mismatches_on_one_and_on_several_workgroups(hip):
    cases = cc.count_cases()
    per_block = hip.compare_geometry()[1]
    assert any(c["got"].nbytes > 2 * per_block for c in cases) and any(c["got"].nbytes <= per_block for c in cases)
    _check(hip, cases)


@pytest.mark.parametrize("atol,rtol", [(0.0, 0.0), (cc.FLOAT_ATOL, cc.FLOAT_RTOL), (0.0, cc.FLOAT_RTOL),
                                       (cc.FLOAT_ATOL, 0.0)])
def test_float_special_values_in_both_modes(hip, atol, rtol):
    _check(hip, cc.float_cases(), atol, rtol)


def test_noise_around_the_tolerance(hip):
    cases = cc.noise_cases()
    _check(hip, cases, cc.NOISE_ATOL, cc.NOISE_RTOL)
    _check(hip, cases)


def test_64_mixed_pairs_and_an_empty_one_in_one_launch(hip):
    cases = cc.mixed_launch()
    assert len(cases) == hip.COMPARE_MAX_PAIRS
    for atol in (0.0, 1e-2):
        recs = _launch(hip, cases, atol, atol)
        for c, r in zip(cases, recs):
            assert tuple(r.tolist()) == cc.reference(c["got"], c["exp"], c["datatype"], atol, atol), c["name"]
    assert tuple(recs[31].tolist()) == (0, cc.NO_INDEX, 0.0, 0, 0)


def test_index_past_2_to_31(hip):
    """Element indices are 64-bit: the only mismatches of 2^31 + 17 bytes are the last element and one past 2^31."""
    import torch

    n = 2**31 + 17
    got = torch.zeros(n + 1, dtype=torch.uint8, device="cuda")[1:]  # got one byte past a boundary
    exp = torch.zeros(n + 3, dtype=torch.uint8, device="cuda")[3:]
    got[n - 1] = 7
    exp[2**31 + 2] = 9
    rec = torch.zeros(RECORD.itemsize, dtype=torch.uint8, device="cuda")
    hip.compare_expected([(got.data_ptr(), exp.data_ptr(), n, "UINT8")], rec.data_ptr(), 0.0, 0.0,
                         torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert tuple(rec.cpu().numpy().view(RECORD)[0].tolist()) == (2, 2**31 + 2, 0.0, 0, 9)


def test_refused_before_any_launch(hip):
    import torch

    buf = torch.zeros(256, dtype=torch.uint8, device="cuda")
    p, rec = buf.data_ptr(), buf.data_ptr() + 128
    hip.compare_expected([], rec)
    for bad in ([(p + 2, p, 4, "FP32")], [(p, p + 1, 4, "INT16")], [(0, p, 4, "UINT8")], [(p, p, 4, "FP32")] * 65):
        with pytest.raises((hip.HipError, ValueError)):
            hip.compare_expected(bad, rec)
    for atol, rtol in ((-1.0, 0.0), (0.0, float("nan")), (float("inf"), 0.0)):
        with pytest.raises(hip.HipError):
            hip.compare_expected([(p, p, 4, "FP32")], rec, atol, rtol)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# tritonclient.utils.hip_shared_memory.compare_shared_memory_region
# ---------------------------------------------------------------------------
def test_compare_shared_memory_region_with_offset(hip):
    from tritonclient.utils import cuda_shared_memory, hip_shared_memory as shm, serialize_byte_tensor

    assert cuda_shared_memory.compare_shared_memory_region is shm.compare_shared_memory_region
    a = np.arange(1000, dtype=np.int32).reshape(10, 100)
    b = np.linspace(-3, 3, 777, dtype=np.float32)
    s = serialize_byte_tensor(np.array([b"mi355x", b"", b"k26" * 9], dtype=np.object_))
    off = 36  # the arrays sit at 4-byte, not 16-byte, aligned addresses
    h = shm.create_shared_memory_region("cmp0", off + a.nbytes + b.nbytes + len(s.item()), 0)
    try:
        shm.set_shared_memory_region(h, [a, b, s], offset=off)
        assert shm.compare_shared_memory_region(h, [a, b, s], offset=off) == [(0, -1, 0.0)] * 3
        a2, b2 = a.copy(), b.copy()
        a2[3, 7] += 1
        a2[9, 99] = 0
        b2[5] = np.nextafter(b2[5], np.float32(9))
        b2[700] += np.float32(0.5)
        s2 = serialize_byte_tensor(np.array([b"mi355x", b"", b"k27" + b"k26" * 8], dtype=np.object_))
        d5, d700 = float(abs(b[5] - b2[5])), float(abs(b[700] - b2[700]))
        assert shm.compare_shared_memory_region(h, [a2, b2, s2], offset=off) == [
            (2, 307, 0.0), (2, 5, max(d5, d700)), (1, 4 + 6 + 4 + 4 + 2, 0.0)]
        # tolerance mode passes the one-ulp element and still fails the large one; integers stay exact
        assert shm.compare_shared_memory_region(h, [a2, b2, s], atol=1e-3, rtol=1e-3, offset=off) == [
            (2, 307, 0.0), (1, 700, max(d5, d700)), (0, -1, 0.0)]
        with pytest.raises(shm.CudaSharedMemoryException):
            shm.compare_shared_memory_region(h, [a, b, s], offset=off + 4)  # past the end of the region
        with pytest.raises(shm.CudaSharedMemoryException):
            shm.compare_shared_memory_region(h, [a], atol=-1.0)
    finally:
        shm.destroy_shared_memory_region(h)


def test_compare_shared_memory_region_bf16_convention(hip):
    """datatype="BF16": float32 expectations are truncated on the device on the
    way up, as set_shared_memory_region(datatype="BF16") writes them."""
    from tritonclient.utils import hip_shared_memory as shm

    v = np.linspace(-2, 2, 515, dtype=np.float32)
    h = shm.create_shared_memory_region("cmp1", 2 * v.size + 2, 0)
    try:
        shm.set_shared_memory_region(h, [v], offset=2, datatype="BF16")
        assert shm.compare_shared_memory_region(h, [v], offset=2, datatype="BF16") == [(0, -1, 0.0)]
        bits = (v.view(np.uint32) >> 16).astype(np.uint16)
        assert shm.compare_shared_memory_region(h, [bits], offset=2, datatype="BF16") == [(0, -1, 0.0)]
        w = v.copy()
        w[100] += 0.25

        def trunc(x):
            return float((np.array([x], np.float32).view(np.uint32) & 0xffff0000).view(np.float32)[0])

        d = abs(trunc(v[100]) - trunc(w[100]))
        assert shm.compare_shared_memory_region(h, [w], offset=2, datatype="BF16") == [(1, 100, d)]
        assert shm.compare_shared_memory_region(h, [w], atol=0.5, offset=2, datatype="BF16") == [(0, -1, d)]
    finally:
        shm.destroy_shared_memory_region(h)


# ---------------------------------------------------------------------------
# perf_analyzer --shared-memory hip: outputs validated on the device
# ---------------------------------------------------------------------------
FAST = ["--measurement-mode", "count_windows", "--measurement-request-count", "60", "-r", "3"]


def _pa(args):
    from triton_client_amd.perf import native

    return subprocess.run([native.BIN_PATH] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


def _simple_data(tmp_path, wrong=None):
    entries = []
    for k in range(3):
        a, b = [k + i for i in range(16)], [3 * k + 1] * 16
        entries.append(({"INPUT0": a, "INPUT1": b},
                        {"OUTPUT0": [x + y for x, y in zip(a, b)], "OUTPUT1": [x - y for x, y in zip(a, b)]}))
    if wrong is not None:
        entries[wrong[0]][1]["OUTPUT1"][wrong[1]] = 4242
    f = tmp_path / "data.json"
    f.write_text(json.dumps({"data": [e[0] for e in entries], "validation_data": [e[1] for e in entries]}))
    return f


def test_perf_analyzer_hip_shm_validation_data(gpu_server, tmp_path):
    """Three entries, four requests in flight, simple's two INT32 outputs in HIP
    shared memory: K26 on the lane's stream passes every response; with one wrong
    element the run ends after its window and names it."""
    base = ["-m", "simple", "-i", "grpc", "-u", gpu_server.grpc_url, "--shared-memory", "hip",
            "--concurrency-range", "4"]
    j = tmp_path / "r.json"
    r = _pa(base + ["--input-data", _simple_data(tmp_path), "--json-report", j] + FAST)
    assert r.returncode == 0, r.stderr + r.stdout
    assert "outputs validated against validation_data (exact) on the device by K26" in r.stdout
    v = json.load(open(j))["points"][0]["validation"]
    assert v["validated"] >= 180 and v["validation_failed"] == 0
    r = _pa(base + ["--input-data", _simple_data(tmp_path, wrong=(2, 13)), "--json-report", j] + FAST)
    assert r.returncode != 0, r.stdout
    # entry 2 sends INPUT0[13] = 15 and INPUT1 = 7
    assert "output validation failed: output OUTPUT1 of data entry 2: element 13 is 8, expected 4242 (1 mismatching" \
        in r.stderr, r.stderr
    v = json.load(open(j))["points"][0]["validation"]
    assert v["validation_failed"] > 0 and v["validated"] > 0


def test_perf_analyzer_hip_shm_validate_first(gpu_server, tmp_path):
    """Device-filled synthetic inputs (K1), nothing on the host: the first
    response is copied device to device and every later one compared with it,
    the slots alternating between their two sets of output regions."""
    j = tmp_path / "r.json"
    r = _pa(["-m", "simple", "-i", "grpc", "-u", gpu_server.grpc_url, "--shared-memory", "hip",
             "--concurrency-range", "4", "--validate-outputs", "first", "--json-report", j, "--measurement-mode", "count_windows",
             "--measurement-request-count", "150", "-r", "3"])
    assert r.returncode == 0, r.stderr + r.stdout
    assert "inputs filled on device by K1" in r.stdout
    assert "each entry's first response (exact) on the device by K26" in r.stdout
    v = json.load(open(j))["points"][0]["validation"]
    assert v["validated"] >= 400 and v["validation_failed"] == 0


def test_perf_analyzer_hip_shm_two_lanes_validate(gpu_server, tmp_path):
    """Two lanes (both on GPU 0): each validates on its own stream against its own device copy of the expectations."""
    j = tmp_path / "r.json"
    r = _pa(["-m", "simple", "-i", "grpc", "-u", gpu_server.grpc_url, "--shared-memory", "hip", "--devices", "0,0",
             "--fanout", "host", "--concurrency-range", "6", "--input-data", _simple_data(tmp_path), "--json-report", j]
            + FAST)
    assert r.returncode == 0, r.stderr + r.stdout
    p = json.load(open(j))["points"][0]
    lanes = [g["validation"] for g in p["per_gpu"]]
    assert len(lanes) == 2 and all(v["validated"] > 0 and v["validation_failed"] == 0 for v in lanes)
    assert p["validation"]["validated"] == sum(v["validated"] for v in lanes) >= 180

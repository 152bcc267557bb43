"""perf_analyzer output validation against the CPU test server: the
"validation_data" array of the --input-data JSON, --validate-outputs first and
--validation-tolerance, in every issue mode, and the reports with and without
it.  The model is ``simple``: INT32 [1, 16], OUTPUT0 = INPUT0 + INPUT1,
OUTPUT1 = INPUT0 - INPUT1.  Everything here runs on CPU."""

import csv
import json
import re

import pytest

from tests.test_perf_analyzer import _pa
from triton_client_amd.perf import native

pytestmark = pytest.mark.skipif(not native.available(), reason="csrc/cpp not built")

# what a report held before validation existed: runs without it must keep exactly these
REPORT_KEYS = ["model", "gpus", "batch_size", "protocol", "shared_memory", "mode", "data", "points"]
POINT_KEYS = ["load", "stable", "request_count", "window_s", "throughput", "avg_us", "std_us", "p50_us", "p90_us",
              "p95_us", "p99_us", "client_send_us", "client_recv_us", "errors", "server"]
CSV_HEADER = ["Concurrency", "Inferences/Second", "Client Send", "Network+Server Send/Recv", "Server Queue",
              "Server Compute Input", "Server Compute Infer", "Server Compute Output", "Client Recv", "p50 latency",
              "p90 latency", "p95 latency", "p99 latency", "Avg latency", "request/response", "response wait"]
FAST = ["--measurement-mode", "count_windows", "--measurement-request-count", "40", "-r", "3"]


def _entry(k):
    a, b = [k + i for i in range(16)], [3 * k + 1] * 16
    return ({"INPUT0": a, "INPUT1": b},
            {"OUTPUT0": [x + y for x, y in zip(a, b)], "OUTPUT1": [x - y for x, y in zip(a, b)]})


def _data(tmp_path, n=1, edit=None, name="data.json"):
    pairs = [_entry(k) for k in range(n)]
    doc = {"data": [p[0] for p in pairs], "validation_data": [p[1] for p in pairs]}
    if edit:
        edit(doc)
    f = tmp_path / name
    f.write_text(json.dumps(doc))
    return f


def _validation(report):
    return json.load(open(report))["points"][-1]["validation"]


@pytest.mark.parametrize("mode", [["-i", "http"], ["-i", "grpc"], ["-i", "http", "--sync"], ["-i", "grpc", "--sync"],
                                  ["-i", "grpc", "--streaming"], ["-i", "grpc", "--shared-memory", "system"],
                                  ["-i", "http", "--shared-memory", "system", "--sync"]],
                         ids=lambda m: "-".join(x.strip("-") for x in m[1:]))
def test_correct_validation_data_passes(cpu_server, tmp_path, mode):
    url = cpu_server.http_url if mode[1] == "http" else cpu_server.grpc_url
    j = tmp_path / "r.json"
    r = _pa(["-m", "simple", "-u", url, "--input-data", _data(tmp_path), "--concurrency-range", "2", "--json-report", j]
            + mode + FAST)
    assert r.returncode == 0, r.stderr + r.stdout
    assert "outputs validated against validation_data (exact)" in r.stdout
    v = _validation(j)
    assert v["validated"] > 0 and v["validation_failed"] == 0
    assert re.search(r"Validated responses: [1-9]\d* \(failed validation: 0\)", r.stdout)


@pytest.mark.parametrize("mode", [["-i", "grpc"], ["-i", "http", "--shared-memory", "system"]],
                         ids=["inband", "system"])
def test_one_wrong_element_fails_and_is_named(cpu_server, tmp_path, mode):
    def edit(doc):
        doc["validation_data"][1]["OUTPUT1"][11] = 4242

    url = cpu_server.http_url if mode[1] == "http" else cpu_server.grpc_url
    j, f = tmp_path / "r.json", tmp_path / "r.csv"
    r = _pa(["-m", "simple", "-u", url, "--input-data", _data(tmp_path, 2, edit), "--json-report", j, "-f", f]
            + mode + FAST)
    assert r.returncode != 0, r.stdout
    # entry 1 sends INPUT0[11] = 12 and INPUT1 = 4: OUTPUT1[11] is 8
    assert "output validation failed: output OUTPUT1 of data entry 1: element 11 is 8, expected 4242" in r.stderr, \
        r.stderr
    assert "1 mismatching element(s)" in r.stderr
    v = _validation(j)
    assert v["validation_failed"] > 0 and v["validated"] > 0  # entry 0 still passes
    row = next(csv.DictReader(open(f)))
    assert int(row["Validation Failed"]) == v["validation_failed"] and int(row["Validated"]) == v["validated"]


def test_responses_are_matched_to_the_entry_their_slot_sent(cpu_server, tmp_path):
    """Three entries with different expectations, four requests in flight: all
    pass; with the expectations of two entries swapped the run fails."""
    base = ["-m", "simple", "-i", "grpc", "-u", cpu_server.grpc_url, "--concurrency-range", "4"] + FAST
    j = tmp_path / "r.json"
    r = _pa(base + ["--input-data", _data(tmp_path, 3), "--json-report", j])
    assert r.returncode == 0, r.stderr
    assert "3 entries, cycled per request" in r.stdout
    v = _validation(j)
    assert v["validated"] >= 120 and v["validation_failed"] == 0

    def swap(doc):
        vd = doc["validation_data"]
        vd[0], vd[2] = vd[2], vd[0]

    r = _pa(base + ["--input-data", _data(tmp_path, 3, swap, "swapped.json"), "--json-report", j])
    assert r.returncode != 0
    assert re.search(r"output OUTPUT0 of data entry [02]: element 0 is", r.stderr), r.stderr
    v = _validation(j)
    assert v["validation_failed"] > 0 and v["validated"] > 0  # entry 1 kept its own


def test_validate_outputs_first(cpu_server, tmp_path):
    plain = tmp_path / "plain.json"
    plain.write_text(json.dumps({"data": [_entry(k)[0] for k in range(3)]}))
    j = tmp_path / "r.json"
    for extra in (["--input-data", plain], ["--shared-memory", "system"], ["--streaming"], []):
        r = _pa(["-m", "simple", "-i", "grpc", "-u", cpu_server.grpc_url, "--validate-outputs", "first",
                 "--concurrency-range", "4", "--json-report", j] + extra + FAST)
        assert r.returncode == 0, r.stderr + r.stdout
        assert "outputs validated against each entry's first response" in r.stdout
        v = _validation(j)
        assert v["validated"] >= 100 and v["validation_failed"] == 0
    r = _pa(["-m", "simple", "-u", cpu_server.http_url, "--validate-outputs", "first", "--input-data", _data(tmp_path)])
    assert r.returncode == 1 and "cannot be combined" in r.stderr
    r = _pa(["-m", "simple", "--validate-outputs", "last"])
    assert r.returncode == 1 and "--validate-outputs" in r.stderr


def test_malformed_validation_data_fails_before_any_request(cpu_server, tmp_path):
    def too_short(doc):
        doc["validation_data"].pop()

    def unknown(doc):
        doc["validation_data"][0]["OUTPUT7"] = [0] * 16

    def wrong_count(doc):
        doc["validation_data"][1]["OUTPUT0"] = [0] * 15

    def wrong_count_for_shape(doc):
        doc["validation_data"][1]["OUTPUT0"] = {"content": [0] * 16, "shape": [8]}

    for k, (edit, msg) in enumerate([(too_short, "\"validation_data\" has 1 entries, \"data\" has 2"),
                                     (unknown, "'OUTPUT7', which is not an output"),
                                     (wrong_count, "OUTPUT0 has 15 elements, its shape has 16"),
                                     (wrong_count_for_shape, "OUTPUT0 has 16 elements, its shape has 8")]):
        st0 = _inference_count(cpu_server)
        r = _pa(["-m", "simple", "-i", "grpc", "-u", cpu_server.grpc_url, "--input-data",
                 _data(tmp_path, 2, edit, "bad%d.json" % k)] + FAST)
        assert r.returncode == 1 and msg in r.stderr, (r.stderr, msg)
        assert "Request concurrency" not in r.stdout
        assert _inference_count(cpu_server) == st0, "a request was sent"


def _inference_count(srv):
    import tritonclient.grpc as grpcclient

    c = grpcclient.InferenceServerClient(srv.grpc_url)
    st = c.get_inference_statistics("simple", as_json=True)
    c.close()
    return int(st["model_stats"][0].get("inference_count", 0)) if st.get("model_stats") else 0


def test_reports_without_validation_are_unchanged(cpu_server, tmp_path):
    """Neither the flag nor the array: exactly the keys and columns of before."""
    d = tmp_path / "plain.json"
    d.write_text(json.dumps({"data": [_entry(0)[0]]}))
    j, f = tmp_path / "r.json", tmp_path / "r.csv"
    r = _pa(["-m", "simple", "-i", "grpc", "-u", cpu_server.grpc_url, "--input-data", d, "--json-report", j, "-f", f]
            + FAST)
    assert r.returncode == 0, r.stderr
    assert "Validated responses" not in r.stdout and "outputs validated" not in r.stdout
    rep = json.load(open(j))
    assert list(rep) == REPORT_KEYS
    assert list(rep["points"][0]) == POINT_KEYS
    assert next(csv.reader(open(f))) == CSV_HEADER
    assert "outputs validated" not in rep["data"]
    # two lanes: the per-GPU rows too
    url = cpu_server.grpc_url
    r = _pa(["-m", "simple", "-i", "grpc", "-u", url, "--gpus", "2", "--concurrency-range", "2", "--json-report", j,
             "-f", f] + FAST)
    assert r.returncode == 0, r.stderr
    rep = json.load(open(j))
    assert list(rep["points"][0]) == POINT_KEYS + ["per_gpu"]
    assert "validation" not in rep["points"][0]["per_gpu"][0]
    assert next(csv.reader(open(f))) == ["GPU"] + CSV_HEADER


def test_every_lane_validates(cpu_server, tmp_path):
    """--gpus 2 on CPU: each lane checks its own responses; per-GPU rows and the aggregate carry the counts."""
    j, f = tmp_path / "r.json", tmp_path / "r.csv"
    url = cpu_server.grpc_url
    r = _pa(["-m", "simple", "-i", "grpc", "-u", url, "--gpus", "2", "--concurrency-range", "4", "--input-data",
             _data(tmp_path, 3), "--json-report", j, "-f", f] + FAST)
    assert r.returncode == 0, r.stderr
    p = json.load(open(j))["points"][0]
    lanes = [g["validation"] for g in p["per_gpu"]]
    assert all(v["validated"] > 0 and v["validation_failed"] == 0 for v in lanes)
    assert p["validation"]["validated"] == sum(v["validated"] for v in lanes)
    rows = list(csv.DictReader(open(f)))
    assert [int(x["Validated"]) for x in rows] == [p["validation"]["validated"]] + [v["validated"] for v in lanes]


def test_request_rate_mode_validates(cpu_server, tmp_path):
    j = tmp_path / "r.json"
    r = _pa(["-m", "simple", "-u", cpu_server.http_url, "--request-rate-range", "200", "--input-data",
             _data(tmp_path, 2), "--json-report", j, "-p", "300", "-r", "3"])
    assert r.returncode == 0, r.stderr
    v = _validation(j)
    assert v["validated"] > 20 and v["validation_failed"] == 0


def test_tolerance_mode_on_an_fp32_output(cpu_server, tmp_path):
    """identity_fp32 returns its input: an expectation off by less than the
    tolerance passes, one off by more fails; exact mode fails on both."""
    x = [0.5, -1.25, 3.0, 100.0, 0.0, -0.0, 7.75, 1e-3]

    def run(expected, tol):
        d = tmp_path / "f.json"
        d.write_text(json.dumps({"data": [{"INPUT0": {"content": x, "shape": [8]}}],
                                 "validation_data": [{"OUTPUT0": {"content": expected, "shape": [8]}}]}))
        return _pa(["-m", "identity_fp32", "-i", "grpc", "-u", cpu_server.grpc_url, "--input-data", d, "--shape",
                    "INPUT0:8"] + (["--validation-tolerance", tol] if tol else []) + FAST)

    r = run(x, None)
    assert r.returncode == 0, r.stderr
    near = [v + 0.004 for v in x]  # within 0.005 + 1e-3 * |v|, a margin far above fp32 rounding
    r = run(near, "0.005,0.001")
    assert r.returncode == 0, r.stderr
    assert "(atol 0.005, rtol 0.001)" in r.stdout
    r = run(near, None)
    assert r.returncode != 0, r.stdout
    assert "output OUTPUT0 of data entry 0: element 0 is 0.5, expected 0.504" in r.stderr, r.stderr
    far = list(near)
    far[3] = x[3] + 0.25  # 0.25 > 0.005 + 1e-3 * 100.25
    r = run(far, "0.005,0.001")
    assert r.returncode != 0 and "element 3 is 100, expected 100.25 " in r.stderr, r.stderr
    assert "1 mismatching element(s)" in r.stderr
    r = _pa(["-m", "simple", "--validation-tolerance", "-1"])
    assert r.returncode == 1 and "--validation-tolerance" in r.stderr


def test_native_session_reports_validation(cpu_server, tmp_path):
    """The C ABI, appended to: a session without validation says None, one with it counts fixed runs too."""
    base = ["-m", "simple", "-i", "grpc", "-u", cpu_server.grpc_url, "--concurrency-range", "4"]
    with native.PerfSession(base) as s:
        s.run_fixed(2, 20)
        assert s.validation() is None
    with native.PerfSession(base + ["--input-data", str(_data(tmp_path, 3))]) as s:
        lat, _ = s.run_fixed(4, 90)
        assert len(lat) == 90
        assert s.validation() == {"validated": 90, "validation_failed": 0, "first_failure": ""}

    def edit(doc):
        doc["validation_data"][2]["OUTPUT0"][0] = -5

    with native.PerfSession(base + ["--input-data", str(_data(tmp_path, 3, edit, "bad.json"))]) as s:
        s.run_fixed(4, 90)
        v = s.validation()
        assert v["validated"] == 60 and v["validation_failed"] == 30
        assert v["first_failure"].startswith("output OUTPUT0 of data entry 2: element 0 is 9, expected -5")
        with pytest.raises(native.PerfError, match="output validation failed"):
            s.profile(2)

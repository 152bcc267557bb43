"""Closed-loop classification load on densenet_onnx, and K19's own time.

    python tools/classify_bench.py                # served: class_count=3, bs 8, HIP-shm input, concurrency 48
    python tools/classify_bench.py --kernel       # K19 topk_rows alone: rows 256, C 1000, k 3, HIP events

The served mode starts the bench server (2 densenet_onnx instances) as a child
process, keeps ``--concurrency`` gRPC ``async_infer`` requests in flight, each
with ``InferRequestedOutput("fc6_1", class_count=K)`` and its input in a HIP
shared-memory region, and prints one JSON line: infer/s (images), request/s,
p50/p99 request latency and the server's compute_output time per batch.  It
uses only the public client API, so it runs unchanged on a tree whose server
relays classification requests to the Python path.
"""

import argparse
import json
import os
import sys
import threading
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def kernel_time(rows, C, k, iters):
    import numpy as np
    import torch

    from triton_client_amd.ops import hip

    torch.cuda.set_device(0)
    x = torch.randn(rows, C, device="cuda")
    kd = torch.full((rows,), k, dtype=torch.int32, device="cuda")
    pairs = torch.zeros(rows, k, 2, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream

    def launch():
        hip.topk_rows(x.data_ptr(), C * 4, rows, C, kd.data_ptr(), k, pairs.data_ptr(), stream=s)

    for _ in range(10):
        launch()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launch()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    ref = torch.topk(x, k, dim=1).indices.cpu().numpy()
    got = pairs.cpu().numpy()[:, :, 1]
    print(json.dumps({"kernel": "K19 topk_rows", "rows": rows, "C": C, "k": k, "launches": iters,
                      "mean_us": round(float(np.mean(times)), 2), "min_us": round(float(np.min(times)), 2),
                      "max_us": round(float(np.max(times)), 2), "indices_match_torch_topk": bool((ref == got).all())}))


def served(args):
    import numpy as np

    import tritonclient.grpc as grpcclient
    from triton_client_amd.perf.harness import ServerProcess
    from tritonclient.utils import hip_shared_memory as hipshm

    log = os.path.abspath(args.server_log) if args.server_log else None
    if log:
        os.makedirs(os.path.dirname(log), exist_ok=True)
    srv = ServerProcess(device=0, models="densenet_onnx", log_path=log, extra_args=["--instance-count", "2"])
    region = None
    try:
        srv.wait_ready(timeout=900, model="densenet_onnx")
        x = np.random.default_rng(0).standard_normal((args.batch, 3, 224, 224)).astype(np.float32)
        region = hipshm.create_shared_memory_region("clsb_in", x.nbytes, 0)
        hipshm.set_shared_memory_region(region, [x])
        c = grpcclient.InferenceServerClient(srv.grpc_url)
        c.register_cuda_shared_memory("clsb_in", hipshm.get_raw_handle(region), 0, x.nbytes)
        inp = grpcclient.InferInput("data_0", list(x.shape), "FP32")
        inp.set_shared_memory("clsb_in", x.nbytes)
        outs = [grpcclient.InferRequestedOutput("fc6_1", class_count=args.k)]
        first = c.infer("densenet_onnx", [inp], outputs=outs).as_numpy("fc6_1")
        assert first.shape == (args.batch, args.k), first.shape

        lock = threading.Lock()
        done = threading.Event()
        state = {"lat": [], "errors": 0, "stop": False, "inflight": 0, "measure": False}

        def send():
            t0 = time.perf_counter()

            def cb(result, error):
                t1 = time.perf_counter()
                with lock:
                    if error is not None:
                        state["errors"] += 1
                    elif state["measure"]:
                        state["lat"].append(t1 - t0)
                    again = not state["stop"]
                    if not again:
                        state["inflight"] -= 1
                        if state["inflight"] == 0:
                            done.set()
                if again:
                    send()

            c.async_infer("densenet_onnx", [inp], outputs=outs, callback=cb)

        def stats():
            s = c.get_inference_statistics("densenet_onnx", as_json=True)["model_stats"][0]
            return int(s.get("execution_count", 0)), int(s["inference_stats"]["compute_output"].get("ns", 0))

        with lock:
            state["inflight"] = args.concurrency
        for _ in range(args.concurrency):
            send()
        time.sleep(args.warmup)
        e0, o0 = stats()
        with lock:
            state["measure"] = True
            state["lat"] = []
        t0 = time.perf_counter()
        time.sleep(args.seconds)
        with lock:
            lat = list(state["lat"])
            state["measure"] = False
        dt = time.perf_counter() - t0
        e1, o1 = stats()
        with lock:
            state["stop"] = True
        done.wait(30)
        lat.sort()
        n = len(lat)
        print(json.dumps({
            "model": "densenet_onnx", "class_count": args.k, "batch": args.batch, "concurrency": args.concurrency,
            "seconds": round(dt, 2), "requests": n, "errors": state["errors"],
            "infer_per_s": round(n * args.batch / dt, 1), "requests_per_s": round(n / dt, 1),
            "p50_ms": round(lat[n // 2] * 1e3, 3) if n else None,
            "p99_ms": round(lat[min(n - 1, int(n * 0.99))] * 1e3, 3) if n else None,
            "server_batches": e1 - e0,
            "compute_output_us_per_batch": round((o1 - o0) / 1e3 / max(1, e1 - e0), 2),
        }))
        c.unregister_cuda_shared_memory()
        c.close()
    finally:
        srv.stop()
        if region is not None:
            hipshm.destroy_shared_memory_region(region)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--kernel", action="store_true", help="time K19 alone instead of the served loop")
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--concurrency", type=int, default=48)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--warmup", type=float, default=3.0)
    ap.add_argument("--rows", type=int, default=256, help="--kernel: rows per launch")
    ap.add_argument("--classes", type=int, default=1000, help="--kernel: values per row")
    ap.add_argument("--iters", type=int, default=50, help="--kernel: timed launches (after 10 warm-up)")
    ap.add_argument("--server-log", default="", metavar="PATH", help="keep the server's log in this file")
    args = ap.parse_args()
    if args.kernel:
        kernel_time(args.rows, args.classes, args.k, args.iters)
    else:
        served(args)


if __name__ == "__main__":
    main()

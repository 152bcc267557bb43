#!/usr/bin/env python
"""K33 ``search_topk`` (csrc/kernels/embed_search.hip: both launches) against
``torch.topk(q @ C.T, k)`` in fp32, in one run on one seeded corpus of unit
vectors.  Per (rows, N): warm-up, then ``--windows`` timed windows per route,
the routes taking turns; a window is timed with device events around ``iters``
calls (sized from a first call so that a window lasts about ``--window-s``).
Reported: the median window's time per call and the spread (min .. max) over
the windows, K33's corpus bytes per second (the hi and lo planes, N * D * 4
bytes, counted once, over the time per call), and whether the two routes agree
on every row's nearest corpus row.  Needs a GPU; prints one JSON line per
point and a markdown table at the end.

``--index q8`` adds K34 ``search_topk_q8`` (csrc/kernels/embed_search_q8.hip:
all three launches) as a third route taking turns with the other two, its int8
index built beside K33's planes; per point also the median over the windows'
count of single timed calls of its coarse launch and of its shortlist + rescore
launches (device events inside the call), its bytes per second over the int8
codes (N * D bytes, counted once) and whether it names every row's nearest
corpus row as torch does."""

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def window(torch, fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters  # us per call


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", default="1,16,128")
    ap.add_argument("--n", default="65536,1048576")
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("-k", type=int, default=10)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--window-s", type=float, default=0.3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--index", choices=("x3", "q8"), default="x3", help="q8: K34 as a third route")
    args = ap.parse_args()

    import torch

    from triton_client_amd.ops import hip

    if not torch.cuda.is_available():
        sys.exit("search_bench needs a GPU")
    dev, D, k = torch.device("cuda"), args.dim, args.k
    gen = torch.Generator(device=dev)
    gen.manual_seed(33)
    table = []
    for N in (int(v) for v in args.n.split(",")):
        corpus = torch.randn(N, D, generator=gen, device=dev)
        corpus /= corpus.norm(dim=1, keepdim=True)
        hi, lo = hip.search_index(corpus)
        q8 = hip.search_index_q8(corpus) if args.index == "q8" else None
        for rows in (int(v) for v in args.rows.split(",")):
            q = torch.randn(rows, D, generator=gen, device=dev)
            q /= q.norm(dim=1, keepdim=True)
            k_row = torch.full((rows,), k, dtype=torch.int32, device=dev)
            ws = torch.zeros(hip.search_workspace(rows, N), dtype=torch.uint8, device=dev)
            idx = torch.zeros(rows, k, dtype=torch.int32, device=dev)
            sc = torch.zeros(rows, k, dtype=torch.float32, device=dev)
            ptrs = (q.data_ptr(), D * 4, rows, hi.data_ptr(), lo.data_ptr(), N, D, k_row.data_ptr(), k, ws.data_ptr(),
                    idx.data_ptr(), sc.data_ptr())
            routes = {"k33": lambda: hip.search_topk(*ptrs), "torch": lambda: torch.topk(q @ corpus.T, k)}
            if q8 is not None:
                ws8 = torch.zeros(hip.search_q8_workspace(rows, N), dtype=torch.uint8, device=dev)
                idx8, sc8 = torch.zeros_like(idx), torch.zeros_like(sc)
                ptrs8 = (q.data_ptr(), D * 4, rows, q8[0].data_ptr(), q8[1].data_ptr(), hi.data_ptr(), lo.data_ptr(),
                         N, D, k_row.data_ptr(), k, k, ws8.data_ptr(), idx8.data_ptr(), sc8.data_ptr())
                routes["k34"] = lambda: hip.search_topk_q8(*ptrs8)
            iters, times = {}, {name: [] for name in routes}
            for name, fn in routes.items():
                for _ in range(args.warmup):
                    fn()
                iters[name] = int(min(5000, max(5, args.window_s * 1e6 / window(torch, fn, 3))))
            for _ in range(args.windows):
                for name, fn in routes.items():
                    times[name].append(window(torch, fn, iters[name]))
            agree = bool((idx[:, 0].long() == torch.topk(q @ corpus.T, k).indices[:, 0]).all().item())
            point = {"rows": rows, "N": N, "D": D, "k": k, "slices": hip.search_plan(rows, N)[0], "top1_agree": agree}
            for name, t in times.items():
                point[name] = {"us": round(statistics.median(t), 1), "min_us": round(min(t), 1),
                               "max_us": round(max(t), 1), "iters": iters[name], "windows": len(t)}
            point["k33_corpus_GBps"] = round(N * D * 4 / point["k33"]["us"] / 1e3, 1)
            if q8 is not None:
                parts = [hip.search_topk_q8_timed(*ptrs8) for _ in range(args.windows)]
                top = torch.topk(q @ corpus.T, k).indices
                point.update(k34_slices=hip.search_q8_plan(rows, N)[0],
                             k34_coarse_us=round(statistics.median(a for a, _ in parts), 1),
                             k34_rest_us=round(statistics.median(b for _, b in parts), 1),
                             k34_codes_GBps=round(N * D / point["k34"]["us"] / 1e3, 1),
                             k34_top1_agree=bool((idx8[:, 0].long() == top[:, 0]).all().item()),
                             k34_equals_k33=bool((idx8 == idx).all().item() and (sc8 == sc).all().item()))
            print(json.dumps(point), flush=True)
            table.append(point)
        del corpus, hi, lo
    print("\n| rows | N | K33 us (min .. max) | torch us (min .. max) | K33 / torch | K33 corpus GB/s |")
    print("|---|---|---|---|---|---|")
    for p in table:
        a, b = p["k33"], p["torch"]
        print("| %d | %d | %.1f (%.1f .. %.1f) | %.1f (%.1f .. %.1f) | %.2f | %.0f |"
              % (p["rows"], p["N"], a["us"], a["min_us"], a["max_us"], b["us"], b["min_us"], b["max_us"],
                 a["us"] / b["us"], p["k33_corpus_GBps"]))
    if args.index == "q8":
        print("\n| rows | N | K34 us (min .. max) | K34 / K33 | K34 / torch | coarse us | shortlist + rescore us "
              "| K34 codes GB/s | = K33 |")
        print("|---|---|---|---|---|---|---|---|---|")
        for p in table:
            c = p["k34"]
            print("| %d | %d | %.1f (%.1f .. %.1f) | %.2f | %.2f | %.1f | %.1f | %.0f | %s |"
                  % (p["rows"], p["N"], c["us"], c["min_us"], c["max_us"], c["us"] / p["k33"]["us"],
                     c["us"] / p["torch"]["us"], p["k34_coarse_us"], p["k34_rest_us"], p["k34_codes_GBps"],
                     "yes" if p["k34_equals_k33"] else "no"))


if __name__ == "__main__":
    main()

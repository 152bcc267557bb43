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
corpus row as torch does.

``--index ivf`` adds K35 ``search_topk_ivf`` (csrc/kernels/embed_search_ivf.hip:
all three launches) beside those three, one route per value of ``--nprobe``
(clamped to nlist), over the clustered index of ``search_index_ivf`` (``--nlist``,
default ceil(sqrt(N))).  Per point and nprobe also recall@k against K33 (the
share of K33's k rows that K35 returns, over the point's rows) and the mean
share of the corpus rows that a query's probed lists hold.  ``--corpus`` names
the corpora to run: ``gauss``, the seeded Gaussian unit vectors of the other
modes, which have no cluster structure, and ``clustered``: N / 256 seeded unit
centres, every row and every query a centre plus half a unit of Gaussian
noise, normalised."""

import argparse
import json
import math
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
    ap.add_argument("--index", choices=("x3", "q8", "ivf"), default="x3",
                    help="q8: K34 as a third route; ivf: K34 and K35, a route per --nprobe value")
    ap.add_argument("--corpus", default="gauss", help="gauss,clustered (the second with --index ivf)")
    ap.add_argument("--nprobe", default="1,4,16,64")
    ap.add_argument("--nlist", type=int, default=0, help="0 = ceil(sqrt(N))")
    args = ap.parse_args()

    import torch

    from triton_client_amd.ops import hip

    if not torch.cuda.is_available():
        sys.exit("search_bench needs a GPU")
    dev, D, k = torch.device("cuda"), args.dim, args.k
    gen = torch.Generator(device=dev)
    gen.manual_seed(33)
    table = []

    def unit(n, centres=None):  # seeded unit rows; with centres: one of them plus half a unit of noise, normalised
        x = torch.randn(n, D, generator=gen, device=dev)
        x /= x.norm(dim=1, keepdim=True)
        if centres is not None:
            x *= 0.5
            x += centres[torch.randint(len(centres), (n,), generator=gen, device=dev)]
            x /= x.norm(dim=1, keepdim=True)
        return x

    for kind, N in ((c, int(v)) for c in args.corpus.split(",") for v in args.n.split(",")):
        if kind not in ("gauss", "clustered"):
            sys.exit("--corpus takes gauss and clustered")
        centres = unit(max(1, N // 256)) if kind == "clustered" else None
        corpus = unit(N, centres)
        hi, lo = hip.search_index(corpus)
        q8 = hip.search_index_q8(corpus) if args.index in ("q8", "ivf") else None
        ivf = None
        if args.index == "ivf":
            ivf = hip.search_index_ivf(corpus, args.nlist or math.ceil(math.sqrt(N)))
            sizes = (ivf["offsets"][1:] - ivf["offsets"][:-1]).float()
        for rows in (int(v) for v in args.rows.split(",")):
            q = unit(rows, centres)
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
            k35 = {}  # nprobe -> the tensors of its route
            for nprobe in sorted({min(int(v), ivf["nlist"]) for v in args.nprobe.split(",")} if ivf else ()):
                t = {"probe": torch.full((rows,), nprobe, dtype=torch.int32, device=dev), "idx": torch.zeros_like(idx),
                     "sc": torch.zeros_like(sc),
                     "ws": torch.zeros(hip.search_ivf_workspace(rows, ivf["nlist"]), dtype=torch.uint8, device=dev)}
                a = (q.data_ptr(), D * 4, rows, ivf, k_row.data_ptr(), t["probe"].data_ptr(), k, nprobe,
                     t["ws"].data_ptr(), t["idx"].data_ptr(), t["sc"].data_ptr())
                routes["k35_p%d" % nprobe] = lambda a=a: hip.search_topk_ivf(*a)
                k35[nprobe] = t
            iters, times = {}, {name: [] for name in routes}
            for name, fn in routes.items():
                for _ in range(args.warmup):
                    fn()
                iters[name] = int(min(5000, max(5, args.window_s * 1e6 / window(torch, fn, 3))))
            for _ in range(args.windows):
                for name, fn in routes.items():
                    times[name].append(window(torch, fn, iters[name]))
            agree = bool((idx[:, 0].long() == torch.topk(q @ corpus.T, k).indices[:, 0]).all().item())
            point = {"corpus": kind, "rows": rows, "N": N, "D": D, "k": k, "slices": hip.search_plan(rows, N)[0],
                     "top1_agree": agree}
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
            for nprobe, t in k35.items():
                torch.cuda.synchronize()
                lists = t["ws"][:rows * nprobe * 4].view(torch.int32).reshape(rows, nprobe).long()  # the coarse step's
                hit = (t["idx"].unsqueeze(2) == idx.unsqueeze(1)).any(2).float().mean().item()
                point["k35_p%d" % nprobe].update(
                    nlist=ivf["nlist"], parts=hip.search_ivf_plan(rows, nprobe), recall=round(hit, 4),
                    scanned=round((sizes[lists.clamp(min=0)] * (lists >= 0)).sum(1).mean().item() / N, 5))
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
    if args.index == "ivf":
        print("\n| corpus | rows | N | nlist | nprobe | parts | K35 us (min .. max) | K35 / K33 | K35 / K34 | recall@%d "
              "| corpus share scanned |" % k)
        print("|---|---|---|---|---|---|---|---|---|---|---|")
        for p in table:
            for name in sorted((n for n in p if n.startswith("k35_p")), key=lambda n: int(n[5:])):
                c = p[name]
                print("| %s | %d | %d | %d | %s | %d | %.1f (%.1f .. %.1f) | %.2f | %.2f | %.3f | %.4f |"
                      % (p["corpus"], p["rows"], p["N"], c["nlist"], name[5:], c["parts"], c["us"], c["min_us"],
                         c["max_us"], c["us"] / p["k33"]["us"], c["us"] / p["k34"]["us"], c["recall"], c["scanned"]))
    if args.index in ("q8", "ivf"):
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

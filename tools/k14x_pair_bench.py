#!/usr/bin/env python3
"""K14x pair (two dense layers per launch, one read of the block input)
against the two single-layer K14x launches it replaces, per K, interleaved
round by round in one process (median, min and max of the rounds).

    python tools/k14x_pair_bench.py --imgs 128 --ks 256,512,960
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.k14x_bench import timeit  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hw", type=int, default=14)
    ap.add_argument("--tiles", type=int, default=2)
    ap.add_argument("--imgs", default="128")
    ap.add_argument("--ks", default="256,512,960")
    ap.add_argument("--ldx", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    import torch

    from triton_client_amd.ops import hip

    dev = "cuda"
    st = torch.cuda.current_stream().cuda_stream
    hw, tiles = a.hw, a.tiles
    rows = []

    def split(t):
        h = t.to(torch.bfloat16)
        return h.contiguous(), (t - h.float()).to(torch.bfloat16).contiguous()

    def layer(K):
        s = torch.rand(K, device=dev) + 0.5
        t = torch.randn(K, device=dev) * 0.1
        f1 = [hip.x3_w1_fragments(u) for u in split(torch.randn(128, K, device=dev) / K ** 0.5)]
        b1 = torch.randn(128, device=dev) * 0.1
        f2 = [hip.x3_w3f_fragments(u) for u in split(torch.randn(32, 9 * 128, device=dev) * 0.03)]
        keep = (s, t, f1[0], f1[1], b1, f2[0], f2[1])
        return keep, tuple(u.data_ptr() for u in keep)

    for imgs in [int(v) for v in a.imgs.split(",")]:
        M = imgs * hw * hw
        for K in [int(v) for v in a.ks.split(",")]:
            ldx = max(K + 64, a.ldx)
            x = torch.randn(M, ldx, device=dev)
            (k1, p1), (k2, p2) = layer(K), layer(K + 32)
            xp = x.data_ptr()

            def two():
                hip.x3_dense_small(xp, ldx, imgs, hw, hw, K, *p1, xp + 4 * K, ldx, stream=st, tiles=tiles)
                hip.x3_dense_small(xp, ldx, imgs, hw, hw, K + 32, *p2, xp + 4 * (K + 32), ldx, stream=st, tiles=tiles)

            def pair():
                hip.x3_dense_small_pair(xp, ldx, imgs, hw, hw, K, p1, p2, xp + 4 * K, ldx, stream=st, tiles=tiles)

            arms = {"two": two, "pair": pair}
            for f in arms.values():
                f()
            torch.cuda.synchronize()
            ts = {k: [] for k in arms}
            for _ in range(a.rounds):
                for k, f in arms.items():
                    ts[k].append(timeit(torch, f, a.iters))
            row = {"hw": hw, "tiles": tiles, "imgs": imgs, "K": K}
            for k, v in ts.items():
                v = sorted(v)
                row[k + "_us"] = round(v[len(v) // 2], 2)
                row[k + "_min_max"] = [round(v[0], 2), round(v[-1], 2)]
            rows.append(row)
            print(json.dumps(row), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""K11x A/B: time the fused dense-layer kernel versions on the same inputs,
interleaved (v1, v3, v1, v3, ...) so box drift hits both arms alike, and
check every version against v1's output.

    python tools/k11x_ab.py --shapes 56:64,56:224,28:128,28:480 --imgs 128 --versions 1,3

A shape is H[xW]:K[@imgs] (W = H and --imgs when left out).

A/B of two builds of the library: one process per build (TCAMD_HIP_LIB names
the other build's libtcamd_hip.so), alternating; each row carries the median
and [min, max] of its rounds.  Bit-identity of two builds:

    TCAMD_HIP_LIB=parent/libtcamd_hip.so python tools/k11x_ab.py --save-outputs DIR
    python tools/k11x_ab.py --expect DIR

--save-outputs writes every shape's and version's y; --expect compares with
torch.equal against such files and exits 1 on any difference or missing file.

Version 5 is the K11w probe (tools/probes/k11w.hip): it needs TCAMD_HIP_LIB to
name a library that exports its entry point (tools/probes/k11w.py says how).
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="56:64,56:128,56:224,28:128,28:224,28:480")
    ap.add_argument("--imgs", default="128")
    ap.add_argument("--versions", default="1,3")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default="")
    ap.add_argument("--save-outputs", default="", metavar="DIR", help="write each shape's and version's y to DIR")
    ap.add_argument("--expect", default="", metavar="DIR",
                    help="compare each y with the file --save-outputs wrote to DIR (torch.equal); exit 1 on a difference")
    a = ap.parse_args()

    import torch

    from triton_client_amd.ops import hip

    dev = "cuda"
    st = torch.cuda.current_stream().cuda_stream
    fns = {1: hip.x3_dense_fused, 3: hip.x3_dense_fused3}
    vers = [int(v) for v in a.versions.split(",")]
    if 5 in vers:
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "probes"))
        import k11w

        fns[5] = k11w.require()  # exits with the build instructions when the symbol is missing
    rows = []
    unequal = []
    if a.save_outputs:
        os.makedirs(a.save_outputs, exist_ok=True)
    for imgs_arg in [int(v) for v in a.imgs.split(",")]:
        for sh in a.shapes.split(","):
            sh, _, own = sh.partition("@")
            imgs = int(own) if own else imgs_arg
            dims, K = sh.split(":")
            K = int(K)
            hw, _, wd = dims.partition("x")
            hw = int(hw)
            wd = int(wd) if wd else hw
            M = imgs * hw * wd
            ldx = max(256, K + 32)
            g = torch.Generator(device=dev).manual_seed(hw * 1000 + K)
            x = torch.randn(M, ldx, device=dev, generator=g)

            def split(t):
                h = t.to(torch.bfloat16)
                return h.contiguous(), (t - h.float()).to(torch.bfloat16).contiguous()
            s = torch.rand(K, device=dev, generator=g) + 0.5
            t = torch.randn(K, device=dev, generator=g) * 0.1
            w1h, w1l = split(torch.randn(128, K, device=dev, generator=g) / K ** 0.5)
            b1 = torch.randn(128, device=dev, generator=g) * 0.1
            w3h, w3l = split(torch.randn(32, 9 * 128, device=dev, generator=g) * 0.03)
            f1h, f1l = hip.x3_w1_fragments(w1h), hip.x3_w1_fragments(w1l)
            frag = {v: (hip.x3_w3f_fragments(w3h), hip.x3_w3f_fragments(w3l)) for v in vers}
            outs = {}

            def run(v):
                fh, fl = frag[v]
                fns[v](x.data_ptr(), ldx, imgs, hw, wd, K, s.data_ptr(), t.data_ptr(), f1h.data_ptr(), f1l.data_ptr(),
                       b1.data_ptr(), fh.data_ptr(), fl.data_ptr(), x.data_ptr() + K * 4, ldx, stream=st)
            for v in vers:
                run(v)
                torch.cuda.synchronize()
                outs[v] = x[:, K:K + 32].clone()
                name = "y_%dx%dx%d_k%d_v%d.pt" % (imgs, hw, wd, K, v)
                if a.save_outputs:
                    torch.save(outs[v].cpu(), os.path.join(a.save_outputs, name))
                if a.expect:
                    f = os.path.join(a.expect, name)
                    if not os.path.exists(f) or not torch.equal(torch.load(f), outs[v].cpu()):
                        unequal.append(name)
            times = {v: [] for v in vers}
            for _ in range(a.rounds):
                for v in vers:
                    for _ in range(2):
                        run(v)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(a.iters):
                        run(v)
                    torch.cuda.synchronize()
                    times[v].append(1e6 * (time.perf_counter() - t0) / a.iters)
            ref = outs[vers[0]].double()
            row = {"imgs": imgs, "hw": hw, "K": K}
            if wd != hw:
                row["w"] = wd
            for v in vers:
                if not times[v]:
                    continue
                row["v%d_us" % v] = round(min(times[v]), 1)
                row["v%d_us_med" % v] = round(sorted(times[v])[len(times[v]) // 2], 1)
                row["v%d_us_max" % v] = round(max(times[v]), 1)
                row["v%d_us_all" % v] = [round(u, 1) for u in times[v]]
            for v in vers:
                row["v%d_rel_vs_v%d" % (v, vers[0])] = float((outs[v].double() - ref).norm() / ref.norm())
            rows.append(row)
            print(json.dumps(row), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    if a.expect:
        print("expect %s: %s" % (a.expect, "all equal" if not unequal else "DIFFERENT " + " ".join(unequal)), flush=True)
        if unequal:
            sys.exit(1)


if __name__ == "__main__":
    main()

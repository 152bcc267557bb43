"""Time one BERT-large (seq 384) forward per batch size on the GPU; run under
``rocprofv3 --kernel-trace --stats`` for the per-kernel split.

  python tools/bert_probe.py --batch 64 --iters 10
  python tools/bert_probe.py --batch 1 8 64 --gemm lib,auto,ours --graphs   # projection routing A/B, HIP graphs
  python tools/bert_probe.py --packed --batch 1 8 32 64 128 --fill 64 128 192 256   # padded against padding-free
  python tools/bert_probe.py --packed --fp32 --batch 1 8 32 64 --fill 64 128 192 256  # ... on the fp32-parity model

``--packed``: the graph forward as served, the padded arm (the masked graph of
``forward``) against the packed arm (``forward_packed`` at the t_cap the served
model would pick: rows x the smallest fill of 128 / 256 that holds the
tokens), alternating inside one run, every round's time printed; rows of
random lengths around each ``--fill`` (mean tokens per row).  Then the kernels
alone at the same shapes, HIP events around ``--iters`` launches: K12 (masked)
against K12v, and the plan, packed-embedding and unpack launches.  With
``--fp32`` both arms run the fp32-parity model (the padded arm is its served
padded graph) and the kernels are K12x (masked) against K12xv and the fp32
packed embedding.
"""

import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from triton_client_amd.models import bert  # noqa: E402


def _lengths(rows, fill, seed):
    """``rows`` lengths, uniform in [fill / 2, 3 fill / 2] clipped to 1..384, trimmed so they fit rows x 256 tokens."""
    g = torch.Generator().manual_seed(seed)
    n = torch.randint(max(1, fill // 2), min(384, fill + fill // 2) + 1, (rows,), generator=g)
    while int(n.sum()) > rows * 256:
        n = (n - 1).clamp(min=1)
    return n


def _event_ms(launch, iters):
    for _ in range(3):
        launch()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        launch()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def packed_probe(a, model, dev):
    import json
    import math

    from triton_client_amd.ops import hip
    from triton_client_amd.server.gpu_models import BertLarge

    S = 384
    for b in a.batch:
        for fill in a.fill:
            lens = _lengths(b, fill, 1000 * b + fill)
            tokens = int(lens.sum())
            f = next(x for x in BertLarge.PACKED_FILL if tokens <= b * x)
            t_cap = b * f
            mask = (torch.arange(S)[None, :] < lens[:, None]).to(torch.int32).to(dev)
            ids = (torch.randint(0, bert.VOCAB, (b, S), dtype=torch.int32).to(dev) * mask).contiguous()
            tt = torch.zeros(b, S, device=dev, dtype=torch.int32)
            arms = {"padded": lambda: model(ids.long(), mask, tt.long()),
                    "packed": lambda: model.forward_packed(ids, mask, tt, t_cap)}
            graphs, outs = {}, {}
            with torch.no_grad():
                for name, run in arms.items():
                    s = torch.cuda.Stream()
                    s.wait_stream(torch.cuda.current_stream())
                    with torch.cuda.stream(s):
                        for _ in range(2):
                            run()
                        g = torch.cuda.CUDAGraph()
                        with torch.cuda.graph(g, stream=s):
                            outs[name] = run()
                    torch.cuda.current_stream().wait_stream(s)
                    graphs[name] = g
                torch.cuda.synchronize()
                ts = {k: [] for k in arms}
                for _ in range(a.rounds):
                    for name in arms:
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        for _ in range(a.iters):
                            graphs[name].replay()
                        torch.cuda.synchronize()
                        ts[name].append((time.perf_counter() - t0) / a.iters * 1e3)
            valid = mask >= 1
            diff = max(((outs["packed"][k][valid] - outs["padded"][k][valid]).norm()
                        / outs["padded"][k][valid].norm()).item() for k in range(2))
            print(json.dumps({"probe": "graph", "fp32": a.fp32, "rows": b, "fill": fill, "tokens": tokens, "t_cap": t_cap,
                              "padded_ms": [round(x, 3) for x in ts["padded"]],
                              "packed_ms": [round(x, 3) for x in ts["packed"]],
                              "packed_vs_padded_rel_l2": float("%.3g" % diff)}), flush=True)
            # the kernels alone
            dt = torch.float32 if a.fp32 else torch.bfloat16
            qkv = (torch.randn(b * S, 3 * bert.HIDDEN, device=dev) * 1.5).to(dt)
            out = torch.empty(b * S, bert.HIDDEN, device=dev, dtype=dt)
            plan = bert.pack_plan(mask, t_cap, True)
            scale = 1.0 / math.sqrt(64)
            x = torch.empty(t_cap, bert.HIDDEN, device=dev, dtype=dt)
            x3 = torch.empty(t_cap, 3 * bert.HIDDEN, device=dev, dtype=torch.bfloat16) if a.fp32 else None
            lg = torch.randn(2, t_cap, device=dev)
            o2 = torch.empty(2, b * S, device=dev)
            w = model
            launches = {
                "k12_masked": lambda: hip.attention(qkv.data_ptr(), mask.data_ptr(), out.data_ptr(), b, S, bert.HEADS,
                                                    scale),
                "k12v": lambda: hip.attention_packed(qkv.data_ptr(), plan.row_len.data_ptr(), plan.cu.data_ptr(),
                                                     out.data_ptr(), b, t_cap, bert.HEADS, scale),
                "plan": lambda: bert.pack_plan(mask, t_cap, True),
                "embed_packed": lambda: hip.embed_layernorm_packed(
                    ids.data_ptr(), tt.data_ptr(), plan.tok_src.data_ptr(), w.word.weight.data_ptr(),
                    w.pos.weight.data_ptr(), w.tok_type.weight.data_ptr(), w.ln.weight.data_ptr(),
                    w.ln.bias.data_ptr(), x.data_ptr(), t_cap, b * S, S, bert.HIDDEN, bert.VOCAB, bert.TYPES, 1e-12),
                "unpack": lambda: hip.unpack_logits(lg[0].data_ptr(), lg[1].data_ptr(), plan.tok_of.data_ptr(),
                                                    o2[0].data_ptr(), o2[1].data_ptr(), b * S, t_cap),
            }
            if a.fp32:
                del launches["k12_masked"], launches["k12v"]
                launches = {
                    "k12x_masked": lambda: hip.attention_f32(qkv.data_ptr(), mask.data_ptr(), out.data_ptr(), b, S,
                                                             bert.HEADS, scale),
                    "k12xv": lambda: hip.attention_f32_packed(qkv.data_ptr(), plan.row_len.data_ptr(),
                                                              plan.cu.data_ptr(), out.data_ptr(), b, t_cap, bert.HEADS,
                                                              scale),
                    **launches,
                    "embed_packed": lambda: hip.embed_layernorm_packed(
                        ids.data_ptr(), tt.data_ptr(), plan.tok_src.data_ptr(), w.word.weight.data_ptr(),
                        w.pos.weight.data_ptr(), w.tok_type.weight.data_ptr(), w.ln.weight.data_ptr(),
                        w.ln.bias.data_ptr(), x.data_ptr(), t_cap, b * S, S, bert.HIDDEN, bert.VOCAB, bert.TYPES, 1e-12,
                        f32=True, out3=x3.data_ptr()),
                }
            us = {k: [] for k in launches}
            for _ in range(a.rounds):
                for name, launch in launches.items():
                    us[name].append(round(_event_ms(launch, a.iters) * 1e3, 2))
            print(json.dumps({"probe": "kernels_us", "fp32": a.fp32, "rows": b, "fill": fill, "tokens": tokens, "t_cap": t_cap,
                              "plan_includes": "4 torch.empty and the launch", **us}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[64])
    ap.add_argument("--seq", type=int, default=384)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--tuned-table", default="",
                    help="A/B against TunableOp reading this solution table (tuning off), e.g. "
                         "triton_client_amd/models/tuned/bert_large_gfx950.csv")
    ap.add_argument("--tunable", default="",
                    help="A/B against PyTorch TunableOp (hipBLASLt / rocBLAS solution search per GEMM shape); "
                         "the tuned results go to this CSV path")
    ap.add_argument("--gemm", default="", help="A/B the projection routing modes (bert.GEMM), e.g. lib,auto,ours")
    ap.add_argument("--graphs", action="store_true", help="time HIP-graph replays of the forward (as served)")
    ap.add_argument("--fp32", action="store_true", help="the fp32-parity model (bert_large_fp32: bf16x3 projections)")
    ap.add_argument("--packed", action="store_true",
                    help="padded graph against padding-free graph at each --batch (rows) and --fill, then the kernels")
    ap.add_argument("--fill", type=int, nargs="+", default=[64, 128, 192, 256],
                    help="--packed: mean valid tokens per row")
    ap.add_argument("--layers", type=int, default=bert.LAYERS)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    if a.packed:
        if a.fp32:
            return packed_probe(a, bert.prepare_x3(bert.build(device=dev, dtype=torch.float32, layers=a.layers)), dev)
        return packed_probe(a, bert.build(device=dev, layers=a.layers), dev)
    model = (bert.prepare_x3(bert.build(device=dev, dtype=torch.float32)) if a.fp32 else bert.build(device=dev))
    for b in a.batch:
        ids = torch.randint(0, bert.VOCAB, (b, a.seq), device=dev)
        mask = torch.ones(b, a.seq, device=dev, dtype=torch.int64)
        tt = torch.zeros(b, a.seq, device=dev, dtype=torch.int64)
        variants = {"default": 0}
        if a.gemm:
            variants = {m: 0 for m in a.gemm.split(",")}
        tun = None
        if a.tuned_table:
            import torch.cuda.tunable as tun

            assert bert.use_tuned_gemms(a.tuned_table), "the table does not load in this process"
            variants = {"default": 0, "tunableop": 0}
        elif a.tunable:
            import torch.cuda.tunable as tun

            tun.set_filename(a.tunable)
            variants = {"default": 0, "tunableop": 0}
            with torch.no_grad():  # tune every GEMM shape of this batch once, outside the timed rounds
                tun.enable(True)
                tun.tuning_enable(True)
                model(ids, mask, tt)
                torch.cuda.synchronize()
                tun.tuning_enable(False)
                tun.enable(False)
        ts = {k: [] for k in variants}
        graphs = {}
        with torch.no_grad():
            for name in variants:
                if tun is not None:
                    tun.enable(name == "tunableop")
                if a.gemm:
                    bert.GEMM = name
                s = torch.cuda.Stream()
                s.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(s):  # warm-up on the capture stream (K17 allocates its workspace there)
                    for _ in range(2):
                        model(ids, mask, tt)
                torch.cuda.current_stream().wait_stream(s)
                if a.graphs:
                    with torch.cuda.stream(s):
                        g = torch.cuda.CUDAGraph()
                        with torch.cuda.graph(g, stream=s):
                            model(ids, mask, tt)
                    torch.cuda.current_stream().wait_stream(s)
                    graphs[name] = g
            torch.cuda.synchronize()
            for _ in range(a.rounds):
                for name in variants:
                    if tun is not None:
                        tun.enable(name == "tunableop")
                    if a.gemm:
                        bert.GEMM = name
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(a.iters):
                        if a.graphs:
                            graphs[name].replay()
                        else:
                            model(ids, mask, tt)
                    torch.cuda.synchronize()
                    ts[name].append((time.perf_counter() - t0) / a.iters)
        for name, v in ts.items():
            dt = sorted(v)[len(v) // 2]
            tf = bert.flops_per_sequence(a.seq) * b / dt / 1e12
            print({"batch": b, "variant": name, "fp32": a.fp32, "ms": round(dt * 1e3, 3), "seq_per_s": round(b / dt, 1),
                   "tflops": round(tf, 1)}, flush=True)


if __name__ == "__main__":
    main()

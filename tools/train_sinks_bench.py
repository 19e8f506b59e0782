"""What attention sinks cost in training on the MI355X (profiles/train_sinks.md): the forward with ``sinks=`` against the sink-less
forward forced to the same 8-wave kernel (selector 44: the price of the epilogue) and against the default sink-less forward (the
persistent assembly kernel where it takes the problem: the price of leaving it), and the sink-gradient launches against the backward
they follow.  All paths of a row are alternated in one process.

Per row every path is one captured graph that runs the call once over each operand set of a pool of >= 768 MiB of q, k, v (the 256 MiB
Infinity Cache cannot serve them), replayed ``--reps`` times between device events.  The table gives the median time of a call, the two
ratios and the run-to-run spread of the sink-less paths: the distance between two medians of the same path and the (max - min) / median
of its replays.  The tool asserts nothing about time.

    python tools/train_sinks_bench.py [--reps 9] [--quick] [--json out.jsonl]

Rows: C3 (B 4, H 16, S 4096, D 128, causal), C2 (B 4, H 12, S 1024, D 64, full), one packed batch (H 16 / Hkv 4, D 64, causal, lengths
4096, 2048, 1024, 512, 300, 200, 12: 8192 rows), and for C3 the backward with and without the sink-gradient launches."""

from __future__ import annotations

import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from photonic_flash_attention_amd import ops  # noqa: E402

MIN_POOL = 768 << 20
BF16 = torch.bfloat16
PACKED_LENS = [4096, 2048, 1024, 512, 300, 200, 12]


def timed(paths, n, reps):
    """{name: sweep} -> {name: [us per call]}: each sweep captured once, the graphs replayed alternately."""
    graphs = {}
    for name, sweep in paths.items():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            sweep()                                    # warm-up: code objects, allocator
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            sweep()
        graphs[name] = g
    times = {p: [] for p in graphs}
    for g in graphs.values():
        g.replay()
    torch.cuda.synchronize()
    for _ in range(reps):
        for name, g in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / n)
    return times


def med(t):
    return sorted(t)[len(t) // 2]


def spread(a, b):
    """(distance of the two medians, (max - min) of all replays), both over the mean median"""
    m = 0.5 * (med(a) + med(b))
    return abs(med(a) - med(b)) / m, (max(a + b) - min(a + b)) / m


def forward_row(name, B, H, Hkv, S, D, causal, reps, dev):
    n = max(2, math.ceil(MIN_POOL / ((B * S * H * D + 2 * B * S * Hkv * D) * 2)))
    pool = [tuple(torch.randn(B, S, h, D, device=dev, dtype=BF16).permute(0, 2, 1, 3) for h in (H, Hkv, Hkv)) for _ in range(n)]
    out = torch.empty(B, S, H, D, device=dev, dtype=BF16).permute(0, 2, 1, 3)
    sinks = torch.randn(H, device=dev) + math.log(S / 2 if causal else S)          # of the order of the rows' LSE

    def sweep(**kw):
        return lambda: [ops.fa3_forward(q, k, v, causal=causal, out=out, **kw) for q, k, v in pool]

    t = timed({"w8_a": sweep(_variant=44), "default_a": sweep(), "sinks": sweep(sinks=sinks), "w8_b": sweep(_variant=44), "default_b": sweep()},
              n, reps)
    return finish(name, t, n)


def packed_row(name, H, Hkv, D, reps, dev):
    total = sum(PACKED_LENS)
    cu = torch.tensor([0] + list(torch.tensor(PACKED_LENS).cumsum(0)), dtype=torch.int32, device=dev)
    kw = dict(cu_seqlens_q=cu, cu_seqlens_k=cu, max_seqlen_q=max(PACKED_LENS), max_seqlen_k=max(PACKED_LENS), causal=True)
    n = max(2, math.ceil(MIN_POOL / ((total * H * D + 2 * total * Hkv * D) * 2)))
    pool = [tuple(torch.randn(total, h, D, device=dev, dtype=BF16) for h in (H, Hkv, Hkv)) for _ in range(n)]
    out = torch.empty(total, H, D, device=dev, dtype=BF16)
    sinks = torch.randn(H, device=dev) + 6.0

    def sweep(**more):
        return lambda: [ops.fa3_varlen_forward(q, k, v, out=out, **kw, **more) for q, k, v in pool]

    # (the packed forward has one kernel: "default" is the 8-wave kernel's packed mode itself)
    t = timed({"w8_a": sweep(), "default_a": sweep(), "sinks": sweep(sinks=sinks), "w8_b": sweep(), "default_b": sweep()}, n, reps)
    return finish(name, t, n)


def finish(name, t, n):
    w8, dflt = 0.5 * (med(t["w8_a"]) + med(t["w8_b"])), 0.5 * (med(t["default_a"]) + med(t["default_b"]))
    ab, rng = spread(t["w8_a"], t["w8_b"])
    return dict(row=name, n_sets=n, w8_us=round(w8, 2), default_us=round(dflt, 2), sinks_us=round(med(t["sinks"]), 2),
                sinks_over_w8=round(med(t["sinks"]) / w8, 4), sinks_over_default=round(med(t["sinks"]) / dflt, 4), w8_ab=round(ab, 4),
                w8_range=round(rng, 4), default_ab=round(spread(t["default_a"], t["default_b"])[0], 4))


def backward_row(name, B, H, S, D, causal, reps, dev):
    n = max(2, math.ceil(MIN_POOL / (5 * B * S * H * D * 2)))
    sinks = torch.randn(H, device=dev) + math.log(S / 2 if causal else S)
    pool = []
    for _ in range(n):
        q, k, v, g = (torch.randn(B, S, H, D, device=dev, dtype=BF16).permute(0, 2, 1, 3) for _ in range(4))
        o, lse = ops.fa3_forward(q, k, v, causal=causal, return_lse=True, sinks=sinks)
        pool.append((q, k, v, o, g, lse))

    def sweep(**kw):
        return lambda: [ops.fa3_backward(*ops_, causal=causal, **kw) for ops_ in pool]

    delta = torch.randn(B, H, S, device=dev)
    grad_only = lambda: [ops.fa3_sink_grad(p[5], delta, sinks) for p in pool]      # noqa: E731
    t = timed({"bwd_a": sweep(), "bwd_sinks": sweep(sinks=sinks), "sink_grad": grad_only, "bwd_b": sweep()}, n, reps)
    bwd = 0.5 * (med(t["bwd_a"]) + med(t["bwd_b"]))
    ab, rng = spread(t["bwd_a"], t["bwd_b"])
    return dict(row=name, n_sets=n, bwd_us=round(bwd, 2), bwd_sinks_us=round(med(t["bwd_sinks"]), 2), sink_grad_us=round(med(t["sink_grad"]), 2),
                bwd_sinks_over_bwd=round(med(t["bwd_sinks"]) / bwd, 4), sink_grad_over_bwd=round(med(t["sink_grad"]) / bwd, 4),
                bwd_ab=round(ab, 4), bwd_range=round(rng, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--quick", action="store_true", help="C2 forward and the C3 backward only")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    print("| forward | 8-wave us | default us | sinks us | sinks / 8-wave | sinks / default | 8-wave A vs B | 8-wave (max - min) / median | default A vs B |")
    print("|---|---|---|---|---|---|---|---|---|")
    fwd = [lambda: forward_row("C2: B4 H12 S1024 D64 full", 4, 12, 12, 1024, 64, False, args.reps, dev)]
    if not args.quick:
        fwd = [lambda: forward_row("C3: B4 H16 S4096 D128 causal", 4, 16, 16, 4096, 128, True, args.reps, dev)] + fwd + \
              [lambda: packed_row("packed: H16/4 D64 causal, 8192 rows", 16, 4, 64, args.reps, dev)]
    for make in fwd:
        r = make()
        rows.append(r)
        print(f"| {r['row']} | {r['w8_us']} | {r['default_us']} | {r['sinks_us']} | {r['sinks_over_w8']:.4f} | {r['sinks_over_default']:.4f} | "
              f"{r['w8_ab']:.4f} | {r['w8_range']:.4f} | {r['default_ab']:.4f} |", flush=True)
        torch.cuda.empty_cache()
    print()
    print("| backward | backward us | backward + sink grad us | sink grad alone us | (backward + sink grad) / backward | sink grad / backward | "
          "backward A vs B | backward (max - min) / median |")
    print("|---|---|---|---|---|---|---|---|")
    r = backward_row("C3: B4 H16 S4096 D128 causal", 4, 16, 4096, 128, True, args.reps, dev)
    rows.append(r)
    print(f"| {r['row']} | {r['bwd_us']} | {r['bwd_sinks_us']} | {r['sink_grad_us']} | {r['bwd_sinks_over_bwd']:.4f} | {r['sink_grad_over_bwd']:.4f} | "
          f"{r['bwd_ab']:.4f} | {r['bwd_range']:.4f} |", flush=True)
    if args.json:
        with open(args.json, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()

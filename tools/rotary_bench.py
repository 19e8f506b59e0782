"""What the fused rotary embedding of the training calls costs on the MI355X (profiles/rotary_train.md): ``ops.apply_rotary`` -- one
launch for q and k, one conjugate launch as its backward -- against the torch composition a user writes today, Hugging Face's
``x * cos + rotate_half(x) * sin`` in the operands' dtype with its autograd backward.  All paths of a row are alternated in one process.

Per row every path is one captured graph that runs the call once over each operand set of a pool of >= 768 MiB of q and k (the 256 MiB
Infinity Cache cannot serve them), replayed ``--reps`` times between device events.  The table gives the median time of a call, the
ratios, the bytes per second the fused forward reaches -- every element of q and k read once and written once -- and the run-to-run
spread of the fused forward: the distance between two medians of the same path and the (max - min) / median of its replays.  The tool
asserts nothing about time.

    python tools/rotary_bench.py [--reps 9] [--quick] [--json out.jsonl]

Rows: C3 (B 4, H 16, S 4096, D 128), a GQA shape (B 4, H 32 / Hkv 8, S 4096, D 64), both as the [B, S, H, D] views a projection leaves,
and one packed batch (H 16 / Hkv 4, D 64, lengths 4096, 2048, 1024, 512, 300, 200, 12: 8192 rows).  The rotation covers the whole head."""

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


def rotate_half(x):
    x1, x2 = x[..., : x.shape[-1] // 2], x[..., x.shape[-1] // 2:]
    return torch.cat((-x2, x1), dim=-1)


def hf_rotary(q, k, cos, sin):
    """Hugging Face's apply_rotary_pos_emb: cos / sin in the operands' dtype, broadcast over the heads."""
    return q * cos + rotate_half(q) * sin, k * cos + rotate_half(k) * sin


def row(name, shape_of, H, Hkv, D, reps, dev, fused_kw, hf_tables):
    """One row: ``shape_of(heads)`` makes an operand; ``fused_kw``: what ``ops.apply_rotary`` takes; ``hf_tables``: (cos, sin) for ``hf_rotary``."""
    elems = sum(shape_of(h).numel() for h in (H, Hkv))
    n = max(2, math.ceil(MIN_POOL / (2 * elems * 2)))       # q, k and their incoming gradients
    pool = [tuple(shape_of(h).requires_grad_(True) for h in (H, Hkv)) + tuple(shape_of(h) for h in (H, Hkv)) for _ in range(n)]
    hc, hs = hf_tables

    def fwd(f):
        def sweep():
            with torch.no_grad():
                return [f(q, k) for q, k, _, _ in pool]
        return sweep

    def fwdbwd(f):
        return lambda: [torch.autograd.grad(f(q, k), (q, k), (gq, gk)) for q, k, gq, gk in pool]

    def inplace():
        with torch.no_grad():
            for _, _, gq, gk in pool:                      # (the gradients' buffers: data nobody keeps)
                ops.apply_rotary(gq, gk, inplace=True, **fused_kw)

    fused, torch_ = (lambda q, k: ops.apply_rotary(q, k, **fused_kw)), (lambda q, k: hf_rotary(q, k, hc, hs))
    t = timed({"fused_a": fwd(fused), "torch": fwd(torch_), "inplace": inplace, "fused_fb": fwdbwd(fused), "torch_fb": fwdbwd(torch_),
               "fused_b": fwd(fused)}, n, reps)
    f = 0.5 * (med(t["fused_a"]) + med(t["fused_b"]))
    ab, rng = spread(t["fused_a"], t["fused_b"])
    moved = 2 * elems * 2                                   # bytes: every element of q and k read once and written once
    return dict(row=name, n_sets=n, fused_us=round(f, 2), torch_us=round(med(t["torch"]), 2), inplace_us=round(med(t["inplace"]), 2),
                fused_fwdbwd_us=round(med(t["fused_fb"]), 2), torch_fwdbwd_us=round(med(t["torch_fb"]), 2),
                torch_over_fused=round(med(t["torch"]) / f, 3), torch_over_fused_fwdbwd=round(med(t["torch_fb"]) / med(t["fused_fb"]), 3),
                fused_tb_s=round(moved / f / 1e6, 3), inplace_tb_s=round(moved / med(t["inplace"]) / 1e6, 3),
                fwdbwd_tb_s=round(2 * moved / med(t["fused_fb"]) / 1e6, 3), fused_ab=round(ab, 4), fused_range=round(rng, 4))


def dense_row(name, B, H, Hkv, S, D, reps, dev):
    cos, sin = ops.rotary_tables(S, D, device=dev)
    hf = tuple(torch.cat((t, t), dim=-1).to(BF16)[None, None] for t in (cos, sin))          # [1, 1, S, D]
    return row(name, lambda h: torch.randn(B, S, h, D, device=dev, dtype=BF16).permute(0, 2, 1, 3), H, Hkv, D, reps, dev,
               dict(rotary_cos=cos, rotary_sin=sin), hf)


def packed_row(name, H, Hkv, D, reps, dev):
    total = sum(PACKED_LENS)
    cu = torch.tensor([0] + torch.tensor(PACKED_LENS).cumsum(0).tolist(), dtype=torch.int32, device=dev)
    cos, sin = ops.rotary_tables(max(PACKED_LENS), D, device=dev)
    pos = torch.cat([torch.arange(n, device=dev) for n in PACKED_LENS])                     # what a user gathers the tables by
    hf = tuple(torch.cat((t, t), dim=-1).to(BF16)[pos][:, None] for t in (cos, sin))        # [total, 1, D]
    return row(name, lambda h: torch.randn(total, h, D, device=dev, dtype=BF16), H, Hkv, D, reps, dev,
               dict(rotary_cos=cos, rotary_sin=sin, cu_seqlens=cu, max_seqlen=max(PACKED_LENS)), hf)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--quick", action="store_true", help="the packed row only")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = [lambda: packed_row("packed: H16/4 D64, 8192 rows", 16, 4, 64, args.reps, dev)]
    if not args.quick:
        rows = [lambda: dense_row("C3: B4 H16 S4096 D128", 4, 16, 16, 4096, 128, args.reps, dev),
                lambda: dense_row("GQA: B4 H32/8 S4096 D64", 4, 32, 8, 4096, 64, args.reps, dev)] + rows
    print("| shape | fused fwd us | torch fwd us | torch / fused | fused fwd TB/s | in place us | in place TB/s | fused fwd+bwd us | torch fwd+bwd us | "
          "torch / fused, fwd+bwd | fused fwd+bwd TB/s | fused A vs B | fused (max - min) / median |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    done = []
    for make in rows:
        r = make()
        done.append(r)
        print(f"| {r['row']} | {r['fused_us']} | {r['torch_us']} | {r['torch_over_fused']:.3f} | {r['fused_tb_s']:.3f} | {r['inplace_us']} | "
              f"{r['inplace_tb_s']:.3f} | {r['fused_fwdbwd_us']} | {r['torch_fwdbwd_us']} | {r['torch_over_fused_fwdbwd']:.3f} | {r['fwdbwd_tb_s']:.3f} | "
              f"{r['fused_ab']:.4f} | {r['fused_range']:.4f} |", flush=True)
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "a") as f:
            for r in done:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()

"""What the fused QK-norm with rotary of the training calls costs on the MI355X (profiles/qk_norm.md): ``ops.qk_norm`` -- one launch for
the norm and the rotation of q and k, two launches as its backward -- against the compositions a user writes today, with the method of
tools/rotary_bench.py:

  (a)  Hugging Face's ``Qwen3RMSNorm`` on q and k in torch, then ``ops.apply_rotary``, with autograd's backward;
  (b)  the same norm, then the torch ``x * cos + rotate_half(x) * sin``.

All paths of a row are alternated in one process, ``ops.apply_rotary`` alone among them, so that the bytes per second the fused call
reaches stand beside the plain rotation's in the same run.  Per row every path is one captured graph that runs the call once over each
operand set of a pool of >= 768 MiB of q and k (the 256 MiB Infinity Cache cannot serve them), replayed ``--reps`` times between device
events.  The table gives the median time of a call, the ratios, the bytes per second -- every element of q and k read once and written
once; in the backward x and dy read and dx written -- and the run-to-run spread of the fused forward.

The one pass mark: the fused forward is not slower than (a) at C3's shape; the tool exits with status 1 if it is.  Every other figure is
written down and not judged.

    python tools/qk_norm_bench.py [--reps 9] [--quick] [--json out.jsonl]

Rows: C3 (B 4, H 16, S 4096, D 128), two GQA shapes (B 4, H 32 / Hkv 8, S 4096, D 64 and D 128), as the [B, S, H, D] views a projection
leaves, and one packed batch (H 16 / Hkv 4, D 64, lengths 4096, 2048, 1024, 512, 300, 200, 12: 8192 rows).  The rotation covers the
whole head; the weights are bf16 parameters."""

from __future__ import annotations

import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from photonic_flash_attention_amd import ops  # noqa: E402
from rotary_bench import BF16, MIN_POOL, PACKED_LENS, hf_rotary, med, spread, timed  # noqa: E402

EPS = 1e-6


def hf_rmsnorm(x, w):
    """Hugging Face's Qwen3RMSNorm.forward over the head dim."""
    dt = x.dtype
    x = x.to(torch.float32)
    var = x.pow(2).mean(-1, keepdim=True)
    x = x * torch.rsqrt(var + EPS)
    return w * x.to(dt)


def row(name, shape_of, H, Hkv, D, reps, dev, rot_kw, hf_tables):
    elems = sum(shape_of(h).numel() for h in (H, Hkv))
    n = max(2, math.ceil(MIN_POOL / (2 * elems * 2)))       # q, k and their incoming gradients
    pool = [tuple(shape_of(h).requires_grad_(True) for h in (H, Hkv)) + tuple(shape_of(h) for h in (H, Hkv)) for _ in range(n)]
    wq, wk = ((1.0 + 0.1 * torch.randn(D, device=dev)).to(BF16).requires_grad_(True) for _ in range(2))
    hc, hs = hf_tables

    def fused(q, k):
        return ops.qk_norm(q, k, q_weight=wq, k_weight=wk, eps=EPS, **rot_kw)

    def comp_a(q, k):
        return ops.apply_rotary(hf_rmsnorm(q, wq), hf_rmsnorm(k, wk), **rot_kw)

    def comp_b(q, k):
        return hf_rotary(hf_rmsnorm(q, wq), hf_rmsnorm(k, wk), hc, hs)

    def rotary(q, k):
        return ops.apply_rotary(q, k, **rot_kw)

    def fwd(f):
        def sweep():
            with torch.no_grad():
                return [f(q, k) for q, k, _, _ in pool]
        return sweep

    def fwdbwd(f, weights=True):
        leaves = (lambda q, k: (q, k, wq, wk)) if weights else (lambda q, k: (q, k))
        return lambda: [torch.autograd.grad(f(q, k), leaves(q, k), (gq, gk)) for q, k, gq, gk in pool]

    t = timed({"fused_a": fwd(fused), "comp_a": fwd(comp_a), "comp_b": fwd(comp_b), "rotary": fwd(rotary), "fused_fb": fwdbwd(fused),
               "comp_a_fb": fwdbwd(comp_a), "comp_b_fb": fwdbwd(comp_b), "rotary_fb": fwdbwd(rotary, False), "fused_b": fwd(fused)}, n, reps)
    m = {k: med(v) for k, v in t.items()}
    f = 0.5 * (m["fused_a"] + m["fused_b"])
    ab, rng = spread(t["fused_a"], t["fused_b"])
    moved = 2 * elems * 2                                   # bytes of a forward: every element of q and k read once and written once
    bwd = m["fused_fb"] - f                                 # the backward's two launches: x and dy read, dx written
    return dict(row=name, n_sets=n, fused_us=round(f, 2), comp_a_us=round(m["comp_a"], 2), comp_b_us=round(m["comp_b"], 2),
                rotary_us=round(m["rotary"], 2), a_over_fused=round(m["comp_a"] / f, 3), b_over_fused=round(m["comp_b"] / f, 3),
                fused_tb_s=round(moved / f / 1e6, 3), rotary_tb_s=round(moved / m["rotary"] / 1e6, 3),
                fused_fwdbwd_us=round(m["fused_fb"], 2), comp_a_fwdbwd_us=round(m["comp_a_fb"], 2), comp_b_fwdbwd_us=round(m["comp_b_fb"], 2),
                rotary_fwdbwd_us=round(m["rotary_fb"], 2), a_over_fused_fwdbwd=round(m["comp_a_fb"] / m["fused_fb"], 3),
                b_over_fused_fwdbwd=round(m["comp_b_fb"] / m["fused_fb"], 3), fused_bwd_us=round(bwd, 2),
                fused_bwd_tb_s=round(1.5 * moved / bwd / 1e6, 3), fused_ab=round(ab, 4), fused_range=round(rng, 4))


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


COLUMNS = [("fused fwd us", "fused_us"), ("(a) fwd us", "comp_a_us"), ("(b) fwd us", "comp_b_us"), ("(a) / fused", "a_over_fused"),
           ("(b) / fused", "b_over_fused"), ("apply_rotary fwd us", "rotary_us"), ("fused fwd TB/s", "fused_tb_s"),
           ("apply_rotary fwd TB/s", "rotary_tb_s"), ("fused fwd+bwd us", "fused_fwdbwd_us"), ("(a) fwd+bwd us", "comp_a_fwdbwd_us"),
           ("(b) fwd+bwd us", "comp_b_fwdbwd_us"), ("(a) / fused, fwd+bwd", "a_over_fused_fwdbwd"), ("(b) / fused, fwd+bwd", "b_over_fused_fwdbwd"),
           ("apply_rotary fwd+bwd us", "rotary_fwdbwd_us"), ("fused bwd us", "fused_bwd_us"), ("fused bwd TB/s", "fused_bwd_tb_s"),
           ("fused A vs B", "fused_ab"), ("fused (max - min) / median", "fused_range")]


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
                lambda: dense_row("GQA: B4 H32/8 S4096 D64", 4, 32, 8, 4096, 64, args.reps, dev),
                lambda: dense_row("GQA: B4 H32/8 S4096 D128", 4, 32, 8, 4096, 128, args.reps, dev)] + rows
    print("| shape | " + " | ".join(c for c, _ in COLUMNS) + " |")
    print("|" + "---|" * (len(COLUMNS) + 1))
    done = []
    for make in rows:
        r = make()
        done.append(r)
        print(f"| {r['row']} | " + " | ".join(str(r[k]) for _, k in COLUMNS) + " |", flush=True)
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "a") as f:
            for r in done:
                f.write(json.dumps(r) + "\n")
    c3 = [r for r in done if r["row"].startswith("C3")]
    if c3 and c3[0]["fused_us"] > c3[0]["comp_a_us"]:
        print("PASS MARK MISSED: the fused forward is slower than composition (a) at C3's shape")
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())

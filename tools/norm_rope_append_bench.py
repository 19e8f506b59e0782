"""What the fused write side of a serving step costs on the MI355X (profiles/norm_rope_append.md): ``ops.norm_rope_append`` -- QK-norm,
rotary, the append and, over an FP8 cache, the quantising store in one launch -- against what the library offered for the same result
before it, with the method of tools/rotary_bench.py:

  16-bit cache   ``ops.qk_norm(rot_dim 0, inplace=True)`` on q and k, then ``ops.rope_append``                       (two launches)
  FP8 cache      ``ops.qk_norm`` with the tables into temporaries, then the quantising ``ops.kv_append``              (two launches)

The paths of a row are alternated in one process, the fused call twice, so that the spread of repeats stands in front of every ratio.
Per row every path is one captured graph that runs the call once over each operand set of a pool of >= 768 MiB of q, k_new and v_new
(the 256 MiB Infinity Cache cannot serve them) and over as many caches as 768 MiB hold, replayed ``--reps`` times between device events.

The one pass mark: at the decode step over a 16-bit cache the fused call is not slower than the composition; the tool exits with
status 1 if it is.  Every other figure is written down and not judged.

    python tools/norm_rope_append_bench.py [--reps 9] [--out profiles/norm_rope_append.md]

Rows: a decode step (B 64, H 32 / Hkv 8, D 128, one row a sequence, paged, lengths 1000 .. 1063) and a chunk (B 4 x 2048 rows, the same
heads, contiguous caches), bf16, R = D, fp32 weights."""

from __future__ import annotations

import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from photonic_flash_attention_amd import ops  # noqa: E402
from rotary_bench import BF16, MIN_POOL, med, spread, timed  # noqa: E402

H, HKV, D, PAGE, MAX_POS = 32, 8, 128, 64, 4096


def row(name, B, Sq, lens, paged, fp8, reps, dev):
    """One row of the table: -> (name, launches of the baseline, {path: [us]}, bytes moved by a call)."""
    rows_bytes = B * Sq * (H + 2 * HKV) * D * 2
    n = max(2, math.ceil(MIN_POOL / rows_bytes))
    sets = [tuple(torch.randn(B, Sq, h, D, device=dev).to(BF16).transpose(1, 2) for h in (H, HKV, HKV)) for _ in range(n)]
    Smax = -(-max(lens) // PAGE) * PAGE
    pages = Smax // PAGE
    cdt, cbytes = (torch.uint8, 1) if fp8 else (BF16, 2)
    shape = (B * pages, PAGE, HKV, D) if paged else (B, Smax, HKV, D)
    n_caches = max(2, min(n, math.ceil(MIN_POOL / (2 * math.prod(shape) * cbytes))))
    caches = [tuple(torch.zeros(shape, dtype=cdt, device=dev).transpose(1, 2) for _ in range(2)) for _ in range(n_caches)]
    if fp8:
        caches = [tuple(c.view(ops.FP8) for c in pair) for pair in caches]
    seqlens = torch.tensor(lens, dtype=torch.int32, device=dev)
    where = dict(cache_seqlens=seqlens)
    if paged:
        where["block_table"] = torch.randperm(B * pages, device=dev).to(torch.int32).view(B, pages)
    cos, sin = ops.rotary_tables(MAX_POS, D, device=dev)
    wq, wk = (1.0 + 0.1 * torch.randn(D, device=dev) for _ in range(2))
    first = seqlens - Sq                                          # the position of a sequence's first new row, for the baseline's qk_norm
    descales = dict(k_descale=torch.full((HKV,), 0.05, device=dev), v_descale=torch.full((HKV,), 0.05, device=dev)) if fp8 else {}

    def fused(i):
        q, k, v = sets[i]
        ops.norm_rope_append(k, v, *caches[i % n_caches], q=q, q_out=q, q_weight=wq, k_weight=wk, rotary_cos=cos, rotary_sin=sin,
                             **where, **descales)

    def composed(i):
        q, k, v = sets[i]
        if fp8:
            q2, k2 = ops.qk_norm(q, k, q_weight=wq, k_weight=wk, rotary_cos=cos, rotary_sin=sin, pos_offsets=first)
            ops.kv_append(k2, v, *caches[i % n_caches], **where, **descales)
        else:
            ops.qk_norm(q, k, q_weight=wq, k_weight=wk, inplace=True)
            ops.rope_append(k, v, *caches[i % n_caches], q=q, q_out=q, rotary_cos=cos, rotary_sin=sin, **where)

    sweep = lambda call: lambda: [call(i) for i in range(n)]
    times = timed({"fused": sweep(fused), "composed": sweep(composed), "fused again": sweep(fused)}, n, reps)
    kept = B * min(Sq, max(lens)) * 2 * HKV * D                  # cache elements written
    return name, times, rows_bytes + B * Sq * H * D * 2 + kept * cbytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "norm_rope_append.md"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    decode = dict(B=64, Sq=1, lens=[1000 + b for b in range(64)], paged=True)
    chunk = dict(B=4, Sq=2048, lens=[2048, 4096, 3000, 2500], paged=False)
    rows = [row(f"{label}, {'FP8' if fp8 else '16-bit'} cache", fp8=fp8, reps=a.reps, dev=dev, **shape)
            for label, shape in (("decode step (B 64 x 1 row, paged)", decode), ("chunk (B 4 x 2048 rows)", chunk)) for fp8 in (False, True)]
    lines = ["# `ops.norm_rope_append` against the two-launch compositions (tools/norm_rope_append_bench.py)", "",
             f"One MI355X, bf16, H {H} / Hkv {HKV}, D {D}, R = D, fp32 weights; captured calls alternated in one process, {a.reps} replays a path,",
             "operands cycled past the Infinity Cache; the median time of one call.  Spread: the distance of the two fused medians and",
             "(max - min) over all fused replays, both over the mean median.  A ratio inside the spread says nothing.", "",
             "| row | fused, us | composed, us | composed / fused | fused GB/s | spread (medians, range) |", "|---|---|---|---|---|---|"]
    for name, t, nbytes in rows:
        f, c = med(t["fused"] + t["fused again"]), med(t["composed"])
        s_med, s_rng = spread(t["fused"], t["fused again"])
        lines.append(f"| {name} | {f:.2f} | {c:.2f} | {c / f:.2f} | {nbytes / f / 1e3:.0f} | {100 * s_med:.1f} %, {100 * s_rng:.1f} % |")
    t = rows[0][1]
    ok = med(t["fused"] + t["fused again"]) <= med(t["composed"])
    lines += ["", f"Pass mark (the fused call is not slower than the composition at the decode step over a 16-bit cache): **{'held' if ok else 'MISSED'}**.",
              "No other ratio is judged."]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()

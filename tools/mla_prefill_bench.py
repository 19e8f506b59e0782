"""Non-absorbed MLA prefill on the MI355X: ``ops.mla_prefill`` (bf16, H 128 and H 16, one shared rotary key head) against
(a) what a user had without it -- q and k padded from 192 to 256 columns, v from 128 to 256, the rotary key expanded over the heads,
through ``ops.fa3_prefill_cache`` at D 256 -- timed on operands padded beforehand and with the padding copies; (b)
``scaled_dot_product_attention`` on the padded operands; (c) as a yardstick of rate, ``ops.fa3_varlen_forward`` at D 128 on the same
(row, key) pairs.

Causal self-attention over 8192 tokens cut into sequences of 1024 / 4096 / 8192, and a 512-row chunk over 8192 / 32768 context keys,
not causal.  The paths are timed alternately in one process with device events, minimum and maximum over the repetitions.  Flops are
2 * 320 * visible (row, key) pairs * H for every path: what the operation needs, not what a padded path executes.

    python tools/mla_prefill_bench.py [--reps 5] [--out profiles/mla_prefill.md]
"""

from __future__ import annotations

import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from photonic_flash_attention_amd import ops  # noqa: E402

SCALE = 192 ** -0.5
BF = torch.bfloat16


def _time(paths, reps, inner):
    """name -> (min, max) microseconds a call, the paths alternating; a path that raises is reported, not timed."""
    failed = {}
    for name, f in paths.items():
        try:
            f(), f()
        except (RuntimeError, ValueError) as e:
            failed[name] = str(e).splitlines()[0][:80]
    paths = {name: f for name, f in paths.items() if name not in failed}
    torch.cuda.synchronize()
    times = {name: [] for name in paths}
    for _ in range(reps):
        for name, f in paths.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                f()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / inner)
    return {**{name: (min(t), max(t)) for name, t in times.items()}, **{name: (None, why) for name, why in failed.items()}}


def bench_shape(H, B, Sq, Sk, causal, reps, dev):
    """B sequences of Sq rows over Sk keys each -> (visible pairs per head, results)."""
    tq, tk = B * Sq, B * Sk
    q = torch.randn(tq, H, 192, device=dev, dtype=BF)
    kv = torch.randn(tk, H, 256, device=dev, dtype=BF)                     # the projection output: k_nope | v
    kn, v = kv[..., :128], kv[..., 128:]
    kr = torch.randn(tk, 1, 64, device=dev, dtype=BF)
    cu_q = torch.arange(B + 1, dtype=torch.int32, device=dev) * Sq
    cu_k = torch.arange(B + 1, dtype=torch.int32, device=dev) * Sk

    def pad():                                                             # what path (a) needs: [B, heads, S, 256] views
        q256 = F.pad(q, (0, 64)).view(B, Sq, H, 256).transpose(1, 2)
        k256 = F.pad(torch.cat([kn, kr.expand(-1, H, -1)], dim=-1), (0, 64)).view(B, Sk, H, 256).transpose(1, 2)
        v256 = F.pad(v, (0, 128)).view(B, Sk, H, 256).transpose(1, 2)
        return q256, k256, v256

    q256, k256, v256 = pad()
    q128, k128 = q[..., :128].contiguous(), kn.contiguous()
    paths = {
        "mla_prefill": lambda: ops.mla_prefill(q, kn, kr, v, cu_seqlens_q=cu_q, cu_seqlens_k=cu_k, max_seqlen_q=Sq, max_seqlen_k=Sk,
                                               softmax_scale=SCALE, causal=causal),
        "(a) fa3_prefill_cache D 256, padded beforehand": lambda: ops.fa3_prefill_cache(q256, k256, v256, causal=causal, softmax_scale=SCALE),
        "(a) ... with the padding copies": lambda: ops.fa3_prefill_cache(*pad(), causal=causal, softmax_scale=SCALE),
        "(b) torch sdpa on the padded operands": lambda: F.scaled_dot_product_attention(q256, k256, v256, is_causal=causal and Sq == Sk,
                                                                                         scale=SCALE),
        "(c) fa3_varlen_forward D 128, same pairs": lambda: ops.fa3_varlen_forward(q128, k128, v, cu_seqlens_q=cu_q, cu_seqlens_k=cu_k,
                                                                                   max_seqlen_q=Sq, max_seqlen_k=Sk, causal=causal),
    }
    pairs = B * (Sq * (Sq + 1) // 2 + Sq * (Sk - Sq) if causal else Sq * Sk)
    inner = max(3, min(50, int(5e13 / (640 * pairs * H))))                 # tens of milliseconds of the new call per timed window
    return pairs, _time(paths, reps, inner)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = ["# MLA prefill: `ops.mla_prefill` against the padded D 256 cache prefill, torch sdpa and the D 128 packed forward", "",
             f"bf16, one shared rotary key head, paths alternating in one process, {a.reps} repetitions (min .. max); "
             f"{torch.cuda.get_device_name(0)}.  TFLOP/s = 2 * 320 * visible pairs * H / min time for every path.", "",
             "| H | sequences x rows x keys | causal | path | us a call (min .. max) | TFLOP/s (at min) | time / mla_prefill |", "|---|---|---|---|---|---|---|"]
    shapes = [(8, 1024, 1024, True), (2, 4096, 4096, True), (1, 8192, 8192, True), (1, 512, 8192, False), (1, 512, 32768, False)]
    for H in (128, 16):
        for B, Sq, Sk, causal in shapes:
            pairs, res = bench_shape(H, B, Sq, Sk, causal, a.reps, dev)
            base = res["mla_prefill"][0] or float("nan")
            first = len(lines)
            for name, (lo, hi) in res.items():
                if lo is None:
                    lines.append(f"| {H} | {B} x {Sq} x {Sk} | {causal} | {name} | not measured: {hi} | | |")
                    continue
                lines.append(f"| {H} | {B} x {Sq} x {Sk} | {causal} | {name} | {lo:.0f} .. {hi:.0f} | {640 * pairs * H / lo / 1e6:.0f} | {lo / base:.2f} |")
            print("\n".join(lines[first:]), flush=True)
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

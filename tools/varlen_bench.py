"""Packed variable-length attention for training on the MI355X: ``ops.fa3_varlen_forward`` / ``fa3_varlen_backward`` against what a
caller has without them, forward and forward + backward, causal self-attention, bf16, H 16 / Hkv 4, D 128.

Three length distributions at about 16k tokens in all:

  uniform   16 sequences of 1024 tokens: nothing is padded, what the packed mode itself costs;
  one_long  one sequence of 8192 tokens with 64 of 128: the padded batch is 87 % padding;
  mix       a fine-tuning mix (a seeded draw from a log-normal around 400 tokens, clipped to 16 .. 4096, topped up to 16384).

Three paths:

  (a) varlen   the packed call;
  (b) padded   today's path: the batch padded to its longest sequence, ``ops.fa3_forward(seqlens_k=)`` / ``ops.fa3_backward(seqlens_k=)``
               on the library's default kernel choice (for aligned shapes that is the persistent assembly forward, which the packed path
               does not have);
  (c) loop     a Python loop of per-sequence dense calls (views of the packed tensors, no copies).

One process; the paths are timed alternately with device events after a warm-up, ``--reps`` windows of ``--iters`` calls each, the
median reported with the minimum and maximum.  (b) is in every comparison twice (``padded`` and ``padded_again``): the ratio of the two
medians is the run-to-run spread a ratio has to clear before it means anything.  Also reported: the share of padded rows in (b) and
the share of the packed grids' workgroups that find no rows / keys of their sequence and return at once.

    python tools/varlen_bench.py [--reps 7] [--iters 10] [--only uniform,one_long,mix] [--json out.jsonl]
"""

from __future__ import annotations

import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from photonic_flash_attention_amd import ops  # noqa: E402

BF = torch.bfloat16
H, HKV, D = 16, 4, 128


def lengths(name):
    if name == "uniform":
        return [1024] * 16
    if name == "one_long":
        return [8192] + [128] * 64
    g = torch.Generator().manual_seed(1234)
    draw = torch.exp(math.log(400.0) + 0.9 * torch.randn(200, generator=g)).clamp(16, 4096).long().tolist()
    out, total = [], 0
    for n in draw:
        if total + n > 16384:
            break
        out.append(n)
        total += n
    if total < 16384:
        out.append(16384 - total)
    return out


def _timed(paths, n, reps):
    """Alternate the paths, `reps` windows of `n` calls each.  -> {name: [us per call, ...]}"""
    for f in paths.values():
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    times = {name: [] for name in paths}
    for _ in range(reps):
        for name, f in paths.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                f()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / n)
    return times


def _empty_share(lens, block, heads):
    """share of a packed grid's workgroups (B * heads * ceil(max / block)) that return at once"""
    nb = math.ceil(max(lens) / block)
    live = sum(math.ceil(n / block) for n in lens)
    return 1.0 - live / (len(lens) * nb)


def bench(name, reps, iters, dev):
    lens = lengths(name)
    B, total, smax = len(lens), sum(lens), max(lens)
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    q, dout = (torch.randn(total, H, D, device=dev, dtype=BF) for _ in range(2))
    k, v = (torch.randn(total, HKV, D, device=dev, dtype=BF) for _ in range(2))
    cu_t = torch.tensor(cu, dtype=torch.int32, device=dev)
    kw = dict(cu_seqlens_q=cu_t, cu_seqlens_k=cu_t, max_seqlen_q=smax, max_seqlen_k=smax, causal=True)
    # (b): the padded batch [B, smax, heads, D], built once outside the timed region
    qp, dp = (torch.zeros(B, smax, H, D, device=dev, dtype=BF) for _ in range(2))
    kp, vp = (torch.zeros(B, smax, HKV, D, device=dev, dtype=BF) for _ in range(2))
    for b, n in enumerate(lens):
        for dst, src in ((qp, q), (dp, dout), (kp, k), (vp, v)):
            dst[b, :n] = src[cu[b]:cu[b + 1]]
    qp, kp, vp, dp = (t.permute(0, 2, 1, 3) for t in (qp, kp, vp, dp))
    sl = torch.tensor(lens, dtype=torch.int32, device=dev)
    views = [tuple(t[cu[b]:cu[b + 1]].transpose(0, 1)[None] for t in (q, k, v, dout)) for b in range(B)]

    def varlen_f():
        return ops.fa3_varlen_forward(q, k, v, return_lse=True, **kw)

    def padded_f():
        return ops.fa3_forward(qp, kp, vp, causal=True, seqlens_k=sl, return_lse=True)

    def loop_f():
        return [ops.fa3_forward(a, b_, c, causal=True, return_lse=True) for a, b_, c, _ in views]

    def varlen_fb():
        o, lse = varlen_f()
        return ops.fa3_varlen_backward(q, k, v, o, dout, lse, **kw)

    def padded_fb():
        o, lse = padded_f()
        return ops.fa3_backward(qp, kp, vp, o, dp, lse, causal=True, seqlens_k=sl)

    def loop_fb():
        return [ops.fa3_backward(a, b_, c, o, g, lse, causal=True) for (a, b_, c, g), (o, lse) in zip(views, loop_f())]

    res = dict(case=name, sequences=B, total_tokens=total, max_len=smax, padded_rows_share=round(1.0 - total / (B * smax), 4),
               empty_wg_share_fwd_dq=round(_empty_share(lens, 256, H), 4), empty_wg_share_dkdv=round(_empty_share(lens, 128, HKV), 4))
    for tag, paths in (("fwd", dict(varlen=varlen_f, padded=padded_f, loop=loop_f, padded_again=padded_f)),
                       ("fwd_bwd", dict(varlen=varlen_fb, padded=padded_fb, loop=loop_fb, padded_again=padded_fb))):
        times = _timed(paths, iters, reps)
        for p, ts in times.items():
            ts = sorted(ts)
            res[f"{tag}_{p}_us"] = round(ts[len(ts) // 2], 1)
            res[f"{tag}_{p}_us_minmax"] = [round(ts[0], 1), round(ts[-1], 1)]
        res[f"{tag}_varlen_over_padded"] = round(res[f"{tag}_varlen_us"] / res[f"{tag}_padded_us"], 4)
        res[f"{tag}_varlen_over_loop"] = round(res[f"{tag}_varlen_us"] / res[f"{tag}_loop_us"], 4)
        res[f"{tag}_padded_again_over_padded"] = round(res[f"{tag}_padded_again_us"] / res[f"{tag}_padded_us"], 4)
    # the backward alone, as the difference of the medians (same launches, same order)
    for p in ("varlen", "padded", "loop"):
        res[f"bwd_{p}_us"] = round(res[f"fwd_bwd_{p}_us"] - res[f"fwd_{p}_us"], 1)
    res["bwd_varlen_over_padded"] = round(res["bwd_varlen_us"] / res["bwd_padded_us"], 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--only", default="uniform,one_long,mix")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    out = open(a.json, "w") if a.json else None
    for name in a.only.split(","):
        res = bench(name, a.reps, a.iters, dev)
        print(json.dumps(res), flush=True)
        if out:
            out.write(json.dumps(res) + "\n")
            out.flush()
    if out:
        out.close()


if __name__ == "__main__":
    main()

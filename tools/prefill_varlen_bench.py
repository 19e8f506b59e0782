"""The ragged forward over a KV cache on the MI355X: ``ops.fa3_prefill_varlen`` (one launch for sequences with different numbers of
query rows) against what a caller has without it.

  (a) mode   a UNIFORM batch through the ragged entry against ``ops.fa3_prefill_cache`` at the same shape: what the mode itself costs
             (the cu_seqlens_q loads in the prologue, the packed addressing);
  (b) ragged a ragged batch in one launch against the loop of uniform calls a caller needs today, one per distinct length (sequences
             of equal length share a call);
  (c) mixed  a serving step -- many one-row decode sequences plus one long chunk -- against ``ops.fa3_decode`` for the rows plus
             ``ops.fa3_prefill_cache`` for the chunk.  The ragged kernel spends a 256-row workgroup per query head on a one-row
             sequence and re-reads its K/V head once per head of the group, so this is where it is expected to lose.

One process.  Every path cycles through enough distinct caches (>= 768 MiB of K + V in all) that the 256 MiB Infinity Cache cannot
serve them; the paths of a comparison are timed alternately with device events, ``--reps`` windows each, the median reported with the
minimum and maximum in the JSON.  The baseline is in every comparison twice (``base`` and ``base_again``): the ratio of the two
medians is the run-to-run spread a ratio has to clear before it means anything.

    python tools/prefill_varlen_bench.py [--reps 7] [--only mode,ragged,mixed] [--json out.jsonl]
"""

from __future__ import annotations

import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from photonic_flash_attention_amd import _capi, ops  # noqa: E402

MIN_POOL = 768 << 20
BF = torch.bfloat16


def _timed(paths, n, reps):
    """Alternate the paths, `reps` windows of `n` calls each.  -> {name: [us per call, ...]}"""
    for f in paths.values():          # warm-up: code objects, allocator
        for i in range(min(2, n)):
            f(i)
    torch.cuda.synchronize()
    times = {name: [] for name in paths}
    for _ in range(reps):
        for name, f in paths.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(n):
                f(i)
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / n)
    return times


def _med(ts):
    return sorted(ts)[len(ts) // 2]


def _stats(res, times):
    for name, ts in times.items():
        res[f"{name}_us"] = round(_med(ts), 2)
        res[f"{name}_us_min"], res[f"{name}_us_max"] = round(min(ts), 2), round(max(ts), 2)
    res["varlen_over_base"] = round(res["varlen_us"] / res["base_us"], 4)
    res["base_again_over_base"] = round(res["base_again_us"] / res["base_us"], 4)


def _caches(B, Hkv, S, D, dev):
    one = 2 * B * Hkv * S * D * 2
    n = max(2, math.ceil(MIN_POOL / one))
    return [(torch.randn(B, Hkv, S, D, device=dev, dtype=BF), torch.randn(B, Hkv, S, D, device=dev, dtype=BF)) for _ in range(n)], one


def _describe(q, k, cu_len, max_q, Hkv):
    total, H, D = q.shape
    a = _capi.make_prefill_varlen_args(B=cu_len - 1, H=H, Hkv=Hkv, total_q=total, max_seqlen_q=max_q, Smax=k.shape[2], D=D, q=1 << 12,
                                       k_cache=1 << 12, v_cache=1 << 12, o=1 << 12, cu_seqlens_q=1 << 12, q_stride_s=H * D, q_stride_h=D,
                                       o_stride_s=H * D, o_stride_h=D, k_stride_b=k.stride(0), k_stride_h=k.stride(1), k_stride_s=k.stride(2),
                                       v_stride_b=k.stride(0), v_stride_h=k.stride(1), v_stride_s=k.stride(2), dtype_in=0, dtype_out=0,
                                       causal=1, softmax_scale=D ** -0.5)
    return _capi.describe_prefill_varlen(a)


def _flops(q_lens, prefix, H, D):
    return 4.0 * D * H * sum(n * prefix + n * (n + 1) // 2 for n in q_lens)


def bench(kind, H, Hkv, D, q_lens, prefix, reps, dev):
    """q_lens: rows per sequence, equal lengths adjacent; every sequence holds `prefix` keys before its own rows."""
    B, total, max_q = len(q_lens), sum(q_lens), max(q_lens)
    S = prefix + max_q
    caches, one = _caches(B, Hkv, S, D, dev)
    n = len(caches)
    cu = [0]
    for x in q_lens:
        cu.append(cu[-1] + x)
    cu_t = torch.tensor(cu, dtype=torch.int32, device=dev)
    sl = torch.tensor([prefix + x for x in q_lens], dtype=torch.int32, device=dev)
    q = torch.randn(total, H, D, device=dev, dtype=BF)
    name, wgs = _describe(q, caches[0][0], len(cu), max_q, Hkv)
    res = dict(kind=kind, B=B, H=H, Hkv=Hkv, D=D, q_lens=_short(q_lens), prefix=prefix, total_q=total, max_seqlen_q=max_q,
               cache_MB=round(one / 1e6, 1), n_caches=n, reps=reps, kernel=name, workgroups=wgs, gflop=round(_flops(q_lens, prefix, H, D) / 1e9, 2))

    def varlen(i):
        ops.fa3_prefill_varlen(q, caches[i][0], caches[i][1], cu_seqlens_q=cu_t, max_seqlen_q=max_q, cache_seqlens=sl)

    # the baseline: one uniform call per run of equal lengths, on views of the same tensors
    runs, b0 = [], 0
    while b0 < B:
        b1 = b0
        while b1 < B and q_lens[b1] == q_lens[b0]:
            b1 += 1
        rows = q_lens[b0]
        qv = q[cu[b0]:cu[b1]].unflatten(0, (b1 - b0, rows)).permute(0, 2, 1, 3)          # [b, H, rows, D]
        runs.append((b0, b1, rows, qv, sl[b0:b1]))
        b0 = b1
    res["baseline_calls"] = len(runs)

    def base(i):
        k, v = caches[i]
        for b0, b1, rows, qv, s in runs:
            if kind == "mixed" and rows == 1:
                ops.fa3_decode(qv, k[b0:b1], v[b0:b1], cache_seqlens=s)
            else:
                ops.fa3_prefill_cache(qv, k[b0:b1], v[b0:b1], cache_seqlens=s)

    _stats(res, _timed({"base": base, "varlen": varlen, "base_again": base}, n, reps))
    res["varlen_tflops"] = round(_flops(q_lens, prefix, H, D) / res["varlen_us"] / 1e6, 1)
    del caches
    torch.cuda.empty_cache()
    return res


def _short(q_lens):
    out, i = [], 0
    while i < len(q_lens):
        j = i
        while j < len(q_lens) and q_lens[j] == q_lens[i]:
            j += 1
        out.append(f"{q_lens[i]}x{j - i}" if j - i > 1 else str(q_lens[i]))
        i = j
    return ",".join(out)


SHAPES = {
    # (a) the mode's own cost: uniform batches, the shapes of profiles/prefill_cache.md
    "mode": [(32, 8, 128, [512] * 8, 0), (32, 8, 128, [512] * 8, 8192), (32, 8, 128, [2048] * 8, 8192), (32, 8, 128, [512], 8192),
             (32, 8, 64, [512] * 8, 8192), (32, 8, 128, [1] * 64, 8192)],
    # (b) ragged batches against one uniform call per distinct length
    "ragged": [(32, 8, 128, [2048, 512, 300, 33, 5, 1, 1, 1], 4096), (32, 8, 128, [1024, 768, 512, 384, 256, 128, 64, 32], 4096),
               (32, 8, 128, [300, 257, 33, 1], 8192), (32, 8, 64, [2048, 512, 300, 33, 5, 1, 1, 1], 4096)],
    # (c) a serving step: one chunk plus decode rows, against fa3_prefill_cache + fa3_decode
    "mixed": [(32, 8, 128, [512] + [1] * 63, 4096), (32, 8, 128, [2048] + [1] * 31, 4096), (32, 8, 128, [512] + [1] * 15, 8192),
              (32, 32, 128, [512] + [1] * 63, 4096)],
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", default="mode,ragged,mixed")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "prefill_varlen_bench measures on the GPU"
    dev = torch.device("cuda:0")
    rows = []
    print(f"{'kind':>6} {'H':>3} {'Hkv':>3} {'D':>4} {'prefix':>6} {'WGs':>5} {'calls':>5} | {'base us':>9} {'varlen us':>9} {'varlen/base':>11} "
          f"{'base again/base':>15} {'TF/s':>6} | q_lens", flush=True)
    for kind in args.only.split(","):
        for H, Hkv, D, q_lens, prefix in SHAPES[kind]:
            r = bench(kind, H, Hkv, D, q_lens, prefix, args.reps, dev)
            rows.append(r)
            print(f"{kind:>6} {H:>3} {Hkv:>3} {D:>4} {prefix:>6} {r['workgroups']:>5} {r['baseline_calls']:>5} | {r['base_us']:>9.1f} "
                  f"{r['varlen_us']:>9.1f} {r['varlen_over_base']:>11.3f} {r['base_again_over_base']:>15.3f} {r['varlen_tflops']:>6.1f} | "
                  f"{r['q_lens']}", flush=True)
            if args.json:                 # after every shape: a run that is cut short keeps what it measured
                with open(args.json, "w") as f:
                    for x in rows:
                        f.write(json.dumps(x) + "\n")


if __name__ == "__main__":
    main()

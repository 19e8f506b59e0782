"""Chunked prefill over a KV cache on the MI355X: ``ops.fa3_prefill_cache`` (a chunk of Sq new rows against prefix + Sq cached
keys, bottom-right causal) against

  * today's path: gather the pages with torch ops, then ``ops.fa3_forward`` with the bottom-right ``[B,1,Sq,Sk]`` mask (gather and
    attention timed separately; the mask is built once outside the timed window, which flatters this path);
  * itself, paged against contiguous: pools in the ``[P,Hkv,page,D]`` ("hpsd") and ``[P,page,Hkv,D]`` ("phsd") layouts, pages of 64
    and 256 keys, random page order;
  * at prefix 0, where the problem is the plain causal forward: ``fa3_forward(causal=True, _variant=44)`` (the same schedule without
    the cache logic) and variant 0 (the library's choice, the assembly kernel: the head-room still open).

One process.  Every path cycles through enough distinct caches (>= 768 MiB of K + V in all) that the 256 MiB Infinity Cache cannot
serve them; the paths of a comparison are timed alternately with device events, ``--reps`` windows each, the median reported with
the minimum and maximum in the JSON.  TFLOP/s = 4 D x visible (row, key) pairs x B x H / time.

    python tools/prefill_cache_bench.py [--reps 5] [--quick] [--no-paged] [--no-today] [--json out.jsonl]
    python tools/prefill_cache_bench.py --shapes "B,H,Hkv,D,chunk,prefix;..."

``--window W`` adds the sliding window: ``fa3_prefill_cache(..., window=W)`` timed alternately with the call without a window on the
same caches (``prefill_win_us``, ``window_over_none``), TFLOP/s over the pairs the window leaves visible.

    python tools/prefill_cache_bench.py --window 4096 --shapes "8,32,8,128,2048,30720" --no-paged --no-today
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
MAX_CACHE = 24 << 30
N_CU = 256
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


def _stats(res, times):
    for name, ts in times.items():
        res[f"{name}_us"] = round(sorted(ts)[len(ts) // 2], 2)
        res[f"{name}_us_min"], res[f"{name}_us_max"] = round(min(ts), 2), round(max(ts), 2)


def _pools(B, Hkv, S, D, page, layout, n, dev, seed):
    """n pools of B * S / page pages (random contents: only the time is taken) with a random page order each."""
    pages = S // page
    out = []
    for i in range(n):
        perm = torch.randperm(B * pages, generator=torch.Generator().manual_seed(seed + i)).to(dev)
        if layout == "phsd":        # flash-attn style, a token's heads adjacent; passed transposed
            kp = torch.randn(B * pages, page, Hkv, D, device=dev, dtype=BF).transpose(1, 2)
            vp = torch.randn(B * pages, page, Hkv, D, device=dev, dtype=BF).transpose(1, 2)
        else:                       # a head's tokens adjacent, like the contiguous [B, Hkv, S, D] cache
            kp = torch.randn(B * pages, Hkv, page, D, device=dev, dtype=BF)
            vp = torch.randn(B * pages, Hkv, page, D, device=dev, dtype=BF)
        out.append((kp, vp, perm.to(torch.int32).reshape(B, pages).contiguous()))
    return out


def bench_shape(B, H, Hkv, D, Sq, prefix, reps, dev, paged=True, today=True, window=None):
    S = prefix + Sq                                     # keys in the cache when the chunk attends (its own included)
    cache_bytes = 2 * B * Hkv * S * D * 2
    if cache_bytes > MAX_CACHE:
        return None
    n = max(1, math.ceil(MIN_POOL / cache_bytes))
    pairs = Sq * prefix + Sq * (Sq + 1) // 2            # visible (row, key) pairs per (batch, head)
    flops = 4.0 * D * pairs * B * H
    q = torch.randn(B, Sq, H, D, device=dev, dtype=BF).permute(0, 2, 1, 3)
    sl = torch.full((B,), S, dtype=torch.int32, device=dev)
    caches = [(torch.randn(B, Hkv, S, D, device=dev, dtype=BF), torch.randn(B, Hkv, S, D, device=dev, dtype=BF)) for _ in range(n)]
    a = _capi.make_decode_args(B=B, H=H, Hkv=Hkv, Sq=Sq, Smax=S, D=D, q=1 << 12, k_cache=1 << 12, v_cache=1 << 12, o=1 << 12,
                               q_stride_b=Sq * H * D, q_stride_h=D, q_stride_s=H * D, k_stride_b=Hkv * S * D, k_stride_h=S * D, k_stride_s=D,
                               v_stride_b=Hkv * S * D, v_stride_h=S * D, v_stride_s=D, o_stride_b=Sq * H * D, o_stride_h=D, o_stride_s=H * D,
                               dtype_in=0, dtype_out=0, causal=1, softmax_scale=D ** -0.5)
    name, wgs = _capi.describe_prefill(a)
    res = dict(B=B, H=H, Hkv=Hkv, D=D, chunk=Sq, prefix=prefix, Skv=S, cache_MB=round(cache_bytes / 1e6, 1), n_caches=n, reps=reps,
               kernel=name, workgroups=wgs, workgroups_per_cu=round(wgs / N_CU, 2), gflop=round(flops / 1e9, 2))

    def prefill(i):
        ops.fa3_prefill_cache(q, caches[i][0], caches[i][1], cache_seqlens=sl)

    paths = {"prefill": prefill}
    if window:
        paths["prefill_win"] = lambda i: ops.fa3_prefill_cache(q, caches[i][0], caches[i][1], cache_seqlens=sl, window=window)
    if today:        # the element-mask path on the (already gathered) cache
        mask = (torch.arange(S, device=dev)[None, :] <= torch.arange(Sq, device=dev)[:, None] + prefix)[None, None].expand(B, 1, Sq, S)
        paths["mask_attention"] = lambda i: ops.fa3_forward(q, caches[i][0], caches[i][1], mask=mask)
    if prefix == 0:
        paths["fwd_v44"] = lambda i: ops.fa3_forward(q, caches[i][0], caches[i][1], causal=True, _variant=44)
        paths["fwd_v0"] = lambda i: ops.fa3_forward(q, caches[i][0], caches[i][1], causal=True, _variant=0)
    _stats(res, _timed(paths, n, reps))
    res["prefill_tflops"] = round(flops / res["prefill_us"] / 1e6, 1)
    if window:
        wpairs = sum(min(window, prefix + i + 1) for i in range(Sq))
        res["window"] = window
        res["prefill_win_tflops"] = round(4.0 * D * wpairs * B * H / res["prefill_win_us"] / 1e6, 1)
        res["window_over_none"] = round(res["prefill_win_us"] / res["prefill_us"], 4)
        res["visible_pairs_ratio"] = round(wpairs / pairs, 4)
    if prefix == 0:
        res["prefill_over_v44"] = round(res["prefill_us"] / res["fwd_v44_us"], 4)
        res["prefill_over_v0"] = round(res["prefill_us"] / res["fwd_v0_us"], 4)
    mask = None
    if paged:
        for layout in ("hpsd", "phsd"):
            for page in (64, 256):
                if S % page:
                    continue
                pools = _pools(B, Hkv, S, D, page, layout, n, dev, seed=page)
                tag = f"{layout}{page}"
                t = _timed({"contiguous": prefill,
                            "paged": lambda i: ops.fa3_prefill_cache(q, pools[i][0], pools[i][1], cache_seqlens=sl, block_table=pools[i][2])},
                           n, reps)
                c, p = sorted(t["contiguous"])[reps // 2], sorted(t["paged"])[reps // 2]
                res[f"paged_{tag}_us"], res[f"paged_{tag}_ratio"] = round(p, 2), round(p / c, 4)
                res[f"paged_{tag}_contiguous_spread"] = round(max(t["contiguous"]) / min(t["contiguous"]), 4)
                if today and layout == "phsd" and page == 256:       # what the paged call replaces, part one: the gather
                    pages = S // page

                    def gather(i):
                        kp, vp, bt = pools[i]
                        idx = bt.flatten().long()
                        kp.index_select(0, idx).reshape(B, pages, Hkv, page, D).permute(0, 2, 1, 3, 4).reshape(B, Hkv, S, D)
                        vp.index_select(0, idx).reshape(B, pages, Hkv, page, D).permute(0, 2, 1, 3, 4).reshape(B, Hkv, S, D)

                    tg = _timed({"gather": gather}, n, reps)
                    _stats(res, tg)
                del pools
                torch.cuda.empty_cache()
    if today and "gather_us" in res:
        res["today_us"] = round(res["gather_us"] + res["mask_attention_us"], 2)
        res["today_over_prefill"] = round(res["today_us"] / res.get("paged_phsd256_us", res["prefill_us"]), 2)
    del caches
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="H 32 / Hkv 8, D 128, B 8, chunk 512 only")
    ap.add_argument("--no-paged", action="store_true")
    ap.add_argument("--no-today", action="store_true", help="skip the gather + element-mask baseline")
    ap.add_argument("--shapes", default=None, help='"B,H,Hkv,D,chunk,prefix;..." instead of the profiles/prefill_cache.md shapes')
    ap.add_argument("--window", type=int, default=None, help="also time fa3_prefill_cache(window=W) against the call without a window")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "prefill_cache_bench measures on the GPU"
    dev = torch.device("cuda:0")
    if args.shapes:
        shapes = [tuple(int(x) for x in s.split(",")) for s in args.shapes.split(";") if s]
    elif args.quick:
        shapes = [(8, 32, 8, 128, 512, p) for p in (0, 8192, 32768)]
    else:
        shapes = [(B, H, Hkv, 128, c, p) for (H, Hkv) in ((32, 8), (32, 32)) for B in (1, 8) for c in (512, 2048) for p in (0, 8192, 32768)]
        shapes += [(8, 32, 8, 64, 512, p) for p in (0, 8192, 32768)]
    rows = []
    print(f"{'B':>2} {'H':>3} {'Hkv':>3} {'D':>4} {'chunk':>5} {'prefix':>6} {'WGs':>5} | {'prefill us':>10} {'TF/s':>6} | {'gather us':>9} {'mask-attn us':>12} "
          f"{'today/new':>9} | {'hpsd64':>6} {'hpsd256':>7} {'phsd64':>6} {'phsd256':>7} | {'/v44':>6} {'/v0':>6}", flush=True)
    for B, H, Hkv, D, c, p in shapes:
        r = bench_shape(B, H, Hkv, D, c, p, args.reps, dev, paged=not args.no_paged, today=not args.no_today, window=args.window)
        if r is None:
            print(f"{B:>2} {H:>3} {Hkv:>3} {D:>4} {c:>5} {p:>6}  skipped: one cache exceeds {MAX_CACHE >> 30} GiB", flush=True)
            continue
        rows.append(r)
        g = lambda key, fmt: format(r[key], fmt) if key in r else "-"      # noqa: E731
        print(f"{B:>2} {H:>3} {Hkv:>3} {D:>4} {c:>5} {p:>6} {r['workgroups']:>5} | {r['prefill_us']:>10.1f} {r['prefill_tflops']:>6.1f} | "
              f"{g('gather_us', '.1f'):>9} {g('mask_attention_us', '.1f'):>12} {g('today_over_prefill', '.2f'):>9} | "
              f"{g('paged_hpsd64_ratio', '.3f'):>6} {g('paged_hpsd256_ratio', '.3f'):>7} {g('paged_phsd64_ratio', '.3f'):>6} "
              f"{g('paged_phsd256_ratio', '.3f'):>7} | {g('prefill_over_v44', '.3f'):>6} {g('prefill_over_v0', '.3f'):>6}"
              + (f" | W {args.window}: {r['prefill_win_us']:.1f} us [{r['prefill_win_us_min']:.1f}, {r['prefill_win_us_max']:.1f}] "
                 f"{r['prefill_win_tflops']:.1f} TF/s, x{r['window_over_none']:.3f} of no window [{r['prefill_us_min']:.1f}, {r['prefill_us_max']:.1f}]"
                 if args.window else ""), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()

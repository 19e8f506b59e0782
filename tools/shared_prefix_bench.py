"""A decode step over a batch whose sequences share a long prefix, on the MI355X: ``ops.fa3_decode(..., shared_prefix=P)`` (the prefix
streamed once for all rows, each sequence's own keys, ``attn_merge``) against the plain call, and ``ops.attn_merge`` alone.

Two cache layouts, because they answer different questions:

* ``paged``: the realistic one.  Every sequence's block table names the SAME physical prefix pages and its own private pages, so the
  plain call re-reads the same bytes B times -- from HBM once and from L2 / the Infinity Cache afterwards, as far as they hold them.
* ``contiguous``: every sequence has its own copy of the prefix, so the plain call streams B distinct copies from HBM (the traffic
  argument at its strongest; shared_prefix reads sequence 0's copy).  Skipped where one cache would exceed 12 GiB.

Timing follows tools/decode_bench.py: each path cycles through enough distinct caches (>= 768 MiB in all, like a model's layers)
that the 256 MiB Infinity Cache cannot carry a cache from one call to its next use; the paths are timed alternately with device
events, median of ``--reps`` rounds with min and max.  ``--graphs`` also captures one ``torch.cuda.graph`` per cache and path and times
the replays: the figure without Python and allocator cost on the host, which is how a serving step would run it.  The plain call is
the path without the keyword: the code that ran before ``shared_prefix`` existed.

    python tools/shared_prefix_bench.py [--reps 5] [--graphs] [--layouts paged,contiguous] [--json out.jsonl]
    python tools/shared_prefix_bench.py --dry          # the plan (bytes, caches per shape) without a GPU

The merge alone: N = 2 fp32 parts into a bf16 result (what shared_prefix launches) at B * Sq = ``rows`` rows of 32 heads, D 128, cycling
through >= 768 MiB of distinct buffers; GB/s over the bytes it must move (parts, LSEs, result)."""

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
MAX_CACHE = 12 << 30
MAX_CACHES = 96
PAGE = 256
H, HKV, D, PRIVATE = 32, 8, 128, 256
# (B, Sq, P): the decode grid, and one speculative step of 16 rows
SHAPES = [(B, 1, P) for P in (2048, 8192, 32768) for B in (8, 32, 128)] + [(32, 16, 8192)]


def plan(B, Sq, P, layout):
    """-> (bytes of one cache that a plain call must read, bytes a shared_prefix call must read, distinct bytes held, caches cycled)."""
    row = 2 * HKV * D * 2                                         # K and V bytes of one key
    own = PRIVATE + Sq
    plain, shared = B * (P + own) * row, (P + B * own) * row
    own_pages = -(-own // PAGE)
    held = (P + B * own_pages * PAGE) * row if layout == "paged" else B * (P + own_pages * PAGE) * row
    return plain, shared, held, min(MAX_CACHES, max(1, math.ceil(MIN_POOL / held)))


def make_caches(B, Sq, P, layout, n, dev):
    own_pages = -(-(PRIVATE + Sq) // PAGE)
    lens = torch.full((B,), P + PRIVATE + Sq, dtype=torch.int32, device=dev)
    out = []
    for i in range(n):
        if layout == "paged":
            n_pre = P // PAGE
            n_pages = n_pre + B * own_pages
            kp = torch.randn(n_pages, PAGE, HKV, D, device=dev, dtype=torch.bfloat16).transpose(1, 2)
            vp = torch.randn(n_pages, PAGE, HKV, D, device=dev, dtype=torch.bfloat16).transpose(1, 2)
            perm = torch.randperm(n_pages, generator=torch.Generator().manual_seed(i))
            table = torch.cat([perm[:n_pre].expand(B, n_pre), perm[n_pre:].reshape(B, own_pages)], dim=1).to(torch.int32).contiguous().to(dev)
            out.append((kp, vp, dict(cache_seqlens=lens, block_table=table)))
        else:
            S = P + own_pages * PAGE
            k = torch.randn(B, S, HKV, D, device=dev, dtype=torch.bfloat16).transpose(1, 2)
            v = torch.randn(B, S, HKV, D, device=dev, dtype=torch.bfloat16).transpose(1, 2)
            out.append((k, v, dict(cache_seqlens=lens)))
    return out


def timed(fns, counts, reps):
    """Median / min / max microseconds per call of each path, the paths alternating."""
    times = {name: [] for name in fns}
    for _ in range(reps):
        for name, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(counts[name]):
                f(i)
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / counts[name])
    return {name: (sorted(ts)[len(ts) // 2], min(ts), max(ts)) for name, ts in times.items()}


def bench_shape(B, Sq, P, layout, reps, graphs, dev):
    plain_b, shared_b, held, n = plan(B, Sq, P, layout)
    if held > MAX_CACHE:
        return None
    caches = make_caches(B, Sq, P, layout, n, dev)
    q = torch.randn(B, Sq, H, D, device=dev, dtype=torch.bfloat16).transpose(1, 2)
    o = torch.empty(B, Sq, H, D, device=dev, dtype=torch.bfloat16).transpose(1, 2)

    def plain(i):
        k, v, kw = caches[i]
        ops.fa3_decode(q, k, v, out=o, **kw)

    def shared(i):
        k, v, kw = caches[i]
        ops.fa3_decode(q, k, v, out=o, shared_prefix=P, **kw)

    fns = {"plain": plain, "shared": shared}
    counts = {name: n for name in fns}
    for f in fns.values():                     # warm-up: code objects, allocator
        for i in range(min(2, n)):
            f(i)
    torch.cuda.synchronize()
    if graphs:
        side = torch.cuda.Stream()
        for name, f in (("plain", plain), ("shared", shared)):
            gs = []
            for i in range(n):
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    f(i)
                torch.cuda.current_stream().wait_stream(side)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    f(i)
                gs.append(g)
            fns[name + "_graph"] = lambda i, gs=gs: gs[i].replay()
            counts[name + "_graph"] = n
        for name in ("plain_graph", "shared_graph"):
            fns[name](0)
        torch.cuda.synchronize()
    res = dict(layout=layout, B=B, Sq=Sq, P=P, private=PRIVATE, H=H, Hkv=HKV, D=D, page=PAGE if layout == "paged" else 0, n_caches=n,
               held_MB=round(held / 1e6, 1), cycled_MB=round(n * held / 1e6, 1), plain_read_MB=round(plain_b / 1e6, 2),
               shared_read_MB=round(shared_b / 1e6, 2), reps=reps)
    for name, (med, lo, hi) in timed(fns, counts, reps).items():
        res[f"{name}_us"], res[f"{name}_us_min"], res[f"{name}_us_max"] = round(med, 2), round(lo, 2), round(hi, 2)
    res["plain_TBs"] = round(plain_b / res["plain_us"] / 1e6, 3)          # of the bytes the call asks for, wherever they come from
    res["shared_TBs"] = round(shared_b / res["shared_us"] / 1e6, 3)
    res["plain_over_shared"] = round(res["plain_us"] / res["shared_us"], 3)
    if graphs:
        res["plain_over_shared_graph"] = round(res["plain_graph_us"] / res["shared_graph_us"], 3)
    del caches, fns
    torch.cuda.empty_cache()
    return res


def bench_merge(rows, reps, dev):
    one = rows * H * (2 * (D * 4 + 4) + D * 2)                    # two fp32 parts with their LSEs in, one bf16 result out
    n = min(MAX_CACHES, max(2, math.ceil(MIN_POOL / one)))
    sets = []
    for _ in range(n):
        outs = [torch.randn(1, rows, H, D, device=dev).transpose(1, 2) for _ in range(2)]
        lses = [torch.randn(1, H, rows, device=dev) for _ in range(2)]
        sets.append((outs, lses, torch.empty(1, rows, H, D, device=dev, dtype=torch.bfloat16).transpose(1, 2)))

    def merge(i):
        outs, lses, out = sets[i]
        ops.attn_merge(outs, lses, out=out)

    merge(0), merge(1)
    torch.cuda.synchronize()
    med, lo, hi = timed({"merge": merge}, {"merge": n}, reps)["merge"]
    res = dict(rows=rows, H=H, D=D, n_parts=2, part="fp32", out="bf16", MB=round(one / 1e6, 2), n_sets=n, merge_us=round(med, 2),
               merge_us_min=round(lo, 2), merge_us_max=round(hi, 2), merge_GBs=round(one / med / 1e3, 1))
    del sets
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--graphs", action="store_true", help="also time one captured graph per cache and path")
    ap.add_argument("--layouts", default="paged,contiguous")
    ap.add_argument("--merge-rows", default="128,2048,16384")
    ap.add_argument("--json", default=None)
    ap.add_argument("--dry", action="store_true", help="print the plan and stop: no GPU needed")
    args = ap.parse_args()
    layouts = [x for x in args.layouts.split(",") if x]
    if args.dry:
        for layout in layouts:
            for B, Sq, P in SHAPES:
                plain_b, shared_b, held, n = plan(B, Sq, P, layout)
                print(f"{layout:>10} B {B:>3} Sq {Sq:>2} P {P:>5}: plain reads {plain_b / 1e6:9.1f} MB, shared {shared_b / 1e6:8.1f} MB "
                      f"({plain_b / shared_b:5.1f} x), one cache {held / 1e6:9.1f} MB"
                      + (f", {n} caches cycled" if held <= MAX_CACHE else f": skipped (above {MAX_CACHE >> 30} GiB)"))
        return
    assert torch.cuda.is_available(), "shared_prefix_bench measures on the GPU"
    dev = torch.device("cuda:0")
    rows_out = []
    for layout in layouts:
        for B, Sq, P in SHAPES:
            r = bench_shape(B, Sq, P, layout, args.reps, args.graphs, dev)
            if r is None:
                print(f"{layout:>10} B {B:>3} Sq {Sq:>2} P {P:>5}: skipped (one cache above {MAX_CACHE >> 30} GiB)", flush=True)
                continue
            rows_out.append(r)
            line = (f"{layout:>10} B {B:>3} Sq {Sq:>2} P {P:>5} ({r['n_caches']:>2} caches, {r['cycled_MB']:>7.0f} MB): plain {r['plain_us']:>8.2f} us "
                    f"[{r['plain_us_min']:.2f}, {r['plain_us_max']:.2f}] | shared {r['shared_us']:>8.2f} us [{r['shared_us_min']:.2f}, "
                    f"{r['shared_us_max']:.2f}] | plain / shared {r['plain_over_shared']:.3f}")
            if args.graphs:
                line += (f" || graphs: plain {r['plain_graph_us']:.2f} us, shared {r['shared_graph_us']:.2f} us, "
                         f"plain / shared {r['plain_over_shared_graph']:.3f}")
            print(line, flush=True)
    for rows in (int(x) for x in args.merge_rows.split(",") if x):
        r = bench_merge(rows, args.reps, dev)
        rows_out.append(dict(merge=r))
        print(f"attn_merge rows {rows:>6} ({r['MB']:.1f} MB a call, {r['n_sets']} sets): {r['merge_us']:.2f} us "
              f"[{r['merge_us_min']:.2f}, {r['merge_us_max']:.2f}] {r['merge_GBs']:.0f} GB/s", flush=True)
    if args.json:
        with open(args.json, "w") as f:
            for r in rows_out:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()

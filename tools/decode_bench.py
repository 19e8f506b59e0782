"""Decode step (one query row per batch against a KV cache) on the MI355X: ``ops.fa3_decode`` against today's path
(``ops.fa3_forward`` with Sq = 1 and a key mask) and ``torch.nn.functional.scaled_dot_product_attention``.

Timing cycles through enough distinct caches (>= 768 MiB in all, like a model's layers) that the 256 MiB Infinity Cache cannot
serve them; the three paths are timed alternately with device events.  ``--warm`` adds the single-cache (cache-resident) figure,
labelled as such.  Rate = K + V cache bytes / time, and its share of the ~6.3 TB/s achievable HBM read rate.  Also prints the
host (Python + ctypes) cost of one call and the time of one graph replay.

    python tools/decode_bench.py [--reps 5] [--quick] [--warm] [--json out.jsonl]

``--paged PAGE_SIZE`` measures the paged cache instead: the same caches scattered over page pools in a seeded random page order
(``ops.fa3_decode(..., block_table=...)``), timed alternately with the contiguous call under the same cache-cycling rule, plus
(``--gather``) what the paged call replaces: gathering the pages into a contiguous cache with torch ops and decoding that.
``--shapes B,H,Hkv,D,Skv[;...]`` picks the shapes.

    python tools/decode_bench.py --paged 256 [--gather] [--shapes "8,32,8,128,32768;1,32,8,128,32768"] [--reps 7]

``--window W[,W...]`` measures the sliding window: per shape the call without a window, the call with each window over the same full
cache (``ops.fa3_decode(..., window=W)``), and, as the bound a windowed call should approach, the call without a window over a cache
that holds only ``Skv = W`` keys -- all timed alternately, every path cycling through its own >= 768 MiB of keys and values: the
windowed calls take their lengths from a list that slides the window to a different, disjoint span of the caches on every call.
TB/s of a windowed call is taken over the bytes of its span (the W keys and the up to 63 below them in the first tile).

    python tools/decode_bench.py --window 1024,4096 [--shapes "8,32,8,128,32768;8,32,8,128,131072"] [--reps 7]
"""

from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from photonic_flash_attention_amd import _capi, ops  # noqa: E402

HBM_TBS = 6.3
MIN_POOL = 768 << 20
MAX_CACHE = 12 << 30


def _caches(B, Hkv, S, D, n, dev):
    return [(torch.randn(B, Hkv, S, D, device=dev, dtype=torch.bfloat16), torch.randn(B, Hkv, S, D, device=dev, dtype=torch.bfloat16))
            for _ in range(n)]


def bench_shape(B, H, Hkv, D, S, reps, warm, dev):
    cache_bytes = 2 * B * Hkv * S * D * 2
    if cache_bytes > MAX_CACHE:
        return None
    n = max(1, math.ceil(MIN_POOL / cache_bytes))
    pool = _caches(B, Hkv, S, D, n, dev)
    q = torch.randn(B, H, 1, D, device=dev, dtype=torch.bfloat16)
    km = torch.ones(B, S, dtype=torch.bool, device=dev)
    g = H // Hkv

    def new(k, v):
        ops.fa3_decode(q, k, v, key_mask=km)

    def old(k, v):
        ops.fa3_forward(q, k, v, key_mask=km)

    def sdpa(k, v):
        torch.nn.functional.scaled_dot_product_attention(q, k, v, attn_mask=km[:, None, None, :], enable_gqa=g > 1)

    paths = {"fa3_decode": new, "fa3_forward": old, "sdpa": sdpa}
    for f in paths.values():          # warm-up: code objects, algorithm choices, allocator
        for k, v in pool[:2]:
            f(k, v)
    torch.cuda.synchronize()
    times = {name: [] for name in paths}
    for _ in range(reps):
        for name, f in paths.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for k, v in pool:
                f(k, v)
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / n)
    res = dict(B=B, H=H, Hkv=Hkv, D=D, Skv=S, cache_MB=round(cache_bytes / 1e6, 2), n_caches=n)
    a = _capi.make_decode_args(B=B, H=H, Hkv=Hkv, Sq=1, Smax=S, D=D, q=1 << 12, k_cache=1 << 12, v_cache=1 << 12, o=1 << 12,
                               q_stride_b=H * D, q_stride_h=D, q_stride_s=H * D, k_stride_b=Hkv * S * D, k_stride_h=S * D, k_stride_s=D,
                               v_stride_b=Hkv * S * D, v_stride_h=S * D, v_stride_s=D, o_stride_b=H * D, o_stride_h=D, o_stride_s=H * D,
                               dtype_in=0, dtype_out=0, softmax_scale=D ** -0.5, workspace=1 << 12, workspace_bytes=1 << 40)
    _, wgs, nsplit = _capi.describe_decode(a)
    res.update(workgroups=wgs, nsplit=nsplit)
    for name, ts in times.items():
        us = sorted(ts)[len(ts) // 2]
        res[f"{name}_us"] = round(us, 2)
        res[f"{name}_TBs"] = round(cache_bytes / us / 1e6, 3)
        res[f"{name}_pct_hbm"] = round(100 * cache_bytes / us / 1e6 / HBM_TBS, 1)
    if warm:                           # one cache, replayed back to back: cache-resident when it fits the Infinity Cache
        k, v = pool[0]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        new(k, v)
        e0.record()
        for _ in range(20):
            new(k, v)
        e1.record()
        e1.synchronize()
        res["fa3_decode_warm_single_cache_us"] = round(e0.elapsed_time(e1) * 1e3 / 20, 2)
    del pool
    torch.cuda.empty_cache()
    return res


def bench_paged(B, H, Hkv, D, S, page, reps, gather, dev, layout="phsd", seed=0):
    """Contiguous and paged fa3_decode of one shape, timed alternately.  Pool i holds cache i's pages in a random order of its own."""
    cache_bytes = 2 * B * Hkv * S * D * 2
    if cache_bytes > MAX_CACHE or S % page:
        return None
    n = max(1, math.ceil(MIN_POOL / cache_bytes))
    pages = S // page
    q = torch.randn(B, H, 1, D, device=dev, dtype=torch.bfloat16)
    sl = torch.full((B,), S, dtype=torch.int32, device=dev)
    contiguous = _caches(B, Hkv, S, D, n, dev)
    paged = []
    for i in range(n):                  # one pool per cache: flash-attn style [num_pages, page, Hkv, D] passed transposed ("phsd"),
        perm = torch.randperm(B * pages, generator=torch.Generator().manual_seed(seed + i)).to(dev)     # or [num_pages, Hkv, page, D] ("hpsd")
        if layout == "phsd":
            kp = torch.randn(B * pages, page, Hkv, D, device=dev, dtype=torch.bfloat16).transpose(1, 2)
            vp = torch.randn(B * pages, page, Hkv, D, device=dev, dtype=torch.bfloat16).transpose(1, 2)
        else:
            kp = torch.randn(B * pages, Hkv, page, D, device=dev, dtype=torch.bfloat16)
            vp = torch.randn(B * pages, Hkv, page, D, device=dev, dtype=torch.bfloat16)
        paged.append((kp, vp, perm.to(torch.int32).reshape(B, pages).contiguous()))

    def run_contiguous(i):
        k, v = contiguous[i]
        ops.fa3_decode(q, k, v, cache_seqlens=sl)

    def run_paged(i):
        kp, vp, bt = paged[i]
        ops.fa3_decode(q, kp, vp, cache_seqlens=sl, block_table=bt)

    def run_gather(i):                  # pages -> contiguous [B, Hkv, S, D] copy, then the contiguous call
        kp, vp, bt = paged[i]
        idx = bt.flatten().long()
        k = kp.index_select(0, idx).reshape(B, pages, Hkv, page, D).permute(0, 2, 1, 3, 4).reshape(B, Hkv, S, D)
        v = vp.index_select(0, idx).reshape(B, pages, Hkv, page, D).permute(0, 2, 1, 3, 4).reshape(B, Hkv, S, D)
        ops.fa3_decode(q, k, v, cache_seqlens=sl)

    paths = {"contiguous": run_contiguous, "paged": run_paged}
    if gather:
        paths["gather_then_decode"] = run_gather
    for f in paths.values():
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
    res = dict(B=B, H=H, Hkv=Hkv, D=D, Skv=S, page=page, pool_layout=layout, cache_MB=round(cache_bytes / 1e6, 2), n_caches=n, reps=reps)
    for name, ts in times.items():
        us = sorted(ts)[len(ts) // 2]
        res[f"{name}_us"] = round(us, 2)
        res[f"{name}_us_min"], res[f"{name}_us_max"] = round(min(ts), 2), round(max(ts), 2)
        res[f"{name}_TBs"] = round(cache_bytes / us / 1e6, 3)
    res["paged_over_contiguous"] = round(res["paged_us"] / res["contiguous_us"], 4)
    del contiguous, paged
    torch.cuda.empty_cache()
    return res


def main_paged(args, dev):
    if args.shapes:
        shapes = [tuple(int(x) for x in s.split(",")) for s in args.shapes.split(";") if s]
    else:               # the shapes DESIGN 4.6 reports
        shapes = [(8, 32, 8, 128, 32768), (8, 32, 8, 128, 131072), (1, 32, 8, 128, 32768), (32, 32, 32, 128, 4096)]
    rows = []
    print(f"{'B':>3} {'H':>3} {'Hkv':>3} {'D':>4} {'Skv':>7} {'page':>5} {'MB':>8} | {'contig us':>9} {'TB/s':>5} | {'paged us':>9} {'TB/s':>5} "
          f"{'ratio':>6}" + (f" | {'gather+decode us':>16}" if args.gather else ""), flush=True)
    for B, H, Hkv, D, S in shapes:
        r = bench_paged(B, H, Hkv, D, S, args.paged, args.reps, args.gather, dev, layout=args.pool_layout)
        if r is None:
            print(f"{B:>3} {H:>3} {Hkv:>3} {D:>4} {S:>7}  skipped (cache above {MAX_CACHE >> 30} GiB, or Skv no multiple of the page)", flush=True)
            continue
        rows.append(r)
        print(f"{B:>3} {H:>3} {Hkv:>3} {D:>4} {S:>7} {args.paged:>5} {r['cache_MB']:>8.1f} | {r['contiguous_us']:>9.2f} {r['contiguous_TBs']:>5.2f} | "
              f"{r['paged_us']:>9.2f} {r['paged_TBs']:>5.2f} {r['paged_over_contiguous']:>6.3f}"
              + (f" | {r['gather_then_decode_us']:>16.2f}" if args.gather else ""), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


def bench_window(B, H, Hkv, D, S, windows, reps, dev):
    """No window, each window over the full cache, and no window over a cache of W keys (the bound), timed alternately."""
    cache_bytes = 2 * B * Hkv * S * D * 2
    if cache_bytes > MAX_CACHE:
        return None
    q = torch.randn(B, H, 1, D, device=dev, dtype=torch.bfloat16)
    n = max(1, math.ceil(MIN_POOL / cache_bytes))
    full = _caches(B, Hkv, S, D, n, dev)
    sl = torch.full((B,), S, dtype=torch.int32, device=dev)
    paths, counts = {"none": lambda i: ops.fa3_decode(q, full[i][0], full[i][1], cache_seqlens=sl)}, {"none": n}
    span_bytes, small = {}, {}
    for W in windows:
        # a windowed call touches only its span: call i reads cache i % n at length S - (i // n) * step, so that the spans of one
        # timed window are disjoint and exceed the pool size together (as far as the caches are long enough)
        span = S - max(0, S - W) // 64 * 64
        span_bytes[W] = 2 * B * Hkv * span * D * 2
        step = (W + 127) // 64 * 64
        per_cache = max(1, min(math.ceil(MIN_POOL / span_bytes[W] / n), (S - W) // step + 1))
        lens = [torch.full((B,), S - j * step, dtype=torch.int32, device=dev) for j in range(per_cache)]
        paths[f"win{W}"] = lambda i, W=W, lens=lens: ops.fa3_decode(q, full[i % n][0], full[i % n][1], cache_seqlens=lens[i // n], window=W)
        counts[f"win{W}"] = n * per_cache
        m = max(1, math.ceil(MIN_POOL / (2 * B * Hkv * W * D * 2)))
        small[W] = _caches(B, Hkv, W, D, m, dev)
        paths[f"bound{W}"] = lambda i, W=W: ops.fa3_decode(q, small[W][i][0], small[W][i][1])
        counts[f"bound{W}"] = m
    for name, f in paths.items():
        for i in range(min(2, counts[name])):
            f(i)
    torch.cuda.synchronize()
    times = {name: [] for name in paths}
    for _ in range(reps):
        for name, f in paths.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(counts[name]):
                f(i)
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / counts[name])
    res = dict(B=B, H=H, Hkv=Hkv, D=D, Skv=S, cache_MB=round(cache_bytes / 1e6, 2), n_caches=n, reps=reps)
    for name, ts in times.items():
        res[f"{name}_us"] = round(sorted(ts)[len(ts) // 2], 2)
        res[f"{name}_us_min"], res[f"{name}_us_max"] = round(min(ts), 2), round(max(ts), 2)
    res["none_TBs"] = round(cache_bytes / res["none_us"] / 1e6, 3)
    for W in windows:
        res[f"win{W}_span_TBs"] = round(span_bytes[W] / res[f"win{W}_us"] / 1e6, 3)
        res[f"win{W}_cycled_span_MB"] = round(counts[f"win{W}"] * span_bytes[W] / 1e6, 1)       # below 256 MB the spans can sit in the Infinity Cache
        res[f"bound{W}_TBs"] = round(2 * B * Hkv * W * D * 2 / res[f"bound{W}_us"] / 1e6, 3)
        res[f"win{W}_over_bound"] = round(res[f"win{W}_us"] / res[f"bound{W}_us"], 3)
    del full, small
    torch.cuda.empty_cache()
    return res


def main_window(args, dev):
    windows = [int(x) for x in args.window.split(",") if x]
    if args.shapes:
        shapes = [tuple(int(x) for x in s.split(",")) for s in args.shapes.split(";") if s]
    else:
        shapes = [(8, 32, 8, 128, 32768), (8, 32, 8, 128, 131072)]
    rows = []
    for B, H, Hkv, D, S in shapes:
        r = bench_window(B, H, Hkv, D, S, windows, args.reps, dev)
        if r is None:
            print(f"B {B} H {H} Hkv {Hkv} D {D} Skv {S}: skipped (cache above {MAX_CACHE >> 30} GiB)", flush=True)
            continue
        rows.append(r)
        print(f"B {B} H {H} Hkv {Hkv} D {D} Skv {S}: no window {r['none_us']:.2f} us [{r['none_us_min']:.2f}, {r['none_us_max']:.2f}] "
              f"{r['none_TBs']:.2f} TB/s", flush=True)
        for W in windows:
            print(f"    W {W:>6}: {r[f'win{W}_us']:.2f} us [{r[f'win{W}_us_min']:.2f}, {r[f'win{W}_us_max']:.2f}] {r[f'win{W}_span_TBs']:.2f} TB/s "
                  f"of the span ({r[f'win{W}_cycled_span_MB']:.0f} MB of spans cycled) | Skv = W without a window {r[f'bound{W}_us']:.2f} us "
                  f"[{r[f'bound{W}_us_min']:.2f}, {r[f'bound{W}_us_max']:.2f}] | ratio {r[f'win{W}_over_bound']:.3f}", flush=True)
    if args.json:
        with open(args.json, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


def host_cost(dev):
    """Python + ctypes cost of one fa3_decode call (enqueue only: the GPU side is tiny), and one graph replay of it."""
    B, H, Hkv, D, S = 1, 32, 8, 128, 4096
    q = torch.randn(B, H, 1, D, device=dev, dtype=torch.bfloat16)
    k = torch.randn(B, Hkv, S, D, device=dev, dtype=torch.bfloat16)
    v = torch.randn_like(k)
    sl = torch.full((B,), S, dtype=torch.int32, device=dev)
    for _ in range(50):
        ops.fa3_decode(q, k, v, cache_seqlens=sl)
    torch.cuda.synchronize()
    out = {}
    for label, kw in (("host_us_per_call_seqlens", dict(cache_seqlens=sl)), ("host_us_per_call_keymask",
                                                                              dict(key_mask=torch.ones(B, S, dtype=torch.bool, device=dev)))):
        t0 = time.perf_counter()
        for _ in range(500):
            ops.fa3_decode(q, k, v, **kw)
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        out[label] = round((t1 - t0) / 500 * 1e6, 2)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.fa3_decode(q, k, v, cache_seqlens=sl)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.fa3_decode(q, k, v, cache_seqlens=sl)
    graph.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(200):
        graph.replay()
    e1.record()
    e1.synchronize()
    out["graph_replay_us_per_call"] = round(e0.elapsed_time(e1) * 1e3 / 200, 2)
    t0 = time.perf_counter()
    for _ in range(200):
        graph.replay()
    out["graph_replay_host_us"] = round((time.perf_counter() - t0) / 200 * 1e6, 2)
    torch.cuda.synchronize()
    out["shape"] = dict(B=B, H=H, Hkv=Hkv, D=D, Skv=S)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="B 1 and 8, Llama-3-8B heads only")
    ap.add_argument("--warm", action="store_true")
    ap.add_argument("--json", default=None)
    ap.add_argument("--paged", type=int, default=0, metavar="PAGE_SIZE", help="measure the paged cache with pages of this many keys")
    ap.add_argument("--gather", action="store_true", help="with --paged: also time gathering the pages with torch ops, then decoding")
    ap.add_argument("--pool-layout", choices=("phsd", "hpsd"), default="phsd",
                    help="with --paged: pools as [num_pages, page, Hkv, D] (flash-attn style, a token's heads adjacent) or [num_pages, Hkv, page, D] "
                         "(a head's tokens adjacent, like the contiguous [B, Hkv, S, D] caches this tool times)")
    ap.add_argument("--shapes", default=None, help='with --paged / --window: "B,H,Hkv,D,Skv;..." instead of the DESIGN 4.6 shapes')
    ap.add_argument("--window", default=None, metavar="W[,W...]", help="measure sliding windows of these many keys against no window")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "decode_bench measures on the GPU"
    dev = torch.device("cuda:0")
    if args.paged:
        main_paged(args, dev)
        return
    if args.window:
        main_window(args, dev)
        return
    heads = [(32, 8, 128), (64, 8, 128), (32, 32, 128), (16, 16, 64)]
    Bs, Ss = [1, 8, 32], [4096, 32768, 131072]
    if args.quick:
        heads, Bs, Ss = heads[:1], [1, 8], [32768]
    rows = []
    hdr = f"{'B':>3} {'H':>3} {'Hkv':>3} {'D':>4} {'Skv':>7} {'MB':>8} {'split':>5} | {'decode us':>9} {'TB/s':>5} {'%':>5} | " \
          f"{'fwd us':>9} {'TB/s':>5} | {'sdpa us':>9} {'TB/s':>5}"
    print(hdr, flush=True)
    for H, Hkv, D in heads:
        for B in Bs:
            for S in Ss:
                r = bench_shape(B, H, Hkv, D, S, args.reps, args.warm, dev)
                if r is None:
                    print(f"{B:>3} {H:>3} {Hkv:>3} {D:>4} {S:>7}  skipped: one cache exceeds {MAX_CACHE >> 30} GiB", flush=True)
                    continue
                rows.append(r)
                print(f"{B:>3} {H:>3} {Hkv:>3} {D:>4} {S:>7} {r['cache_MB']:>8.1f} {r['nsplit']:>5} | {r['fa3_decode_us']:>9.2f} "
                      f"{r['fa3_decode_TBs']:>5.2f} {r['fa3_decode_pct_hbm']:>5.1f} | {r['fa3_forward_us']:>9.2f} {r['fa3_forward_TBs']:>5.2f} | "
                      f"{r['sdpa_us']:>9.2f} {r['sdpa_TBs']:>5.2f}"
                      + (f"   warm single cache {r['fa3_decode_warm_single_cache_us']:.2f} us" if args.warm else ""), flush=True)
    hc = host_cost(dev)
    print("host cost:", json.dumps(hc), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
            f.write(json.dumps({"host": hc}) + "\n")


if __name__ == "__main__":
    main()

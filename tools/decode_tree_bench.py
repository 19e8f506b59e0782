"""Tree verification step on the MI355X: ``ops.fa3_decode(tree_mask=)`` against (a) the plain causal call of the same shapes and (b) the
workaround it replaces -- the Sq nodes folded into the batch as ``B * Sq`` one-row sequences with a byte ``key_mask`` and a repeated
block table -- with the mask build inside and outside the timed step.

Every variant is a captured graph over a paged cache (pages of ``--page`` keys, head-major pools); timing cycles through enough
distinct pools (>= 768 MiB in all) that the 256 MiB Infinity Cache cannot serve them, and the variants are timed alternately with
device events.  The causal call is captured twice ("causal", "causal_again"): the ratio of the two identical graphs and each variant's
[min, max] over the repetitions are the run-to-run spread the tree / causal ratio has to be read against.  Seeded.

    python tools/decode_tree_bench.py [--reps 7] [--shapes "B,H,Hkv,D,Skv,Sq;..."] [--page 256] [--no-folded] [--json out.jsonl]
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

MIN_POOL = 768 << 20
MAX_CACHE = 12 << 30
DEFAULT_SHAPES = [(B, 32, 8, 128, S, Sq) for B in (8, 32) for S in (8192, 32768) for Sq in (16, 64)]


def random_tree(B, Sq, seed, dev):
    g = torch.Generator().manual_seed(seed)
    parents = torch.stack([torch.randint(-1, i, (B,), generator=g) if i else torch.full((B,), -1) for i in range(Sq)], dim=1)
    return ops.tree_mask_from_parents(parents.to(dev))[0]


def folded_mask(words, lens, Sq, S):
    """The workaround's byte mask [B * Sq, S] from the words: row i of sequence b sees key j iff j < off_b or bit j - off_b is set."""
    j = torch.arange(S, device=words.device)
    rel = j[None, :] - (lens.long() - Sq)[:, None]
    bit = ((words[:, :, None] >> rel.clamp(0, 63)[:, None, :]) & 1).bool()
    return ((rel < 0)[:, None, :] | bit).reshape(-1, S)


def capture(step):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    return graph


def bench_shape(B, H, Hkv, D, S, Sq, page, reps, folded, dev, seed=0):
    cache_bytes = 2 * B * Hkv * S * D * 2
    if cache_bytes > MAX_CACHE or S % page:
        return None
    torch.manual_seed(seed)
    n = max(1, math.ceil(MIN_POOL / cache_bytes))
    pages = S // page
    q = torch.randn(B, Sq, H, D, device=dev, dtype=torch.bfloat16).permute(0, 2, 1, 3)
    lens = torch.full((B,), S, dtype=torch.int32, device=dev)
    words = random_tree(B, Sq, seed + 1, dev)
    pools = []
    for i in range(n):
        perm = torch.randperm(B * pages, generator=torch.Generator().manual_seed(seed + 10 + i)).to(dev)
        kp = torch.randn(B * pages, Hkv, page, D, device=dev, dtype=torch.bfloat16)
        vp = torch.randn(B * pages, Hkv, page, D, device=dev, dtype=torch.bfloat16)
        pools.append((kp, vp, perm.to(torch.int32).reshape(B, pages).contiguous()))
    # the workaround's operands
    qf = q.permute(0, 2, 1, 3).reshape(B * Sq, H, 1, D)
    lens_f = lens.repeat_interleave(Sq)
    mask_f = folded_mask(words, lens, Sq, S)

    def causal(i):
        kp, vp, bt = pools[i]
        return lambda: ops.fa3_decode(q, kp, vp, cache_seqlens=lens, block_table=bt)

    def tree(i):
        kp, vp, bt = pools[i]
        return lambda: ops.fa3_decode(q, kp, vp, cache_seqlens=lens, block_table=bt, tree_mask=words)

    def fold(i, build):
        kp, vp, bt = pools[i]
        btf = bt.repeat_interleave(Sq, dim=0)

        def step():
            m = folded_mask(words, lens, Sq, S) if build else mask_f
            t = bt.repeat_interleave(Sq, dim=0) if build else btf
            ops.fa3_decode(qf, kp, vp, cache_seqlens=lens_f, block_table=t, key_mask=m, causal=False)
        return step

    makers = {"causal": causal, "tree": tree, "causal_again": causal}
    if folded:
        makers["folded"] = lambda i: fold(i, False)
        makers["folded_with_mask_build"] = lambda i: fold(i, True)
    graphs = {name: [capture(mk(i)) for i in range(n)] for name, mk in makers.items()}
    for gs in graphs.values():
        for g in gs:
            g.replay()
    torch.cuda.synchronize()
    times = {name: [] for name in graphs}
    for _ in range(reps):
        for name, gs in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for g in gs:
                g.replay()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / n)
    res = dict(B=B, H=H, Hkv=Hkv, D=D, Skv=S, Sq=Sq, page=page, cache_MB=round(cache_bytes / 1e6, 2), n_pools=n, reps=reps,
               folded_mask_MB=round(B * Sq * S / 1e6, 2))
    for name, ts in times.items():
        res[f"{name}_us"] = round(sorted(ts)[len(ts) // 2], 2)
        res[f"{name}_us_min"], res[f"{name}_us_max"] = round(min(ts), 2), round(max(ts), 2)
    res["causal_TBs"] = round(cache_bytes / res["causal_us"] / 1e6, 3)
    res["tree_over_causal"] = round(res["tree_us"] / res["causal_us"], 4)
    res["causal_again_over_causal"] = round(res["causal_again_us"] / res["causal_us"], 4)
    res["causal_spread"] = round((res["causal_us_max"] - res["causal_us_min"]) / res["causal_us"], 4)
    if folded:
        res["folded_over_tree"] = round(res["folded_us"] / res["tree_us"], 2)
        res["folded_with_mask_build_over_tree"] = round(res["folded_with_mask_build_us"] / res["tree_us"], 2)
    del graphs, pools
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--page", type=int, default=256)
    ap.add_argument("--shapes", default=None, help='"B,H,Hkv,D,Skv,Sq;..." instead of B 8 / 32, H 32 / Hkv 8, D 128, Skv 8192 / 32768, Sq 16 / 64')
    ap.add_argument("--no-folded", action="store_true", help="leave out the folded workaround (it streams the cache Sq times)")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "decode_tree_bench measures on the GPU"
    dev = torch.device("cuda:0")
    shapes = DEFAULT_SHAPES if not args.shapes else [tuple(int(x) for x in s.split(",")) for s in args.shapes.split(";") if s]
    rows = []
    for B, H, Hkv, D, S, Sq in shapes:
        r = bench_shape(B, H, Hkv, D, S, Sq, args.page, args.reps, not args.no_folded, dev)
        if r is None:
            print(f"B {B} H {H} Hkv {Hkv} D {D} Skv {S} Sq {Sq}: skipped (cache above {MAX_CACHE >> 30} GiB, or Skv no multiple of the page)", flush=True)
            continue
        rows.append(r)
        line = (f"B {B:>2} H {H} Hkv {Hkv} D {D} Skv {S:>6} Sq {Sq:>2}: causal {r['causal_us']:.2f} us [{r['causal_us_min']:.2f}, {r['causal_us_max']:.2f}] "
                f"{r['causal_TBs']:.2f} TB/s | tree {r['tree_us']:.2f} us [{r['tree_us_min']:.2f}, {r['tree_us_max']:.2f}] ratio {r['tree_over_causal']:.4f} | "
                f"causal again {r['causal_again_us']:.2f} us ratio {r['causal_again_over_causal']:.4f}")
        if not args.no_folded:
            line += (f" | folded {r['folded_us']:.1f} us ({r['folded_over_tree']:.1f} x tree), with the mask build "
                     f"{r['folded_with_mask_build_us']:.1f} us ({r['folded_with_mask_build_over_tree']:.1f} x); mask {r['folded_mask_MB']:.1f} MB")
        print(line, flush=True)
        if args.json:                                   # after every shape: a run cut short keeps what it measured
            with open(args.json, "w") as f:
                for x in rows:
                    f.write(json.dumps(x) + "\n")


if __name__ == "__main__":
    main()

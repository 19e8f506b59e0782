"""What attention sinks cost on the MI355X: every call over the KV cache with ``sinks=`` against the same call without, alternated in
one process (profiles/attn_sinks.md).

Per row three paths are timed alternately -- the call without sinks, the call with sinks, the call without sinks again -- each as one
captured graph that runs the call once over every cache of a pool of >= 768 MiB of keys and values (like a model's layers: the
256 MiB Infinity Cache cannot serve them), replayed ``--reps`` times between device events.  The table gives the median of each, the
ratio sinks / plain, and the run-to-run spread of the sink-less call: the distance between its two medians and the (max - min) / median of
its replays.  The expectation is a ratio inside that spread -- a load and a few operations per row, outside the tile loop -- and it is an
expectation, not a pass mark: the tool asserts nothing about time.

    python tools/attn_sinks_bench.py [--reps 9] [--quick] [--json out.jsonl]

Rows: decode B 8 and B 1, H 64 / Hkv 8, D 64, Skv 32768, with and without a 128-key window; prefill of a 2048-row chunk and of a
256-row chunk (``key_splits="auto"``) over 8192 keys, B 1."""

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
H, HKV, D = 64, 8, 64

ROWS = [  # (name, call, B, Sq, Skv, extra keywords)
    ("decode B8", "decode", 8, 1, 32768, {}),
    ("decode B8 W128", "decode", 8, 1, 32768, dict(window=128)),
    ("decode B1", "decode", 1, 1, 32768, {}),
    ("decode B1 W128", "decode", 1, 1, 32768, dict(window=128)),
    ("prefill 2048 rows", "prefill", 1, 2048, 8192, {}),
    ("prefill 256 rows, key_splits auto", "prefill", 1, 256, 8192, dict(key_splits="auto")),
]


def bench_row(name, call, B, Sq, Skv, kw, reps, dev):
    cache_bytes = 2 * B * HKV * Skv * D * 2
    n = max(2, math.ceil(MIN_POOL / cache_bytes))
    pool = [(torch.randn(B, HKV, Skv, D, device=dev, dtype=torch.bfloat16), torch.randn(B, HKV, Skv, D, device=dev, dtype=torch.bfloat16))
            for _ in range(n)]
    q = torch.randn(B, Sq, H, D, device=dev, dtype=torch.bfloat16).permute(0, 2, 1, 3)
    lens = torch.full((B,), Skv, dtype=torch.int32, device=dev)
    sinks = torch.randn(H, device=dev) + math.log(Skv if "window" not in kw else kw["window"])      # of the order of the rows' LSE
    fn = ops.fa3_decode if call == "decode" else ops.fa3_prefill_cache
    out = torch.empty(B, Sq, H, D, device=dev, dtype=torch.bfloat16).permute(0, 2, 1, 3)

    def sweep(s):
        for k, v in pool:
            fn(q, k, v, cache_seqlens=lens, sinks=s, out=out, **kw)

    graphs = {}
    for path, s in (("plain_a", None), ("sinks", sinks), ("plain_b", None)):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            sweep(s)                                   # warm-up: code objects, allocator
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            sweep(s)
        graphs[path] = g
    times = {p: [] for p in graphs}
    for g in graphs.values():
        g.replay()
    torch.cuda.synchronize()
    for _ in range(reps):
        for path, g in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            e1.synchronize()
            times[path].append(e0.elapsed_time(e1) * 1e3 / n)
    med = {p: sorted(t)[len(t) // 2] for p, t in times.items()}
    plain = 0.5 * (med["plain_a"] + med["plain_b"])
    both = times["plain_a"] + times["plain_b"]
    res = dict(row=name, B=B, Sq=Sq, Skv=Skv, n_caches=n, plain_us=round(plain, 2), sinks_us=round(med["sinks"], 2),
               ratio=round(med["sinks"] / plain, 4), plain_a_us=round(med["plain_a"], 2), plain_b_us=round(med["plain_b"], 2),
               plain_ab=round(abs(med["plain_a"] - med["plain_b"]) / plain, 4), plain_range=round((max(both) - min(both)) / plain, 4),
               sinks_range=round((max(times["sinks"]) - min(times["sinks"])) / med["sinks"], 4), **{k: str(v) for k, v in kw.items()})
    del pool, graphs
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--quick", action="store_true", help="the first and the last row only")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = [ROWS[0], ROWS[-1]] if args.quick else ROWS
    print("| call | plain us | sinks us | sinks / plain | plain A vs B | plain (max - min) / median | sinks (max - min) / median |")
    print("|---|---|---|---|---|---|---|")
    for row in rows:
        r = bench_row(*row, args.reps, dev)
        print(f"| {r['row']} | {r['plain_us']} | {r['sinks_us']} | {r['ratio']:.4f} | {r['plain_ab']:.4f} | {r['plain_range']:.4f} | "
              f"{r['sinks_range']:.4f} |", flush=True)
        if args.json:
            with open(args.json, "a") as f:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()

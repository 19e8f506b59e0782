"""The forward over a KV cache with its keys split over workgroups, on the MI355X: ``ops.fa3_prefill_cache(..., key_splits=)`` against
the call without the keyword, and ``prefix_key_splits=`` on the shared-prefix step (``profiles/prefill_split.md``).

Two sweeps, H 32 / Hkv 8, D 128, bf16:

* ``chunk``: chunked prefill at B = 1, causal -- Sq in {256, 512, 1024, 2048} new rows against a cache that holds 8192, 32768 or 131072
  keys (the rows' own included), contiguous and in pages of 256.  B * H * ceil(Sq / 256) is 32 .. 256 workgroups.
* ``prefix``: the decode step of tools/shared_prefix_bench.py (shared prefix pages, 256 private keys) at the shapes whose prefix pass
  has more than 64 rows and therefore is ``fa3_prefill_cache`` over one sequence of B * Sq rows, plus B 64 (64 rows: the decode
  kernel serves the pass and the keyword changes nothing).

Timing follows tools/shared_prefix_bench.py: every variant is a captured graph per cache (one graph pool, so the workspace is one
buffer as in a serving step), the caches cycle through >= 768 MiB so that the 256 MiB Infinity Cache cannot carry one to its next use,
the variants are timed alternately with device events, median of ``--reps`` rounds with min and max.  Inputs are seeded per shape.

The baseline of every ratio is the PARENT commit, measured in the same session on the same inputs: build the parent in a directory of
its own, copy this file and shared_prefix_bench.py into its tools/, run it there with ``--variants none --json parent.jsonl`` (``none``
passes no keyword, so the file runs on a build that has none), then run this build with ``--baseline parent.jsonl``.  Several baseline
files (the parent before and after) give the spread of repeated baseline runs: a row's ``parent_us`` is their median, and
``parent_spread`` is (max - min) / median over them.

    python tools/prefill_split_bench.py [--sweeps chunk,prefix] [--variants none,2,4,8,auto] [--prefix-variants none,auto] [--reps 5]
                                        [--json out.jsonl] [--baseline parent_a.jsonl parent_b.jsonl]
    python tools/prefill_split_bench.py --dry          # shapes, workgroups, workspace and the plan's count without a GPU"""

from __future__ import annotations

import argparse
import ctypes as C
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from photonic_flash_attention_amd import _capi, ops  # noqa: E402
import shared_prefix_bench as spb  # noqa: E402

MIN_POOL = 768 << 20
MAX_CACHES = 32
PAGE = 256
H, HKV, D = 32, 8, 128
CHUNK_SHAPES = [(Sq, L) for L in (8192, 32768, 131072) for Sq in (256, 512, 1024, 2048)]
PREFIX_SHAPES = [(128, 1, 32768), (32, 16, 32768), (64, 1, 8192), (128, 1, 8192), (32, 16, 8192)]


def parse_variant(s):
    return None if s == "none" else "auto" if s == "auto" else int(s)


def resolved(B, Sq, Smax, variant):
    """The number of splits ``variant`` resolves to for a [B, H, Sq, D] query over Smax keys (1 for None; None on a build without the
    entry point)."""
    if variant is None:
        return 1
    if "pfa_fa3_prefill_split_plan" not in _capi.EXPORTS:
        return None
    a = _capi.make_decode_args(B=B, H=H, Hkv=HKV, Sq=Sq, Smax=Smax, D=D)
    return int(_capi.load().pfa_fa3_prefill_split_plan(C.byref(a), 0 if variant == "auto" else variant))


def workspace_mb(B, Sq, n):
    return 0.0 if not n or n < 2 else round(n * B * Sq * H * (D + 1) * 4 / 1e6, 2)


def capture_all(fns, n):
    """One captured graph per cache for every path, all in one pool -> name -> replay(i)."""
    side, pool, out = torch.cuda.Stream(), torch.cuda.graph_pool_handle(), {}
    for name, f in fns.items():
        gs = []
        for i in range(n):
            if i < 2:                                   # warm-up: code objects, allocator
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    f(i)
                torch.cuda.current_stream().wait_stream(side)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, pool=pool):
                f(i)
            gs.append(g)
        out[name] = lambda i, gs=gs: gs[i].replay()
        out[name](0)
    torch.cuda.synchronize()
    return out


def chunk_caches(L, layout, n, dev):
    lens = torch.full((1,), L, dtype=torch.int32, device=dev)
    out = []
    for i in range(n):
        if layout == "paged":
            pages = L // PAGE
            kp = torch.randn(pages, PAGE, HKV, D, device=dev, dtype=torch.bfloat16).transpose(1, 2)
            vp = torch.randn(pages, PAGE, HKV, D, device=dev, dtype=torch.bfloat16).transpose(1, 2)
            table = torch.randperm(pages, generator=torch.Generator().manual_seed(i)).to(torch.int32).reshape(1, pages).to(dev)
            out.append((kp, vp, dict(cache_seqlens=lens, block_table=table)))
        else:
            k = torch.randn(1, L, HKV, D, device=dev, dtype=torch.bfloat16).transpose(1, 2)
            v = torch.randn(1, L, HKV, D, device=dev, dtype=torch.bfloat16).transpose(1, 2)
            out.append((k, v, dict(cache_seqlens=lens)))
    return out


def bench_chunk(Sq, L, layout, variants, reps, dev):
    torch.manual_seed(Sq * 7 + L)
    held = 2 * L * HKV * D * 2
    n = min(MAX_CACHES, max(2, math.ceil(MIN_POOL / held)))
    caches = chunk_caches(L, layout, n, dev)
    q = torch.randn(1, Sq, H, D, device=dev, dtype=torch.bfloat16).transpose(1, 2)
    o = torch.empty(1, Sq, H, D, device=dev, dtype=torch.bfloat16).transpose(1, 2)

    def path(variant):
        kw = {} if variant is None else dict(key_splits=variant)
        return lambda i: ops.fa3_prefill_cache(q, caches[i][0], caches[i][1], out=o, causal=True, **caches[i][2], **kw)

    fns = capture_all({str(v).lower(): path(v) for v in variants}, n)
    times = spb.timed(fns, {name: n for name in fns}, reps)
    rows = []
    for v in variants:
        med, lo, hi = times[str(v).lower()]
        ns = resolved(1, Sq, L, v)
        rows.append(dict(sweep="chunk", layout=layout, B=1, Sq=Sq, keys=L, H=H, Hkv=HKV, D=D, page=PAGE if layout == "paged" else 0,
                         variant=str(v).lower(), nsplit=ns, workgroups=None if ns is None else H * -(-Sq // 256) * ns,
                         workspace_MB=workspace_mb(1, Sq, ns), n_caches=n, reps=reps, us=round(med, 2), us_min=round(lo, 2), us_max=round(hi, 2)))
    del caches, fns
    torch.cuda.empty_cache()
    return rows


def bench_prefix(B, Sq, P, variants, reps, dev):
    torch.manual_seed(B * 1000 + Sq * 10 + P)
    _, _, held, n = spb.plan(B, Sq, P, "paged")
    n = min(MAX_CACHES, max(2, n))
    caches = spb.make_caches(B, Sq, P, "paged", n, dev)
    q = torch.randn(B, Sq, H, D, device=dev, dtype=torch.bfloat16).transpose(1, 2)
    o = torch.empty(B, Sq, H, D, device=dev, dtype=torch.bfloat16).transpose(1, 2)

    def path(variant):
        kw = {} if variant is None else dict(prefix_key_splits=variant)
        return lambda i: ops.fa3_decode(q, caches[i][0], caches[i][1], out=o, shared_prefix=P, **caches[i][2], **kw)

    fns = {str(v).lower(): path(v) for v in variants}
    fns["plain"] = lambda i: ops.fa3_decode(q, caches[i][0], caches[i][1], out=o, **caches[i][2])        # the step without shared_prefix
    fns = capture_all(fns, n)
    times = spb.timed(fns, {name: n for name in fns}, reps)
    rows = []
    for v in list(variants) + ["plain"]:
        med, lo, hi = times[str(v).lower()]
        rowsq = B * Sq
        ns = 1 if v == "plain" else resolved(1, rowsq, P, v) if rowsq > 64 else 1
        rows.append(dict(sweep="prefix", layout="paged", B=B, Sq=Sq, keys=P, private=spb.PRIVATE, H=H, Hkv=HKV, D=D, page=PAGE,
                         variant=str(v).lower(), prefix_pass="none" if v == "plain" else "fa3_decode" if rowsq <= 64 else "fa3_prefill_cache",
                         nsplit=ns, workgroups=None if ns is None else H * -(-rowsq // 256) * ns, workspace_MB=workspace_mb(1, rowsq, ns),
                         n_caches=n, reps=reps, us=round(med, 2), us_min=round(lo, 2), us_max=round(hi, 2)))
    del caches, fns
    torch.cuda.empty_cache()
    return rows


def key_of(r):
    return (r["sweep"], r["layout"], r["B"], r["Sq"], r["keys"])


def load_baselines(paths):
    """(shape key) -> the ``none`` rows' times, one per baseline file."""
    base = {}
    for p in paths or ():
        with open(p) as f:
            for line in f:
                r = json.loads(line)
                if r.get("variant") == "none":
                    base.setdefault(key_of(r), []).append(r["us"])
    return base


def add_baseline(r, base):
    ts = sorted(base.get(key_of(r), ()))
    if ts:
        med = ts[len(ts) // 2] if len(ts) % 2 else (ts[len(ts) // 2 - 1] + ts[len(ts) // 2]) / 2
        r["parent_us"], r["parent_runs"], r["parent_spread"] = round(med, 2), ts, round((ts[-1] - ts[0]) / med, 4)
        r["parent_over_this"] = round(med / r["us"], 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweeps", default="chunk,prefix")
    ap.add_argument("--variants", default="none,2,4,8,auto")
    ap.add_argument("--prefix-variants", default="none,auto", help="of the prefix sweep (those of --variants that are listed here)")
    ap.add_argument("--layouts", default="contiguous,paged", help="of the chunk sweep")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--baseline", nargs="*", default=None, help="JSON lines of the parent commit's runs (--variants none)")
    ap.add_argument("--dry", action="store_true", help="print shapes, workgroups, workspace and the plan and stop: no GPU needed")
    args = ap.parse_args()
    variants = [parse_variant(s) for s in args.variants.split(",") if s]
    sweeps = [s for s in args.sweeps.split(",") if s]
    if args.dry:
        for Sq, L in CHUNK_SHAPES:
            ns = resolved(1, Sq, L, "auto")
            print(f"chunk  B 1 Sq {Sq:>4} keys {L:>6}: {H * -(-Sq // 256):>3} workgroups unsplit, plan {ns}, workspace {workspace_mb(1, Sq, ns)} MB "
                  f"(8 splits: {workspace_mb(1, Sq, 8)} MB)")
        for B, Sq, P in PREFIX_SHAPES:
            rows = B * Sq
            ns = resolved(1, rows, P, "auto") if rows > 64 else 1
            print(f"prefix B {B:>3} Sq {Sq:>2} P {P:>5}: prefix pass of {rows} rows, {H * -(-rows // 256):>3} workgroups unsplit, plan {ns}, "
                  f"workspace {workspace_mb(1, rows, ns)} MB")
        return
    assert torch.cuda.is_available(), "prefill_split_bench measures on the GPU"
    dev = torch.device("cuda:0")
    base = load_baselines(args.baseline)
    out = []

    def report(rows):
        for r in rows:
            add_baseline(r, base)
            out.append(r)
            line = (f"{r['sweep']:>6} {r['layout']:>10} B {r['B']:>3} Sq {r['Sq']:>4} keys {r['keys']:>6} {r['variant']:>5} (N {r['nsplit']}, "
                    f"{r['workgroups']} wg, ws {r['workspace_MB']} MB): {r['us']:>9.2f} us [{r['us_min']:.2f}, {r['us_max']:.2f}]")
            if "parent_us" in r:
                line += f" | parent {r['parent_us']:.2f} us (spread {100 * r['parent_spread']:.1f} %), parent / this {r['parent_over_this']:.3f}"
            print(line, flush=True)

    if "chunk" in sweeps:
        for layout in (x for x in args.layouts.split(",") if x):
            for Sq, L in CHUNK_SHAPES:
                report(bench_chunk(Sq, L, layout, variants, args.reps, dev))
    if "prefix" in sweeps:
        allowed = [parse_variant(x) for x in args.prefix_variants.split(",") if x]
        pv = [v for v in variants if v in allowed]
        for B, Sq, P in PREFIX_SHAPES:
            report(bench_prefix(B, Sq, P, pv, args.reps, dev))
    if args.json:
        with open(args.json, "w") as f:
            for r in out:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()

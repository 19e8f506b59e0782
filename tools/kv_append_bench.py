"""The device-side KV-cache append on the MI355X: ``PagedKVCache.advance`` + ``write_step`` (``ops.kv_append``, one HIP copy kernel that
places a step's rows from the device table and lengths) against the path it stands next to, ``PagedKVCache.append_varlen`` (a Python
loop per token that builds an index list, its upload, two ``index_copy_``), and against a plain ``torch`` device copy of the same
bytes as the roof.

Per step shape, two kinds of number:
  host   wall time per step of the whole append, host bookkeeping included, a window of ``--calls`` successive steps that ends in a
         device synchronise (the sequences grow over the window; the slots are freed and re-allocated between windows):
         ``append_varlen`` against ``advance`` + ``write_step`` with a device ``cu_seqlens_q`` (the form a graph holds);
  device HIP-event time per launch of the device part alone, back to back with no host work in between: ``write_step`` (the
         kernel), the two ``index_copy_`` of the parent path with a prebuilt index, and ``copy_`` of K and V into contiguous
         buffers (the roof).  bytes = 2 tensors x rows x Hkv x D x 2 B, read once and written once.
The paths of a comparison are timed alternately, ``--reps`` windows each; the median is reported with minimum and maximum in the
JSON, and the first path is timed twice (``*_again``): the ratio of its two medians is the spread a ratio has to clear.

    python tools/kv_append_bench.py [--reps 5] [--calls 20] [--only decode,chunk,mixed] [--json out.jsonl]
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from photonic_flash_attention_amd import _capi  # noqa: E402
from photonic_flash_attention_amd.integration.pytorch import PagedKVCache  # noqa: E402

BF, HKV, D, PAGE = torch.bfloat16, 8, 128, 64
SHAPES = {
    "decode": [1] * 64,                   # B 64 x 1 token
    "chunk": [2048],                      # one 2048-token chunk
    "mixed": [512] + [1] * 63,            # a chunk plus decode rows
}


def _med(ts):
    return sorted(ts)[len(ts) // 2]


def _host_windows(paths, reset, calls, reps):
    """-> {name: [us per step, ...]}: wall time of `calls` successive steps, ended by a synchronise."""
    times = {name: [] for name in paths}
    for rep in range(reps + 1):               # window 0 warms up
        for name, f in paths.items():
            reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                f()
            torch.cuda.synchronize()
            if rep:
                times[name].append((time.perf_counter() - t0) * 1e6 / calls)
    return times


def _device_windows(paths, calls, reps):
    """-> {name: [us per launch, ...]} from device events around `calls` back-to-back launches."""
    times = {name: [] for name in paths}
    for rep in range(reps + 1):
        for name, f in paths.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                f()
            e1.record()
            e1.synchronize()
            if rep:
                times[name].append(e0.elapsed_time(e1) * 1e3 / calls)
    return times


def bench(kind, q_lens, calls, reps, dev):
    B, total, max_q = len(q_lens), sum(q_lens), max(q_lens)
    per_seq = [-(-calls * x // PAGE) + 1 for x in q_lens]
    cache = PagedKVCache(num_pages=sum(per_seq), page_size=PAGE, Hkv=HKV, D=D, dtype=BF, device=dev, max_batch=B, max_pages_per_seq=max(per_seq))
    slots = list(range(B))
    k, v = torch.randn(total, HKV, D, device=dev, dtype=BF), torch.randn(total, HKV, D, device=dev, dtype=BF)
    at = [0]
    for x in q_lens:
        at.append(at[-1] + x)
    cu = torch.tensor(at, dtype=torch.int32, device=dev)
    live = []

    def reset():
        for s in live:
            cache.free(s)
        live[:] = [cache.allocate() for _ in range(B)]

    def parent():
        cache.append_varlen(slots, k, v, q_lens)

    def new():
        cache.advance(slots, q_lens)
        cache.write_step(k, v, cu_seqlens_q=cu, max_seqlen_q=max_q)

    a = _capi.make_kv_append_args(k_new=1 << 12, v_new=1 << 12, k_cache=1 << 12, v_cache=1 << 12, cu_seqlens_q=1 << 12, cache_seqlens=1 << 12,
                                  block_table=1 << 12, block_table_stride_b=max(per_seq), page_size=PAGE, num_pages=sum(per_seq), B=B, Hkv=HKV,
                                  total_new=total, max_seqlen_q=max_q, Smax=max(per_seq) * PAGE, D=D, kn_stride_s=HKV * D, kn_stride_h=D,
                                  vn_stride_s=HKV * D, vn_stride_h=D, k_stride_b=PAGE * HKV * D, k_stride_s=HKV * D, k_stride_h=D,
                                  v_stride_b=PAGE * HKV * D, v_stride_s=HKV * D, v_stride_h=D)
    name, wgs = _capi.describe_kv_append(a)
    nbytes = 2 * 2 * total * HKV * D * 2
    res = dict(kind=kind, B=B, Hkv=HKV, D=D, page=PAGE, q_lens=f"{q_lens[0]}" + (f"+{B - 1}x{q_lens[-1]}" if B > 1 else ""), rows=total,
               calls=calls, reps=reps, kernel=name, workgroups=wgs, bytes=nbytes)
    host = _host_windows({"parent": parent, "new": new, "parent_again": parent}, reset, calls, reps)

    # the device parts alone, at one fixed state: every launch writes the same destinations
    reset()
    cache.advance(slots, q_lens)
    idx = torch.tensor(cache._dst_rows(slots, [0] * B, q_lens), dtype=torch.int64, device=dev)
    rows = cache.num_pages * PAGE
    kflat, vflat = cache.k_pool.view(rows, HKV, D), cache.v_pool.view(rows, HKV, D)
    kdst, vdst = torch.empty_like(k), torch.empty_like(v)

    def kernel():
        cache.write_step(k, v, cu_seqlens_q=cu, max_seqlen_q=max_q)

    def index_copy():
        kflat.index_copy_(0, idx, k)
        vflat.index_copy_(0, idx, v)

    def roof():
        kdst.copy_(k)
        vdst.copy_(v)

    devt = _device_windows({"kernel": kernel, "index_copy": index_copy, "roof": roof, "kernel_again": kernel}, max(calls, 50), reps)
    for group, times in (("host", host), ("device", devt)):
        for n, ts in times.items():
            res[f"{group}_{n}_us"] = round(_med(ts), 2)
            res[f"{group}_{n}_us_min"], res[f"{group}_{n}_us_max"] = round(min(ts), 2), round(max(ts), 2)
    res["host_new_over_parent"] = round(res["host_new_us"] / res["host_parent_us"], 4)
    res["host_parent_again_over_parent"] = round(res["host_parent_again_us"] / res["host_parent_us"], 4)
    res["device_kernel_over_index_copy"] = round(res["device_kernel_us"] / res["device_index_copy_us"], 4)
    res["device_kernel_over_roof"] = round(res["device_kernel_us"] / res["device_roof_us"], 4)
    res["device_kernel_again_over_kernel"] = round(res["device_kernel_again_us"] / res["device_kernel_us"], 4)
    res["device_kernel_GBps"] = round(nbytes / res["device_kernel_us"] / 1e3, 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--only", default="decode,chunk,mixed")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "kv_append_bench measures on the GPU"
    dev = torch.device("cuda:0")
    out = []
    print(f"{'kind':>6} {'rows':>5} {'WGs':>5} | host us/step: {'parent':>9} {'new':>9} {'new/parent':>10} {'again/parent':>12} | "
          f"device us/launch: {'kernel':>8} {'index_copy':>10} {'roof':>8} {'k/ic':>6} {'k/roof':>6} {'again/k':>7} {'GB/s':>7}", flush=True)
    for kind in args.only.split(","):
        r = bench(kind, SHAPES[kind], args.calls, args.reps, dev)
        out.append(r)
        print(f"{kind:>6} {r['rows']:>5} {r['workgroups']:>5} |               {r['host_parent_us']:>9.1f} {r['host_new_us']:>9.1f} "
              f"{r['host_new_over_parent']:>10.3f} {r['host_parent_again_over_parent']:>12.3f} |                   "
              f"{r['device_kernel_us']:>8.2f} {r['device_index_copy_us']:>10.2f} {r['device_roof_us']:>8.2f} "
              f"{r['device_kernel_over_index_copy']:>6.2f} {r['device_kernel_over_roof']:>6.2f} {r['device_kernel_again_over_kernel']:>7.3f} "
              f"{r['device_kernel_GBps']:>7.1f}", flush=True)
        if args.json:                     # after every shape: a run that is cut short keeps what it measured
            with open(args.json, "w") as f:
                for x in out:
                    f.write(json.dumps(x) + "\n")


if __name__ == "__main__":
    main()

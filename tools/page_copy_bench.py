"""Copy-on-write for the paged KV cache on the MI355X: the page-copy kernel (``ops.page_copy`` / ``pfa_page_copy``), what its idle
launch costs a captured step, and ``PagedKVCache.fork`` against copying the history.

  a  the kernel alone, HIP-event time per launch, back to back: ``n_pairs`` whole pages of K and of V copied inside the pools (Hkv 8,
     D 128, bf16), against the torch ops that do the same, ``index_select`` + ``index_copy_`` on K and on V.  Every launch takes the
     next of ``sets`` disjoint pair lists, enough pages that a launch finds none of its lines in the 256 MiB Infinity Cache (at least
     1 GiB of pages in the cycle).  bytes = n_pairs x page_size x Hkv x D x 2 B x 2 pools, read once and written once; GB/s counts both.
  b  a captured serving step (``write_step`` + ``decode``, one token for each of B sequences) on a ``copy_on_write=True`` cache, whose
     graph holds one more launch -- ``page_copy`` over the empty pending table -- against the same step on a ``copy_on_write=False``
     cache, which enqueues exactly the launches of the commit before this feature.  HIP-event time per replay.
  c  one 8192-key sequence (and one of 8228 keys, whose tail page is partly filled) forked into 8 branches that append one token each:
     ``fork`` x 8 + ``append`` (the copy-on-write kernel moves the tail page where there is one) against ``gather`` + ``allocate`` +
     ``append`` of the history per branch + the same ``append``.  Host wall time of the whole operation, ended by a synchronise.
The paths of a comparison are timed alternately, ``--reps`` windows each; the median is reported with minimum and maximum in the JSON,
and the first path is timed twice (``*_again``): the ratio of its two medians is the spread a ratio has to clear.

    python tools/page_copy_bench.py [--reps 7] [--only a,b,c] [--json out.jsonl] [--dry]

``--dry`` prints part a's plan (pages, sets, bytes, workgroups) without a GPU.
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from photonic_flash_attention_amd import _capi, ops  # noqa: E402
from photonic_flash_attention_amd.integration.pytorch import PagedKVCache  # noqa: E402

BF, HKV, D, H = torch.bfloat16, 8, 128, 32
CYCLE_BYTES = 1 << 30                     # pages one cycle of pair lists touches, at least: four times the Infinity Cache


def _med(ts):
    return sorted(ts)[len(ts) // 2]


def _device_windows(paths, calls, reps):
    """-> {name: [us per call, ...]} from device events around `calls` back-to-back calls; window 0 warms up."""
    times = {name: [] for name in paths}
    for rep in range(reps + 1):
        for name, f in paths.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for n in range(calls):
                f(n)
            e1.record()
            e1.synchronize()
            if rep:
                times[name].append(e0.elapsed_time(e1) * 1e3 / calls)
    return times


def _host_windows(paths, reset, reps):
    """-> {name: [us, ...]}: wall time of one call, ended by a synchronise; `reset` runs untimed in front of each; window 0 warms up."""
    times = {name: [] for name in paths}
    for rep in range(reps + 1):
        for name, f in paths.items():
            reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            if rep:
                times[name].append((time.perf_counter() - t0) * 1e6)
    return times


def _report(res, group, times):
    for n, ts in times.items():
        res[f"{group}_{n}_us"] = round(_med(ts), 2)
        res[f"{group}_{n}_us_min"], res[f"{group}_{n}_us_max"] = round(min(ts), 2), round(max(ts), 2)


def plan_a(n_pairs, page):
    page_bytes = page * HKV * D * 2 * 2                       # K and V
    launch_bytes = 2 * n_pairs * page_bytes                   # read + written
    sets = max(1, -(-CYCLE_BYTES // (2 * n_pairs * page_bytes)))
    a = _capi.make_page_copy_args(k_pool=1 << 12, v_pool=1 << 12, pairs=1 << 12, pairs_stride=2, k_stride_b=page * HKV * D, k_stride_h=D,
                                  k_stride_s=HKV * D, v_stride_b=page * HKV * D, v_stride_h=D, v_stride_s=HKV * D, n_pairs=n_pairs, Hkv=HKV,
                                  D=D, page_size=page, num_pages=2 * n_pairs * sets, dtype=0)
    name, wgs = _capi.describe_page_copy(a)
    return dict(part="a", n_pairs=n_pairs, page=page, Hkv=HKV, D=D, sets=sets, num_pages=2 * n_pairs * sets, bytes=launch_bytes, kernel=name,
                workgroups=wgs)


def bench_a(n_pairs, page, reps, dev):
    res = plan_a(n_pairs, page)
    sets, num_pages = res["sets"], res["num_pages"]
    k = torch.randn(num_pages, page, HKV, D, device=dev, dtype=BF)
    v = torch.randn_like(k)
    perm = torch.randperm(num_pages, generator=torch.Generator().manual_seed(n_pairs + page)).view(sets, n_pairs, 2)
    pairs = perm.to(torch.int32).to(dev)                      # set j: pairs[j], disjoint pages, sources and destinations scattered
    src, dst = perm[:, :, 0].contiguous().to(dev), perm[:, :, 1].contiguous().to(dev)
    kp, vp = k.transpose(1, 2), v.transpose(1, 2)

    def kernel(n):
        ops.page_copy(kp, vp, pairs[n % sets])

    def torch_ops(n):
        j = n % sets
        k.index_copy_(0, dst[j], k.index_select(0, src[j]))
        v.index_copy_(0, dst[j], v.index_select(0, src[j]))

    kernel(0)
    torch.cuda.synchronize()
    s0, d0 = perm[0, 0].tolist()
    assert torch.equal(k[d0], k[s0]) and torch.equal(v[d0], v[s0])
    calls = max(sets, min(200, max(20, (8 << 30) // res["bytes"])))
    res["calls"] = calls
    _report(res, "device", _device_windows({"kernel": kernel, "torch": torch_ops, "kernel_again": kernel}, calls, reps))
    res["kernel_GBps"] = round(res["bytes"] / res["device_kernel_us"] / 1e3, 1)
    res["torch_GBps"] = round(res["bytes"] / res["device_torch_us"] / 1e3, 1)
    res["kernel_over_torch"] = round(res["device_kernel_us"] / res["device_torch_us"], 4)
    res["kernel_again_over_kernel"] = round(res["device_kernel_again_us"] / res["device_kernel_us"], 4)
    return res


def bench_b(B, keys, reps, dev):
    page = 64
    per = keys // page + 2
    steps = {}
    keep = []
    for cow in (False, True):
        c = PagedKVCache(num_pages=B * per, page_size=page, Hkv=HKV, D=D, dtype=BF, device=dev, max_batch=B, max_pages_per_seq=per,
                         copy_on_write=cow)
        c.k_pool.normal_()
        c.v_pool.normal_()
        for _ in range(B):
            c.allocate()
        c.advance(list(range(B)), [keys + 1] * B)             # the lengths after the step the graph holds
        k_s, v_s = torch.randn(B, HKV, D, device=dev, dtype=BF), torch.randn(B, HKV, D, device=dev, dtype=BF)
        q_s = torch.randn(B, H, 1, D, device=dev, dtype=BF)
        cu = torch.arange(B + 1, dtype=torch.int32, device=dev)

        def step(c=c, k_s=k_s, v_s=v_s, q_s=q_s, cu=cu):
            c.write_step(k_s, v_s, cu_seqlens_q=cu, max_seqlen_q=1)
            return c.decode(q_s)

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = step()
        keep.append((c, k_s, v_s, q_s, cu, out))
        steps["cow" if cow else "plain"] = lambda n, g=graph: g.replay()
    res = dict(part="b", B=B, keys=keys, H=H, Hkv=HKV, D=D, page=page, calls=200)
    _report(res, "device", _device_windows({"plain": steps["plain"], "cow": steps["cow"], "plain_again": steps["plain"]}, 200, reps))
    res["cow_minus_plain_us"] = round(res["device_cow_us"] - res["device_plain_us"], 2)
    res["plain_again_minus_plain_us"] = round(res["device_plain_again_us"] - res["device_plain_us"], 2)
    return res


def bench_c(keys, reps, dev):
    page, branches = 64, 8
    per = keys // page + 2
    c = PagedKVCache(num_pages=(branches + 1) * per, page_size=page, Hkv=HKV, D=D, dtype=BF, device=dev, max_batch=branches + 1,
                     max_pages_per_seq=per, copy_on_write=True)
    p = c.allocate()
    c.append(p, torch.randn(1, HKV, keys, D, device=dev, dtype=BF), torch.randn(1, HKV, keys, D, device=dev, dtype=BF))
    k1, v1 = torch.randn(branches, HKV, 1, D, device=dev, dtype=BF), torch.randn(branches, HKV, 1, D, device=dev, dtype=BF)
    kids = []

    def reset():
        for s in kids:
            c.free(s)
        del kids[:]

    def fork():
        kids.extend(c.fork(p) for _ in range(branches))
        c.append(kids, k1, v1)

    def copy():
        for _ in range(branches):
            k, v = c.gather(p)
            s = c.allocate()
            c.append(s, k[None], v[None])
            kids.append(s)
        c.append(kids, k1, v1)

    fork()
    mine = [c.gather(s) for s in kids]
    reset()
    copy()
    torch.cuda.synchronize()
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(mine, (c.gather(s) for s in kids)))
    res = dict(part="c", keys=keys, branches=branches, Hkv=HKV, D=D, page=page, tail_rows=keys % page)
    _report(res, "host", _host_windows({"fork": fork, "copy": copy, "fork_again": fork}, reset, reps))
    res["fork_over_copy"] = round(res["host_fork_us"] / res["host_copy_us"], 5)
    res["fork_again_over_fork"] = round(res["host_fork_again_us"] / res["host_fork_us"], 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", default="a,b,c")
    ap.add_argument("--json", default=None)
    ap.add_argument("--dry", action="store_true")
    args = ap.parse_args()
    shapes_a = [(n, page) for page in (64, 256, 1024) for n in (1, 8, 64, 512)]
    if args.dry:
        for n, page in shapes_a:
            print(json.dumps(plan_a(n, page)))
        return
    assert torch.cuda.is_available(), "page_copy_bench measures on the GPU"
    dev = torch.device("cuda:0")
    out = []

    def emit(r):
        out.append(r)
        print(json.dumps(r), flush=True)
        if args.json:                     # after every record: a run that is cut short keeps what it measured
            with open(args.json, "w") as f:
                for x in out:
                    f.write(json.dumps(x) + "\n")

    only = args.only.split(",")
    if "a" in only:
        for n, page in shapes_a:
            emit(bench_a(n, page, args.reps, dev))
    if "b" in only:
        for B, keys in ((32, 2048), (64, 4096)):
            emit(bench_b(B, keys, args.reps, dev))
    if "c" in only:
        for keys in (8192, 8228):
            emit(bench_c(keys, args.reps, dev))


if __name__ == "__main__":
    main()

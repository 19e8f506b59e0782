"""The rotary embedding fused into the KV-cache append on the MI355X: ``ops.rope_append`` (one HIP kernel that rotates Q and the new K
at positions derived on the device, and places K and V in the paged cache) against what a user does without it, and against the
traffic floor of the same bytes.

Per step shape (those of tools/kv_append_bench.py: B 64 x 1 token, one 2048-token chunk, a chunk of 512 plus 63 decode rows; H 32,
Hkv 8, D 128, rot_dim 128, bf16, pages of 64 keys), HIP-event time per step of three paths at one fixed cache state (every step
writes the same destinations), twice: ``eager``, a window of ``--calls`` steps enqueued back to back from Python -- what a caller
without graphs sees, the host's enqueue included -- and ``graph``, the same ``--calls`` steps captured once in a graph and
replayed, which is the device's time for the step:
  fused  (a) ``ops.rope_append`` with q: one launch;
  torch  (b) positions built on the device from cache_seqlens and cu_seqlens_q (``repeat_interleave`` with a fixed output size, so
         nothing synchronises), cos / sin rows gathered, Q and K rotated with torch ops in the ``rotate_half`` form in fp32 and
         rounded, then ``ops.kv_append`` of the rotated K;
  floor  (c) ``ops.kv_append`` plus a device copy of Q's bytes: what the same tensors cost to move without any arithmetic.
bytes = (H + 2 Hkv) x rows x D x 2 B, read once and written once, plus the gathered table rows.
The paths are timed alternately, ``--reps`` windows each; the median is reported with minimum and maximum in the JSON, and the
first path is timed twice (``fused_again``): the ratio of its two medians is the spread a ratio has to clear.  Each shape runs in a
process of its own under a time limit (``--limit`` seconds), and the run stops at the first shape that fails.

    python tools/rope_append_bench.py [--reps 5] [--calls 50] [--only decode,chunk,mixed] [--json out.jsonl]
"""

from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from photonic_flash_attention_amd import _capi, ops  # noqa: E402
from photonic_flash_attention_amd.integration.pytorch import PagedKVCache  # noqa: E402

BF, H, HKV, D, PAGE, MAX_POS = torch.bfloat16, 32, 8, 128, 64, 8192
SHAPES = {
    "decode": [1] * 64,                   # B 64 x 1 token
    "chunk": [2048],                      # one 2048-token chunk
    "mixed": [512] + [1] * 63,            # a chunk plus decode rows
}


def _med(ts):
    return sorted(ts)[len(ts) // 2]


def _device_windows(paths, calls, reps):
    """-> {name: [us per step, ...]} from device events around `calls` back-to-back steps."""
    times = {name: [] for name in paths}
    for rep in range(reps + 1):               # window 0 warms up
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


def _graph_windows(paths, calls, reps):
    """-> {name: [us per step, ...]}: `calls` steps of a path captured once in a graph, device events around one replay -- the
    device's time for the step, free of the host's enqueue."""
    graphs = {}
    for name, f in paths.items():
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(calls):
                f()
        graphs[name] = g
    return _device_windows({name: g.replay for name, g in graphs.items()}, 1, reps), calls


def _rotate_half(x):
    return torch.cat((-x[..., D // 2:], x[..., :D // 2]), dim=-1)


def bench(kind, q_lens, calls, reps, dev):
    B, total, max_q = len(q_lens), sum(q_lens), max(q_lens)
    prior = 1024                              # tokens each sequence holds before the step
    per_seq = -(-(prior + max_q) // PAGE)
    cache = PagedKVCache(num_pages=B * per_seq, page_size=PAGE, Hkv=HKV, D=D, dtype=BF, device=dev, max_batch=B, max_pages_per_seq=per_seq)
    slots = [cache.allocate() for _ in range(B)]
    cache.advance(slots, [prior + x for x in q_lens])
    q, k, v = (torch.randn(total, h, D, device=dev, dtype=BF) for h in (H, HKV, HKV))
    at = [0]
    for x in q_lens:
        at.append(at[-1] + x)
    cu = torch.tensor(at, dtype=torch.int32, device=dev)
    cos, sin = ops.rotary_tables(MAX_POS, D, device=dev)
    q_out, q_copy = torch.empty_like(q), torch.empty_like(q)
    lens, table = cache.cache_seqlens, cache.block_table
    kpool, vpool = cache.k_pool.transpose(1, 2), cache.v_pool.transpose(1, 2)
    seq_of_row = torch.repeat_interleave(torch.arange(B, device=dev), torch.tensor(q_lens, device=dev))   # host knowledge, built once

    def fused():
        ops.rope_append(k, v, kpool, vpool, cache_seqlens=lens, rotary_cos=cos, rotary_sin=sin, q=q, q_out=q_out, cu_seqlens_q=cu,
                        max_seqlen_q=max_q, block_table=table)

    def torch_ops():
        sq = cu[1:] - cu[:-1]
        pos = (lens - sq)[seq_of_row].long() + (torch.arange(total, device=dev) - cu[:-1].long()[seq_of_row])
        c = torch.cat((cos[pos], cos[pos]), -1)[:, None, :]
        s = torch.cat((sin[pos], sin[pos]), -1)[:, None, :]
        qf, kf = q.float(), k.float()
        q_out.copy_(qf * c + _rotate_half(qf) * s)
        k_rot = (kf * c + _rotate_half(kf) * s).to(BF)
        ops.kv_append(k_rot, v, kpool, vpool, cache_seqlens=lens, cu_seqlens_q=cu, max_seqlen_q=max_q, block_table=table)

    def floor():
        ops.kv_append(k, v, kpool, vpool, cache_seqlens=lens, cu_seqlens_q=cu, max_seqlen_q=max_q, block_table=table)
        q_copy.copy_(q)

    # the paths agree before anything is timed: (b) computes what (a) computes
    fused()
    want_q, want_k = q_out.clone(), cache.k_pool.clone()
    torch_ops()
    torch.cuda.synchronize()
    assert torch.equal(q_out, want_q) and torch.equal(cache.k_pool, want_k), "the torch-op path and the kernel disagree"

    a = _capi.make_rope_append_args(
        q=1 << 12, q_out=1 << 12, k_new=1 << 12, v_new=1 << 12, k_cache=1 << 12, v_cache=1 << 12, cos=1 << 12, sin=1 << 12, cu_seqlens_q=1 << 12,
        cache_seqlens=1 << 12, block_table=1 << 12, block_table_stride_b=per_seq, page_size=PAGE, num_pages=B * per_seq, B=B, H=H, Hkv=HKV,
        total_new=total, max_seqlen_q=max_q, Smax=per_seq * PAGE, D=D, rot_dim=D, max_pos=MAX_POS, cs_stride=D // 2,
        q_stride_s=H * D, q_stride_h=D, qo_stride_s=H * D, qo_stride_h=D, kn_stride_s=HKV * D, kn_stride_h=D, vn_stride_s=HKV * D, vn_stride_h=D,
        k_stride_b=PAGE * HKV * D, k_stride_s=HKV * D, k_stride_h=D, v_stride_b=PAGE * HKV * D, v_stride_s=HKV * D, v_stride_h=D)
    name, wgs = _capi.describe_rope_append(a)
    nbytes = 2 * (H + 2 * HKV) * total * D * 2 + 2 * total * (D // 2) * 4
    res = dict(kind=kind, B=B, H=H, Hkv=HKV, D=D, page=PAGE, q_lens=f"{q_lens[0]}" + (f"+{B - 1}x{q_lens[-1]}" if B > 1 else ""), rows=total,
               calls=calls, reps=reps, kernel=name, workgroups=wgs, bytes=nbytes)
    paths = {"fused": fused, "torch": torch_ops, "floor": floor, "fused_again": fused}
    eager = _device_windows(paths, calls, reps)
    replay, per = _graph_windows(paths, calls, reps)
    for group, times, div in (("eager", eager, 1), ("graph", replay, per)):
        for n, ts in times.items():
            ts = [t / div for t in ts]
            res[f"{group}_{n}_us"] = round(_med(ts), 2)
            res[f"{group}_{n}_us_min"], res[f"{group}_{n}_us_max"] = round(min(ts), 2), round(max(ts), 2)
        res[f"{group}_fused_over_torch"] = round(res[f"{group}_fused_us"] / res[f"{group}_torch_us"], 4)
        res[f"{group}_fused_over_floor"] = round(res[f"{group}_fused_us"] / res[f"{group}_floor_us"], 4)
        res[f"{group}_fused_again_over_fused"] = round(res[f"{group}_fused_again_us"] / res[f"{group}_fused_us"], 4)
    res["graph_fused_GBps"] = round(nbytes / res["graph_fused_us"] / 1e3, 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--only", default="decode,chunk,mixed")
    ap.add_argument("--json", default=None)
    ap.add_argument("--limit", type=int, default=120, help="seconds one shape's process may take")
    ap.add_argument("--one", default=None, help=argparse.SUPPRESS)      # the child: one shape, its JSON on the last line
    args = ap.parse_args()
    if args.one:
        assert torch.cuda.is_available(), "rope_append_bench measures on the GPU"
        print(json.dumps(bench(args.one, SHAPES[args.one], args.calls, args.reps, torch.device("cuda:0"))), flush=True)
        return
    out = []
    print(f"{'kind':>6} {'rows':>5} {'WGs':>6} {'':>5} | device us/step: {'fused':>8} {'torch':>9} {'floor':>8} {'f/torch':>8} {'f/floor':>8} "
          f"{'again/f':>7} {'GB/s':>7}", flush=True)
    for kind in args.only.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--one", kind, "--reps", str(args.reps), "--calls", str(args.calls)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)      # a fault or a hang ends the run here
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            sys.exit(f"{kind}: exit status {p.returncode}; nothing more is started")
        r = json.loads(p.stdout.strip().splitlines()[-1])
        out.append(r)
        for g in ("eager", "graph"):
            gbps = f"{r['graph_fused_GBps']:>7.1f}" if g == "graph" else f"{'':>7}"
            print(f"{kind:>6} {r['rows']:>5} {r['workgroups']:>6} {g:>5} |                 {r[g + '_fused_us']:>8.2f} {r[g + '_torch_us']:>9.2f} "
                  f"{r[g + '_floor_us']:>8.2f} {r[g + '_fused_over_torch']:>8.3f} {r[g + '_fused_over_floor']:>8.3f} "
                  f"{r[g + '_fused_again_over_fused']:>7.3f} {gbps}", flush=True)
        if args.json:                     # after every shape: a run that is cut short keeps what it measured
            with open(args.json, "w") as f:
                for x in out:
                    f.write(json.dumps(x) + "\n")


if __name__ == "__main__":
    main()

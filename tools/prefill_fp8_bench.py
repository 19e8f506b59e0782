"""Prefill over an FP8 (e4m3fn) KV cache on the MI355X: ``ops.fa3_prefill_cache`` with ``torch.float8_e4m3fn`` caches
(``pfa_fa3_prefill_q8``: bytes loaded into registers, converted, written into the LDS tile images) against the same call on
``cache.to(bf16)`` (``pfa_fa3_prefill_ex``: LDS-DMA straight into the images), in one process: a chunk of Sq new rows against
prefix + Sq cached keys, bottom-right causal, contiguous and paged (``[P,page,Hkv,D]`` pools of 256-key pages, random page order).

The 16-bit call is the yardstick: its kernels are, instruction for instruction, the ones of the commit before the FP8 prefill
(``tools/isa_same.py``).  Every path cycles through enough distinct caches (>= 768 MiB of FP8 K + V in all, so twice that in bf16) that
the 256 MiB Infinity Cache cannot serve them; the two paths are timed alternately with device events, ``--reps`` windows each, the
median reported with the minimum and maximum, and ``spread`` = max / min of the bf16 windows.  ratio = FP8 time / bf16 time.

    python tools/prefill_fp8_bench.py [--reps 5] [--quick] [--no-paged] [--out32] [--json out.jsonl]
    python tools/prefill_fp8_bench.py --shapes "B,H,Hkv,D,chunk,prefix;..."
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
PAGE = 256


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


def _pair(tag, res, t):
    med = {name: sorted(ts)[len(ts) // 2] for name, ts in t.items()}
    for name, ts in t.items():
        res[f"{tag}{name}_us"], res[f"{tag}{name}_us_min"], res[f"{tag}{name}_us_max"] = round(med[name], 2), round(min(ts), 2), round(max(ts), 2)
    res[f"{tag}ratio"] = round(med["fp8"] / med["bf16"], 4)
    res[f"{tag}bf16_spread"] = round(max(t["bf16"]) / min(t["bf16"]), 4)
    res[f"{tag}fp8_spread"] = round(max(t["fp8"]) / min(t["fp8"]), 4)


def _codes(shape, dev):
    """Random finite e4m3 codes of both signs (only the time is taken)."""
    x = torch.randint(0, 0x7f, shape, device=dev, dtype=torch.uint8)
    return (x | (torch.randint(0, 2, shape, device=dev, dtype=torch.uint8) << 7)).view(ops.FP8)


def bench_shape(B, H, Hkv, D, Sq, prefix, reps, dev, paged=True, out32=False):
    S = prefix + Sq                                     # keys in the cache when the chunk attends (its own included)
    bytes8 = 2 * B * Hkv * S * D
    if 2 * bytes8 > MAX_CACHE:
        return None
    n = max(1, math.ceil(MIN_POOL / bytes8))
    pairs = Sq * prefix + Sq * (Sq + 1) // 2            # visible (row, key) pairs per (batch, head)
    flops = 4.0 * D * pairs * B * H
    q = torch.randn(B, Sq, H, D, device=dev, dtype=BF).permute(0, 2, 1, 3)
    sl = torch.full((B,), S, dtype=torch.int32, device=dev)
    kd = torch.full((Hkv,), 1.0 / 64, device=dev)
    vd = torch.full((Hkv,), 1.0 / 32, device=dev)
    c8 = [(_codes((B, Hkv, S, D), dev), _codes((B, Hkv, S, D), dev)) for _ in range(n)]
    c16 = [(k.float().to(BF), v.float().to(BF)) for k, v in c8]
    a = _capi.make_decode_args(B=B, H=H, Hkv=Hkv, Sq=Sq, Smax=S, D=D, q=1 << 12, k_cache=1 << 12, v_cache=1 << 12, o=1 << 12,
                               q_stride_b=Sq * H * D, q_stride_h=D, q_stride_s=H * D, k_stride_b=Hkv * S * D, k_stride_h=S * D, k_stride_s=D,
                               v_stride_b=Hkv * S * D, v_stride_h=S * D, v_stride_s=D, o_stride_b=Sq * H * D, o_stride_h=D, o_stride_s=H * D,
                               dtype_in=0, dtype_out=2 if out32 else 0, causal=1, softmax_scale=D ** -0.5)
    name, wgs = _capi.describe_prefill_q8(a, None, _capi.make_kv_quant(k_descale=1 << 12, v_descale=1 << 12))
    res = dict(out="fp32" if out32 else "bf16", B=B, H=H, Hkv=Hkv, D=D, chunk=Sq, prefix=prefix, Skv=S, fp8_cache_MB=round(bytes8 / 1e6, 1), n_caches=n, reps=reps,
               kernel=name, workgroups=wgs, workgroups_per_cu=round(wgs / N_CU, 2), gflop=round(flops / 1e9, 2))
    scale = D ** -0.5 / 64                              # the bf16 call sees the undescaled values: the same logits
    okw = dict(out_dtype=torch.float32) if out32 else {}

    t = _timed({"bf16": lambda i: ops.fa3_prefill_cache(q, c16[i][0], c16[i][1], cache_seqlens=sl, softmax_scale=scale, **okw),
                "fp8": lambda i: ops.fa3_prefill_cache(q, c8[i][0], c8[i][1], cache_seqlens=sl, k_descale=kd, v_descale=vd, **okw)}, n, reps)
    _pair("", res, t)
    res["bf16_tflops"] = round(flops / res["bf16_us"] / 1e6, 1)
    res["fp8_tflops"] = round(flops / res["fp8_us"] / 1e6, 1)
    del c8, c16
    torch.cuda.empty_cache()
    if paged and S % PAGE == 0:
        pages = S // PAGE
        p8, p16, tabs = [], [], []
        for i in range(n):
            kp, vp = _codes((B * pages, PAGE, Hkv, D), dev), _codes((B * pages, PAGE, Hkv, D), dev)
            p8.append((kp.transpose(1, 2), vp.transpose(1, 2)))
            p16.append((kp.float().to(BF).transpose(1, 2), vp.float().to(BF).transpose(1, 2)))
            perm = torch.randperm(B * pages, generator=torch.Generator().manual_seed(i)).to(dev)
            tabs.append(perm.to(torch.int32).reshape(B, pages).contiguous())
        t = _timed({"bf16": lambda i: ops.fa3_prefill_cache(q, p16[i][0], p16[i][1], cache_seqlens=sl, block_table=tabs[i], softmax_scale=scale, **okw),
                    "fp8": lambda i: ops.fa3_prefill_cache(q, p8[i][0], p8[i][1], cache_seqlens=sl, block_table=tabs[i], k_descale=kd,
                                                           v_descale=vd, **okw)}, n, reps)
        _pair("paged_", res, t)
        del p8, p16
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="H 32 / Hkv 8, D 128, B 8, chunk 512 only")
    ap.add_argument("--no-paged", action="store_true")
    ap.add_argument("--out32", action="store_true", help="fp32 output (the SPLITP kernels) instead of the 16-bit output")
    ap.add_argument("--shapes", default=None, help='"B,H,Hkv,D,chunk,prefix;..." instead of the profiles/prefill_cache.md shapes')
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "prefill_fp8_bench measures on the GPU"
    dev = torch.device("cuda:0")
    if args.shapes:
        shapes = [tuple(int(x) for x in s.split(",")) for s in args.shapes.split(";") if s]
    elif args.quick:
        shapes = [(8, 32, 8, 128, 512, p) for p in (0, 8192, 32768)]
    else:
        shapes = [(B, H, Hkv, 128, c, p) for (H, Hkv) in ((32, 8), (32, 32)) for B in (1, 8) for c in (512, 2048) for p in (0, 8192, 32768)]
        shapes += [(8, 32, 8, 64, 512, p) for p in (0, 8192, 32768)]
    rows = []
    print(f"{'B':>2} {'H':>3} {'Hkv':>3} {'D':>4} {'chunk':>5} {'prefix':>6} {'WGs':>5} | {'bf16 us':>9} {'[min':>9} {'max]':>9} {'TF/s':>6} | "
          f"{'fp8 us':>9} {'[min':>9} {'max]':>9} {'TF/s':>6} | {'ratio':>6} {'bf16 spread':>11} | {'paged bf16':>10} {'paged fp8':>9} {'ratio':>6} "
          f"{'spread':>6}", flush=True)
    for B, H, Hkv, D, c, p in shapes:
        r = bench_shape(B, H, Hkv, D, c, p, args.reps, dev, paged=not args.no_paged, out32=args.out32)
        if r is None:
            print(f"{B:>2} {H:>3} {Hkv:>3} {D:>4} {c:>5} {p:>6}  skipped: one cache exceeds {MAX_CACHE >> 30} GiB", flush=True)
            continue
        rows.append(r)
        g = lambda key, fmt: format(r[key], fmt) if key in r else "-"      # noqa: E731
        print(f"{B:>2} {H:>3} {Hkv:>3} {D:>4} {c:>5} {p:>6} {r['workgroups']:>5} | {r['bf16_us']:>9.1f} {r['bf16_us_min']:>9.1f} {r['bf16_us_max']:>9.1f} "
              f"{r['bf16_tflops']:>6.1f} | {r['fp8_us']:>9.1f} {r['fp8_us_min']:>9.1f} {r['fp8_us_max']:>9.1f} {r['fp8_tflops']:>6.1f} | "
              f"{r['ratio']:>6.3f} {r['bf16_spread']:>11.3f} | {g('paged_bf16_us', '.1f'):>10} {g('paged_fp8_us', '.1f'):>9} "
              f"{g('paged_ratio', '.3f'):>6} {g('paged_bf16_spread', '.3f'):>6}", flush=True)
    if args.json:
        with open(args.json, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()

"""The decode over an FP8 (e4m3fn) KV cache against the bf16 call of the same build, and the quantising append against the 16-bit one.

    python tools/decode_fp8_bench.py [--reps 7] [--shapes "B,H,Hkv,D,Skv[;...]"] [--page 256] [--append] [--error] [--bf16-only] [--json out.jsonl]

Per shape four paths, timed alternately in one process with device events, each cycling through its own >= 768 MiB of distinct caches
(so the 256 MiB Infinity Cache cannot serve them; the FP8 paths hold twice as many caches): bf16 contiguous, FP8 contiguous, bf16
paged, FP8 paged (pools ``[num_pages, Hkv, page, D]`` in a seeded random page order).  One JSON line per shape: time, TB/s of K + V
cache bytes, and the FP8 / bf16 time ratio (the traffic bound is 0.5).  Sq 1, full lengths, descales per K/V head.

``--append``: ``ops.kv_append`` into an FP8 cache (``pfa_kv_append_q8``) against the same call into a bf16 cache, at the step shapes of
profiles/kv_append.md (B 64 x 1 token, one 2048-token chunk, 512 + 63 rows; Hkv 8, D 128, pages of 64 keys), kernel time from events.
``--error``: max-abs of the FP8 decode against the fp64 reference on the ORIGINAL bf16 cache, per-head absmax descales, one shape."""

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
MAX_BYTES = 24 << 30
SHAPES = "8,32,8,128,32768;8,32,8,128,131072;1,32,8,128,32768;32,32,32,128,4096"


def _median_us(paths, n_of, reps):
    """Each path's median time of one call, the paths taken in turn in every repetition; path(i) runs on its i-th cache."""
    for name, f in paths.items():
        for i in range(min(2, n_of[name])):
            f(i)
    torch.cuda.synchronize()
    times = {name: [] for name in paths}
    for _ in range(reps):
        for name, f in paths.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(n_of[name]):
                f(i)
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / n_of[name])
    return {name: sorted(ts)[len(ts) // 2] for name, ts in times.items()}


def bench_bf16_only(B, H, Hkv, D, S, reps, dev):
    """The bf16 contiguous call alone (``--bf16-only``): what two builds of the library are compared on, process against process."""
    bytes16 = 2 * B * Hkv * S * D * 2
    n = max(1, math.ceil(MIN_POOL / bytes16))
    q = torch.randn(B, H, 1, D, device=dev, dtype=torch.bfloat16)
    sl = torch.full((B,), S, dtype=torch.int32, device=dev)
    c16 = [(torch.randn(B, Hkv, S, D, device=dev, dtype=torch.bfloat16), torch.randn(B, Hkv, S, D, device=dev, dtype=torch.bfloat16))
           for _ in range(n)]
    us = _median_us({"bf16": lambda i: ops.fa3_decode(q, *c16[i], cache_seqlens=sl)}, {"bf16": n}, reps)
    return dict(B=B, H=H, Hkv=Hkv, D=D, Skv=S, bf16_us=round(us["bf16"], 2), bf16_TBs=round(bytes16 / us["bf16"] / 1e6, 3))


def bench_shape(B, H, Hkv, D, S, page, reps, dev):
    bytes16 = 2 * B * Hkv * S * D * 2
    n16 = max(1, math.ceil(MIN_POOL / bytes16))
    n8 = 2 * n16
    if 4 * n16 * bytes16 > MAX_BYTES or S % page:
        return None
    pages = S // page
    q = torch.randn(B, H, 1, D, device=dev, dtype=torch.bfloat16)
    sl = torch.full((B,), S, dtype=torch.int32, device=dev)
    kd = torch.full((Hkv,), 0.011, device=dev)
    vd = torch.full((Hkv,), 0.013, device=dev)

    def rand8(*shape):            # random bytes with the NaN codes (exponent and mantissa all ones) cleared
        return (torch.randint(0, 256, shape, device=dev, dtype=torch.uint8) & 0xf7).view(ops.FP8)

    c16 = [(torch.randn(B, Hkv, S, D, device=dev, dtype=torch.bfloat16), torch.randn(B, Hkv, S, D, device=dev, dtype=torch.bfloat16))
           for _ in range(n16)]
    c8 = [(rand8(B, Hkv, S, D), rand8(B, Hkv, S, D)) for _ in range(n8)]
    p16 = [(torch.randn(B * pages, Hkv, page, D, device=dev, dtype=torch.bfloat16), torch.randn(B * pages, Hkv, page, D, device=dev, dtype=torch.bfloat16))
           for _ in range(n16)]
    p8 = [(rand8(B * pages, Hkv, page, D), rand8(B * pages, Hkv, page, D)) for _ in range(n8)]
    tables = [torch.randperm(B * pages, generator=torch.Generator().manual_seed(i)).to(torch.int32).reshape(B, pages).to(dev) for i in range(n8)]
    paths = {
        "bf16": lambda i: ops.fa3_decode(q, *c16[i], cache_seqlens=sl),
        "fp8": lambda i: ops.fa3_decode(q, *c8[i], cache_seqlens=sl, k_descale=kd, v_descale=vd),
        "bf16_paged": lambda i: ops.fa3_decode(q, *p16[i], cache_seqlens=sl, block_table=tables[i]),
        "fp8_paged": lambda i: ops.fa3_decode(q, *p8[i], cache_seqlens=sl, block_table=tables[i], k_descale=kd, v_descale=vd),
    }
    us = _median_us(paths, {"bf16": n16, "fp8": n8, "bf16_paged": n16, "fp8_paged": n8}, reps)
    res = dict(B=B, H=H, Hkv=Hkv, D=D, Skv=S, page=page, n_caches_bf16=n16, n_caches_fp8=n8)
    for name, t in us.items():
        nbytes = bytes16 // 2 if name.startswith("fp8") else bytes16
        res[f"{name}_us"] = round(t, 2)
        res[f"{name}_TBs"] = round(nbytes / t / 1e6, 3)
    res["fp8_over_bf16"] = round(us["fp8"] / us["bf16"], 3)
    res["fp8_over_bf16_paged"] = round(us["fp8_paged"] / us["bf16_paged"], 3)
    return res


def bench_append(reps, dev):
    Hkv, D, page = 8, 128, 64
    out = []
    for name, lens in (("B 64 x 1 token", [1] * 64), ("one 2048-token chunk", [2048]), ("512 + 63 x 1", [512] + [1] * 63)):
        B, total, msq = len(lens), sum(lens), max(lens)
        pages = 4096 // page
        n = 8                                                                    # distinct pools, taken in turn
        cu = torch.tensor([sum(lens[:i]) for i in range(B + 1)], dtype=torch.int32, device=dev)
        after = torch.tensor([1000 + x for x in lens], dtype=torch.int32, device=dev)
        table = torch.randperm(B * pages, generator=torch.Generator().manual_seed(1)).to(torch.int32).reshape(B, pages).to(dev)
        kn, vn = (torch.randn(total, Hkv, D, device=dev, dtype=torch.bfloat16) for _ in range(2))
        kd, vd = torch.full((Hkv,), 0.011, device=dev), torch.full((Hkv,), 0.013, device=dev)
        pool16 = [tuple(torch.zeros(B * pages, page, Hkv, D, device=dev, dtype=torch.bfloat16).transpose(1, 2) for _ in range(2)) for _ in range(n)]
        pool8 = [tuple(torch.zeros(B * pages, page, Hkv, D, device=dev, dtype=torch.uint8).view(ops.FP8).transpose(1, 2) for _ in range(2)) for _ in range(n)]
        kw = dict(cache_seqlens=after, cu_seqlens_q=cu, max_seqlen_q=msq, block_table=table)
        us = _median_us({"bf16": lambda i: ops.kv_append(kn, vn, *pool16[i], **kw),
                         "fp8": lambda i: ops.kv_append(kn, vn, *pool8[i], k_descale=kd, v_descale=vd, **kw)}, {"bf16": n, "fp8": n}, reps)
        out.append(dict(step=name, rows=total, kv_append_us=round(us["bf16"], 2), kv_append_q8_us=round(us["fp8"], 2),
                        q8_over_16=round(us["fp8"] / us["bf16"], 3)))
    return out


def quantisation_error(dev):
    """max-abs of the FP8 decode against fp64 attention on the original bf16 cache: the whole quantisation error, for users."""
    B, H, Hkv, D, S = 2, 32, 8, 128, 4096
    g = torch.Generator(device=dev).manual_seed(3)
    q = torch.randn(B, H, 1, D, device=dev, generator=g).to(torch.bfloat16)
    k, v = (torch.randn(B, Hkv, S, D, device=dev, generator=g).to(torch.bfloat16) for _ in range(2))
    kd = (k.float().abs().amax(dim=(0, 2, 3)) / ops.FP8_MAX).contiguous()
    vd = (v.float().abs().amax(dim=(0, 2, 3)) / ops.FP8_MAX).contiguous()
    k8, v8 = ops.quantize_kv(k.cpu(), kd.cpu()).to(dev), ops.quantize_kv(v.cpu(), vd.cpu()).to(dev)
    o8, _ = ops.fa3_decode(q, k8, v8, k_descale=kd, v_descale=vd, out_dtype=torch.float32)
    o16, _ = ops.fa3_decode(q, k, v, out_dtype=torch.float32)
    s = (q.double() @ k.double().repeat_interleave(H // Hkv, 1).transpose(-1, -2)) * D ** -0.5
    ref = torch.softmax(s, -1) @ v.double().repeat_interleave(H // Hkv, 1)
    return dict(shape=[B, H, Hkv, D, S], fp8_max_abs=float((o8.double() - ref).abs().max()), bf16_max_abs=float((o16.double() - ref).abs().max()),
                ref_max_abs=float(ref.abs().max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--page", type=int, default=256)
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--error", action="store_true")
    ap.add_argument("--bf16-only", action="store_true", help="time the bf16 contiguous call alone (comparing two builds)")
    ap.add_argument("--json")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for spec in a.shapes.split(";"):
        if not spec:
            continue
        B, H, Hkv, D, S = (int(x) for x in spec.split(","))
        r = bench_bf16_only(B, H, Hkv, D, S, a.reps, dev) if a.bf16_only else bench_shape(B, H, Hkv, D, S, a.page, a.reps, dev)
        if r is not None:
            rows.append(r)
            print(json.dumps(r), flush=True)
        torch.cuda.empty_cache()
    if a.append:
        for r in bench_append(a.reps, dev):
            rows.append(r)
            print(json.dumps(r), flush=True)
    if a.error:
        r = quantisation_error(dev)
        rows.append(r)
        print(json.dumps(r), flush=True)
    if a.json:
        with open(a.json, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()

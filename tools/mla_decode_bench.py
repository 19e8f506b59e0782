"""MLA decode step over a latent KV cache on the MI355X: ``ops.mla_decode`` (bf16, Sq 1, H 16 and 128) against (a) ``ops.fa3_decode`` at
D 256 (H 16 / Hkv 4) on a cache of the same byte size -- the project's own HBM-bound yardstick -- and (b) the torch composition a user
has without the kernel: ``scaled_dot_product_attention`` of q against the latent rows as one K/V head, V their first 512 columns; and
(c) ``ops.mla_decode`` over the FP8 (e4m3fn) cache of the same keys, half the bytes.

Every path cycles through its own >= 768 MiB of caches (the 256 MiB Infinity Cache cannot serve them), the paths are timed alternately
in one process with device events, and the minimum and maximum over the repetitions are kept.  Rate = cache bytes / time.  The H 128 /
H 16 time ratio of ``mla_decode`` is the test of the block order: eight row blocks stream the same keys, 8 workgroup ids apart.

The append section times ``ops.mla_append`` (16-bit and quantising, one new row per sequence and a 2048-row chunk) against the torch
composition ``torch.cat`` + ``index_copy_`` into the same cache; bytes = rows read + rows written.

    python tools/mla_decode_bench.py [--reps 5] [--paths mla_decode,fp8] [--no-append] [--note TEXT] [--out profiles/mla_fp8.md]

--paths: only the paths whose name contains one of the comma-separated words (a library built with another PFA_MLA_KV8_SETS, or the
parent commit's library, is measured by a run of its own: PFA_HIP_LIB names the library)."""

from __future__ import annotations

import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from photonic_flash_attention_amd import ops  # noqa: E402

MIN_POOL = 768 << 20
SCALE = 192 ** -0.5
BF = torch.bfloat16
FP8 = torch.float8_e4m3fn


def _time(paths, pools, reps):
    """name -> (min, max) microseconds a call, the paths alternating; pools[name] is the list of argument tuples a path cycles through."""
    failed = {}
    for name, f in paths.items():
        try:
            for args in pools[name][:2]:
                f(*args)
        except (RuntimeError, ValueError) as e:                   # a path torch cannot run here is reported, not timed
            failed[name] = str(e).splitlines()[0][:80]
    paths = {name: f for name, f in paths.items() if name not in failed}
    torch.cuda.synchronize()
    times = {name: [] for name in paths}
    for _ in range(reps):
        for name, f in paths.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for args in pools[name]:
                f(*args)
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / len(pools[name]))
    return {**{name: (min(t), max(t)) for name, t in times.items()}, **{name: (None, why) for name, why in failed.items()}}


def _wanted(paths, words):
    return {n: f for n, f in paths.items() if not words or any(w in n for w in words)}


def bench_shape(B, S, reps, dev, words):
    nbytes = B * S * 576 * 2
    n = max(2, math.ceil(MIN_POOL / nbytes))
    lens = torch.full((B,), S, dtype=torch.int32, device=dev)
    desc = torch.full((B,), 0.37, dtype=torch.float32, device=dev)
    q16, q128 = (torch.randn(B, 1, h, 576, device=dev, dtype=BF).permute(0, 2, 1, 3) for h in (16, 128))
    q256 = torch.randn(B, 1, 16, 256, device=dev, dtype=BF).permute(0, 2, 1, 3)
    paths = _wanted({
        "mla_decode H 16": lambda kv: ops.mla_decode(q16, kv, cache_seqlens=lens, softmax_scale=SCALE),
        "mla_decode H 128": lambda kv: ops.mla_decode(q128, kv, cache_seqlens=lens, softmax_scale=SCALE),
        "mla_decode fp8 H 16": lambda kv: ops.mla_decode(q16, kv, cache_seqlens=lens, softmax_scale=SCALE, kv_descale=desc),
        "mla_decode fp8 H 128": lambda kv: ops.mla_decode(q128, kv, cache_seqlens=lens, softmax_scale=SCALE, kv_descale=desc),
        "fa3_decode D 256 (same bytes)": lambda k, v: ops.fa3_decode(q256, k, v),
        "torch sdpa H 16": lambda kv: torch.nn.functional.scaled_dot_product_attention(q16, kv[:, None], kv[:, None, :, :512], scale=SCALE,
                                                                                       enable_gqa=True),
        "torch sdpa H 128": lambda kv: torch.nn.functional.scaled_dot_product_attention(q128, kv[:, None], kv[:, None, :, :512], scale=SCALE,
                                                                                        enable_gqa=True),
    }, words)
    kinds = {name: "d256" if "fa3_decode" in name else "fp8" if "fp8" in name else "lat" for name in paths}
    made = {}
    if "lat" in kinds.values():
        made["lat"] = [(torch.randn(B, S, 576, device=dev, dtype=BF),) for _ in range(n)]
    if "fp8" in kinds.values():                                   # the FP8 path cycles through the same number of BYTES: twice the caches
        made["fp8"] = [(torch.randint(0, 0x78, (B, S, 576), device=dev, dtype=torch.uint8).view(FP8),) for _ in range(2 * n)]
    if "d256" in kinds.values():
        S256 = nbytes // (2 * B * 4 * 256 * 2)                                     # K + V at Hkv 4, D 256: the same bytes
        made["d256"] = [tuple(torch.randn(B, 4, S256, 256, device=dev, dtype=BF) for _ in range(2)) for _ in range(n)]
    return nbytes, _time(paths, {name: made[kinds[name]] for name in paths}, reps)


def bench_append(B, Sq, reps, dev):
    """One step's append into [B, 4096, 576] caches: ``ops.mla_append`` (16-bit, FP8) against cat + index_copy_ -> rows of the table."""
    S, n = 4096, 8
    lens = torch.full((B,), 2048 + Sq, dtype=torch.int32, device=dev)
    desc = torch.full((B,), 0.37, dtype=torch.float32, device=dev)
    src = [torch.randn(B, Sq, 576, device=dev, dtype=BF) for _ in range(n)]
    c16 = [torch.zeros(B, S, 576, device=dev, dtype=BF) for _ in range(n)]
    c8 = [torch.zeros(B, S, 576, device=dev, dtype=torch.uint8).view(FP8) for _ in range(n)]
    flat = (torch.arange(B, device=dev)[:, None] * S + 2048 + torch.arange(Sq, device=dev)[None]).flatten()
    paths = {
        "mla_append 16-bit": lambda x, c, _: ops.mla_append(x[..., :512], x[..., 512:], c, cache_seqlens=lens),
        "mla_append fp8": lambda x, _, c: ops.mla_append(x[..., :512], x[..., 512:], c, cache_seqlens=lens, kv_descale=desc),
        "torch cat + index_copy_ 16-bit": lambda x, c, _: c.view(-1, 576).index_copy_(0, flat, torch.cat([x[..., :512], x[..., 512:]], -1).view(-1, 576)),
    }
    pool = list(zip(src, c16, c8))
    res = _time(paths, {name: pool for name in paths}, reps)
    rows = []
    for name, (lo, hi) in res.items():
        moved = B * Sq * 576 * (3 if "fp8" in name else 4)
        rows.append(f"| {B} | {Sq} | {name} | {lo:.1f} .. {hi:.1f} | {moved / lo / 1e3:.1f} |" if lo is not None
                    else f"| {B} | {Sq} | {name} | not measured: {hi} | |")
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--paths", default="")
    ap.add_argument("--no-append", action="store_true")
    ap.add_argument("--note", default="")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    words = [w for w in a.paths.split(",") if w]
    dev = torch.device("cuda:0")
    lines = ["# MLA decode: `ops.mla_decode`, 16-bit and FP8 cache, against the D 256 decode on the same bytes and the torch composition", "",
             f"bf16, Sq 1, every path over >= 768 MiB of distinct caches, alternating, {a.reps} repetitions (min .. max); "
             f"{torch.cuda.get_device_name(0)}.  cache MiB and TB/s count the 16-bit cache's bytes for the 16-bit paths and half of them "
             f"for the fp8 paths.{' ' + a.note if a.note else ''}", "",
             "| B | keys | cache MiB | path | us a call (min .. max) | TB/s (at min) |", "|---|---|---|---|---|---|"]
    for B in (1, 8, 32):
        for S in (8192, 32768):
            nbytes, res = bench_shape(B, S, a.reps, dev, words)
            first = len(lines)
            for name, (lo, hi) in res.items():
                nb = nbytes // 2 if "fp8" in name else nbytes
                if lo is None:
                    lines.append(f"| {B} | {S} | {nb / 2 ** 20:.0f} | {name} | not measured: {hi} | |")
                    continue
                lines.append(f"| {B} | {S} | {nb / 2 ** 20:.0f} | {name} | {lo:.1f} .. {hi:.1f} | {nb / lo / 1e6:.2f} |")
            for what, num, den in (("H 128 / H 16 time ratio of mla_decode", "mla_decode H 128", "mla_decode H 16"),
                                   ("fp8 / 16-bit time ratio, H 16", "mla_decode fp8 H 16", "mla_decode H 16"),
                                   ("fp8 / 16-bit time ratio, H 128", "mla_decode fp8 H 128", "mla_decode H 128")):
                if res.get(num, (None,))[0] and res.get(den, (None,))[0]:
                    lines.append(f"| {B} | {S} | | {what} | {res[num][0] / res[den][0]:.2f} | |")
            print("\n".join(lines[first:]), flush=True)
    if not a.no_append:
        lines += ["", "## `ops.mla_append` against `torch.cat` + `index_copy_`", "",
                  "Into [B, 4096, 576] caches at key 2048, 8 distinct source / cache sets, alternating; GB/s = (rows read + rows written) / time.", "",
                  "| B | rows a sequence | path | us a call (min .. max) | GB/s (at min) |", "|---|---|---|---|---|"]
        for B, Sq in ((32, 1), (128, 1), (4, 2048)):
            lines += bench_append(B, Sq, a.reps, dev)
        print("\n".join(lines[-12:]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

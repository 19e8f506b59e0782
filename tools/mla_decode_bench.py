"""MLA decode step over a latent KV cache on the MI355X: ``ops.mla_decode`` (bf16, Sq 1, H 16 and 128) against (a) ``ops.fa3_decode`` at
D 256 (H 16 / Hkv 4) on a cache of the same byte size -- the project's own HBM-bound yardstick -- and (b) the torch composition a user
has without the kernel: ``scaled_dot_product_attention`` of q against the latent rows as one K/V head, V their first 512 columns.

Every path cycles through its own >= 768 MiB of caches (the 256 MiB Infinity Cache cannot serve them), the paths are timed alternately
in one process with device events, and the minimum and maximum over the repetitions are kept.  Rate = cache bytes / time.  The H 128 /
H 16 time ratio of ``mla_decode`` is the test of the block order: eight row blocks stream the same keys, 8 workgroup ids apart.

    python tools/mla_decode_bench.py [--reps 5] [--out profiles/mla_decode.md]
"""

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


def bench_shape(B, S, reps, dev):
    nbytes = B * S * 576 * 2
    n = max(2, math.ceil(MIN_POOL / nbytes))
    lens = torch.full((B,), S, dtype=torch.int32, device=dev)
    lat = [(torch.randn(B, S, 576, device=dev, dtype=BF),) for _ in range(n)]
    S256 = nbytes // (2 * B * 4 * 256 * 2)                                     # K + V at Hkv 4, D 256: the same bytes
    kv256 = [tuple(torch.randn(B, 4, S256, 256, device=dev, dtype=BF) for _ in range(2)) for _ in range(n)]
    q16, q128 = (torch.randn(B, 1, h, 576, device=dev, dtype=BF).permute(0, 2, 1, 3) for h in (16, 128))
    q256 = torch.randn(B, 1, 16, 256, device=dev, dtype=BF).permute(0, 2, 1, 3)
    paths = {
        "mla_decode H 16": lambda kv: ops.mla_decode(q16, kv, cache_seqlens=lens, softmax_scale=SCALE),
        "mla_decode H 128": lambda kv: ops.mla_decode(q128, kv, cache_seqlens=lens, softmax_scale=SCALE),
        "fa3_decode D 256 (same bytes)": lambda k, v: ops.fa3_decode(q256, k, v),
        "torch sdpa H 16": lambda kv: torch.nn.functional.scaled_dot_product_attention(q16, kv[:, None], kv[:, None, :, :512], scale=SCALE,
                                                                                       enable_gqa=True),
        "torch sdpa H 128": lambda kv: torch.nn.functional.scaled_dot_product_attention(q128, kv[:, None], kv[:, None, :, :512], scale=SCALE,
                                                                                        enable_gqa=True),
    }
    pools = {name: (kv256 if "fa3_decode" in name else lat) for name in paths}
    return nbytes, _time(paths, pools, reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = ["# MLA decode: `ops.mla_decode` against the D 256 decode on the same bytes and the torch composition", "",
             f"bf16, Sq 1, every path over >= 768 MiB of distinct caches, alternating, {a.reps} repetitions (min .. max); "
             f"{torch.cuda.get_device_name(0)}.", "",
             "| B | keys | cache MiB | path | us a call (min .. max) | TB/s (at min) |", "|---|---|---|---|---|---|"]
    for B in (1, 8, 32):
        for S in (8192, 32768):
            nbytes, res = bench_shape(B, S, a.reps, dev)
            for name, (lo, hi) in res.items():
                if lo is None:
                    lines.append(f"| {B} | {S} | {nbytes / 2 ** 20:.0f} | {name} | not measured: {hi} | |")
                    continue
                lines.append(f"| {B} | {S} | {nbytes / 2 ** 20:.0f} | {name} | {lo:.1f} .. {hi:.1f} | {nbytes / lo / 1e6:.2f} |")
            ratio = res["mla_decode H 128"][0] / res["mla_decode H 16"][0]
            lines.append(f"| {B} | {S} | | H 128 / H 16 time ratio of mla_decode | {ratio:.2f} | |")
            print("\n".join(lines[-6:]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

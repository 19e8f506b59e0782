"""GPU tests of the decode at head dim 256 (``ops.fa3_decode`` -> ``pfa_fa3_decode_d256``; csrc/fa3_decode_d256_kernel.h).

The fp64 reference and the bounds -- per element for a 16-bit output, 1e-3 for an fp32 output, 2e-3 on the LSE with exact -inf rows --
are tests/kvcache_testlib.py's; the exact visibility probes are tests/probe_testlib.py's, driven as tests/test_hip_cache_probes.py drives
them.  The shapes are the smallest that reach every edge of this kernel: a wave tile is 16 keys, a round of the four waves 64, a split
boundary a multiple of 64, and with B * Hkv * row blocks <= 128 the plan cuts Smax 1024 into four splits (partials + combine) and leaves
Smax 128 one split (the direct epilogue).  Every case fails on a library without the kernel, where ``ops.fa3_decode`` raises at D 256."""

from __future__ import annotations

import pytest
import torch

from kvcache_testlib import both, capture, device, gen, guard, i32, problem, run_and_check, scatter, window_lo
from photonic_flash_attention_amd import _capi_decode_d256, ops
from probe_testlib import cache_visible, check_probe, count, expected, probe_v, stair, unseen_keys

pytestmark = pytest.mark.gpu

BF, FP, F32 = torch.bfloat16, torch.float16, torch.float32
D = 256
LENS = (0, 1, 15, 16, 17, 64, 65, 257, 1000, 1024)          # one ragged batch: empty, below / at / past a tile, a wave round, a split
HEADS = [(8, 2), (4, 4), (16, 1)]


def _splits(q, k, v, **kw):
    a = ops._cache_call_args("pfa_fa3_decode", q, k, v, True, None, None, None, None)[0]
    a.workspace, a.workspace_bytes = 0x1000, 1 << 40
    return _capi_decode_d256.describe_decode_d256(a, **kw)[2]


@pytest.mark.parametrize("Smax", [1024, 128])
@pytest.mark.parametrize("Sq", [1, 5, 64])
@pytest.mark.parametrize("H,Hkv", HEADS)
@pytest.mark.parametrize("dtype", [BF, FP], ids=["bf16", "fp16"])
def test_against_fp64_on_a_ragged_batch(dtype, H, Hkv, Sq, Smax):
    q, k, v = problem(len(LENS), H, Hkv, Sq, Smax, D, dtype, seed=H + Sq + Smax)
    if Sq < 64:
        assert _splits(q, k, v) == (4 if Smax == 1024 else 1)
    run_and_check(ops.fa3_decode, q, k, v, [min(n, Smax) for n in LENS], what=f"d256 H {H}/{Hkv} Sq {Sq} Smax {Smax}")


@pytest.mark.parametrize("kw", [dict(out_dtype=F32), dict(causal=False)], ids=["o32", "not-causal"])
@pytest.mark.parametrize("Smax", [1024, 128])
def test_fp32_output_and_no_causal_cut(Smax, kw):
    q, k, v = problem(len(LENS), 8, 2, 5, Smax, D, BF, seed=Smax + 1)
    run_and_check(ops.fa3_decode, q, k, v, [min(n, Smax) for n in LENS], what=f"d256 {kw}", **kw)


@pytest.mark.parametrize("Sq", [1, 5])
@pytest.mark.parametrize("W", [1, 16, 17, 100])
def test_window(W, Sq):
    q, k, v = problem(len(LENS), 8, 2, Sq, 1024, D, FP if W % 2 else BF, seed=W + Sq)
    run_and_check(ops.fa3_decode, q, k, v, list(LENS), window=W, what=f"d256 window {W} Sq {Sq}")     # NaN below floor64(lo_b)


def test_left_padding_key_mask_with_lengths():
    q, k, v = problem(3, 8, 2, 1, 1024, D, BF, seed=5)
    km = torch.ones(3, 1024, dtype=torch.bool, device=q.device)
    km[1, :300] = False           # left padding
    km[2, :250] = False
    km[0, 500:533] = False        # a hole
    run_and_check(ops.fa3_decode, q, k, v, [1024, 700, 300], key_mask=km, what="d256 key mask with lengths")
    km[0, 900:] = False           # a key mask alone: each length comes from the last visible key
    km[2] = False                 # ... and a batch whose mask hides everything
    run_and_check(ops.fa3_decode, q, k, v, None, key_mask=km, what="d256 key mask alone")


@pytest.mark.parametrize("W", [None, 100], ids=["plain", "window"])
@pytest.mark.parametrize("page,layout", [(64, "phsd"), (256, "phsd"), (64, "hpsd"), (256, "hpsd")])
def test_paged_equals_contiguous_bit_for_bit(page, layout, W):
    Sq, lens = 5, list(LENS)
    q, k, v = problem(len(lens), 8, 2, Sq, 1024, D, BF, seed=page)
    kn, vn = guard(k, v, lens, Sq, W)
    kp, vp, table = scatter(kn, vn, page, seed=page + 1, layout=layout, first=1, lo=window_lo(lens, Sq, W) if W else None)
    both(ops.fa3_decode, q, kn, vn, kp, vp, table, cache_seqlens=i32(lens), **({} if W is None else dict(window=W)))


def _probe_case(kind, lens, steps, Sq, W, dtype):
    """One probe, contiguous with an fp32 output and over pages of 64 keys with a 16-bit one.  ``probe_v`` is built for D 128; its other
    columns are zero, and so are the 128 more here."""
    B, H, Hkv, S, dev = len(lens), 8, 2, 1024, device()
    vis = cache_visible(B, H, Sq, S, lens, window=W)
    pr = count(B, H, Hkv, Sq, S, D, dtype) if kind == "count" else stair(B, H, Hkv, Sq, S, D, dtype, steps)
    v = torch.cat([probe_v(B, Hkv, S, 128, dtype, unseen_keys(vis, Hkv)), torch.zeros(B, Hkv, S, 128, dtype=dtype)], dim=-1)
    exp = expected(vis, v, pr["steps"])
    for page, odt in ((None, F32), (64, dtype)):
        kn, vn = guard(pr["k"].to(dev), v.to(dev), lens, Sq, W)
        table = None
        if page is not None:
            kn, vn, table = scatter(kn, vn, page, seed=page + Sq, first=1, lo=window_lo(lens, Sq, W) if W else None)
        o, lse = ops.fa3_decode(pr["q"].to(dev), kn, vn, cache_seqlens=i32(lens), block_table=table, softmax_scale=pr["scale"], out_dtype=odt,
                                return_lse=True, **({} if W is None else dict(window=W)))
        torch.cuda.synchronize()
        check_probe(o, lse, exp, odt, f"d256 {kind} window {W} page {page}", kind == "count")


EDGES = (15, 16, 17, 63, 64, 65)


@pytest.mark.parametrize("kind", ["count", "stair"])
@pytest.mark.parametrize("W", [None, 33], ids=["lengths", "window-edges"])
def test_probes_at_tile_and_round_edges(kind, W):
    """Lengths at 15 / 16 / 17 and 63 / 64 / 65 keys (and past a split), then a window whose lowest key lo_b sits there: the step on lo
    itself is seen by row 0 alone, the 12 on the key below it by nobody."""
    Sq = 3
    if W is None:
        lens = list(EDGES) + [256 + e for e in EDGES] + [1024, 2]
        steps = [{j: h for j, h in ((0, 3), (n - 1, 9), (n - Sq, 5), (n // 2, 11)) if 0 <= j < n} for n in lens]
    else:
        los = list(EDGES) + [640 + e for e in EDGES]
        lens = [lo + Sq + W - 1 for lo in los]
        steps = [{lo: 2, lo - 1: 12, n - 1: 9, lo + 1: 5} for lo, n in zip(los, lens)]
    _probe_case(kind, lens, steps, Sq, W, BF if kind == "count" else FP)


def test_two_runs_are_bit_equal():
    q, k, v = problem(2, 8, 2, 1, 4096, D, BF, seed=3)
    sl = i32([4096, 2500])
    o1, l1 = ops.fa3_decode(q, k, v, cache_seqlens=sl, return_lse=True)
    o2, l2 = ops.fa3_decode(q, k, v, cache_seqlens=sl, return_lse=True)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(o1).all()) and torch.equal(o1, o2) and torch.equal(l1, l2)


def test_a_captured_step_replays_after_lengths_table_and_cache_changed():
    lens = [1024, 300, 65]
    q, k, v = problem(3, 8, 2, 2, 1024, D, BF, seed=6)
    kp, vp, table = scatter(k, v, 64, seed=7)
    sl = i32(lens)
    step = lambda: ops.fa3_decode(q, kp, vp, cache_seqlens=sl, block_table=table, window=500, return_lse=True)     # noqa: E731
    graph, (o, lse) = capture(step)
    for n, new_lens in enumerate(([17, 1000, 640], [1024, 16, 257])):
        sl.copy_(i32(new_lens))
        k2, v2 = (torch.randn(k.shape, generator=gen(60 + n), device=q.device).to(k.dtype) for _ in range(2))
        kp2, vp2, table2 = scatter(k2, v2, 64, seed=70 + n)
        kp.copy_(kp2), vp.copy_(vp2), table.copy_(table2)
        graph.replay()
        torch.cuda.synchronize()
        oe, le = step()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(o).all()) and torch.equal(o, oe) and torch.equal(lse, le), f"replay {n}"
        run_and_check(lambda *a, **kw: (o, lse), q, k2, v2, new_lens, window=500, guarded=False, what=f"d256 replay {n}")


def test_append_with_rotary_equals_rope_append_then_the_plain_call():
    B, H, Hkv, Sq, Smax = 3, 8, 2, 2, 1024
    q, k, v = problem(B, H, Hkv, Sq, Smax, D, BF, seed=8)
    g = gen(9)
    k_new, v_new = (torch.randn(B, Sq, Hkv, D, generator=g, device=q.device).to(BF).permute(0, 2, 1, 3) for _ in range(2))
    cos, sin = ops.rotary_tables(Smax, 128, device=q.device)
    sl = i32([1024, 65, 16])
    k1, v1, k2, v2 = k.clone(), v.clone(), k.clone(), v.clone()
    o1, l1 = ops.fa3_decode(q, k1, v1, cache_seqlens=sl, k_new=k_new, v_new=v_new, rotary_cos=cos, rotary_sin=sin, return_lse=True)
    q_rot = ops.rope_append(k_new, v_new, k2, v2, cache_seqlens=sl, rotary_cos=cos, rotary_sin=sin, q=q)
    o2, l2 = ops.fa3_decode(q_rot, k2, v2, cache_seqlens=sl, return_lse=True)
    torch.cuda.synchronize()
    assert torch.equal(k1, k2) and torch.equal(v1, v2) and not torch.equal(k1, k)
    assert bool(torch.isfinite(o1).all()) and torch.equal(o1, o2) and torch.equal(l1, l2)

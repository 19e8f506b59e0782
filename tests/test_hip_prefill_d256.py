"""GPU tests of the forward over a KV cache at head dim 256 (``ops.fa3_prefill_cache`` / ``ops.fa3_prefill_varlen`` ->
``pfa_fa3_prefill_d256`` / ``pfa_fa3_prefill_varlen_d256``; csrc/fa3_prefill_d256_kernel.h).

The fp64 reference and the bounds -- per element for a 16-bit output, 1e-3 for an fp32 output, 2e-3 on the LSE with exact -inf rows --
are tests/kvcache_testlib.py's.  The shapes are the smallest that reach every edge of this kernel: a wave owns 32 query rows, a
workgroup 128, a K/V tile is 64 keys, and K runs one tile ahead of V, so one, two and three tiles are different prologues.  Every case
fails on a library without the kernel, where the ``ops`` calls raise at D 256."""

from __future__ import annotations

import pytest
import torch

from kvcache_testlib import both, capture, check_lse, check_out, gen, guard, i32, problem, reference, run_and_check, scatter, seq_rows, window_lo
from photonic_flash_attention_amd import ops
from photonic_flash_attention_amd.integration.pytorch.paged_cache import PagedKVCache

pytestmark = pytest.mark.gpu

BF, FP, F32 = torch.bfloat16, torch.float16, torch.float32
D, SMAX = 256, 640
SENTINEL = 7.0


def _lens(Sq):
    """One ragged batch: empty, one key, below / at / past a tile, fewer keys than rows, past two and four tiles, the capacity."""
    return [0, 1, 63, 64, 65, Sq - 1, 129, 257, 640]


@pytest.mark.parametrize("Sq", [1, 33, 128, 129, 300])
@pytest.mark.parametrize("H,Hkv", [(8, 2), (4, 4)])
@pytest.mark.parametrize("dtype", [BF, FP], ids=["bf16", "fp16"])
def test_against_fp64_on_a_ragged_batch(dtype, H, Hkv, Sq):
    q, k, v = problem(9, H, Hkv, Sq, SMAX, D, dtype, seed=H + Sq)
    run_and_check(ops.fa3_prefill_cache, q, k, v, _lens(Sq), what=f"d256 H {H}/{Hkv} Sq {Sq}")


@pytest.mark.parametrize("kw", [dict(out_dtype=F32), dict(causal=False)], ids=["o32", "not-causal"])
def test_fp32_output_and_no_causal_cut(kw):
    q, k, v = problem(9, 8, 2, 129, SMAX, D, BF, seed=11)
    run_and_check(ops.fa3_prefill_cache, q, k, v, _lens(129), what=f"d256 {kw}", **kw)


@pytest.mark.parametrize("W", [1, 64, 65, 200])
def test_window(W):
    q, k, v = problem(9, 8, 2, 129, SMAX, D, FP if W % 2 else BF, seed=W)
    run_and_check(ops.fa3_prefill_cache, q, k, v, _lens(129), window=W, what=f"d256 window {W}")     # NaN below floor64(lo_b)


def test_a_window_of_the_capacity_is_the_call_without_one():
    q, k, v = problem(9, 8, 2, 129, SMAX, D, BF, seed=12)
    kn, vn = guard(k, v, _lens(129))
    kw = dict(cache_seqlens=i32(_lens(129)), return_lse=True)
    o, lse = ops.fa3_prefill_cache(q, kn, vn, **kw)
    ow, lw = ops.fa3_prefill_cache(q, kn, vn, window=SMAX, **kw)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(o).all()) and torch.equal(o, ow) and torch.equal(lse, lw)


@pytest.mark.parametrize("W", [None, 100], ids=["plain", "window"])
@pytest.mark.parametrize("page,layout", [(64, "phsd"), (256, "phsd"), (64, "hpsd"), (256, "hpsd")])
def test_paged_equals_contiguous_bit_for_bit(page, layout, W):
    Sq, lens = 129, [0, 1, 63, 64, 65, 128, 129, 257, 768]
    q, k, v = problem(len(lens), 8, 2, Sq, 768, D, BF, seed=page)
    kn, vn = guard(k, v, lens, Sq, W)
    kp, vp, table = scatter(kn, vn, page, seed=page + 1, layout=layout, first=1, lo=window_lo(lens, Sq, W) if W else None)
    both(ops.fa3_prefill_cache, q, kn, vn, kp, vp, table, cache_seqlens=i32(lens), **({} if W is None else dict(window=W)))


Q_LENS, KV_LENS = [1, 32, 33, 128, 129, 300, 0], [640, 40, 33, 100, 129, 300, 64]      # sequence 3 holds fewer keys than it brings rows
CU = [0, 1, 33, 66, 194, 323, 623, 623]


@pytest.mark.parametrize("W", [None, 100], ids=["causal", "window"])
@pytest.mark.parametrize("max_q", [300, 256])
def test_ragged_equals_per_sequence_uniform_calls_and_fp64(max_q, W):
    """Rows past ``max_seqlen_q`` and the 17 spare rows behind ``cu[B]`` keep the sentinel; the first ``min(Sq_b, max_q)`` rows of a
    sequence are, bit for bit, the uniform call on them with the sequence's length."""
    total, H = 640, 8
    q, k, v = problem(7, H, 2, 1, SMAX, D, BF, seed=20)
    qp = torch.randn(total, H, D, generator=gen(21), device=q.device).to(BF)
    win = {} if W is None else dict(window=W)
    sqs = [min(n, max_q) for n in Q_LENS]
    kn, vn = guard(k, v, KV_LENS, sqs, W)
    out = torch.full((total, H, D), SENTINEL, dtype=BF, device=q.device)
    o, lse = ops.fa3_prefill_varlen(qp, kn, vn, cu_seqlens_q=i32(CU), max_seqlen_q=max_q, cache_seqlens=i32(KV_LENS), return_lse=True, out=out, **win)
    torch.cuda.synchronize()
    written = torch.zeros(total, dtype=torch.bool, device=q.device)
    for b, n in enumerate(sqs):
        if n == 0:
            continue
        cu = [CU[b], CU[b] + n]
        written[cu[0]:cu[1]] = True
        ou, lu = ops.fa3_prefill_cache(seq_rows(qp, cu, 0), kn[b:b + 1], vn[b:b + 1], cache_seqlens=i32(KV_LENS[b:b + 1]), return_lse=True, **win)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(ou).all()) and torch.equal(seq_rows(o, cu, 0), ou) and torch.equal(lse[None, :, cu[0]:cu[1]], lu), f"sequence {b}"
        ro, rl, pn = reference(seq_rows(qp, cu, 0), k[b:b + 1], v[b:b + 1], seqlens=i32(KV_LENS[b:b + 1]), window=W)
        check_out(ou, ro, pn, float(v.abs().max()), BF, f"sequence {b}")
        check_lse(ou, lu, rl, f"sequence {b}")
    assert bool((o[~written] == SENTINEL).all()) and int((~written).sum()) == total - sum(sqs)


def test_a_captured_paged_windowed_step_replays_after_lengths_table_and_cache_changed():
    Sq, lens = 129, [640, 300, 129]
    q, k, v = problem(3, 8, 2, Sq, SMAX, D, BF, seed=6)
    kp, vp, table = scatter(k, v, 64, seed=7)
    sl = i32(lens)
    step = lambda: ops.fa3_prefill_cache(q, kp, vp, cache_seqlens=sl, block_table=table, window=200, return_lse=True)     # noqa: E731
    graph, (o, lse) = capture(step)
    for n, new_lens in enumerate(([130, 640, 257], [640, 64, 500])):
        sl.copy_(i32(new_lens))
        k2, v2 = (torch.randn(k.shape, generator=gen(60 + n), device=q.device).to(k.dtype) for _ in range(2))
        kp2, vp2, table2 = scatter(k2, v2, 64, seed=70 + n)
        kp.copy_(kp2), vp.copy_(vp2), table.copy_(table2)
        graph.replay()
        torch.cuda.synchronize()
        oe, le = step()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(o).all()) and torch.equal(o, oe) and torch.equal(lse, le), f"replay {n}"
        run_and_check(lambda *a, **kw: (o, lse), q, k2, v2, new_lens, window=200, guarded=False, what=f"d256 replay {n}")


def test_two_runs_are_bit_equal():
    q, k, v = problem(2, 8, 2, 300, SMAX, D, BF, seed=3)
    sl = i32([640, 333])
    o1, l1 = ops.fa3_prefill_cache(q, k, v, cache_seqlens=sl, return_lse=True)
    o2, l2 = ops.fa3_prefill_cache(q, k, v, cache_seqlens=sl, return_lse=True)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(o1).all()) and torch.equal(o1, o2) and torch.equal(l1, l2)


def test_append_with_rotary_equals_rope_append_then_the_plain_call():
    B, H, Hkv, Sq = 3, 8, 2, 129
    q, k, v = problem(B, H, Hkv, Sq, SMAX, D, BF, seed=8)
    g = gen(9)
    k_new, v_new = (torch.randn(B, Sq, Hkv, D, generator=g, device=q.device).to(BF).permute(0, 2, 1, 3) for _ in range(2))
    cos, sin = ops.rotary_tables(SMAX, 128, device=q.device)
    sl = i32([640, 129, 300])
    k1, v1, k2, v2 = k.clone(), v.clone(), k.clone(), v.clone()
    o1, l1 = ops.fa3_prefill_cache(q, k1, v1, cache_seqlens=sl, k_new=k_new, v_new=v_new, rotary_cos=cos, rotary_sin=sin, return_lse=True)
    q_rot = ops.rope_append(k_new, v_new, k2, v2, cache_seqlens=sl, rotary_cos=cos, rotary_sin=sin, q=q)
    o2, l2 = ops.fa3_prefill_cache(q_rot, k2, v2, cache_seqlens=sl, return_lse=True)
    torch.cuda.synchronize()
    assert torch.equal(k1, k2) and torch.equal(v1, v2) and not torch.equal(k1, k)
    assert bool(torch.isfinite(o1).all()) and torch.equal(o1, o2) and torch.equal(l1, l2)


def test_paged_cache_prefill_is_the_ops_call_on_its_operands():
    H, Hkv, lens = 8, 2, [200, 129]
    cache = PagedKVCache(num_pages=12, page_size=64, Hkv=Hkv, D=D, dtype=BF, max_batch=2)
    g = gen(30)
    for n in lens:
        slot = cache.allocate(n)
        cache.append(slot, *(torch.randn(1, Hkv, n, D, generator=g, device=cache.device).to(BF) for _ in range(2)))
    q = torch.randn(2, 129, H, D, generator=g, device=cache.device).to(BF).permute(0, 2, 1, 3)
    o, lse = cache.prefill(q, return_lse=True)
    kp, vp, kw = cache.operands()
    oo, lo = ops.fa3_prefill_cache(q, kp, vp, return_lse=True, **kw)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(o).all()) and torch.equal(o, oo) and torch.equal(lse, lo)

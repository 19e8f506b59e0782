"""GPU tests of the forward over a KV cache (``ops.fa3_prefill_cache`` / ``pfa_fa3_prefill``, ``PagedKVCache.prefill``): any number
of query rows against a contiguous or paged cache, bottom-right causal per batch.

Every cache handed to the kernel holds NaN at and past each batch's length, and every pool page no table entry names is NaN, so a
read past ``len_b`` (the descriptor bound) or of a page that is not the sequence's shows as a non-finite output: every test asserts
that the outputs are finite.  The reference is fp64 attention with the bottom-right rule, computed on the device from the clean
tensors, and the bounds are its own (tests/kvcache_testlib.py).  Paged against contiguous needs no tolerance: ``torch.equal``.

Only in-range page ids and legal arguments ever reach the device; refusals are tested on the host (tests/test_prefill_host.py)."""

from __future__ import annotations

import pytest
import torch

from kvcache_testlib import (NAN, both, capture, check_against_cache, check_lse, check_out, device, gen, guard, i32, problem, reference,
                             run_and_check, scatter, share_prefix_pages)

pytestmark = pytest.mark.gpu


def _run_and_check(*a, **kw):
    """The kernel on the NaN-tailed caches against fp64 on the clean ones.  lens: list or None (then nothing is poisoned)."""
    from photonic_flash_attention_amd import ops
    return run_and_check(ops.fa3_prefill_cache, *a, **kw)


# --- against fp64 --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Sq", [1, 33, 65, 200, 257, 300])
@pytest.mark.parametrize("D", [64, 128])
def test_against_fp64(Sq, D):
    lens = [Sq + 1000, Sq + 17]
    for dtype in (torch.bfloat16, torch.float16):
        q, k, v = problem(2, 8, 2, Sq, 2048, D, dtype, seed=Sq + D)
        for causal in (True, False):
            ref = reference(q, k, v, seqlens=i32(lens), causal=causal)
            for out_dtype in (None, torch.float32):
                _run_and_check(q, k, v, lens, causal=causal, out_dtype=out_dtype, ref=ref)


@pytest.mark.parametrize("H,Hkv", [(4, 4), (16, 1)])
@pytest.mark.parametrize("Sq", [65, 300])
def test_head_groups_against_fp64(H, Hkv, Sq):
    lens = [Sq + 1000, Sq + 17]
    for dtype, D in ((torch.bfloat16, 128), (torch.float16, 64)):
        q, k, v = problem(2, H, Hkv, Sq, 2048, D, dtype, seed=H + Sq)
        _run_and_check(q, k, v, lens)
        _run_and_check(q, k, v, lens, causal=False, out_dtype=torch.float32)


# --- edges ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D", [64, 128])
def test_no_prefix_is_the_top_left_causal_forward(D):
    from photonic_flash_attention_amd import ops
    Sq = 300
    q, k, v = problem(2, 8, 2, Sq, 2048, D, torch.bfloat16, seed=40 + D)
    o, lse = _run_and_check(q, k, v, [Sq, Sq])
    ref = reference(q, k, v, seqlens=i32([Sq, Sq]))
    of, lf = ops.fa3_forward(q, k[:, :, :Sq], v[:, :, :Sq], causal=True, return_lse=True)
    torch.cuda.synchronize()
    check_out(of, ref[0], ref[2], float(v.abs().max()), q.dtype)            # the forward meets the bound itself ...
    check_out(o, of.double(), ref[2], float(v.abs().max()), q.dtype)        # ... and the two agree within it
    assert float((lse - lf).abs().max()) <= 2e-3


def test_length_below_the_row_count_leaves_the_leading_rows_zero():
    Sq = 300
    for D, dtype in ((128, torch.bfloat16), (64, torch.float16)):
        q, k, v = problem(2, 8, 2, Sq, 2048, D, dtype, seed=50 + D)
        for lens in ([Sq + 500, 100], [37, Sq + 1]):
            for out_dtype in (None, torch.float32):
                o, lse = _run_and_check(q, k, v, lens, out_dtype=out_dtype)
                b, n = (1, 100) if lens[1] == 100 else (0, 37)
                assert bool((o[b, :, :Sq - n] == 0).all()) and bool((lse[b, :, :Sq - n] == float("-inf")).all())
                assert bool(torch.isfinite(lse[b, :, Sq - n:]).all()) and bool(torch.isfinite(lse[1 - b]).all())
            _run_and_check(q, k, v, lens, causal=False)                   # without the causal cut every row sees the len_b keys


def test_zero_length():
    q, k, v = problem(2, 8, 2, 300, 2048, 128, torch.bfloat16, seed=60)
    for causal in (True, False):
        for out_dtype in (None, torch.float32):
            o, lse = _run_and_check(q, k, v, [0, 300 + 64], causal=causal, out_dtype=out_dtype)
            assert bool((o[0] == 0).all()) and bool((lse[0] == float("-inf")).all())
    o, lse = _run_and_check(q, k, v, [0, 0])
    assert bool((o == 0).all()) and bool((lse == float("-inf")).all())


@pytest.mark.parametrize("D", [64, 128])
def test_full_cache_and_no_lengths(D):
    Smax = 1024
    q, k, v = problem(2, 8, 2, 257, Smax, D, torch.bfloat16, seed=70 + D)
    for causal in (True, False):
        o1, l1 = _run_and_check(q, k, v, [Smax, Smax], causal=causal)            # len_b = Smax
        o2, l2 = _run_and_check(q, k, v, None, causal=causal)                     # cache_seqlens = None
        assert torch.equal(o1, o2) and torch.equal(l1, l2)


@pytest.mark.parametrize("page", [64, 256])
def test_lengths_next_to_tile_and_page_boundaries(page):
    from photonic_flash_attention_amd import ops
    Sq = 40
    q, k, v = problem(2, 8, 2, Sq, 2048, 128, torch.bfloat16, seed=80 + page)
    for lens in ([63, 65], [64, 127], [page - 1, page + 1], [4 * page - 1, 4 * page + 1], [4 * page, 2047]):
        sl = i32(lens)
        kn, vn = guard(k, v, lens)
        kp, vp, table = scatter(kn, vn, page, seed=page)
        for causal in (True, False):
            o, lse = _run_and_check(q, k, v, lens, causal=causal)
            op, lp = ops.fa3_prefill_cache(q, kp, vp, block_table=table, cache_seqlens=sl, causal=causal, return_lse=True)
            torch.cuda.synchronize()
            assert torch.equal(op, o) and torch.equal(lp, lse), lens


# --- paged == contiguous -------------------------------------------------------------------------------------------------------------

def _both(*a, **kw):
    from photonic_flash_attention_amd import ops
    return both(ops.fa3_prefill_cache, *a, **kw)


@pytest.mark.parametrize("page", [64, 128, 256, 1024])
@pytest.mark.parametrize("D", [64, 128])
def test_paged_equals_contiguous(page, D):
    Smax = max(2048, 3 * page)
    for dtype in (torch.bfloat16, torch.float16):
        for Sq in (65, 300):
            q, k, v = problem(2, 8, 2, Sq, Smax, D, dtype, seed=page + D + Sq)
            lens = [Sq + 1000, Sq + 17]
            kn, vn = guard(k, v, lens)
            kp, vp, table = scatter(kn, vn, page, seed=page + Sq)
            for causal in (True, False):
                for out_dtype in (None, torch.float32):
                    _both(q, kn, vn, kp, vp, table, cache_seqlens=i32(lens), causal=causal, out_dtype=out_dtype)
        kp, vp, table = scatter(k, v, page, seed=page)
        _both(q, k, v, kp, vp, table)                                  # no lengths: every page is read
    # the paged call against fp64 as well, so that the suite does not rest on the contiguous path alone
    o, lse = _both(q, kn, vn, *scatter(kn, vn, page, seed=1), cache_seqlens=i32(lens))
    ref = reference(q, k, v, seqlens=i32(lens))
    check_out(o, ref[0], ref[2], float(v.abs().max()), q.dtype)
    check_lse(o, lse, ref[1])


@pytest.mark.parametrize("layout", ["phsd", "hpsd", "slice"])
def test_pool_layouts(layout):
    q, k, v = problem(2, 8, 2, 300, 2048, 128, torch.bfloat16, seed=9)
    lens = [2048, 1111]
    kn, vn = guard(k, v, lens)
    kp, vp, table = scatter(kn, vn, 256, seed=3, layout=layout)
    assert kp.is_contiguous() == (layout == "hpsd")
    _both(q, kn, vn, kp, vp, table, cache_seqlens=i32(lens))


def test_two_sequences_sharing_prefix_pages():
    page, Sq = 128, 200
    q, k, v = problem(3, 8, 2, Sq, 2048, 128, torch.bfloat16, seed=10)
    k[1, :, :5 * page] = k[0, :, :5 * page]          # batches 0 and 1 have a common 640-key prefix
    v[1, :, :5 * page] = v[0, :, :5 * page]
    lens = [2048, 5 * page + Sq + 7, 900]            # batch 1: its 207-row suffix attends to the shared pages
    kn, vn = guard(k, v, lens)
    kp, vp, table = scatter(kn, vn, page, seed=4)
    share_prefix_pages(kp, vp, table, 0, 1, 5)       # ... held once: both tables name the same pages, the duplicate copies are gone
    o, lse = _both(q, kn, vn, kp, vp, table, cache_seqlens=i32(lens))
    ref = reference(q, k, v, seqlens=i32(lens))
    check_out(o, ref[0], ref[2], float(v.abs().max()), q.dtype)
    check_lse(o, lse, ref[1])


# --- views, determinism --------------------------------------------------------------------------------------------------------------

def test_strided_views_of_q_cache_and_out():
    from photonic_flash_attention_amd import ops
    dev = device()
    B, H, Hkv, Sq, Smax, D = 2, 8, 2, 200, 1024, 128
    g = gen(11)
    qkv = torch.randn(B, Sq, 3, H, D, generator=g, device=dev).to(torch.bfloat16)       # a fused projection
    q = qkv[:, :, 0].permute(0, 2, 1, 3)
    big_k = torch.randn(B, Hkv, Smax + 96, D, generator=g, device=dev).to(torch.bfloat16)
    big_v = torch.randn(B, Hkv, Smax + 96, D, generator=g, device=dev).to(torch.bfloat16)
    lens = [Sq + 700, Sq + 1]
    for b, n in enumerate(lens):                     # the tails stay NaN inside the larger buffer
        big_k[b, :, n:] = NAN
        big_v[b, :, n:] = NAN
    k, v = big_k[:, :, :Smax], big_v[:, :, :Smax]    # the first Smax positions of a larger preallocated cache
    assert not q.is_contiguous() and not k.is_contiguous()
    sl = i32(lens)
    ref = reference(q, torch.nan_to_num(k), torch.nan_to_num(v), seqlens=sl)
    vmax = float(torch.nan_to_num(v).abs().max())
    o, lse = ops.fa3_prefill_cache(q, k, v, cache_seqlens=sl, return_lse=True)
    torch.cuda.synchronize()
    check_out(o, ref[0], ref[2], vmax, q.dtype)
    check_lse(o, lse, ref[1])
    # out= given, with strides of its own: a slice of a wider [B, Sq, H, 2 D] buffer, untouched outside the slice
    wide = torch.full((B, Sq, H, 2 * D), 7.0, dtype=torch.bfloat16, device=dev)
    out = wide[..., D:].permute(0, 2, 1, 3)
    o2, _ = ops.fa3_prefill_cache(q, k, v, cache_seqlens=sl, out=out)
    torch.cuda.synchronize()
    assert o2.data_ptr() == out.data_ptr() and torch.equal(o2, o) and bool((wide[..., :D] == 7.0).all())
    # flash-attn style [B, Smax, Hkv, D] cache passed transposed
    kt, vt = k.transpose(1, 2).contiguous().transpose(1, 2), v.transpose(1, 2).contiguous().transpose(1, 2)
    o3, l3 = ops.fa3_prefill_cache(q, kt, vt, cache_seqlens=sl, return_lse=True)
    torch.cuda.synchronize()
    assert torch.equal(o3, o) and torch.equal(l3, lse)


def test_outputs_are_bitwise_reproducible():
    from photonic_flash_attention_amd import ops
    q, k, v = problem(2, 8, 2, 300, 2048, 128, torch.bfloat16, seed=12)
    lens = [2048, 1500]
    kn, vn = guard(k, v, lens)
    kp, vp, table = scatter(kn, vn, 64, seed=7)
    for out_dtype in (None, torch.float32):
        runs = [ops.fa3_prefill_cache(q, kp, vp, block_table=table, cache_seqlens=i32(lens), out_dtype=out_dtype, return_lse=True)
                for _ in range(2)]
        torch.cuda.synchronize()
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
        assert bool(torch.isfinite(runs[0][0]).all())


# --- graph capture over a PagedKVCache -----------------------------------------------------------------------------------------------

def test_graph_capture_replays_while_the_cache_grows_and_pages_move():
    from photonic_flash_attention_amd.integration.pytorch import PagedKVCache
    dev = device()
    H, Hkv, D, page, max_pages, Sq = 8, 2, 128, 64, 12, 100
    cache = PagedKVCache(num_pages=30, page_size=page, Hkv=Hkv, D=D, dtype=torch.bfloat16, device=dev, max_batch=2,
                         max_pages_per_seq=max_pages)
    cache.k_pool.fill_(NAN)                  # whatever is not appended stays NaN: unfilled page tails, unused pages
    cache.v_pool.fill_(NAN)
    g = gen(20)

    def tokens(n, rows=1):
        return (torch.randn(rows, Hkv, n, D, generator=g, device=dev).to(torch.bfloat16),
                torch.randn(rows, Hkv, n, D, generator=g, device=dev).to(torch.bfloat16))

    a, b = cache.allocate(), cache.allocate()
    cache.append(b, *tokens(250))            # b first, so the two sequences' pages interleave in the pool
    cache.append(a, *tokens(60))             # a holds fewer keys than the chunk has rows: its leading rows see nothing
    cache.append(b, *tokens(40))
    cache.reserve(a, 500)                    # pages a will grow into during the replays
    table_ptr, lens_ptr = cache.block_table.data_ptr(), cache.cache_seqlens.data_ptr()
    q = torch.randn(2, Sq, H, D, generator=g, device=dev).to(torch.bfloat16).permute(0, 2, 1, 3)
    graph, (o, lse) = capture(lambda: cache.prefill(q, return_lse=True))

    def replay_and_compare():
        graph.replay()
        torch.cuda.synchronize()
        check_against_cache(cache, q, o, lse, max_pages * page)

    replay_and_compare()
    assert bool((o[a, :, :Sq - 60] == 0).all())
    pages_a = cache.pages(a)
    cache.append(a, *tokens(Sq))             # 60 -> 160: a new chunk's keys, into pages reserved before the capture
    assert cache.pages(a) == pages_a and cache.length(a) == 160
    cache.swap_pages(b, 0, 2)                # b's pages move, data with them
    q.copy_(torch.randn(2, Sq, H, D, generator=g, device=dev).to(torch.bfloat16).permute(0, 2, 1, 3))
    replay_and_compare()
    cache.append([a, b], *tokens(Sq, rows=2))   # 160 -> 260, 290 -> 390 (pages assigned now)
    cache.swap_pages(b, 1, 4)
    cache.swap_pages(a, 0, 3)
    replay_and_compare()
    assert cache.block_table.data_ptr() == table_ptr and cache.cache_seqlens.data_ptr() == lens_ptr


# --- consistency with the decode kernel ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Sq", [1, 8, 64])
def test_prefill_and_decode_both_meet_the_fp64_bound(Sq):
    from photonic_flash_attention_amd import ops
    for D, dtype in ((128, torch.bfloat16), (64, torch.float16)):
        q, k, v = problem(2, 8, 2, Sq, 2048, D, dtype, seed=90 + Sq + D)
        lens = [Sq + 1000, Sq + 17]
        ref = reference(q, k, v, seqlens=i32(lens))
        for out_dtype in (None, torch.float32):
            for fn in (ops.fa3_prefill_cache, ops.fa3_decode):
                run_and_check(fn, q, k, v, lens, out_dtype=out_dtype, ref=ref)

"""GPU tests of the paged KV cache of the decode path (``ops.fa3_decode(..., block_table=...)``, ``PagedKVCache``).

The central check needs no tolerance: a paged call returns the same bits as the contiguous call on the gathered cache -- the
arithmetic and its order are identical, only addresses differ.  Every case builds a contiguous ``[B, Hkv, Smax, D]`` cache,
scatters it into a pool in a seeded random page order with unused pages in between (filled with NaN, so a read of a page no
table entry names shows), runs both calls and asserts ``torch.equal`` on O and on the LSE.  One anchor against the fp64 reference
of tests/kvcache_testlib.py, within its bounds, keeps the suite from resting on the contiguous path alone.

Only in-range page ids are ever put into a table: the kernel's clamp is reviewed in the code, not provoked on the device."""

from __future__ import annotations

import pytest
import torch

from kvcache_testlib import both, capture, contiguous_of, device, gen, problem, reference, run_and_check, scatter, share_prefix_pages

pytestmark = pytest.mark.gpu


def _both(*a, **kw):
    from photonic_flash_attention_amd import ops
    return both(ops.fa3_decode, *a, **kw)


@pytest.mark.parametrize("page", [64, 128, 256, 1024])
@pytest.mark.parametrize("D", [64, 128])
def test_paged_equals_contiguous(page, D):
    Smax = max(2048, 3 * page)
    for dtype in (torch.bfloat16, torch.float16):
        for H, Hkv in ((32, 8), (8, 8), (64, 1)):
            _, k, v = problem(2, H, Hkv, 1, Smax, D, dtype, seed=page + D + H)
            kp, vp, table = scatter(k, v, page, seed=page + H)
            sl = torch.tensor([Smax, Smax // 2 + 17], dtype=torch.int32, device=k.device)
            for Sq in (1, 4, 8):
                q = torch.randn(2, Sq, H, D, generator=gen(Sq), device=k.device).to(dtype).permute(0, 2, 1, 3)
                for causal in ((True, False) if Sq > 1 else (True,)):
                    for out_dtype in (None, torch.float32):
                        _both(q, k, v, kp, vp, table, cache_seqlens=sl, causal=causal, out_dtype=out_dtype)
            _both(q, k, v, kp, vp, table)                                      # no lengths: every page is read


@pytest.mark.parametrize("page", [64, 256, 1024])
def test_ragged_lengths(page):
    Smax = 4 * page
    q, k, v = problem(7, 32, 8, 1, Smax, 128, torch.bfloat16, seed=page)
    kp, vp, table = scatter(k, v, page, seed=1)
    sl = torch.tensor([0, 1, page, page + 1, Smax, 2 * page - 1, 63], dtype=torch.int32, device=q.device)
    o, lse = _both(q, k, v, kp, vp, table, cache_seqlens=sl)
    assert bool((o[0] == 0).all()) and bool(torch.isinf(lse[0]).all())
    _both(q, k, v, kp, vp, table, cache_seqlens=sl, out_dtype=torch.float32)
    # bottom-right causal with rows that see nothing: lengths below Sq - 1
    q4, _, _ = problem(7, 32, 8, 4, Smax, 128, torch.bfloat16, seed=page + 1)
    sl4 = torch.tensor([0, 2, 3, page + 1, Smax, 1, page], dtype=torch.int32, device=q.device)
    o, lse = _both(q4, k, v, kp, vp, table, cache_seqlens=sl4, causal=True)
    assert bool(torch.isinf(lse[1, :, 0]).all()) and bool((o[1, :, 0] == 0).all())      # len 2, Sq 4: row 0 sees key j <= -2
    assert bool(torch.isfinite(lse[1, :, 3]).all())
    _both(q4, k, v, kp, vp, table, cache_seqlens=sl4, causal=False)


@pytest.mark.parametrize("page", [64, 256])
def test_key_mask_left_padding_and_a_hole(page):
    B, Smax = 3, 2048
    q, k, v = problem(B, 32, 8, 1, Smax, 128, torch.bfloat16, seed=5)
    kp, vp, table = scatter(k, v, page, seed=2)
    dev = q.device
    sl = torch.tensor([2048, 1500, 700], dtype=torch.int32, device=dev)
    km = torch.ones(B, Smax, dtype=torch.bool, device=dev)
    km[1, :300] = False           # left padding
    km[2, :650] = False
    km[0, 1000:1100] = False      # a hole
    _both(q, k, v, kp, vp, table, cache_seqlens=sl, key_mask=km)
    # a key mask alone: each batch's length comes from its last visible key
    km2 = km.clone()
    km2[0, 1800:] = False
    _both(q, k, v, kp, vp, table, key_mask=km2)
    km2[2] = False                # a batch whose mask hides everything
    o, lse = _both(q, k, v, kp, vp, table, key_mask=km2)
    assert bool((o[2] == 0).all()) and bool(torch.isinf(lse[2]).all())


@pytest.mark.parametrize("layout", ["phsd", "hpsd", "slice"])
def test_pool_layouts(layout):
    q, k, v = problem(2, 32, 8, 4, 5120, 128, torch.bfloat16, seed=9)
    kp, vp, table = scatter(k, v, 256, seed=3, layout=layout)
    assert kp.is_contiguous() == (layout == "hpsd")
    sl = torch.tensor([5120, 2222], dtype=torch.int32, device=q.device)
    _both(q, k, v, kp, vp, table, cache_seqlens=sl)


def test_two_sequences_sharing_prefix_pages():
    page = 128
    q, k, v = problem(3, 32, 8, 1, 2048, 128, torch.bfloat16, seed=10)
    k[1, :, :5 * page] = k[0, :, :5 * page]          # batches 0 and 1 have a common 640-key prefix
    v[1, :, :5 * page] = v[0, :, :5 * page]
    kp, vp, table = scatter(k, v, page, seed=4)
    share_prefix_pages(kp, vp, table, 0, 1, 5)       # ... held once: both tables name the same pages, the duplicate copies are gone
    sl = torch.tensor([2048, 5 * page + 70, 900], dtype=torch.int32, device=q.device)
    _both(q, k, v, kp, vp, table, cache_seqlens=sl)


@pytest.mark.parametrize("dtype,D", [(torch.bfloat16, 128), (torch.float16, 64)])
def test_paged_against_the_fp64_reference(dtype, D):
    from photonic_flash_attention_amd import ops
    q, k, v = problem(3, 32, 8, 4, 4096, D, dtype, seed=11)
    kp, vp, table = scatter(k, v, 256, seed=5)
    sl = torch.tensor([4096, 1234, 3], dtype=torch.int32, device=q.device)
    km = torch.ones(3, 4096, dtype=torch.bool, device=q.device)
    km[0, :200] = False
    km[1, 500:600] = False
    ref = reference(q, k, v, seqlens=sl, key_mask=km)
    for out_dtype in (None, torch.float32):
        run_and_check(lambda q, kn, vn, **kw: ops.fa3_decode(q, kp, vp, block_table=table, **kw), q, k, v, sl, key_mask=km,
                      out_dtype=out_dtype, ref=ref, guarded=False, what=f"paged decode D {D}")


def test_table_entries_past_a_sequence_are_never_read():
    page = 128
    q, k, v = problem(4, 32, 8, 1, 2048, 128, torch.bfloat16, seed=12)
    kp, vp, table = scatter(k, v, page, seed=6)
    lens = [0, 1, 3 * page, 5 * page + 1]
    sl = torch.tensor(lens, dtype=torch.int32, device=q.device)
    _both(q, k, v, kp, vp, table, cache_seqlens=sl)
    used = set(table.flatten().tolist())
    nan_page = next(p for p in range(kp.shape[0]) if p not in used)          # a valid page of the pool, full of NaN
    assert bool(torch.isnan(kp[nan_page]).all()) and bool(torch.isnan(vp[nan_page]).all())
    t2 = table.clone()
    for b, n in enumerate(lens):
        t2[b, -(-n // page):] = nan_page
    from photonic_flash_attention_amd import ops
    for out_dtype in (None, torch.float32):
        ref, rl = ops.fa3_decode(q, kp, vp, block_table=table, cache_seqlens=sl, out_dtype=out_dtype, return_lse=True)
        o, lse = ops.fa3_decode(q, kp, vp, block_table=t2, cache_seqlens=sl, out_dtype=out_dtype, return_lse=True)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(o).all())
        assert torch.equal(o, ref) and torch.equal(lse, rl)
    # with Sq 4, causal: still nothing past ceil(len / page)
    q4, _, _ = problem(4, 32, 8, 4, 2048, 128, torch.bfloat16, seed=13)
    ref, rl = ops.fa3_decode(q4, k, v, cache_seqlens=sl, return_lse=True)
    o, lse = ops.fa3_decode(q4, kp, vp, block_table=t2, cache_seqlens=sl, return_lse=True)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(o).all()) and torch.equal(o, ref) and torch.equal(lse, rl)


def test_paged_outputs_are_bitwise_reproducible():
    from photonic_flash_attention_amd import ops
    q, k, v = problem(2, 32, 8, 1, 32768, 128, torch.bfloat16, seed=3)
    kp, vp, table = scatter(k, v, 64, seed=7)
    sl = torch.tensor([32768, 20000], dtype=torch.int32, device=q.device)
    o1, l1 = ops.fa3_decode(q, kp, vp, block_table=table, cache_seqlens=sl, return_lse=True)
    o2, l2 = ops.fa3_decode(q, kp, vp, block_table=table, cache_seqlens=sl, return_lse=True)
    torch.cuda.synchronize()
    assert torch.equal(o1, o2) and torch.equal(l1, l2)
    _both(q, k, v, kp, vp, table, cache_seqlens=sl)


def test_graph_capture_replays_while_the_cache_grows_and_pages_move():
    from photonic_flash_attention_amd import ops
    from photonic_flash_attention_amd.integration.pytorch import PagedKVCache
    dev = device()
    H, Hkv, D, page, max_pages = 32, 8, 128, 64, 8
    cache = PagedKVCache(num_pages=24, page_size=page, Hkv=Hkv, D=D, dtype=torch.bfloat16, device=dev, max_batch=2,
                         max_pages_per_seq=max_pages)
    g = gen(20)

    def tokens(n, rows=1):
        return (torch.randn(rows, Hkv, n, D, generator=g, device=dev).to(torch.bfloat16),
                torch.randn(rows, Hkv, n, D, generator=g, device=dev).to(torch.bfloat16))

    a, b = cache.allocate(), cache.allocate()
    cache.append(b, *tokens(150))            # b first, so the two sequences' pages interleave in the pool
    cache.append(a, *tokens(60))
    cache.append(b, *tokens(40))
    cache.reserve(a, 200)                    # pages a will grow into during the replays
    table_ptr, lens_ptr = cache.block_table.data_ptr(), cache.cache_seqlens.data_ptr()
    q = torch.randn(2, 1, H, D, generator=g, device=dev).to(torch.bfloat16).permute(0, 2, 1, 3)
    graph, (o, lse) = capture(lambda: cache.decode(q, return_lse=True))

    def replay_and_compare():
        graph.replay()
        torch.cuda.synchronize()
        kc, vc = contiguous_of(cache, max_pages * page)
        ro, rl = ops.fa3_decode(q, kc, vc, cache_seqlens=cache.cache_seqlens.clone(), return_lse=True)
        torch.cuda.synchronize()
        assert torch.equal(o, ro) and torch.equal(lse, rl)

    replay_and_compare()
    pages_a = cache.pages(a)
    cache.append(a, *tokens(10))             # 60 -> 70: crosses into the page reserved before the capture
    assert cache.pages(a) == pages_a and cache.length(a) == 70
    cache.swap_pages(b, 0, 2)                # b's pages move, data with them
    q.copy_(torch.randn(2, 1, H, D, generator=g, device=dev).to(torch.bfloat16).permute(0, 2, 1, 3))
    replay_and_compare()
    cache.append([a, b], *tokens(70, rows=2))   # 70 -> 140 (two more reserved pages), 190 -> 260 (a page assigned now)
    cache.swap_pages(b, 1, 4)
    replay_and_compare()
    assert cache.block_table.data_ptr() == table_ptr and cache.cache_seqlens.data_ptr() == lens_ptr


def test_generation_loop_on_a_paged_cache_matches_a_contiguous_cache():
    from photonic_flash_attention_amd import ops
    from photonic_flash_attention_amd.integration.pytorch import PagedKVCache
    dev = device()
    H, Hkv, D, page, max_pages = 32, 8, 128, 64, 4
    Smax = page * max_pages
    cache = PagedKVCache(num_pages=10, page_size=page, Hkv=Hkv, D=D, dtype=torch.bfloat16, device=dev, max_batch=2,
                         max_pages_per_seq=max_pages)
    g = gen(30)
    kc = torch.zeros(2, Hkv, Smax, D, dtype=torch.bfloat16, device=dev)
    vc = torch.zeros_like(kc)
    lens = [100, 37]
    for s, n in enumerate(lens):
        assert cache.allocate() == s
        k = torch.randn(1, Hkv, n, D, generator=g, device=dev).to(torch.bfloat16)
        v = torch.randn(1, Hkv, n, D, generator=g, device=dev).to(torch.bfloat16)
        cache.append(s, k, v)
        kc[s, :, :n], vc[s, :, :n] = k[0], v[0]
    for step in range(40):
        k = torch.randn(2, Hkv, 1, D, generator=g, device=dev).to(torch.bfloat16)
        v = torch.randn(2, Hkv, 1, D, generator=g, device=dev).to(torch.bfloat16)
        q = torch.randn(2, 1, H, D, generator=g, device=dev).to(torch.bfloat16).permute(0, 2, 1, 3)
        cache.append([0, 1], k, v)
        for s in range(2):
            kc[s, :, lens[s]], vc[s, :, lens[s]] = k[s, :, 0], v[s, :, 0]
            lens[s] += 1
        sl = torch.tensor(lens, dtype=torch.int32, device=dev)
        op, lp = cache.decode(q, return_lse=True)
        oc, lc = ops.fa3_decode(q, kc, vc, cache_seqlens=sl, return_lse=True)
        torch.cuda.synchronize()
        assert torch.equal(cache.cache_seqlens, sl)
        assert torch.equal(op, oc) and torch.equal(lp, lc), f"step {step}"
        assert bool(torch.isfinite(op).all())
    assert len(cache.pages(0)) == 3 and len(cache.pages(1)) == 2      # 140 and 77 tokens: each crossed a page boundary

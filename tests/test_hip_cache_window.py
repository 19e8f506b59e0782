"""GPU tests of sliding-window attention over the KV cache: ``window=`` of ``ops.fa3_decode``, ``ops.fa3_prefill_cache`` and
``ops.fa3_prefill_varlen`` (``pfa_fa3_*_ex`` with a ``pfa_fa3_cache_ext``) and ``PagedKVCache.release_behind_window``.

The rule: with ``off_b = len_b - Sq_b``, row i of sequence b sees key j iff ``j < len_b``, ``j <= i + off_b`` and ``j > i + off_b - W``.
The reference is fp64 attention with that rule, ``reference(..., window=W)`` of tests/kvcache_testlib.py, within that module's bounds.

The read guarantee: with ``lo_b = max(0, off_b - W + 1)``, keys below ``lo_b`` rounded down to a multiple of 64 and block-table entries
below ``lo_b // page_size`` are never read.  Every kernel call here gets caches whose keys at and past ``len_b`` AND below that boundary
hold NaN (the reference reads clean copies); paged calls get -1 in the table entries below the boundary and NaN in every page no other
entry names, page 0 -- where a clamped -1 lands -- included.  Outputs must be finite.

``release_behind_window(slot, W)`` frees the pages below ``length - W + 1``, the bound of the NEXT rows the sequence appends.  A call that
is re-run on an unchanged cache with Sq rows reaches ``W + Sq - 1`` keys back from the end, so the test of released pages releases in two
steps: for ``W + Sq - 1`` before it repeats the 40-row prefill and the ragged step, then for ``W`` before it repeats the one-row decode.
Each repeat therefore runs with exactly the pages its own read guarantee leaves it."""

from __future__ import annotations

import functools

import pytest
import torch

from kvcache_testlib import (NAN, both, capture, check_lse, check_out, device, guard, i32, ragged_equals_uniform, reference, run_and_check,
                             scatter, seq_rows, window_lo)

pytestmark = pytest.mark.gpu

DT_D = [(torch.bfloat16, 128), (torch.float16, 64), (torch.bfloat16, 64), (torch.float16, 128)]
DT_IDS = ["bf16-d128", "fp16-d64", "bf16-d64", "fp16-d128"]


@functools.lru_cache(maxsize=None)
def _kv(B, Hkv, Smax, D, dtype, seed=0):
    """Clean caches [B,Hkv,Smax,D]; shared and never modified."""
    g = torch.Generator(device=device()).manual_seed(500 + 7 * D + seed + (0 if dtype is torch.bfloat16 else 1))
    k = torch.randn(B, Hkv, Smax, D, generator=g, device=device()).to(dtype)
    v = torch.randn(B, Hkv, Smax, D, generator=g, device=device()).to(dtype)
    return k, v


@functools.lru_cache(maxsize=None)
def _q(shape, dtype, seed=0):
    g = torch.Generator(device=device()).manual_seed(900 + seed + shape[-1])
    return torch.randn(*shape, generator=g, device=device()).to(dtype)


def _q4(B, H, Sq, D, dtype, seed=0):
    """[B,H,Sq,D] view of a [B,Sq,H,D] buffer, as a model hands it over."""
    return _q((B, Sq, H, D), dtype, seed).permute(0, 2, 1, 3)


LENS2 = [1000, 517]
WINDOWS_DECODE = [1, 63, 64, 65, 200, 512, 2000]


# --- 1. decode ---------------------------------------------------------------------------------------------------------------------

def _decode_and_check(dtype, D, H, Hkv, Sq, W, lens, Smax=1024, **kw):
    from photonic_flash_attention_amd import ops
    B = len(lens)
    k, v = _kv(B, Hkv, Smax, D, dtype)
    return run_and_check(ops.fa3_decode, _q4(B, H, Sq, D, dtype), k, v, lens, window=W, what=f"decode Sq {Sq} W {W}", **kw)


@pytest.mark.parametrize("dtype,D", DT_D, ids=DT_IDS)
def test_decode_window_against_fp64(dtype, D):
    # lengths 1000 and 517: windows inside a tile, on a tile edge, on a split edge (256-key splits) and larger than the cache; five
    # rows give five different lower bounds inside one item
    for Sq in (1, 5):
        for W in WINDOWS_DECODE:
            _decode_and_check(dtype, D, 8, 2, Sq, W, LENS2)


def test_decode_window_many_row_blocks_share_a_split_range():
    for W in (65, 200, 512):
        _decode_and_check(torch.bfloat16, 128, 64, 1, 5, W, LENS2)          # 320 rows of one K/V head: 20 row blocks
    _decode_and_check(torch.float16, 64, 64, 1, 5, 200, LENS2, out_dtype=torch.float32)


def test_decode_window_combined_with_a_left_padding_key_mask():
    Smax = 1024
    for pad, W in (([100, 0], 200), ([900, 500], 200), ([37, 460], 65)):      # the second: the window of batch 0 reaches into the padding
        km = torch.ones(2, Smax, dtype=torch.bool, device=device())
        for b, n in enumerate(pad):
            km[b, :n] = False
        for Sq in (1, 5):
            _decode_and_check(torch.bfloat16, 128, 8, 2, Sq, W, LENS2, key_mask=km)
    # a window that lies wholly inside the padding: no visible key, O = 0 and LSE = -inf
    km = torch.ones(2, Smax, dtype=torch.bool, device=device())
    km[0, :990] = False
    o, lse = _decode_and_check(torch.bfloat16, 128, 8, 2, 1, 5, [990, 517], key_mask=km)
    assert bool((o[0] == 0).all()) and bool((lse[0] == float("-inf")).all()) and bool(torch.isfinite(lse[1]).all())


# --- 2. prefill --------------------------------------------------------------------------------------------------------------------

WINDOWS_PREFILL = [1, 64, 100, 256, 257, 1000]


def _prefill_and_check(dtype, D, W, lens, Sq=300, Smax=768, **kw):
    from photonic_flash_attention_amd import ops
    B, H, Hkv = len(lens), 4, 2
    k, v = _kv(B, Hkv, Smax, D, dtype, seed=1)
    return run_and_check(ops.fa3_prefill_cache, _q4(B, H, Sq, D, dtype, seed=1), k, v, lens, window=W, what=f"prefill lens {lens} W {W}", **kw)


@pytest.mark.parametrize("dtype,D", DT_D, ids=DT_IDS)
def test_prefill_window_against_fp64(dtype, D):
    # Sq 300: two blocks, the second partial; 700 keys put 400 in front of the chunk, 300 keys none
    for W in WINDOWS_PREFILL:
        _prefill_and_check(dtype, D, W, [700, 300])


def test_prefill_window_fp32_output():
    for W in (100, 257):
        _prefill_and_check(torch.bfloat16, 128, W, [700, 300], out_dtype=torch.float32)


def test_prefill_window_rows_without_a_visible_key():
    for dtype, D in DT_D[:2]:
        for W in (1, 100, 1000):
            o, lse = _prefill_and_check(dtype, D, W, [120, 700])      # 120 keys for 300 rows: the first 180 rows see nothing
            assert bool((o[0, :, :180] == 0).all()) and bool((lse[0, :, :180] == float("-inf")).all())
            assert bool(torch.isfinite(lse[0, :, 180:]).all()) and bool(torch.isfinite(lse[1]).all())


# --- 3. ragged ---------------------------------------------------------------------------------------------------------------------

Q_LENS = [300, 1, 0, 17, 64]
KV_LENS = [700, 900, 0, 17, 333]
CU = [0, 300, 301, 301, 318, 382]
TOTAL, MAXQ, RB, RH, RHKV, RSMAX = 384, 300, 5, 4, 2, 1024


def _ragged(dtype, D, W, out_dtype=None):
    from photonic_flash_attention_amd import ops
    k, v = _kv(RB, RHKV, RSMAX, D, dtype, seed=2)
    q = _q((TOTAL, RH, D), dtype, seed=2)
    kn, vn = guard(k, v, KV_LENS, Q_LENS, W)
    o, lse = ops.fa3_prefill_varlen(q, kn, vn, cu_seqlens_q=i32(CU), max_seqlen_q=MAXQ, cache_seqlens=i32(KV_LENS), window=W,
                                    return_lse=True, out_dtype=out_dtype)
    torch.cuda.synchronize()
    return q, k, v, kn, vn, o, lse


@pytest.mark.parametrize("W", [64, 200])
@pytest.mark.parametrize("dtype,D", DT_D[:2], ids=DT_IDS[:2])
def test_ragged_window_against_fp64_and_per_sequence_calls(dtype, D, W):
    from photonic_flash_attention_amd import ops
    q, k, v, kn, vn, o, lse = _ragged(dtype, D, W)
    for b in range(RB):
        if Q_LENS[b] == 0:
            continue
        got, gl = seq_rows(o, CU, b), lse[None, :, CU[b]:CU[b + 1]]
        ref, rlse, pn = reference(seq_rows(q, CU, b), k[b:b + 1], v[b:b + 1], seqlens=i32(KV_LENS[b:b + 1]), window=W)
        check_out(got, ref, pn, float(v.abs().max()), dtype, f"ragged sequence {b} W {W}")
        check_lse(got, gl, rlse, f"ragged sequence {b} W {W}")
    ragged_equals_uniform(ops.fa3_prefill_cache, o, lse, q, kn, vn, CU, KV_LENS, window=W)


# --- 4. a window that hides nothing changes no bit --------------------------------------------------------------------------------------

def test_a_window_that_hides_nothing_changes_no_bit():
    from photonic_flash_attention_amd import ops
    for dtype, D in DT_D[:2]:
        for Sq, H, Hkv in ((1, 8, 2), (5, 8, 2), (5, 64, 1)):
            k, v = _kv(2, Hkv, 1024, D, dtype)
            q = _q4(2, H, Sq, D, dtype)
            kn, vn = guard(k, v, LENS2)
            a = ops.fa3_decode(q, kn, vn, cache_seqlens=i32(LENS2), return_lse=True)
            b = ops.fa3_decode(q, kn, vn, cache_seqlens=i32(LENS2), return_lse=True, window=1024 + Sq)
            torch.cuda.synchronize()
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), ("decode", D, Sq, H)
        k, v = _kv(2, 2, 768, D, dtype, seed=1)
        q = _q4(2, 4, 300, D, dtype, seed=1)
        for lens in ([700, 300], [120, 700]):
            kn, vn = guard(k, v, lens)
            for od in (None, torch.float32):
                a = ops.fa3_prefill_cache(q, kn, vn, cache_seqlens=i32(lens), return_lse=True, out_dtype=od)
                b = ops.fa3_prefill_cache(q, kn, vn, cache_seqlens=i32(lens), return_lse=True, out_dtype=od, window=768 + 300)
                torch.cuda.synchronize()
                assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), ("prefill", D, lens, od)
        plain = _ragged(dtype, D, None)
        wide = _ragged(dtype, D, RSMAX + MAXQ)
        assert torch.equal(plain[5][:CU[-1]], wide[5][:CU[-1]]) and torch.equal(plain[6][:, :CU[-1]], wide[6][:, :CU[-1]]), ("ragged", D)


# --- 5. paged == contiguous -----------------------------------------------------------------------------------------------------------

def _scatter(kn, vn, page, seed, lens, sqs, window):
    """Pools whose page 0 no table names (a clamped -1 lands there), with -1 in the entries below lo_b // page and NaN in their pages."""
    return scatter(kn, vn, page, seed, first=1, lo=window_lo(lens, sqs, window))


@pytest.mark.parametrize("page", [64, 128])
def test_paged_equals_contiguous_with_a_window(page):
    from photonic_flash_attention_amd import ops
    for dtype, D in DT_D[:2]:
        for W in (65, 200):
            # decode
            for Sq in (1, 5):
                k, v = _kv(2, 2, 1024, D, dtype)
                q = _q4(2, 8, Sq, D, dtype)
                kn, vn = guard(k, v, LENS2, Sq, W)
                both(ops.fa3_decode, q, kn, vn, *_scatter(kn, vn, page, page + D + Sq, LENS2, Sq, W), cache_seqlens=i32(LENS2), window=W)
            # prefill
            k, v = _kv(2, 2, 768, D, dtype, seed=1)
            q = _q4(2, 4, 300, D, dtype, seed=1)
            lens = [700, 300]
            kn, vn = guard(k, v, lens, 300, W)
            both(ops.fa3_prefill_cache, q, kn, vn, *_scatter(kn, vn, page, page + D, lens, 300, W), cache_seqlens=i32(lens), window=W)
            # ragged
            q, _, _, kn, vn, o, lse = _ragged(dtype, D, W)
            kp, vp, table = _scatter(kn, vn, page, page + D + 1, KV_LENS, Q_LENS, W)
            op, lp = ops.fa3_prefill_varlen(q, kp, vp, cu_seqlens_q=i32(CU), max_seqlen_q=MAXQ, cache_seqlens=i32(KV_LENS), window=W,
                                            return_lse=True, block_table=table)
            torch.cuda.synchronize()
            assert bool(torch.isfinite(op[:CU[-1]]).all())
            assert torch.equal(op[:CU[-1]], o[:CU[-1]]) and torch.equal(lp[:, :CU[-1]], lse[:, :CU[-1]]), ("ragged", D, W)


# --- 6. released pages are never read -------------------------------------------------------------------------------------------------

def test_released_pages_are_never_read():
    from photonic_flash_attention_amd.integration.pytorch import PagedKVCache
    dev = device()
    Hq, Hkv, D, page, W, SQ = 8, 2, 128, 64, 128, 40
    cache = PagedKVCache(num_pages=24, page_size=page, Hkv=Hkv, D=D, dtype=torch.bfloat16, device=dev, max_batch=2, max_pages_per_seq=12)
    cache.k_pool.fill_(NAN)
    cache.v_pool.fill_(NAN)
    g = torch.Generator(device=dev).manual_seed(61)

    def tokens(n):
        return (torch.randn(1, Hkv, n, D, generator=g, device=dev).to(torch.bfloat16),
                torch.randn(1, Hkv, n, D, generator=g, device=dev).to(torch.bfloat16))

    slots = [cache.allocate(), cache.allocate()]
    assert slots == [0, 1]
    cache.append(0, *tokens(700))
    cache.append(1, *tokens(333))
    assert cache.pages(0)[0] == 0                                    # page 0 is slot 0's first: a clamped -1 would land on it
    for s in slots:                                                  # the 40 rows of the prefill, appended before it runs
        cache.append(s, *tokens(SQ))
    q1 = torch.randn(2, 1, Hq, D, generator=g, device=dev).to(torch.bfloat16).permute(0, 2, 1, 3)
    q40 = torch.randn(2, SQ, Hq, D, generator=g, device=dev).to(torch.bfloat16).permute(0, 2, 1, 3)
    qr = torch.randn(SQ + 1, Hq, D, generator=g, device=dev).to(torch.bfloat16)

    def prefill_and_ragged():
        r = [cache.prefill(q40, window=W, return_lse=True), cache.prefill_varlen(qr, [SQ, 1], window=W, return_lse=True)]
        torch.cuda.synchronize()
        return r

    def decode():
        r = cache.decode(q1, window=W, return_lse=True)
        torch.cuda.synchronize()
        return r

    def poison_free_pages():
        free = torch.tensor(cache._free_pages, dtype=torch.int64, device=dev)
        cache.k_pool[free] = NAN
        cache.v_pool[free] = NAN
        return set(cache._free_pages)

    before_p, before_d = prefill_and_ragged(), decode()
    for o, lse in before_p + [before_d]:
        assert bool(torch.isfinite(o).all()) and bool(torch.isfinite(lse).all())
    # against fp64 on the gathered caches, while they can still be gathered
    for s in slots:
        gk, gv = cache.gather(s)
        n = cache.length(s)
        for qq, (o, lse) in ((q40, before_p[0]), (q1, before_d)):
            ref, rlse, pn = reference(qq[s:s + 1], gk[None], gv[None], seqlens=i32([n]), window=W)
            check_out(o[s:s + 1], ref, pn, float(gv.abs().max()), torch.bfloat16, f"slot {s} Sq {qq.shape[2]}")
            check_lse(o[s:s + 1], lse[s:s + 1], rlse)

    # step 1: the 40-row calls reach W + 39 keys back
    n0 = [cache.release_behind_window(s, W + SQ - 1) for s in slots]
    assert n0 == [(740 - (W + SQ - 1) + 1) // page, (373 - (W + SQ - 1) + 1) // page] == [8, 3]
    assert 0 in poison_free_pages()
    assert cache.block_table[0, :8].tolist() == [-1] * 8 and cache.block_table[1, :3].tolist() == [-1] * 3
    after_p = prefill_and_ragged()
    for (o0, l0), (o1, l1) in zip(before_p, after_p):
        assert bool(torch.isfinite(o1).all()), "a released page was read"
        assert torch.equal(o0, o1) and torch.equal(l0, l1)
    # step 2: the one-row decode reaches W keys back
    n1 = [cache.release_behind_window(s, W) for s in slots]
    assert n1 == [(740 - W + 1) // page - 8, (373 - W + 1) // page - 3] == [1, 0]
    poison_free_pages()
    after_d = decode()
    assert bool(torch.isfinite(after_d[0]).all()), "a released page was read"
    assert torch.equal(before_d[0], after_d[0]) and torch.equal(before_d[1], after_d[1])
    # the sequences go on: one more token each, on fresh pages where needed, and the decode still meets fp64 on what is left
    kt, vt = tokens(1)
    tail = {}
    for s in slots:
        live_from = cache.pages(s).count(-1) * page
        pg = torch.tensor([p for p in cache.pages(s) if p >= 0], dtype=torch.int64, device=dev)
        tail[s] = (live_from, cache.k_pool[pg].reshape(-1, Hkv, D), cache.v_pool[pg].reshape(-1, Hkv, D))
    cache.append(0, kt, vt)
    cache.append(1, kt, vt)
    o, lse = decode()
    for s in slots:
        n = cache.length(s)
        live_from, kk, vv = tail[s]
        kfull = torch.zeros(1, Hkv, n, D, dtype=torch.bfloat16, device=dev)
        vfull = torch.zeros_like(kfull)
        kfull[0, :, live_from:n - 1] = kk[:n - 1 - live_from].permute(1, 0, 2)
        vfull[0, :, live_from:n - 1] = vv[:n - 1 - live_from].permute(1, 0, 2)
        kfull[0, :, n - 1] = kt[0, :, 0]
        vfull[0, :, n - 1] = vt[0, :, 0]
        ref, rlse, pn = reference(q1[s:s + 1], kfull, vfull, seqlens=i32([n]), window=W)
        check_out(o[s:s + 1], ref, pn, float(vfull.abs().max()), torch.bfloat16, f"slot {s} after release and append")
        check_lse(o[s:s + 1], lse[s:s + 1], rlse)


# --- 7. reproducibility and graphs ----------------------------------------------------------------------------------------------------

def test_windowed_outputs_are_bitwise_reproducible():
    from photonic_flash_attention_amd import _capi, ops
    dtype, D, W = torch.bfloat16, 128, 512
    k, v = _kv(2, 2, 1024, D, dtype)
    q = _q4(2, 8, 5, D, dtype)
    a = ops.fa3_decode(q, k, v, cache_seqlens=i32(LENS2), return_lse=True, window=W)
    b = ops.fa3_decode(q, k, v, cache_seqlens=i32(LENS2), return_lse=True, window=W)
    torch.cuda.synchronize()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    args = ops._cache_call_args("pfa_fa3_decode", q, k, v, True, None, None, None, None)[0]
    args.workspace, args.workspace_bytes = 0x1000, 1 << 40
    name, _, nsplit = _capi.describe_decode_ex(args, _capi.make_cache_ext(window=W))
    assert nsplit > 1 and name == "fa3_decode_bf16_d128_o16_win+combine"                 # several splits were merged
    k, v = _kv(2, 2, 768, D, dtype, seed=1)
    q = _q4(2, 4, 300, D, dtype, seed=1)
    a = ops.fa3_prefill_cache(q, k, v, cache_seqlens=i32([700, 300]), return_lse=True, window=100)
    b = ops.fa3_prefill_cache(q, k, v, cache_seqlens=i32([700, 300]), return_lse=True, window=100)
    torch.cuda.synchronize()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_graph_replays_of_windowed_decode_and_ragged_prefill():
    from photonic_flash_attention_amd import ops
    dtype, D, W = torch.bfloat16, 128, 200
    g = torch.Generator(device=device()).manual_seed(71)
    # decode
    k, v = (t.clone() for t in _kv(2, 2, 1024, D, dtype))
    q = _q4(2, 8, 5, D, dtype)
    lens = i32(LENS2)
    graph, (o, lse) = capture(lambda: ops.fa3_decode(q, k, v, cache_seqlens=lens, return_lse=True, window=W))
    for new in (None, [300, 1024], [5, 0]):
        if new is not None:
            lens.copy_(i32(new))
            k.copy_(torch.randn(k.shape, generator=g, device=k.device).to(dtype))
            v.copy_(torch.randn(v.shape, generator=g, device=v.device).to(dtype))
        graph.replay()
        torch.cuda.synchronize()
        oe, le = ops.fa3_decode(q, k, v, cache_seqlens=lens, return_lse=True, window=W)
        torch.cuda.synchronize()
        assert torch.equal(o, oe) and torch.equal(lse, le), new
        ref, rlse, pn = reference(q, k, v, seqlens=lens, window=W)
        check_out(o, ref, pn, float(v.abs().max()), dtype, f"graph decode {new}")
        check_lse(o, lse, rlse)
    # ragged prefill
    k, v = (t.clone() for t in _kv(RB, RHKV, RSMAX, D, dtype, seed=2))
    q = _q((TOTAL, RH, D), dtype, seed=2)
    cu, lens = i32(CU), i32(KV_LENS)
    out = torch.full((TOTAL, RH, D), 7.0, dtype=dtype, device=q.device)

    def call(o_):
        return ops.fa3_prefill_varlen(q, k, v, cu_seqlens_q=cu, max_seqlen_q=MAXQ, cache_seqlens=lens, return_lse=True, window=W, out=o_)

    graph, (o, lse) = capture(lambda: call(out))
    states = [(None, None), ([0, 64, 64, 364, 380, 384], [1024, 0, 300, 16, 77]), (CU, KV_LENS)]
    results = []
    for new_cu, new_lens in states:
        if new_cu is not None:
            cu.copy_(i32(new_cu))
            lens.copy_(i32(new_lens))
            k.copy_(torch.randn(k.shape, generator=g, device=k.device).to(dtype))
            v.copy_(torch.randn(v.shape, generator=g, device=v.device).to(dtype))
        rows = int(cu[-1])
        o.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        oe, le = call(torch.full_like(out, 7.0))
        torch.cuda.synchronize()
        assert bool(torch.isfinite(o).all())
        assert torch.equal(o, oe) and torch.equal(lse[:, :rows], le[:, :rows]), new_cu
        assert bool((o[rows:] == 7.0).all())
        results.append(o.clone())
        cl, cul = lens.tolist(), cu.tolist()
        for b in range(RB):
            if cul[b + 1] == cul[b]:
                continue
            ref, rlse, pn = reference(seq_rows(q, cul, b), k[b:b + 1], v[b:b + 1], seqlens=i32(cl[b:b + 1]), window=W)
            got = seq_rows(o, cul, b)
            check_out(got, ref, pn, float(v.abs().max()), dtype, f"graph ragged sequence {b}")
            check_lse(got, lse[None, :, cul[b]:cul[b + 1]], rlse)
    assert not torch.equal(results[0], results[1])

"""GPU tests of the ragged forward over a KV cache (``ops.fa3_prefill_varlen`` / ``pfa_fa3_prefill_varlen``,
``PagedKVCache.append_varlen`` / ``prefill_varlen``): sequences with different numbers of query rows, packed into one
``[total_q, H, D]`` tensor, in one launch.

One ragged fixture serves every test: B 5, H 4, Hkv 2, Smax 1024, ``q_lens = [1, 300, 0, 33, 257]`` against
``cache_seqlens = [777, 300, 512, 20, 1000]``, packed buffers of 640 rows (591 used, 49 spare behind ``cu[B]``), ``max_seqlen_q = 300``:
a one-row sequence, two multi-block sequences (one with a single row in its second block), an empty one, ``len_b == Sq_b``,
``len_b < Sq_b`` (the first 13 rows of sequence 3 see no key) and a neighbour on both sides of every sequence boundary.  Sequences 0
and 4 start with the same 256 keys, so that a paged layout can hold that prefix once.

Two oracles.  The ragged call must be ``torch.equal`` to ``ops.fa3_prefill_cache`` called per sequence (B = 1) on that sequence's
rows, cache and length: same Q clamp, same padding rows, same rescale points.  And, independently of the uniform kernel, it must
meet fp64 attention with the bottom-right rule within its bounds (the reference and the bounds of tests/kvcache_testlib.py).

Every cache tail at and past ``len_b`` and every pool page no table entry names holds NaN, and every packed output buffer holds a
sentinel before the call, so a read past a length, of a foreign page, or a write outside a sequence's rows shows.  Only legal
arguments and in-range device data ever reach the GPU; refusals are tested on the host (tests/test_prefill_varlen_host.py).

A sequence longer than ``max_seqlen_q`` is computed as the issue defines it: ``Sq_b = min(cu[b+1] - cu[b], max_seqlen_q)`` rows,
aligned ``off_b = len_b - Sq_b``; with that ``Sq_b`` the uniform call it must equal has Sq = 256 and length ``len_b - (Sq_b - 256)``."""

from __future__ import annotations

import ctypes as C
import functools

import pytest
import torch

from kvcache_testlib import (NAN, capture, check_lse, check_out, device, guard, i32, ragged_equals_uniform, reference, scatter, seq_rows,
                             share_prefix_pages)

pytestmark = pytest.mark.gpu

O_SENTINEL, LSE_SENTINEL = 7.0, 12345.0

B, H, HKV, SMAX, TOTAL, MAXQ = 5, 4, 2, 1024, 640, 300
Q_LENS = [1, 300, 0, 33, 257]
KV_LENS = [777, 300, 512, 20, 1000]
CU = [0, 1, 301, 301, 334, 591]
SHARED = 256                        # keys sequences 0 and 4 have in common

CASES = [(dt, D, causal, None) for dt in (torch.bfloat16, torch.float16) for D in (64, 128) for causal in (True, False)] \
    + [(torch.bfloat16, 128, True, torch.float32)]
IDS = [f"{'bf16' if dt is torch.bfloat16 else 'fp16'}-d{D}-{'causal' if c else 'full'}{'-o32' if od else ''}" for dt, D, c, od in CASES]


@functools.lru_cache(maxsize=None)
def _fixture(dtype, D):
    """-> (q packed [640,H,D], clean k, v [B,Hkv,Smax,D], NaN-tailed kn, vn); shared and never modified."""
    dev = device()
    g = torch.Generator(device=dev).manual_seed(1000 + D + (0 if dtype is torch.bfloat16 else 1))
    q = torch.randn(TOTAL, H, D, generator=g, device=dev).to(dtype)
    k = torch.randn(B, HKV, SMAX, D, generator=g, device=dev).to(dtype)
    v = torch.randn(B, HKV, SMAX, D, generator=g, device=dev).to(dtype)
    k[4, :, :SHARED] = k[0, :, :SHARED]
    v[4, :, :SHARED] = v[0, :, :SHARED]
    return (q, k, v) + guard(k, v, KV_LENS)


@functools.lru_cache(maxsize=None)
def _ragged(dtype, D, causal, out_dtype):
    """The ragged call on the fixture, into sentinel-filled buffers.  -> (o [640,H,D], lse [H,640])."""
    from photonic_flash_attention_amd import ops
    q, _, _, kn, vn = _fixture(dtype, D)
    out = torch.full((TOTAL, H, D), O_SENTINEL, dtype=out_dtype or dtype, device=q.device)
    o, lse = ops.fa3_prefill_varlen(q, kn, vn, cu_seqlens_q=i32(CU), max_seqlen_q=MAXQ, cache_seqlens=i32(KV_LENS), causal=causal,
                                    out_dtype=out_dtype, return_lse=True, out=out)
    torch.cuda.synchronize()
    assert o.data_ptr() == out.data_ptr() and o.shape == (TOTAL, H, D) and lse.shape == (H, TOTAL) and lse.dtype == torch.float32
    return o, lse


@functools.lru_cache(maxsize=None)
def _fp64(dtype, D, causal):
    """Per sequence with rows: the fp64 (o [1,H,Sq,D], lse [1,H,Sq], pnorm) on the clean caches."""
    q, k, v, _, _ = _fixture(dtype, D)
    return {b: reference(seq_rows(q, CU, b), k[b:b + 1], v[b:b + 1], seqlens=i32(KV_LENS[b:b + 1]), causal=causal)
            for b in range(B) if Q_LENS[b] > 0}


# --- the two oracles -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,D,causal,out_dtype", CASES, ids=IDS)
def test_ragged_call_equals_per_sequence_uniform_calls(dtype, D, causal, out_dtype):
    from photonic_flash_attention_amd import ops
    q, _, _, kn, vn = _fixture(dtype, D)
    o, lse = _ragged(dtype, D, causal, out_dtype)
    ragged_equals_uniform(ops.fa3_prefill_cache, o, lse, q, kn, vn, CU, KV_LENS, causal=causal, out_dtype=out_dtype)


@pytest.mark.parametrize("dtype,D,causal,out_dtype", CASES, ids=IDS)
def test_ragged_call_against_fp64(dtype, D, causal, out_dtype):
    _, _, v, _, _ = _fixture(dtype, D)
    o, lse = _ragged(dtype, D, causal, out_dtype)
    vmax = float(v.abs().max())
    for b, (ro, rl, pn) in _fp64(dtype, D, causal).items():
        got = seq_rows(o, CU, b)
        check_out(got, ro, pn, vmax, dtype)
        check_lse(got, lse[None, :, CU[b]:CU[b + 1]], rl)
    # sequence 3 holds 20 keys for 33 rows: under the causal rule its first 13 rows see nothing, without it every row sees the 20
    head_o, head_l = o[CU[3]:CU[3] + 13], lse[:, CU[3]:CU[3] + 13]
    if causal:
        assert bool((head_o == 0).all()) and bool((head_l == float("-inf")).all())
        assert bool(torch.isfinite(lse[:, CU[3] + 13:CU[4]]).all())
    else:
        assert bool(torch.isfinite(head_l).all()) and bool((head_o != 0).any())


# --- rows no sequence covers ---------------------------------------------------------------------------------------------------------

def _raw_call(q, kn, vn, cu, max_q, lens, out, lse, causal):
    """``pfa_fa3_prefill_varlen`` through ctypes, so that the LSE buffer too is the test's own (``ops`` allocates its LSE)."""
    from photonic_flash_attention_amd import _capi
    total, Hq, D = q.shape
    a = _capi.make_prefill_varlen_args(
        q=q.data_ptr(), k_cache=kn.data_ptr(), v_cache=vn.data_ptr(), o=out.data_ptr(), lse=lse.data_ptr(), cu_seqlens_q=cu.data_ptr(),
        cache_seqlens=lens.data_ptr(), q_stride_s=q.stride(0), q_stride_h=q.stride(1), o_stride_s=out.stride(0), o_stride_h=out.stride(1),
        k_stride_b=kn.stride(0), k_stride_h=kn.stride(1), k_stride_s=kn.stride(2), v_stride_b=vn.stride(0), v_stride_h=vn.stride(1),
        v_stride_s=vn.stride(2), B=cu.numel() - 1, H=Hq, Hkv=kn.shape[1], total_q=total, max_seqlen_q=max_q, Smax=kn.shape[2], D=D,
        dtype_in=0 if q.dtype is torch.bfloat16 else 1, dtype_out=2 if out.dtype is torch.float32 else (0 if q.dtype is torch.bfloat16 else 1),
        causal=1 if causal else 0, softmax_scale=D ** -0.5, device_id=0)
    _capi.check_status(_capi.load().pfa_fa3_prefill_varlen(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()


@pytest.mark.parametrize("out_dtype", [None, torch.float32], ids=["o16", "o32"])
def test_rows_behind_the_last_sequence_are_never_written(out_dtype):
    dtype, D = torch.bfloat16, 128
    q, _, _, kn, vn = _fixture(dtype, D)
    for causal in (True, False):
        out = torch.full((TOTAL, H, D), O_SENTINEL, dtype=out_dtype or dtype, device=q.device)
        lse = torch.full((H, TOTAL), LSE_SENTINEL, dtype=torch.float32, device=q.device)
        _raw_call(q, kn, vn, i32(CU), MAXQ, i32(KV_LENS), out, lse, causal)
        assert bool((out[CU[B]:] == O_SENTINEL).all()), "a spare row of O was written"
        assert bool((lse[:, CU[B]:] == LSE_SENTINEL).all()), "a spare LSE entry was written"
        o_ops, l_ops = _ragged(dtype, D, causal, out_dtype)                      # and the covered rows are the ops call's
        assert torch.equal(out[:CU[B]], o_ops[:CU[B]]) and torch.equal(lse[:, :CU[B]], l_ops[:, :CU[B]])
        assert bool((o_ops[CU[B]:] == O_SENTINEL).all())
        assert not bool((lse[:, :CU[B]] == LSE_SENTINEL).any())                 # every covered entry was written


def test_rows_past_max_seqlen_q_are_never_written_and_the_others_equal_the_uniform_call():
    from photonic_flash_attention_amd import ops
    dtype, D, cap = torch.bfloat16, 128, 256
    q, _, _, kn, vn = _fixture(dtype, D)
    for causal in (True, False):
        out = torch.full((TOTAL, H, D), O_SENTINEL, dtype=dtype, device=q.device)
        lse = torch.full((H, TOTAL), LSE_SENTINEL, dtype=torch.float32, device=q.device)
        _raw_call(q, kn, vn, i32(CU), cap, i32(KV_LENS), out, lse, causal)
        assert bool((out[CU[B]:] == O_SENTINEL).all()) and bool((lse[:, CU[B]:] == LSE_SENTINEL).all())
        o_full, l_full = _ragged(dtype, D, causal, None)
        for b in range(B):
            s, n = CU[b], Q_LENS[b]
            if n == 0:
                continue
            if n <= cap:                                                         # the short sequences are untouched by the cap
                assert torch.equal(out[s:s + n], o_full[s:s + n]) and torch.equal(lse[:, s:s + n], l_full[:, s:s + n])
                continue
            assert bool((out[s + cap:s + n] == O_SENTINEL).all()), f"sequence {b}: a row past max_seqlen_q was written"
            assert bool((lse[:, s + cap:s + n] == LSE_SENTINEL).all())
            sq_b = min(n, cap)
            ln = KV_LENS[b] - (sq_b - cap)
            ou, lu = ops.fa3_prefill_cache(q[s:s + cap].permute(1, 0, 2)[None], kn[b:b + 1], vn[b:b + 1], cache_seqlens=i32([ln]), causal=causal,
                                           return_lse=True)
            torch.cuda.synchronize()
            assert torch.equal(out[s:s + cap].permute(1, 0, 2), ou[0]) and torch.equal(lse[:, s:s + cap], lu[0]), b


# --- paged == contiguous -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["phsd", "hpsd"])
@pytest.mark.parametrize("page", [64, 256])
def test_paged_equals_contiguous_with_a_shared_prefix_page(page, layout):
    from photonic_flash_attention_amd import ops
    for dtype, D in ((torch.bfloat16, 128), (torch.float16, 64)):
        q, _, _, kn, vn = _fixture(dtype, D)
        kp, vp, table = scatter(kn, vn, page, seed=page + D, layout=layout)
        assert kp.is_contiguous() == (layout == "hpsd")
        n = SHARED // page                               # sequences 0 and 4 hold their common prefix once
        share_prefix_pages(kp, vp, table, 0, 4, n)       # the duplicate copies are gone
        for causal, out_dtype in ((True, None), (False, None), (True, torch.float32)):
            if out_dtype is not None and dtype is not torch.bfloat16:
                continue
            oc, lc = _ragged(dtype, D, causal, out_dtype)                 # the contiguous call on the gathered cache
            out = torch.full((TOTAL, H, D), O_SENTINEL, dtype=out_dtype or dtype, device=q.device)
            op, lp = ops.fa3_prefill_varlen(q, kp, vp, cu_seqlens_q=i32(CU), max_seqlen_q=MAXQ, cache_seqlens=i32(KV_LENS),
                                            causal=causal, out_dtype=out_dtype, return_lse=True, out=out, block_table=table)
            torch.cuda.synchronize()
            assert bool(torch.isfinite(op).all()), "a page of another sequence, or a key past len_b, was read"
            assert torch.equal(op, oc), f"O differs: max-abs {float((op.double() - oc.double()).abs().max()):.3e}"
            assert torch.equal(lp[:, :CU[B]], lc[:, :CU[B]]), "LSE differs"


# --- views ---------------------------------------------------------------------------------------------------------------------------

def test_strided_packed_q_from_a_fused_projection():
    from photonic_flash_attention_amd import ops
    for dtype, D in ((torch.bfloat16, 128), (torch.float16, 64)):
        q, _, _, kn, vn = _fixture(dtype, D)
        fused = torch.full((TOTAL, 3 * H * D), NAN, dtype=dtype, device=q.device)        # [total, 3 H D]: q | k | v of the new tokens
        fused[:, :H * D] = q.reshape(TOTAL, H * D)
        qs = fused[:, :H * D].unflatten(1, (H, D))
        assert not qs.is_contiguous() and qs.stride() == (3 * H * D, D, 1)
        for causal in (True, False):
            oc, lc = _ragged(dtype, D, causal, None)
            out = torch.full((TOTAL, H, D), O_SENTINEL, dtype=dtype, device=q.device)
            o, lse = ops.fa3_prefill_varlen(qs, kn, vn, cu_seqlens_q=i32(CU), max_seqlen_q=MAXQ, cache_seqlens=i32(KV_LENS),
                                            causal=causal, return_lse=True, out=out)
            torch.cuda.synchronize()
            assert torch.equal(o, oc) and torch.equal(lse[:, :CU[B]], lc[:, :CU[B]])
    # out= with strides of its own: a slice of a wider buffer, untouched outside the slice
    q, _, _, kn, vn = _fixture(torch.bfloat16, 128)
    wide = torch.full((TOTAL, H, 2 * 128), O_SENTINEL, dtype=torch.bfloat16, device=q.device)
    o, _ = ops.fa3_prefill_varlen(q, kn, vn, cu_seqlens_q=i32(CU), max_seqlen_q=MAXQ, cache_seqlens=i32(KV_LENS), out=wide[..., 128:])
    torch.cuda.synchronize()
    assert torch.equal(o, _ragged(torch.bfloat16, 128, True, None)[0]) and bool((wide[..., :128] == O_SENTINEL).all())


# --- graph capture -------------------------------------------------------------------------------------------------------------------

def test_graph_replays_while_cu_seqlens_lengths_and_table_change():
    from photonic_flash_attention_amd import ops
    dtype, D, page, cap = torch.bfloat16, 128, 64, 512
    q, k, v, _, _ = _fixture(dtype, D)
    kp, vp, table = scatter(k, v, page, seed=77)        # clean caches: every page a table row can name is finite
    cu, lens = i32(CU), i32(KV_LENS)
    out = torch.full((TOTAL, H, D), O_SENTINEL, dtype=dtype, device=q.device)

    def call(o):
        return ops.fa3_prefill_varlen(q, kp, vp, cu_seqlens_q=cu, max_seqlen_q=cap, cache_seqlens=lens, return_lse=True, out=o,
                                      block_table=table)

    graph, (o_g, l_g) = capture(lambda: call(out))

    def replay_and_compare(rows):
        o_g.fill_(O_SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        first = (o_g.clone(), l_g.clone())
        o_g.fill_(O_SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(o_g, first[0]) and torch.equal(l_g[:, :rows], first[1][:, :rows])      # two replays of one state
        o_e, l_e = call(torch.full_like(out, O_SENTINEL))
        torch.cuda.synchronize()
        assert bool(torch.isfinite(o_g).all())
        assert torch.equal(o_g, o_e) and torch.equal(l_g[:, :rows], l_e[:, :rows])
        return first

    a = replay_and_compare(CU[B])
    assert torch.equal(a[0][:CU[B]], _scattered_fixture_result(q, kp, vp, table)[:CU[B]])
    assert bool((a[0][CU[B]:] == O_SENTINEL).all())
    # another step of the same server: other row counts (one sequence fills max_seqlen_q, one is empty, none leaves a spare row),
    # other lengths (30 keys for 63 rows: leading rows see nothing) and the sequences' pages dealt out differently
    cu.copy_(i32([0, 512, 512, 576, 577, 640]))
    lens.copy_(i32([1024, 100, 64, 500, 30]))
    table.copy_(table[[3, 0, 4, 1, 2]].flip(1).contiguous())
    b = replay_and_compare(TOTAL)
    assert not torch.equal(a[0], b[0]) and not bool((b[0] == O_SENTINEL).all(-1).any())              # every row is covered now
    assert bool((b[0][577:577 + 33] == 0).all()) and bool((b[1][:, 577:577 + 33] == float("-inf")).all())
    # and back: the first state's bits again
    cu.copy_(i32(CU))
    lens.copy_(i32(KV_LENS))
    table.copy_(table.flip(1)[[1, 3, 4, 0, 2]].contiguous())
    c = replay_and_compare(CU[B])
    assert torch.equal(c[0], a[0]) and torch.equal(c[1][:, :CU[B]], a[1][:, :CU[B]])


def _scattered_fixture_result(q, kp, vp, table):
    """The fixture's ragged result (max_seqlen_q = 300) on the clean paged cache: what the graph's first state must reproduce."""
    from photonic_flash_attention_amd import ops
    o, _ = ops.fa3_prefill_varlen(q, kp, vp, cu_seqlens_q=i32(CU), max_seqlen_q=MAXQ, cache_seqlens=i32(KV_LENS), block_table=table)
    torch.cuda.synchronize()
    return o


# --- PagedKVCache end to end ---------------------------------------------------------------------------------------------------------

def test_paged_cache_append_varlen_then_prefill_varlen():
    from photonic_flash_attention_amd.integration.pytorch import PagedKVCache
    dev = device()
    Hq, Hkv, D, page = 8, 2, 128, 64
    cache = PagedKVCache(num_pages=24, page_size=page, Hkv=Hkv, D=D, dtype=torch.bfloat16, device=dev, max_batch=3, max_pages_per_seq=8)
    cache.k_pool.fill_(NAN)                  # whatever is not appended stays NaN: unfilled page tails, unused pages
    cache.v_pool.fill_(NAN)
    g = torch.Generator(device=dev).manual_seed(31)

    def tokens(n):
        return (torch.randn(n, Hkv, D, generator=g, device=dev).to(torch.bfloat16),
                torch.randn(n, Hkv, D, generator=g, device=dev).to(torch.bfloat16))

    slots = [cache.allocate() for _ in range(3)]
    cache.append_varlen(slots, *tokens(200 + 0 + 70), [200, 0, 70])      # what the sequences held before this step
    for q_lens in ([5, 300, 1], [260, 1, 0]):                            # two steps: chunk + speculative + decode rows, then one empty
        total = sum(q_lens)
        cache.append_varlen(slots, *tokens(total), q_lens)               # the step's own keys first ...
        q = torch.randn(total + 7, Hq, D, generator=g, device=dev).to(torch.bfloat16)
        o, lse = cache.prefill_varlen(q, q_lens, return_lse=True)        # ... then the ragged call
        torch.cuda.synchronize()
        assert o.shape == (total + 7, Hq, D) and lse.shape == (Hq, total + 7)
        at = 0
        for s, n in zip(slots, q_lens):
            if n:
                gk, gv = cache.gather(s)
                ref = reference(q[at:at + n].permute(1, 0, 2)[None], gk[None], gv[None], seqlens=i32([cache.length(s)]))
                got = o[at:at + n].permute(1, 0, 2)[None]
                check_out(got, ref[0], ref[2], float(gv.abs().max()), torch.bfloat16)
                check_lse(got, lse[None, :, at:at + n], ref[1])
            at += n
    assert [cache.length(s) for s in slots] == [465, 301, 71]

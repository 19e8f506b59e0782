"""CPU-side tests (no GPU) of the ragged forward over a KV cache (``pfa_fa3_prefill_varlen*``, ABI v9 additive):
every validation rule, the launch description, ``ops.fa3_prefill_varlen``'s refusals and the
``PagedKVCache`` plumbing (``append_varlen`` against per-slot ``append``, ``prefill_varlen``'s cu_seqlens_q)."""

from __future__ import annotations

import ctypes as C

import pytest
import torch

from capi_testlib import ALIGN, DTYPE, FLAGS, HEAD_DIM, NULL, SHAPE, SIZE, STRIDE, lib, prefill_varlen_args, prefill_varlen_paged  # noqa: F401
from photonic_flash_attention_amd import _capi, ops


def _args(**over):
    """A valid contiguous call: B 5, H 8, Hkv 2, 640 packed rows of which a sequence has at most 300, Smax 4096, D 128."""
    return prefill_varlen_args(over)


def _pargs(**over):
    """The same logical shape over a pool of 100 pages laid out [num_pages, page_size, Hkv, D], 32 pages per sequence."""
    return prefill_varlen_paged(over, pages=32)


def _check(lib, a):
    return lib.pfa_fa3_prefill_varlen_check(C.byref(a))


def test_the_uniform_prefill_still_takes_the_decode_block(lib):
    a = _capi.make_decode_args(q=0x1000, k_cache=0x1000000, v_cache=0x2000000, o=0x800000, B=2, H=8, Hkv=2, Sq=300, Smax=4096, D=128,
                               q_stride_b=300 * 1024, q_stride_h=128, q_stride_s=1024, k_stride_b=4096 * 256, k_stride_h=128, k_stride_s=256,
                               v_stride_b=4096 * 256, v_stride_h=128, v_stride_s=256, o_stride_b=300 * 1024, o_stride_h=128, o_stride_s=1024,
                               dtype_in=0, dtype_out=0, causal=1, softmax_scale=128 ** -0.5)
    assert lib.pfa_fa3_prefill_check(C.byref(a)) == 0
    assert _capi.describe_prefill(a) == ("fa3_prefill_bf16_d128_o16_causal", 2 * 8 * 2)


def test_varlen_argument_validation(lib):
    assert _check(lib, _args()) == 0
    assert lib.pfa_fa3_prefill_varlen_check(None) == NULL
    bad = _args()
    bad.size = 16
    assert _check(lib, bad) == SIZE
    other = _args()
    other.size = C.sizeof(_capi.PfaFa3DecodeArgs)          # the uniform call's block is not this one
    assert _check(lib, other) == SIZE
    cases = [
        # the rules shared with pfa_fa3_prefill
        (dict(q=0), NULL), (dict(k_cache=0), NULL), (dict(v_cache=0), NULL), (dict(o=0), NULL),
        (dict(B=0), SHAPE), (dict(H=0), SHAPE), (dict(H=8, Hkv=3), SHAPE), (dict(Smax=0), SHAPE), (dict(softmax_scale=0.0), SHAPE),
        (dict(softmax_scale=float("inf")), SHAPE),
        (dict(D=96), HEAD_DIM),
        (dict(dtype_in=2, dtype_out=2), DTYPE), (dict(dtype_out=1), DTYPE),
        (dict(k_stride_s=2 * 128 + 1), STRIDE), (dict(v_stride_h=129), STRIDE), (dict(k_stride_s=-256), STRIDE),
        (dict(k_cache=0x1000008), ALIGN), (dict(q=0x1004), ALIGN), (dict(o=0x800008), ALIGN), (dict(lse=0x7002), ALIGN),
        (dict(cache_seqlens=0x5001), ALIGN),
        (dict(flags=1), FLAGS), (dict(flags=0x100), FLAGS), (dict(reserved0=1), FLAGS),
        (dict(page_size=64), FLAGS), (dict(num_pages=3), FLAGS), (dict(block_table_stride_b=4), FLAGS),
        # the rules of its own
        (dict(cu_seqlens_q=0), NULL),
        (dict(cu_seqlens_q=0x9002), ALIGN),
        (dict(total_q=0), SHAPE), (dict(total_q=-5), SHAPE), (dict(max_seqlen_q=0), SHAPE), (dict(max_seqlen_q=-1), SHAPE),
        (dict(max_seqlen_q=641), SHAPE), (dict(total_q=299), SHAPE),
        (dict(q_stride_s=8 * 128 + 4), STRIDE), (dict(q_stride_h=132), STRIDE),           # q: multiples of 8 elements
        (dict(o_stride_s=8 * 128 + 2), STRIDE), (dict(o_stride_h=130), STRIDE),           # o: multiples of 4
    ]
    for over, want in cases:
        assert _check(lib, _args(**over)) == want, over
    # more workgroups than a grid holds
    assert _check(lib, _args(B=1 << 20, H=1 << 10, Hkv=1 << 10, total_q=1 << 20, max_seqlen_q=1024)) == SHAPE
    paged = [
        (dict(page_size=96), SHAPE), (dict(page_size=32), SHAPE), (dict(page_size=0), SHAPE), (dict(num_pages=0), SHAPE),
        (dict(Smax=32 * 128 + 64), SHAPE), (dict(Smax=33 * 128), SHAPE), (dict(block_table_stride_b=31), SHAPE),
        (dict(block_table=0x8002), ALIGN),
        (dict(block_table=0), FLAGS),
    ]
    for over, want in paged:
        assert _check(lib, _pargs(**over)) == want, over


def test_varlen_accepted_variants(lib):
    for ok in (dict(D=64), dict(dtype_in=1, dtype_out=1), dict(dtype_out=2), dict(dtype_in=1, dtype_out=2), dict(causal=0),
               dict(H=64, Hkv=1), dict(Smax=1), dict(cache_seqlens=0x5000), dict(lse=0x7000), dict(o_stride_s=8 * 128 + 4),
               dict(q_stride_s=3 * 8 * 128),                                             # q inside a fused projection
               dict(max_seqlen_q=640), dict(total_q=300), dict(max_seqlen_q=1), dict(total_q=1, max_seqlen_q=1), dict(B=1)):
        assert _check(lib, _args(**ok)) == 0, ok
    for ok in (dict(), dict(_page=64), dict(_page=192), dict(_page=1024), dict(block_table_stride_b=40), dict(num_pages=1),
               dict(D=64), dict(dtype_out=2), dict(max_seqlen_q=640), dict(max_seqlen_q=1), dict(Smax=128, block_table_stride_b=1)):
        assert _check(lib, _pargs(**ok)) == 0, ok


@pytest.mark.parametrize("max_seqlen_q", [1, 256, 257, 2048])
@pytest.mark.parametrize("B,H,Hkv", [(5, 8, 2), (1, 32, 8), (3, 16, 1)])
def test_varlen_describe_counts_workgroups_from_host_shapes(lib, B, H, Hkv, max_seqlen_q):
    want = B * H * -(-max_seqlen_q // 256)
    for make in (_args, _pargs):
        a = make(B=B, H=H, Hkv=Hkv, total_q=4096, max_seqlen_q=max_seqlen_q, q_stride_s=H * 128, o_stride_s=H * 128,
                 k_stride_s=Hkv * 128, v_stride_s=Hkv * 128)
        name, wgs = _capi.describe_prefill_varlen(a)
        assert wgs == want
        # device-side inputs change neither the name nor the count
        a.cu_seqlens_q, a.cache_seqlens, a.lse = 0xA000, 0x5000, 0x7000
        assert _capi.describe_prefill_varlen(a) == (name, wgs)
        if make is _pargs:
            a.block_table = 0xB000
            assert _capi.describe_prefill_varlen(a) == (name, wgs)
        # and neither does total_q
        a.total_q = 8192
        assert _capi.describe_prefill_varlen(a) == (name, wgs)


def test_varlen_describe_names_the_uniform_kernel_with_varlen_before_paged(lib):
    def uniform(**kw):
        d = kw.get("D", 128)
        base = dict(q=0x1000, k_cache=0x1000000, v_cache=0x2000000, o=0x800000, B=5, H=8, Hkv=2, Sq=300, Smax=4096, D=d,
                    q_stride_b=300 * 8 * d, q_stride_h=d, q_stride_s=8 * d, k_stride_b=4096 * 2 * d, k_stride_h=d, k_stride_s=2 * d,
                    v_stride_b=4096 * 2 * d, v_stride_h=d, v_stride_s=2 * d, o_stride_b=300 * 8 * d, o_stride_h=d, o_stride_s=8 * d,
                    dtype_in=0, dtype_out=0, causal=1, softmax_scale=d ** -0.5)
        base.update(kw)
        return _capi.describe_prefill(_capi.make_decode_args(**base))[0]

    for kw in (dict(), dict(causal=0), dict(D=64, dtype_in=1, dtype_out=1), dict(dtype_out=2), dict(dtype_in=1, dtype_out=2, causal=0)):
        plain = uniform(**kw)
        assert _capi.describe_prefill_varlen(_args(**kw))[0] == plain + "_varlen"
        assert _capi.describe_prefill_varlen(_pargs(**kw))[0] == plain + "_varlen_paged"
    assert _capi.describe_prefill_varlen(_args())[0] == "fa3_prefill_bf16_d128_o16_causal_varlen"
    assert _capi.describe_prefill_varlen(_pargs(causal=0, dtype_out=2))[0] == "fa3_prefill_bf16_d128_o32_varlen_paged"
    with pytest.raises(_capi.PfaError):
        _capi.describe_prefill_varlen(_args(D=96))
    buf = C.create_string_buffer(8)                       # truncated, NUL terminated
    assert lib.pfa_fa3_prefill_varlen_describe(C.byref(_args()), buf, 8) == 5 * 8 * 2 and buf.value == b"fa3_pre"
    assert lib.pfa_fa3_prefill_varlen_describe(C.byref(_args()), None, 0) == 5 * 8 * 2


def test_fa3_prefill_varlen_refuses_host_tensors_and_bad_shapes():
    q = torch.zeros(640, 8, 128, dtype=torch.bfloat16)
    k = torch.zeros(5, 2, 512, 128, dtype=torch.bfloat16)
    cu = torch.tensor([0, 1, 301, 301, 334, 591], dtype=torch.int32)
    with pytest.raises(ValueError, match="pfa_fa3_prefill_varlen needs device tensors"):
        ops.fa3_prefill_varlen(q, k, k.clone(), cu_seqlens_q=cu, max_seqlen_q=300)
    with pytest.raises(ValueError, match="3-D"):
        ops.fa3_prefill_varlen(q[None], k, k.clone(), cu_seqlens_q=cu, max_seqlen_q=300)            # a 4-D q
    with pytest.raises(ValueError, match="3-D"):
        ops.fa3_prefill_varlen(q, k[0], k[0].clone(), cu_seqlens_q=cu, max_seqlen_q=300)
    with pytest.raises(ValueError, match="cu_seqlens_q must be an int32 tensor"):
        ops.fa3_prefill_varlen(q, k, k.clone(), cu_seqlens_q=cu.long(), max_seqlen_q=300)
    with pytest.raises(ValueError, match="cu_seqlens_q must be an int32 tensor"):
        ops.fa3_prefill_varlen(q, k, k.clone(), cu_seqlens_q=cu.tolist(), max_seqlen_q=300)
    with pytest.raises(ValueError, match=r"cu_seqlens_q must be \[B \+ 1\]"):
        ops.fa3_prefill_varlen(q, k, k.clone(), cu_seqlens_q=cu[None], max_seqlen_q=300)
    with pytest.raises(ValueError, match=r"cu_seqlens_q must be \[B \+ 1\]"):
        ops.fa3_prefill_varlen(q, k, k.clone(), cu_seqlens_q=cu[:1], max_seqlen_q=300)
    with pytest.raises(ValueError, match="shape mismatch"):                                          # B = 4 from cu, a cache of 5
        ops.fa3_prefill_varlen(q, k, k.clone(), cu_seqlens_q=cu[:5], max_seqlen_q=300)
    with pytest.raises(ValueError, match="shape mismatch"):
        ops.fa3_prefill_varlen(q, k, k[:, :1].clone(), cu_seqlens_q=cu, max_seqlen_q=300)
    with pytest.raises(ValueError, match="dtype"):
        ops.fa3_prefill_varlen(q.float(), k, k.clone(), cu_seqlens_q=cu, max_seqlen_q=300)
    # pools
    pool = torch.zeros(12, 2, 128, 128, dtype=torch.bfloat16)
    table = torch.zeros(5, 4, dtype=torch.int32)
    with pytest.raises(ValueError, match="shape mismatch"):
        ops.fa3_prefill_varlen(q, pool, pool[:, :1].clone(), cu_seqlens_q=cu, max_seqlen_q=300, block_table=table)
    with pytest.raises(ValueError, match="shape mismatch"):
        ops.fa3_prefill_varlen(q[:, :, :64], pool, pool.clone(), cu_seqlens_q=cu, max_seqlen_q=300, block_table=table)
    with pytest.raises(ValueError, match="multiple of 64"):
        ops.fa3_prefill_varlen(q, pool[:, :, :96], pool[:, :, :96].clone(), cu_seqlens_q=cu, max_seqlen_q=300, block_table=table)
    with pytest.raises(ValueError, match=r"block_table must be \[B, max_pages\] with B = 5"):
        ops.fa3_prefill_varlen(q, pool, pool.clone(), cu_seqlens_q=cu, max_seqlen_q=300, block_table=table[:4])
    with pytest.raises(ValueError, match="block_table must live on the operands' device"):
        ops.fa3_prefill_varlen(q, pool, pool.clone(), cu_seqlens_q=cu, max_seqlen_q=300, block_table=table)
    with pytest.raises(TypeError):
        ops.fa3_prefill_varlen(q, k, k.clone(), cu_seqlens_q=cu, max_seqlen_q=300, key_mask=torch.ones(5, 512, dtype=torch.bool))
    with pytest.raises(TypeError):
        ops.fa3_prefill_varlen(q, k, k.clone())                                                      # cu_seqlens_q / max_seqlen_q are required


def _cache(**kw):
    from photonic_flash_attention_amd.integration.pytorch import PagedKVCache
    base = dict(num_pages=12, page_size=64, Hkv=2, D=64, dtype=torch.bfloat16, device="cpu", max_batch=4, max_pages_per_seq=6)
    base.update(kw)
    c = PagedKVCache(**base)
    c.k_pool.fill_(-7.0)               # what no append wrote stays recognisable
    c.v_pool.fill_(-7.0)
    return c


def _state(c):
    return (c.k_pool.clone(), c.v_pool.clone(), c.block_table.clone(), c.cache_seqlens.clone(),
            [c.pages(s) if c._live[s] else None for s in range(c.max_batch)], c.free_pages)


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a[:4], b[:4])) and a[4:] == b[4:]


def test_append_varlen_equals_per_slot_appends():
    g = torch.Generator().manual_seed(3)
    one, two = _cache(), _cache()
    for c in (one, two):
        for _ in range(3):
            c.allocate()
    for lens in ([100, 1, 65], [0, 130, 27], [64, 0, 0]):      # page boundaries inside a chunk, empty chunks, exact page fills
        total = sum(lens)
        k = torch.randn(total, 2, 64, generator=g).to(torch.bfloat16)
        v = torch.randn(total, 2, 64, generator=g).to(torch.bfloat16)
        one.append_varlen([2, 0, 1], k, v, lens)
        at = 0
        for s, n in zip([2, 0, 1], lens):                       # [n, Hkv, Sq, D] is append's layout
            two.append(s, k[at:at + n].permute(1, 0, 2)[None], v[at:at + n].permute(1, 0, 2)[None])
            at += n
        assert _same(_state(one), _state(two)), lens
        assert [one.length(s) for s in range(3)] == [two.length(s) for s in range(3)]
    assert [one.length(s) for s in (2, 0, 1)] == [164, 131, 92]
    for s in range(3):
        ka, va = one.gather(s)
        kb, vb = two.gather(s)
        assert torch.equal(ka, kb) and torch.equal(va, vb)
    # a single slot as an int
    k = torch.randn(5, 2, 64, generator=g).to(torch.bfloat16)
    one.append_varlen(1, k, k, [5])
    two.append(1, k.permute(1, 0, 2)[None], k.permute(1, 0, 2)[None])
    assert _same(_state(one), _state(two))


def test_append_varlen_is_all_or_nothing_and_checks_its_arguments():
    from photonic_flash_attention_amd.integration.pytorch import PagedCacheFull
    one, two = _cache(num_pages=4), _cache(num_pages=4)
    for c in (one, two):
        c.allocate()
        c.allocate()
    k = torch.ones(70 + 200, 2, 64, dtype=torch.bfloat16)
    before = _state(one)
    with pytest.raises(PagedCacheFull):                         # 2 + 4 pages out of 4
        one.append_varlen([0, 1], k, k, [70, 200])
    assert _same(_state(one), before) and one.length(0) == 0 and one.length(1) == 0 and one.free_pages == 4
    tok = lambda t: t.permute(1, 0, 2)[None]                    # noqa: E731  ([n, Hkv, D] -> append's [1, Hkv, n, D])
    two.append(0, tok(k[:70]), tok(k[:70]))                     # the per-slot appends refuse at the same request, having written slot 0
    with pytest.raises(PagedCacheFull):
        two.append(1, tok(k[70:]), tok(k[70:]))
    assert two.length(0) == 70 and two.length(1) == 0
    big = torch.ones(6 * 64 + 1, 2, 64, dtype=torch.bfloat16)
    with pytest.raises(PagedCacheFull):                         # more tokens than a table row holds
        one.append_varlen([1, 0], big, big, [6 * 64 + 1, 0])
    assert _same(_state(one), before)
    one.append_varlen([0, 1], k[:198], k[:198], [70, 128])      # 2 + 2 pages: exactly the pool
    assert one.free_pages == 0 and one.length(0) == 70 and one.length(1) == 128
    with pytest.raises(PagedCacheFull):                         # slot 0 has room for 58 more, slot 1 for none
        one.append_varlen([0, 1], k[:59], k[:59], [58, 1])
    assert one.length(0) == 70 and one.length(1) == 128 and bool((one.gather(0)[0] == 1).all())
    with pytest.raises(ValueError, match="once per append"):
        one.append_varlen([0, 0], k[:4], k[:4], [2, 2])
    with pytest.raises(ValueError, match="one non-negative token count per slot"):
        one.append_varlen([0, 1], k[:4], k[:4], [4])
    with pytest.raises(ValueError, match="one non-negative token count per slot"):
        one.append_varlen([0, 1], k[:4], k[:4], [5, -1])
    with pytest.raises(ValueError, match="k_new / v_new must be"):
        one.append_varlen([0, 1], k[:5], k[:5], [2, 2])
    with pytest.raises(ValueError, match="k_new / v_new must be"):
        one.append_varlen([0, 1], k[:4].permute(1, 0, 2)[None], k[:4].permute(1, 0, 2)[None], [2, 2])
    with pytest.raises(ValueError, match="dtype"):
        one.append_varlen([0, 1], k[:4].float(), k[:4].float(), [2, 2])
    with pytest.raises(ValueError, match="not allocated"):
        one.append_varlen([3], k[:4], k[:4], [4])


def test_paged_cache_prefill_varlen_hands_its_own_table_and_lengths_to_ops(monkeypatch):
    from photonic_flash_attention_amd.integration.pytorch import paged_cache
    calls = []

    def spy(q, k, v, **kw):
        calls.append((q, k, v, kw))
        return "o", "lse"

    monkeypatch.setattr(paged_cache.ops, "fa3_prefill_varlen", spy)
    c = _cache(num_pages=8, max_batch=3, max_pages_per_seq=4)
    for _ in range(3):
        c.allocate()
    q = torch.zeros(640, 8, 64, dtype=torch.bfloat16)
    assert c.prefill_varlen(q, [300, 0, 33], causal=False, return_lse=True) == ("o", "lse")
    q_, k_, v_, kw = calls.pop()
    assert q_ is q and k_.shape == (8, 2, 64, 64) and v_.shape == (8, 2, 64, 64)
    assert k_.data_ptr() == c.k_pool.data_ptr() and v_.data_ptr() == c.v_pool.data_ptr() and k_.stride() == c.k_pool.transpose(1, 2).stride()
    assert kw["block_table"] is c.block_table and kw["cache_seqlens"] is c.cache_seqlens
    assert kw["cu_seqlens_q"].dtype == torch.int32 and kw["cu_seqlens_q"].tolist() == [0, 300, 300, 333]      # the prefix sums
    assert kw["max_seqlen_q"] == 300 and kw["causal"] is False and kw["return_lse"] is True
    # a bound of the caller's own is kept
    c.prefill_varlen(q, [300, 0, 33], max_seqlen_q=512)
    assert calls.pop()[3]["max_seqlen_q"] == 512
    # a run of consecutive slots: views of the cache's own tensors (capturable); any other list: copies of its rows
    c.prefill_varlen(q, [5, 1], slots=[1, 2])
    kw = calls.pop()[3]
    assert kw["block_table"].data_ptr() == c.block_table[1:].data_ptr() and kw["cache_seqlens"].data_ptr() == c.cache_seqlens[1:].data_ptr()
    assert kw["block_table"].shape == (2, 4) and kw["cu_seqlens_q"].tolist() == [0, 5, 6] and kw["max_seqlen_q"] == 5
    c.prefill_varlen(q, [1, 7], slots=[2, 0])
    kw = calls.pop()[3]
    assert torch.equal(kw["block_table"], c.block_table[[2, 0]]) and torch.equal(kw["cache_seqlens"], c.cache_seqlens[[2, 0]])
    # the graph-capturing caller's own device tensor and bound go through untouched
    cu = torch.tensor([0, 512, 512, 576], dtype=torch.int32)
    c.prefill_varlen(q, cu_seqlens_q=cu, max_seqlen_q=512)
    kw = calls.pop()[3]
    assert kw["cu_seqlens_q"] is cu and kw["max_seqlen_q"] == 512 and kw["block_table"] is c.block_table
    with pytest.raises(ValueError, match="max_seqlen_q"):
        c.prefill_varlen(q, cu_seqlens_q=cu)
    with pytest.raises(ValueError, match="either q_lens"):
        c.prefill_varlen(q)
    with pytest.raises(ValueError, match="either q_lens"):
        c.prefill_varlen(q, [300, 0, 33], cu_seqlens_q=cu, max_seqlen_q=512)
    with pytest.raises(ValueError, match="one non-negative row count per slot"):
        c.prefill_varlen(q, [300, 33])
    with pytest.raises(ValueError, match="rows, q has 640"):
        c.prefill_varlen(q, [300, 300, 41])
    assert not calls
    # append and prefill are what they were: the uniform call goes to fa3_prefill_cache, not here
    monkeypatch.setattr(paged_cache.ops, "fa3_prefill_cache", lambda q, k, v, **kw: ("uniform", kw))
    assert c.prefill(torch.zeros(3, 8, 10, 64, dtype=torch.bfloat16))[0] == "uniform" and not calls
    # and without the spy the CPU cache is refused by ops: there is no CPU path
    monkeypatch.undo()
    with pytest.raises(ValueError, match="device"):
        c.prefill_varlen(q, [300, 0, 33])

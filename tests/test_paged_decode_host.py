"""CPU-side tests (no GPU) of the paged KV cache of the decode path (ABI v9): where the appended fields lie, argument validation,
the workspace / split contract against the contiguous call, ``ops.fa3_decode(block_table=...)`` refusals and the ``PagedKVCache``
bookkeeping on CPU tensors."""

from __future__ import annotations

import ctypes as C

import pytest
import torch

from capi_testlib import decode_paged, lib  # noqa: F401
from photonic_flash_attention_amd import _capi, ops

# offsets of pfa_fa3_decode_args in ABI v8 (the struct before the paging fields were appended); its size was 232
V8_OFFSETS = dict(size=0, flags=4, q=8, k_cache=16, v_cache=24, o=32, lse=40, cache_seqlens=48, key_mask=56,
                  q_stride_b=64, q_stride_h=72, q_stride_s=80, k_stride_b=88, k_stride_h=96, k_stride_s=104,
                  v_stride_b=112, v_stride_h=120, v_stride_s=128, o_stride_b=136, o_stride_h=144, o_stride_s=152,
                  key_mask_stride_b=160, B=168, H=172, Hkv=176, Sq=180, Smax=184, D=188, dtype_in=192, dtype_out=196, causal=200,
                  softmax_scale=204, device_id=208, reserved0=212, workspace=216, workspace_bytes=224)
NEW_FIELDS = ("block_table", "block_table_stride_b", "page_size", "num_pages")


def test_paging_fields_are_appended_behind_the_abi_v8_fields():
    """Against the mirror, whose offsets tests/test_capi_conformance.py holds to the C struct's."""
    A = _capi.PfaFa3DecodeArgs
    assert [f for f, _ in A._fields_] == list(V8_OFFSETS) + list(NEW_FIELDS)
    assert {f: getattr(A, f).offset for f in V8_OFFSETS} == V8_OFFSETS   # every old field where it was
    assert [getattr(A, f).offset for f in NEW_FIELDS] == [232, 240, 248, 252] and C.sizeof(A) == 256


def _pargs(**over):
    """A valid paged call: B 2, H 8, Hkv 2, Sq 1, D 128, 32 pages of 128 keys per sequence (Smax 4096) out of a pool of 100
    pages laid out [num_pages, page_size, Hkv, D], with the workspace the library asks for; the strides move with D only."""
    return decode_paged({**dict(k_cache=0x100000, v_cache=0x4000000, o=0x3000), **over}, Sq=1, pages=32, ws="asked", follow="D")


def _contiguous(a):
    """The contiguous call of the same logical shape."""
    b = _capi.PfaFa3DecodeArgs.from_buffer_copy(a)
    b.block_table, b.block_table_stride_b, b.page_size, b.num_pages = None, 0, 0, 0
    b.k_stride_b = b.v_stride_b = b.Smax * b.Hkv * b.D
    return b


def test_paged_argument_validation(lib):
    assert lib.pfa_fa3_decode_check(C.byref(_pargs())) == 0
    for ok in (dict(_page=64), dict(_page=1024), dict(_page=192), dict(block_table_stride_b=40), dict(num_pages=1),
               dict(Smax=128, block_table_stride_b=1), dict(D=64), dict(dtype_out=2), dict(block_table=0x8004)):
        assert lib.pfa_fa3_decode_check(C.byref(_pargs(**ok))) == 0, ok
    SHAPE, ALIGN, FLAGS = -3, -7, -10
    cases = [
        (dict(page_size=0), SHAPE), (dict(page_size=-128), SHAPE), (dict(page_size=32), SHAPE), (dict(page_size=96), SHAPE),
        (dict(page_size=100), SHAPE), (dict(num_pages=0), SHAPE), (dict(num_pages=-1), SHAPE),
        (dict(Smax=32 * 128 + 64), SHAPE),              # not a whole number of pages
        (dict(block_table_stride_b=31), SHAPE),         # a row shorter than max_pages
        (dict(block_table_stride_b=0), SHAPE),
        (dict(block_table=0x8002), ALIGN), (dict(block_table=0x8001), ALIGN),
        # paging fields without a table
        (dict(block_table=0), FLAGS), (dict(block_table=0, page_size=0, num_pages=0), FLAGS),
        (dict(block_table=0, block_table_stride_b=0, num_pages=0), FLAGS), (dict(block_table=0, block_table_stride_b=0, page_size=0), FLAGS),
        # what the contiguous call refuses is still refused
        (dict(flags=1), FLAGS), (dict(reserved0=1), FLAGS), (dict(k_stride_b=128 * 2 * 128 + 4), -6), (dict(k_cache=0x100008), ALIGN),
        (dict(workspace=0), -1),
    ]
    for over, want in cases:
        assert lib.pfa_fa3_decode_check(C.byref(_pargs(**over))) == want, over
    # the refusals' texts exist
    for st in (SHAPE, ALIGN, FLAGS):
        assert _capi.status_string(st)


def test_null_table_with_zeroed_paging_fields_is_the_contiguous_call(lib):
    a = _contiguous(_pargs())
    assert lib.pfa_fa3_decode_check(C.byref(a)) == 0
    name, wgs, nsplit = _capi.describe_decode(a)
    assert name.startswith("fa3_decode_bf16_d128_o16") and "_paged" not in name and wgs == 2 * 2 * nsplit
    # the old refusals, through the longer struct
    for over, want in ((dict(D=96), -4), (dict(Sq=65), -3), (dict(k_stride_s=2 * 128 + 1), -6), (dict(flags=0x100), -10)):
        b = _contiguous(_pargs())
        for k, v in over.items():
            setattr(b, k, v)
        assert lib.pfa_fa3_decode_check(C.byref(b)) == want, over
    short = _contiguous(_pargs())
    short.size = 232                       # an ABI v8 caller's struct
    assert lib.pfa_fa3_decode_check(C.byref(short)) == -2


@pytest.mark.parametrize("B,H,Hkv,Sq,pages,page,D", [
    (2, 8, 2, 1, 32, 128, 128),        # several splits
    (1, 32, 8, 1, 512, 64, 128),       # B 1, 32768 keys: 64 splits
    (1, 8, 8, 1, 128, 1024, 64),       # 131072 keys
    (8, 32, 8, 1, 32, 1024, 128),
    (2, 8, 2, 1, 1, 64, 128),          # one page, one split, no workspace
    (64, 32, 32, 4, 8, 256, 128),      # enough (batch, head) items for one split
    (3, 64, 1, 8, 5, 192, 64),         # a page size that is no power of two
])
def test_paged_plan_equals_the_contiguous_plan(lib, B, H, Hkv, Sq, pages, page, D):
    a = _pargs(B=B, H=H, Hkv=Hkv, Sq=Sq, Smax=pages * page, D=D, _page=page, block_table_stride_b=pages,
               q_stride_b=Sq * H * D, q_stride_s=H * D, q_stride_h=D, o_stride_b=Sq * H * D, o_stride_s=H * D, o_stride_h=D,
               k_stride_b=page * Hkv * D, k_stride_s=Hkv * D, k_stride_h=D, v_stride_b=page * Hkv * D, v_stride_s=Hkv * D, v_stride_h=D)
    c = _contiguous(a)
    wa, wc = lib.pfa_fa3_decode_workspace_bytes(C.byref(a)), lib.pfa_fa3_decode_workspace_bytes(C.byref(c))
    assert wa == wc
    na, ga, sa = _capi.describe_decode(a)
    nc, gc, sc = _capi.describe_decode(c)
    assert (ga, sa) == (gc, sc)
    assert na == nc + "_paged" and na.endswith("_paged")
    assert (wa == 0) == (sa == 1)


def test_plan_cases_cover_one_split_and_the_split_limit(lib):
    assert _capi.describe_decode(_pargs(Smax=64, _page=64, block_table_stride_b=1))[2] == 1
    a = _pargs(B=1, Smax=512 * 64, _page=64, block_table_stride_b=512)       # 2 (batch, K/V head) items, 32768 keys
    assert _capi.describe_decode(a)[2] == 128


# --- ops.fa3_decode(block_table=...) -----------------------------------------------------------------------------------------------

def _host_problem(page=64, B=2, pages=4, num_pages=12):
    q = torch.zeros(B, 8, 1, 128, dtype=torch.bfloat16)
    pool = torch.zeros(num_pages, 2, page, 128, dtype=torch.bfloat16)
    bt = torch.zeros(B, pages, dtype=torch.int32)
    return q, pool, bt


def test_fa3_decode_paged_refusals():
    q, pool, bt = _host_problem()
    with pytest.raises(ValueError, match="device"):                       # host tensors: there is no CPU path
        ops.fa3_decode(q, pool, pool.clone(), block_table=bt)
    with pytest.raises(ValueError, match="int32"):
        ops.fa3_decode(q, pool, pool.clone(), block_table=bt.long())
    with pytest.raises(ValueError, match="int32"):
        ops.fa3_decode(q, pool, pool.clone(), block_table=[[0, 1, 2, 3]] * 2)
    with pytest.raises(ValueError, match=r"\[B, max_pages\]"):
        ops.fa3_decode(q, pool, pool.clone(), block_table=torch.zeros(3, 4, dtype=torch.int32))
    with pytest.raises(ValueError, match=r"\[B, max_pages\]"):
        ops.fa3_decode(q, pool, pool.clone(), block_table=torch.zeros(8, dtype=torch.int32))
    for page in (16, 32, 96, 100):
        q, pool, bt = _host_problem(page=page)
        with pytest.raises(ValueError, match="multiple of 64"):
            ops.fa3_decode(q, pool, pool.clone(), block_table=bt)
    q, pool, bt = _host_problem()
    with pytest.raises(ValueError, match="shape mismatch"):               # V pool of another shape
        ops.fa3_decode(q, pool, pool[:-1].clone(), block_table=bt)
    with pytest.raises(ValueError, match="contiguous"):
        ops.fa3_decode(q, pool, pool.clone(), block_table=torch.zeros(2, 8, dtype=torch.int32)[:, ::2])


# --- PagedKVCache on CPU tensors ---------------------------------------------------------------------------------------------------

def _cache(**kw):
    from photonic_flash_attention_amd.integration.pytorch import PagedKVCache
    args = dict(num_pages=8, page_size=64, Hkv=2, D=16, dtype=torch.float32, device="cpu", max_batch=3, max_pages_per_seq=4)
    args.update(kw)
    return PagedKVCache(**args)


def _tokens(n, seed, Hkv=2, D=16):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(1, Hkv, n, D, generator=g), torch.randn(1, Hkv, n, D, generator=g)


def test_paged_cache_append_across_pages_and_gather():
    c = _cache()
    ptr_t, ptr_l = c.block_table.data_ptr(), c.cache_seqlens.data_ptr()
    assert c.block_table.shape == (3, 4) and c.block_table.dtype == torch.int32 and c.cache_seqlens.dtype == torch.int32
    assert c.k_pool.shape == (8, 64, 2, 16) and c.v_pool.shape == (8, 64, 2, 16)
    s0, s1 = c.allocate(), c.allocate(10)
    assert (s0, s1) == (0, 1) and c.length(s1) == 0 and len(c.pages(s1)) == 1 and c.pages(s0) == ()
    ks, vs = {s0: [], s1: []}, {s0: [], s1: []}
    seed = 0
    for slot, n in ((s0, 60), (s1, 64), (s0, 5), (s1, 1), (s0, 70), (s1, 63)):     # 60 -> 65 crosses a page, 64 -> 65, 65 -> 135 crosses two
        k, v = _tokens(n, seed)
        seed += 1
        c.append(slot, k, v)
        ks[slot].append(k[0])
        vs[slot].append(v[0])
    k, v = _tokens(1, 99)                                                          # both at once, one token each
    k2, v2 = torch.cat([k, k + 1]), torch.cat([v, v + 1])
    c.append([s0, s1], k2, v2)
    for i, slot in enumerate((s0, s1)):
        ks[slot].append(k2[i])
        vs[slot].append(v2[i])
    assert c.length(s0) == 136 and c.length(s1) == 129
    assert c.cache_seqlens.tolist() == [136, 129, 0]
    assert len(c.pages(s0)) == 3 and len(c.pages(s1)) == 3 and c.free_pages == 2
    assert not set(c.pages(s0)) & set(c.pages(s1))                                 # two live sequences never share a page
    for slot in (s0, s1):
        gk, gv = c.gather(slot)
        assert gk.shape == (2, c.length(slot), 16)
        assert torch.equal(gk, torch.cat(ks[slot], dim=1)) and torch.equal(gv, torch.cat(vs[slot], dim=1))
        assert c.block_table[slot, :3].tolist() == list(c.pages(slot))
    # the device tensors are the ones handed out at the start
    assert c.block_table.data_ptr() == ptr_t and c.cache_seqlens.data_ptr() == ptr_l


def test_paged_cache_free_and_reallocate_reuses_pages():
    c = _cache()
    ptr_t, ptr_l = c.block_table.data_ptr(), c.cache_seqlens.data_ptr()
    a, b = c.allocate(), c.allocate()
    c.append(a, *_tokens(130, 1))
    c.append(b, *_tokens(64, 2))
    freed = set(c.pages(a))
    keep_k, keep_v = c.gather(b)
    c.free(a)
    assert c.free_pages == 7 and c.cache_seqlens.tolist() == [0, 64, 0]
    with pytest.raises(ValueError):
        c.length(a)
    with pytest.raises(ValueError):
        c.append(a, *_tokens(1, 3))
    d = c.allocate()
    assert d == a                                                                  # the freed slot is handed out again
    c.append(d, *_tokens(200, 4))
    assert freed <= set(c.pages(d)) and not set(c.pages(d)) & set(c.pages(b))
    gk, gv = c.gather(b)
    assert torch.equal(gk, keep_k) and torch.equal(gv, keep_v)                     # the neighbour is untouched
    k4, v4 = _tokens(200, 4)
    gk, gv = c.gather(d)
    assert torch.equal(gk, k4[0]) and torch.equal(gv, v4[0])
    assert c.block_table.data_ptr() == ptr_t and c.cache_seqlens.data_ptr() == ptr_l


def test_paged_cache_reserve_assigns_pages_ahead():
    c = _cache()
    s = c.allocate()
    c.append(s, *_tokens(10, 5))
    c.reserve(s, 200)
    pages = c.pages(s)
    assert len(pages) == 4 and c.block_table[s].tolist() == list(pages) and c.length(s) == 10
    c.append(s, *_tokens(180, 6))
    assert c.pages(s) == pages                                                     # grown into the reserved pages, none new
    c.reserve(s, 5)                                                                # never shrinks
    assert c.pages(s) == pages


def test_paged_cache_exhaustion_raises_and_writes_nothing():
    from photonic_flash_attention_amd.integration.pytorch import PagedCacheFull
    c = _cache(num_pages=3, max_pages_per_seq=3)
    a, b = c.allocate(), c.allocate()
    c.append(a, *_tokens(128, 7))
    c.append(b, *_tokens(64, 8))
    before_k, before_len, before_tab = c.k_pool.clone(), c.cache_seqlens.clone(), c.block_table.clone()
    with pytest.raises(PagedCacheFull):
        c.append(b, *_tokens(1, 9))                                                # would need a fourth page
    k, v = _tokens(1, 10)
    with pytest.raises(PagedCacheFull):
        c.append([a, b], torch.cat([k, k]), torch.cat([v, v]))
    with pytest.raises(PagedCacheFull):
        c.reserve(a, 129)
    assert torch.equal(c.k_pool, before_k) and torch.equal(c.cache_seqlens, before_len) and torch.equal(c.block_table, before_tab)
    assert c.length(a) == 128 and c.length(b) == 64 and c.free_pages == 0
    c.allocate()
    with pytest.raises(PagedCacheFull):
        c.allocate()                                                               # no slot left
    # a sequence cannot outgrow its table row even when pages are free
    c2 = _cache(num_pages=8, max_pages_per_seq=2)
    s = c2.allocate()
    with pytest.raises(PagedCacheFull):
        c2.append(s, *_tokens(129, 11))
    assert c2.length(s) == 0 and c2.free_pages == 8
    assert issubclass(PagedCacheFull, RuntimeError)


def test_paged_cache_swap_pages_keeps_the_sequence():
    c = _cache()
    s = c.allocate()
    c.append(s, *_tokens(150, 12))
    k0, v0 = c.gather(s)
    pages = c.pages(s)
    c.swap_pages(s, 0, 2)
    assert c.pages(s) == (pages[2], pages[1], pages[0]) and c.block_table[s, :3].tolist() == list(c.pages(s))
    k1, v1 = c.gather(s)
    assert torch.equal(k0, k1) and torch.equal(v0, v1)
    c.append(s, *_tokens(1, 13))                                                   # lands in the page that now backs logical page 2
    assert torch.equal(c.gather(s)[0][:, :150], k0)


def test_paged_cache_refuses_bad_page_sizes_and_decode_on_cpu():
    for page in (16, 32, 100):
        with pytest.raises(ValueError, match="multiple of 64"):
            _cache(page_size=page)
    c = _cache(dtype=torch.bfloat16, D=64)
    s = c.allocate()
    c.append(s, torch.zeros(1, 2, 3, 64, dtype=torch.bfloat16), torch.zeros(1, 2, 3, 64, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="device"):
        c.decode(torch.zeros(3, 8, 1, 64, dtype=torch.bfloat16))

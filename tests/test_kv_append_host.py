"""CPU-side tests (no GPU) of the device-side KV-cache append (``pfa_kv_append*``, ABI v9 additive):
every validation rule, the launch description, ``ops.kv_append``'s refusals, the plain-torch model of the rule
(``ops.kv_append`` on CPU tensors: the executable specification the GPU tests compare the kernel with) against token-by-token
loops written here, and ``PagedKVCache.advance`` + ``write_step`` against ``append_varlen``.

Every cache or pool holds a sentinel before a call and every packed row no sequence owns holds NaN, so a stray write, a missing
write and a read of a foreign row all show.  Every comparison is ``torch.equal``: a copy is bit-exact."""

from __future__ import annotations

import ctypes as C

import pytest
import torch

from capi_testlib import ALIGN, DTYPE, FLAGS, HEAD_DIM, NULL, SHAPE, SIZE, STRIDE, lib  # noqa: F401
from capi_testlib import kv_append_args as _args, kv_append_paged as _pargs, kv_append_uniform as _uargs
from photonic_flash_attention_amd import _capi, ops

SENTINEL, NAN = -7.0, float("nan")


def _check(lib, a):
    return lib.pfa_kv_append_check(C.byref(a))


def test_kv_append_argument_validation(lib):
    assert _check(lib, _args()) == 0 and _check(lib, _uargs()) == 0 and _check(lib, _pargs()) == 0
    assert lib.pfa_kv_append_check(None) == NULL
    bad = _args()
    bad.size = 16
    assert _check(lib, bad) == SIZE
    other = _args()
    other.size = C.sizeof(_capi.PfaFa3PrefillVarlenArgs)
    assert _check(lib, other) == SIZE
    cases = [
        (dict(k_new=0), NULL), (dict(v_new=0), NULL), (dict(k_cache=0), NULL), (dict(v_cache=0), NULL), (dict(cache_seqlens=0), NULL),
        (dict(B=0), SHAPE), (dict(Hkv=0), SHAPE), (dict(Smax=0), SHAPE), (dict(total_new=0), SHAPE), (dict(total_new=-5), SHAPE),
        (dict(max_seqlen_q=0), SHAPE), (dict(max_seqlen_q=-1), SHAPE),
        (dict(max_seqlen_q=641), SHAPE), (dict(total_new=299), SHAPE),                       # ragged: max_seqlen_q > total_new
        (dict(D=0), HEAD_DIM), (dict(D=4), HEAD_DIM), (dict(D=100), HEAD_DIM), (dict(D=264), HEAD_DIM), (dict(D=512), HEAD_DIM),
        (dict(dtype=2), DTYPE), (dict(dtype=7), DTYPE), (dict(dtype=-1), DTYPE),
        (dict(kn_stride_s=2 * 128 + 4), STRIDE), (dict(kn_stride_h=129), STRIDE), (dict(vn_stride_s=2 * 128 + 1), STRIDE),
        (dict(vn_stride_h=132), STRIDE), (dict(k_stride_b=4096 * 256 + 2), STRIDE), (dict(k_stride_s=2 * 128 + 1), STRIDE),
        (dict(k_stride_h=130), STRIDE), (dict(v_stride_b=7), STRIDE), (dict(v_stride_h=129), STRIDE), (dict(v_stride_s=-3), STRIDE),
        (dict(k_stride_s=-256), STRIDE), (dict(v_stride_s=-256), STRIDE),                    # as the calls that read the cache
        (dict(k_new=0x1008), ALIGN), (dict(v_new=0x3004), ALIGN), (dict(k_cache=0x1000008), ALIGN), (dict(v_cache=0x2000002), ALIGN),
        (dict(cache_seqlens=0x5001), ALIGN), (dict(cu_seqlens_q=0x9002), ALIGN),
        (dict(flags=1), FLAGS), (dict(flags=0x100), FLAGS), (dict(reserved0=1), FLAGS), (dict(reserved1=-1), FLAGS),
        (dict(page_size=64), FLAGS), (dict(num_pages=3), FLAGS), (dict(block_table_stride_b=4), FLAGS),      # paging fields without a table
        (dict(kn_stride_b=8), FLAGS), (dict(vn_stride_b=4096), FLAGS),                       # ragged rows have no batch stride
    ]
    for over, want in cases:
        assert _check(lib, _args(**over)) == want, over
    uniform = [
        (dict(total_new=1499), SHAPE), (dict(B=6), SHAPE), (dict(max_seqlen_q=301), SHAPE),  # B * max_seqlen_q > total_new
        (dict(kn_stride_b=300 * 256 + 4), STRIDE), (dict(vn_stride_b=3), STRIDE),
    ]
    for over, want in uniform:
        assert _check(lib, _uargs(**over)) == want, over
    # the paging rules return what check_cache_args returns for them
    paged = [
        (dict(page_size=96), SHAPE), (dict(page_size=32), SHAPE), (dict(page_size=0), SHAPE), (dict(num_pages=0), SHAPE),
        (dict(Smax=32 * 128 + 64), SHAPE), (dict(Smax=33 * 128), SHAPE), (dict(block_table_stride_b=31), SHAPE),
        (dict(block_table=0x8002), ALIGN),
        (dict(block_table=0), FLAGS),
    ]
    for over, want in paged:
        assert _check(lib, _pargs(**over)) == want, over
        pa = _pargs(**over)
        d = _capi.make_prefill_varlen_args(q=0x1000, k_cache=0x1000000, v_cache=0x2000000, o=0x800000, cu_seqlens_q=0x9000, B=5, H=8, Hkv=2,
                                           total_q=640, max_seqlen_q=300, Smax=pa.Smax, D=128, q_stride_s=1024, q_stride_h=128,
                                           o_stride_s=1024, o_stride_h=128, k_stride_b=pa.k_stride_b, k_stride_h=128, k_stride_s=256,
                                           v_stride_b=pa.v_stride_b, v_stride_h=128, v_stride_s=256, dtype_in=0, dtype_out=0, causal=1,
                                           softmax_scale=0.1, block_table=pa.block_table, block_table_stride_b=pa.block_table_stride_b,
                                           page_size=pa.page_size, num_pages=pa.num_pages)
        assert lib.pfa_fa3_prefill_varlen_check(C.byref(d)) == want, over
    # more workgroups than a grid holds; a sequence's 16-byte pieces past 32 bits
    assert _check(lib, _args(B=1 << 24, total_new=1 << 20, max_seqlen_q=1 << 12)) == SHAPE
    assert _check(lib, _args(B=1, Hkv=1 << 10, total_new=1 << 30, max_seqlen_q=1 << 20, D=256)) == SHAPE
    # the launch refuses what the check refuses, before it touches a device
    assert lib.pfa_kv_append(C.byref(_args(D=100)), None) == HEAD_DIM and lib.pfa_kv_append(None, None) == NULL


def test_kv_append_accepted_variants(lib):
    for ok in (dict(D=8), dict(D=64), dict(D=96), dict(D=256), dict(dtype=1), dict(Hkv=1), dict(Hkv=64), dict(Smax=1), dict(B=1),
               dict(max_seqlen_q=640), dict(max_seqlen_q=1), dict(total_new=300), dict(total_new=1, max_seqlen_q=1),
               dict(kn_stride_s=3 * 8 * 128, vn_stride_s=3 * 8 * 128),                        # k / v inside a fused projection
               dict(k_stride_h=4096 * 128, k_stride_s=128, k_stride_b=2 * 4096 * 128)):       # an [B, Hkv, Smax, D] buffer
        assert _check(lib, _args(**ok)) == 0, ok
    for ok in (dict(), dict(max_seqlen_q=1, total_new=5), dict(kn_stride_b=0, vn_stride_b=0), dict(D=96), dict(dtype=1),
               dict(kn_stride_h=300 * 128, kn_stride_s=128, kn_stride_b=2 * 300 * 128)):      # [B, Hkv, Sq, D] rows
        assert _check(lib, _uargs(**ok)) == 0, ok
    for ok in (dict(), dict(_page=64), dict(_page=192), dict(_page=1024), dict(block_table_stride_b=40), dict(num_pages=1), dict(D=64),
               dict(Smax=128, block_table_stride_b=1), dict(cu_seqlens_q=0, total_new=1500)):
        assert _check(lib, _pargs(**ok)) == 0, ok


@pytest.mark.parametrize("max_seqlen_q", [1, 3, 300, 2048])
@pytest.mark.parametrize("B,Hkv,D", [(5, 2, 128), (64, 8, 128), (3, 1, 64), (2, 2, 96), (1, 3, 8)])
def test_kv_append_describe_counts_workgroups_from_host_shapes(lib, B, Hkv, D, max_seqlen_q):
    want = B * -(-max_seqlen_q * Hkv * (D // 8) // 256)
    for make in (_args, _pargs, _uargs):
        a = make(B=B, Hkv=Hkv, D=D, total_new=B * 4096, max_seqlen_q=max_seqlen_q)
        name, wgs = _capi.describe_kv_append(a)
        assert wgs == want
        # device-side inputs change neither the name nor the count
        a.cache_seqlens, a.k_new = 0x6000, 0x7000
        if make is not _uargs:
            a.cu_seqlens_q = 0xA000
        if make is _pargs:
            a.block_table = 0xB000
        assert _capi.describe_kv_append(a) == (name, wgs)
        # and neither do total_new or the cache's capacity
        a.total_new = B * 8192
        if make is not _pargs:
            a.Smax = 8192
        assert _capi.describe_kv_append(a) == (name, wgs)


def test_kv_append_describe_names(lib):
    assert _capi.describe_kv_append(_args())[0] == "kv_append_bf16_d128_varlen"
    assert _capi.describe_kv_append(_pargs())[0] == "kv_append_bf16_d128_varlen_paged"
    assert _capi.describe_kv_append(_uargs())[0] == "kv_append_bf16_d128"
    assert _capi.describe_kv_append(_pargs(cu_seqlens_q=0, total_new=1500, dtype=1, D=96))[0] == "kv_append_fp16_d96_paged"
    with pytest.raises(_capi.PfaError):
        _capi.describe_kv_append(_args(D=100))
    buf = C.create_string_buffer(8)                       # truncated, NUL terminated
    wgs = 5 * -(-300 * 2 * 16 // 256)
    assert lib.pfa_kv_append_describe(C.byref(_args()), buf, 8) == wgs and buf.value == b"kv_appe"
    assert lib.pfa_kv_append_describe(C.byref(_args()), None, 0) == wgs


def test_kv_append_refusals():
    bf = torch.bfloat16
    kn = torch.zeros(640, 2, 64, dtype=bf)
    k = torch.zeros(5, 2, 512, 64, dtype=bf)
    lens = torch.tensor([100, 300, 0, 20, 400], dtype=torch.int32)
    cu = torch.tensor([0, 1, 301, 301, 334, 591], dtype=torch.int32)
    ok = dict(cache_seqlens=lens, cu_seqlens_q=cu, max_seqlen_q=300)
    ops.kv_append(kn, kn.clone(), k, k.clone(), **ok)                                   # the CPU model takes it
    with pytest.raises(TypeError):
        ops.kv_append(kn, kn.clone(), k, k.clone(), cu_seqlens_q=cu, max_seqlen_q=300)  # cache_seqlens is required
    with pytest.raises(ValueError, match="3-D"):
        ops.kv_append(kn[None], kn[None].clone(), k, k.clone(), **ok)
    with pytest.raises(ValueError, match="3-D"):
        ops.kv_append(kn, kn.clone(), k[0], k[0].clone(), **ok)
    with pytest.raises(ValueError, match="4-D"):
        ops.kv_append(kn, kn.clone(), k, k.clone(), cache_seqlens=lens)                 # uniform rows are [B, Hkv, Sq, D]
    with pytest.raises(ValueError, match="shape mismatch"):
        ops.kv_append(kn, kn[:600].clone(), k, k.clone(), **ok)
    with pytest.raises(ValueError, match="cu_seqlens_q must be an int32 tensor"):
        ops.kv_append(kn, kn.clone(), k, k.clone(), **dict(ok, cu_seqlens_q=cu.long()))
    with pytest.raises(ValueError, match="cu_seqlens_q must be an int32 tensor"):
        ops.kv_append(kn, kn.clone(), k, k.clone(), **dict(ok, cu_seqlens_q=cu.tolist()))
    with pytest.raises(ValueError, match=r"cu_seqlens_q must be \[B \+ 1\]"):
        ops.kv_append(kn, kn.clone(), k, k.clone(), **dict(ok, cu_seqlens_q=cu[None]))
    with pytest.raises(ValueError, match="cu_seqlens_q must be contiguous"):
        ops.kv_append(kn, kn.clone(), k[:3], k[:3].clone(), cache_seqlens=lens[:3], cu_seqlens_q=cu[::2][:4], max_seqlen_q=300)
    with pytest.raises(ValueError, match="needs max_seqlen_q"):
        ops.kv_append(kn, kn.clone(), k, k.clone(), cache_seqlens=lens, cu_seqlens_q=cu)
    with pytest.raises(ValueError, match="must lie in 1 .. 640"):
        ops.kv_append(kn, kn.clone(), k, k.clone(), **dict(ok, max_seqlen_q=641))
    with pytest.raises(ValueError, match="must lie in 1 .. 640"):
        ops.kv_append(kn, kn.clone(), k, k.clone(), **dict(ok, max_seqlen_q=0))
    with pytest.raises(ValueError, match="shape mismatch"):                              # B = 4 from cu, a cache of 5
        ops.kv_append(kn, kn.clone(), k, k.clone(), **dict(ok, cu_seqlens_q=cu[:5]))
    with pytest.raises(ValueError, match="shape mismatch"):
        ops.kv_append(kn, kn.clone(), k, k[:, :1].clone(), **ok)
    with pytest.raises(ValueError, match="shape mismatch"):                              # another head dim
        ops.kv_append(kn[:, :, :32], kn[:, :, :32].clone(), k, k.clone(), **ok)
    with pytest.raises(ValueError, match="dtype"):
        ops.kv_append(kn.float(), kn.float(), k.float(), k.float(), **ok)
    with pytest.raises(ValueError, match="dtype"):
        ops.kv_append(kn, kn.clone(), k.half(), k.half(), **ok)
    with pytest.raises(ValueError, match=r"cache_seqlens must be a \[B\] tensor"):
        ops.kv_append(kn, kn.clone(), k, k.clone(), **dict(ok, cache_seqlens=lens[:4]))
    with pytest.raises(ValueError, match=r"cache_seqlens must be a \[B\] tensor"):
        ops.kv_append(kn, kn.clone(), k, k.clone(), **dict(ok, cache_seqlens=lens.tolist()))
    # uniform
    un = torch.zeros(5, 2, 7, 64, dtype=bf)
    ops.kv_append(un, un.clone(), k, k.clone(), cache_seqlens=lens)
    with pytest.raises(ValueError, match="every sequence brings k_new's 7 rows"):
        ops.kv_append(un, un.clone(), k, k.clone(), cache_seqlens=lens, max_seqlen_q=8)
    with pytest.raises(ValueError, match="shape mismatch"):
        ops.kv_append(un[:4], un[:4].clone(), k, k.clone(), cache_seqlens=lens[:4])
    # pools
    pool = torch.zeros(12, 2, 128, 64, dtype=bf)
    table = torch.zeros(5, 4, dtype=torch.int32)
    ops.kv_append(kn, kn.clone(), pool, pool.clone(), block_table=table, **ok)
    with pytest.raises(ValueError, match="shape mismatch"):
        ops.kv_append(kn, kn.clone(), pool, pool[:, :1].clone(), block_table=table, **ok)
    with pytest.raises(ValueError, match="multiple of 64"):
        ops.kv_append(kn, kn.clone(), pool[:, :, :96], pool[:, :, :96].clone(), block_table=table, **ok)
    with pytest.raises(ValueError, match="block_table must be an int32 tensor"):
        ops.kv_append(kn, kn.clone(), pool, pool.clone(), block_table=table.long(), **ok)
    with pytest.raises(ValueError, match=r"block_table must be \[B, max_pages\] with B = 5"):
        ops.kv_append(kn, kn.clone(), pool, pool.clone(), block_table=table[:4], **ok)
    with pytest.raises(ValueError, match="last dim must be contiguous"):
        ops.kv_append(kn, kn.clone(), pool, pool.clone(), block_table=torch.zeros(5, 8, dtype=torch.int32)[:, ::2], **ok)


def test_attention_calls_refuse_new_rows_without_lengths():
    """``k_new=`` needs ``cache_seqlens``: refused before anything else is looked at, CPU tensors included."""
    bf = torch.bfloat16
    q, k, kn = torch.zeros(2, 4, 1, 64, dtype=bf), torch.zeros(2, 2, 256, 64, dtype=bf), torch.zeros(2, 2, 1, 64, dtype=bf)
    with pytest.raises(ValueError, match="k_new / v_new need cache_seqlens"):
        ops.fa3_decode(q, k, k.clone(), k_new=kn, v_new=kn)
    # without new rows the calls are what they were: no CPU path
    with pytest.raises(ValueError, match="device tensors"):
        ops.fa3_decode(q, k, k.clone())
    import inspect
    for fn in (ops.fa3_decode, ops.fa3_prefill_cache, ops.fa3_prefill_varlen):
        sig = inspect.signature(fn).parameters
        assert sig["k_new"].default is None and sig["v_new"].default is None
        assert sig["k_new"].kind is inspect.Parameter.KEYWORD_ONLY


# ---- the CPU model against token-by-token loops ---------------------------------------------------------------------------------

def _rows(total, Hkv, D, seed, dtype=torch.bfloat16):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(total, Hkv, D, generator=g).to(dtype), torch.randn(total, Hkv, D, generator=g).to(dtype)


def _loop(k_new, v_new, k_cache, v_cache, lens, cu, maxq, table=None):
    """The issue's rule one token at a time on [.., Hkv, S, D]-shaped caches / pools; k_new [total, Hkv, D] (cu) or [B, Hkv, Sq, D]."""
    paged = table is not None
    ps, npages = k_cache.shape[2], k_cache.shape[0]
    Smax = table.shape[1] * ps if paged else k_cache.shape[2]
    total = k_new.shape[0]
    for b, n in enumerate(lens):
        len_b = min(max(n, 0), Smax)
        if cu is not None:
            s = min(max(cu[b], 0), total)
            e = min(max(cu[b + 1], s), total)
            sq = min(e - s, maxq)
        else:
            sq = maxq
        for i in range(sq):
            pos = len_b - sq + i
            if pos < 0:
                continue
            for new, cache in ((k_new, k_cache), (v_new, v_cache)):
                row = new[s + i] if cu is not None else new[b, :, i]
                if not paged:
                    cache[b, :, pos] = row
                else:
                    pg = int(table[b, pos // ps])
                    if 0 <= pg < npages:
                        cache[pg, :, pos % ps] = row


def _both(k_new, v_new, kc, vc, lens, cu=None, maxq=None, table=None):
    """Run the model and the loop on copies -> (model k, model v, loop k, loop v)."""
    mk, mv, lk, lv = kc.clone(), vc.clone(), kc.clone(), vc.clone()
    kw = {} if cu is None else dict(cu_seqlens_q=torch.tensor(cu, dtype=torch.int32), max_seqlen_q=maxq)
    ops.kv_append(k_new, v_new, mk, mv, cache_seqlens=torch.tensor(lens, dtype=torch.int32), block_table=table, **kw)
    _loop(k_new, v_new, lk, lv, lens, cu, maxq if cu is not None else k_new.shape[2], table)
    assert torch.equal(mk, lk) and torch.equal(mv, lv)
    return mk, mv


Q_LENS, KV_LENS, CU = [1, 300, 0, 33, 257], [777, 300, 512, 20, 1000], [0, 1, 301, 301, 334, 591]


def _ragged(D=64):
    kn, vn = _rows(640, 2, D, 11)
    kn[591:], vn[591:] = NAN, NAN                           # the spare rows behind cu[B]
    return kn, vn


def _written(cache, b, lo, hi):
    """Rows lo..hi-1 of sequence b of a [B, Hkv, Smax, D]-shaped cache as [n, Hkv, D]."""
    return cache[b, :, lo:hi].transpose(0, 1)


@pytest.mark.parametrize("token_major", [False, True])
def test_model_ragged_contiguous_in_both_layouts(token_major):
    kn, vn = _ragged()
    shape = (5, 1024, 2, 64) if token_major else (5, 2, 1024, 64)
    kc = torch.full(shape, SENTINEL, dtype=torch.bfloat16)
    vc = torch.full(shape, SENTINEL, dtype=torch.bfloat16)
    if token_major:
        kc, vc = kc.transpose(1, 2), vc.transpose(1, 2)     # the [B, Hkv, Smax, D]-shaped view of a flash-attn buffer
    mk, mv = _both(kn, vn, kc, vc, KV_LENS, CU, 300)
    assert not bool(torch.isnan(mk.float()).any()) and not bool(torch.isnan(mv.float()).any())
    # what landed where, said once more without the rule's own arithmetic
    assert torch.equal(_written(mk, 0, 776, 777), kn[0:1]) and torch.equal(_written(mv, 1, 0, 300), vn[1:301])
    assert torch.equal(_written(mk, 3, 0, 20), kn[301 + 13:334]) and torch.equal(_written(mk, 4, 743, 1000), kn[334:591])
    assert bool((mk[2] == SENTINEL).all())                  # the empty sequence
    written = 1 + 300 + 20 + 257
    assert int((mk != SENTINEL).any(-1).sum()) == written * 2 and int((mv != SENTINEL).any(-1).sum()) == written * 2


@pytest.mark.parametrize("page", [64, 256])
def test_model_ragged_paged_with_shuffled_pages(page):
    kn, vn = _ragged()
    per = 1024 // page
    n_pages = 5 * per + 3                                   # three pages nobody names
    perm = torch.randperm(n_pages, generator=torch.Generator().manual_seed(page))
    table = perm[:5 * per].reshape(5, per).to(torch.int32)
    kp = torch.full((n_pages, 2, page, 64), SENTINEL, dtype=torch.bfloat16)
    mk, mv = _both(kn, vn, kp, kp.clone(), KV_LENS, CU, 300, table)
    # the pools gathered through the table are the contiguous result
    kc = torch.full((5, 2, 1024, 64), SENTINEL, dtype=torch.bfloat16)
    ck, cv = _both(kn, vn, kc, kc.clone(), KV_LENS, CU, 300)
    for b in range(5):
        assert torch.equal(mk[table[b].long()].permute(1, 0, 2, 3).reshape(2, 1024, 64), ck[b])
        assert torch.equal(mv[table[b].long()].permute(1, 0, 2, 3).reshape(2, 1024, 64), cv[b])
    assert bool((mk[perm[5 * per:]] == SENTINEL).all()) and bool((mv[perm[5 * per:]] == SENTINEL).all())


def test_model_uniform_rows_and_views():
    g = torch.Generator().manual_seed(5)
    base = torch.randn(3, 70, 2, 64, generator=g).to(torch.bfloat16)          # [B, Sq, Hkv, D]
    kn_t, vn_t = base.transpose(1, 2), (base * 2).transpose(1, 2)             # transposed views
    kc = torch.full((3, 2, 256, 64), SENTINEL, dtype=torch.bfloat16)
    a = _both(kn_t, vn_t, kc, kc.clone(), [130, 70, 40])
    b = _both(kn_t.contiguous(), vn_t.contiguous(), kc, kc.clone(), [130, 70, 40])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(a[0][0, :, 60:130], kn_t[0]) and torch.equal(a[0][2, :, :40], kn_t[2, :, 30:])   # 30 leading rows dropped
    # paged, Sq 70 from a prior length of 60 with page 64: 4 / 64 / 2 rows over three pages
    table = torch.tensor([[5, 2, 7, 0], [1, 3, 4, 6], [8, 9, 10, 11]], dtype=torch.int32)
    kp = torch.full((12, 2, 64, 64), SENTINEL, dtype=torch.bfloat16)
    mk, _ = _both(kn_t, vn_t, kp, kp.clone(), [130, 130, 130], table=table)
    assert [int((mk[p] != SENTINEL).any(-1)[0].sum()) for p in (5, 2, 7, 0)] == [4, 64, 2, 0]
    one = torch.randn(3, 2, 1, 64, generator=g).to(torch.bfloat16)            # Sq 1
    mk, _ = _both(one, one.clone(), kp, kp.clone(), [1, 64, 65], table=table)
    assert torch.equal(mk[5, :, 0], one[0, :, 0]) and torch.equal(mk[1, :, 63], one[1, :, 0]) and torch.equal(mk[9, :, 0], one[2, :, 0])


def test_model_bad_page_ids_drop_exactly_their_rows():
    kn, vn = _rows(200, 2, 64, 21)
    table = torch.tensor([[3, -1, 1, 0], [2, 6, 5, 4]], dtype=torch.int32)    # 6 pages: -1 and 6 (= num_pages) are outside
    kp = torch.full((6, 2, 64, 64), SENTINEL, dtype=torch.bfloat16)
    # sequence 0: keys 50..149 (pages 3 | -1 | 1); sequence 1: keys 28..127 (pages 2 | 6)
    mk, mv = _both(kn, vn, kp, kp.clone(), [150, 128], [0, 100, 200], 100, table)
    assert torch.equal(mk[3, :, 50:].transpose(0, 1), kn[0:14]) and bool((mk[3, :, :50] == SENTINEL).all())
    assert torch.equal(mk[1, :, :22].transpose(0, 1), kn[78:100]) and bool((mk[1, :, 22:] == SENTINEL).all())
    assert torch.equal(mv[2, :, 28:].transpose(0, 1), vn[100:136]) and bool((mv[2, :, :28] == SENTINEL).all())
    for untouched in (0, 4, 5):                             # a clamp of -1 would have hit page 0, a clamp of 6 page 5
        assert bool((mk[untouched] == SENTINEL).all()) and bool((mv[untouched] == SENTINEL).all())


def test_model_clamps_cu_and_lengths_as_specified():
    kn, vn = _rows(64, 2, 64, 31)
    kc = torch.full((4, 2, 128, 64), SENTINEL, dtype=torch.bfloat16)
    # cu[0] < 0 -> 0; cu[2] < cu[1] -> an empty sequence at s_b = 20; cu[4] > total -> total; a length past Smax and a negative one
    mk, mv = _both(kn, vn, kc, kc.clone(), [10, 500, -3, 128], [-5, 20, 8, 40, 90], 64)
    assert torch.equal(mk[0, :, :10].transpose(0, 1), kn[10:20])                 # 20 rows into a length of 10: the last 10
    assert bool((mk[1] == SENTINEL).all()) and bool((mk[2] == SENTINEL).all())   # empty; 32 rows at length 0: all dropped
    assert torch.equal(mv[3, :, 104:128].transpose(0, 1), vn[40:64])             # 24 rows (40..63), length clamped to 128
    # sequence 1 again, with rows: s_b = 20, e_b = 40, length 500 clamped to Smax = 128
    mk, _ = _both(kn, vn, kc, kc.clone(), [10, 500, -3, 128], [-5, 20, 40, 40, 90], 64)
    assert torch.equal(mk[1, :, 108:128].transpose(0, 1), kn[20:40])


def test_model_rows_past_max_seqlen_q_are_left_alone():
    kn, vn = _rows(320, 2, 64, 41)
    kn[300:], vn[300:] = NAN, NAN
    kc = torch.full((1, 2, 512, 64), SENTINEL, dtype=torch.bfloat16)
    mk, mv = _both(kn, vn, kc, kc.clone(), [400], [0, 300], 256)
    assert torch.equal(mk[0, :, 144:400].transpose(0, 1), kn[:256]) and torch.equal(mv[0, :, 144:400].transpose(0, 1), vn[:256])
    assert bool((mk[0, :, :144] == SENTINEL).all()) and bool((mk[0, :, 400:] == SENTINEL).all())


# ---- PagedKVCache.advance + write_step ------------------------------------------------------------------------------------------

def _cache(**kw):
    from photonic_flash_attention_amd.integration.pytorch import PagedKVCache
    base = dict(num_pages=12, page_size=64, Hkv=2, D=64, dtype=torch.bfloat16, device="cpu", max_batch=4, max_pages_per_seq=6)
    base.update(kw)
    c = PagedKVCache(**base)
    c.k_pool.fill_(SENTINEL)
    c.v_pool.fill_(SENTINEL)
    return c


def _state(c):
    return (c.k_pool.clone(), c.v_pool.clone(), c.block_table.clone(), c.cache_seqlens.clone(),
            [c.pages(s) if c._live[s] else None for s in range(c.max_batch)], [c.length(s) if c._live[s] else None for s in range(c.max_batch)],
            c.free_pages)


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a[:4], b[:4])) and a[4:] == b[4:]


def test_advance_then_write_step_equals_append_varlen_until_the_pool_is_full():
    from photonic_flash_attention_amd.integration.pytorch import PagedCacheFull
    one, two = _cache(), _cache()
    for c in (one, two):
        for _ in range(3):
            c.allocate()
    steps = [([2, 0, 1], [100, 1, 65]), ([2, 0, 1], [0, 130, 27]), ([0, 1, 2], [64, 0, 0]), ([1], [37]), ([0, 1, 2], [1, 1, 1]),
             ([2, 1, 0], [0, 0, 0])]                            # page boundaries inside a chunk, empty chunks, exact fills, no rows
    for n, (slots, lens) in enumerate(steps):
        k, v = _rows(max(sum(lens), 1), 2, 64, 50 + n)
        k, v = k[:sum(lens)], v[:sum(lens)]
        one.append_varlen(slots, k, v, lens)
        two.advance(slots, lens)
        two.write_step(k, v, lens, slots)
        assert _same(_state(one), _state(two)), (slots, lens)
    # a device-style cu_seqlens_q with a bound, over all slots in order (slot 3 is not allocated: length 0, no rows)
    k, v = _rows(40, 2, 64, 70)
    one.append_varlen([0, 1, 2], k[:30], v[:30], [10, 0, 20])
    two.advance([0, 1, 2], [10, 0, 20])
    two.write_step(k, v, cu_seqlens_q=torch.tensor([0, 10, 10, 30, 30], dtype=torch.int32), max_seqlen_q=32)
    assert _same(_state(one), _state(two))
    # the pool runs out: both refuse, and nothing changes
    big_k, big_v = _rows(300, 2, 64, 71)
    for c in (one, two):
        assert c.free_pages == 3
    before = _state(two)
    with pytest.raises(PagedCacheFull):
        one.append_varlen([0, 1], big_k, big_v, [100, 200])
    with pytest.raises(PagedCacheFull):
        two.advance([0, 1], [100, 200])
    assert _same(_state(two), before) and _same(_state(one), before)
    with pytest.raises(PagedCacheFull):                         # more tokens than a table row holds
        two.advance([2], [6 * 64])
    assert _same(_state(two), before)
    with pytest.raises(ValueError, match="once per append"):
        two.advance([0, 0], [1, 1])
    with pytest.raises(ValueError, match="one non-negative token count per slot"):
        two.advance([0, 1], [1])
    with pytest.raises(ValueError, match="one non-negative token count per slot"):
        two.advance([0, 1], [1, -1])
    with pytest.raises(ValueError, match="not allocated"):
        two.advance([3], [1])
    assert _same(_state(two), before)
    with pytest.raises(ValueError, match="either q_lens"):
        two.write_step(k, v)
    with pytest.raises(ValueError, match="max_seqlen_q"):
        two.write_step(k, v, cu_seqlens_q=torch.tensor([0, 10, 10, 30, 30], dtype=torch.int32))
    with pytest.raises(ValueError, match="rows, k_new has 40"):
        two.write_step(k, v, [20, 20, 1, 0])
    assert _same(_state(two), before)


def test_write_step_hands_the_caches_own_table_and_lengths_to_ops(monkeypatch):
    from photonic_flash_attention_amd.integration.pytorch import paged_cache
    calls = []
    monkeypatch.setattr(paged_cache.ops, "kv_append", lambda *a, **kw: calls.append((a, kw)))
    c = _cache(num_pages=8, max_batch=3, max_pages_per_seq=4)
    for _ in range(3):
        c.allocate()
    k, v = _rows(40, 2, 64, 80)
    cu = torch.tensor([0, 10, 10, 30], dtype=torch.int32)
    c.write_step(k, v, cu_seqlens_q=cu, max_seqlen_q=32)
    (k_, v_, kc, vc), kw = calls.pop()
    assert k_ is k and v_ is v and kc.shape == (8, 2, 64, 64) and kc.data_ptr() == c.k_pool.data_ptr() and vc.data_ptr() == c.v_pool.data_ptr()
    assert kw["block_table"] is c.block_table and kw["cache_seqlens"] is c.cache_seqlens          # capturable: the cache's own tensors
    assert kw["cu_seqlens_q"] is cu and kw["max_seqlen_q"] == 32
    c.write_step(k, v, [5, 30], slots=[1, 2])
    kw = calls.pop()[1]
    assert kw["block_table"].data_ptr() == c.block_table[1:].data_ptr() and kw["cu_seqlens_q"].tolist() == [0, 5, 35] and kw["max_seqlen_q"] == 30
    c.write_step(k, v, [0, 0, 0])                                                                 # no rows: no launch
    assert not calls

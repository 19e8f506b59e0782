"""GPU tests of the rotary embedding fused into the KV-cache append (``ops.rope_append`` / ``pfa_rope_append``, the ``rotary_cos=,
rotary_sin=`` keywords of the three calls over a KV cache, ``PagedKVCache.write_step(q=, rotary_*=)``).

The kernel's arithmetic is fixed (operands widened to fp32, the two products and the add / subtract rounded separately, one rounding to
the dtype), so every comparison is ``torch.equal`` -- against the plain-torch model of the rule (``ops.rope_append`` on CPU tensors,
itself checked pair by pair in tests/test_rope_append_host.py) run on copies.  The comparison covers the WHOLE cache or pool and the
whole ``q_out``, all filled with a sentinel before the call, and every packed row no sequence owns holds NaN: a stray write, a missing
write and a read of a foreign row all show.

The ragged fixture is the one of tests/test_hip_kv_append.py (B 5, Hkv 2, Smax 1024, ``q_lens = [1, 300, 0, 33, 257]``, lengths after the
step ``[777, 300, 512, 20, 1000]``, 640 packed rows of which 49 are spare, ``max_seqlen_q = 300``) with H 4 query heads and tables of
1024 positions; sequence 3 (``len_b < Sq_b``) drops the K / V of its first 13 rows and still gets their Q.  The uniform one is B 3.

Only legal arguments and in-range device data ever reach the GPU; out-of-range page ids and malformed ``cu_seqlens_q`` are
exercised on the CPU model (tests/test_rope_append_host.py)."""

from __future__ import annotations

import functools

import pytest
import torch

from kvcache_testlib import NAN, device, i32

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
B, H, HKV, SMAX, TOTAL, MAXQ, MAX_POS = 5, 4, 2, 1024, 640, 300, 1024
Q_LENS = [1, 300, 0, 33, 257]
KV_LENS = [777, 300, 512, 20, 1000]
CU = [0, 1, 301, 301, 334, 591]
SHARED = 256
DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
STYLES = pytest.mark.parametrize("interleaved", [False, True], ids=["half", "interleaved"])


@functools.lru_cache(maxsize=None)
def _tables(R, max_pos=MAX_POS):
    """The standard tables, once per rot_dim: (cos, sin) on the CPU; never modified."""
    from photonic_flash_attention_amd import ops
    return ops.rotary_tables(max_pos, R)


def _rows(shape_of, seed, dtype, used=None):
    """Random Q, K and V rows (CPU) of the shapes ``shape_of(heads)``; rows at and past ``used`` of the first dim hold NaN."""
    g = torch.Generator().manual_seed(seed)
    out = [torch.randn(shape_of(h), generator=g).to(dtype) for h in (H, HKV, HKV)]
    if used is not None:
        for t in out:
            t[used:] = NAN
    return out


def _cpu(t):
    return t.cpu() if isinstance(t, torch.Tensor) else t


def _model(q, k_new, v_new, k_cache, v_cache, lens, cos, sin, table=None, **kw):
    """The CPU model on CPU copies of everything, q_out sentinel-filled -> (q_out or None, k, v)."""
    from photonic_flash_attention_amd import ops
    mk, mv = k_cache.cpu().clone(), v_cache.cpu().clone()
    mq = None if q is None else torch.full_like(q.cpu(), SENTINEL)
    ops.rope_append(k_new.cpu(), v_new.cpu(), mk, mv, cache_seqlens=lens.cpu(), rotary_cos=cos.cpu(), rotary_sin=sin.cpu(), q=_cpu(q), q_out=mq,
                    block_table=_cpu(table), **{n: _cpu(t) for n, t in kw.items()})
    return mq, mk, mv


def _run_and_compare(q, k_new, v_new, k_cache, v_cache, lens, cos, sin, table=None, **kw):
    """The kernel on the given device tensors against the model on copies: the whole cache or pool and the whole q_out."""
    from photonic_flash_attention_amd import ops
    mq, mk, mv = _model(q, k_new, v_new, k_cache, v_cache, lens, cos, sin, table, **kw)
    q_out = None if q is None else torch.full_like(q, SENTINEL)
    got = ops.rope_append(k_new, v_new, k_cache, v_cache, cache_seqlens=lens, rotary_cos=cos, rotary_sin=sin, q=q, q_out=q_out, block_table=table, **kw)
    torch.cuda.synchronize()
    assert got is q_out
    assert torch.equal(k_cache.cpu(), mk), "K differs from the model"
    assert torch.equal(v_cache.cpu(), mv), "V differs from the model"
    assert not bool(torch.isnan(k_cache.float()).any()) and not bool(torch.isnan(v_cache.float()).any()), "a row no sequence owns was read"
    if q is not None:
        assert torch.equal(q_out.cpu(), mq), "Q differs from the model"
        assert not bool(torch.isnan(q_out.float()).any()), "a row no sequence owns was read"
    return q_out, mq, mk, mv


def _shuffled_table(page, seed):
    """Block table [B, SMAX / page] over shuffled pages, sequences 0 and 4 sharing their first 256 keys' pages (no destination of
    the fixture falls there) -> (table, num_pages)."""
    per, shared = SMAX // page, SHARED // page
    n_pages = B * per - shared + 3                           # three pages nobody names
    perm = torch.randperm(n_pages, generator=torch.Generator().manual_seed(seed)).tolist()
    table, at = [], 0
    for b in range(B):
        own = per - shared if b == 4 else per
        table.append((table[0][:shared] if b == 4 else []) + perm[at:at + own])
        at += own
    return torch.tensor(table, dtype=torch.int32), n_pages


def _ragged_case(dtype, D, layout, seed):
    """The ragged fixture on the device -> (q, kn, vn, kc, vc, lens, cu, table)."""
    dev = device()
    q, kn, vn = (t.to(dev) for t in _rows(lambda h: (TOTAL, h, D), seed, dtype, used=CU[-1]))
    table = None
    if layout == "contiguous":
        kc = torch.full((B, HKV, SMAX, D), SENTINEL, dtype=dtype, device=dev)
    elif layout == "token-major":                            # a flash-attn [B, Smax, Hkv, D] buffer as a view
        kc = torch.full((B, SMAX, HKV, D), SENTINEL, dtype=dtype, device=dev).transpose(1, 2)
    else:
        page = int(layout[4:])
        table, n_pages = _shuffled_table(page, page + D)
        table = table.to(dev)
        kc = torch.full((n_pages, page, HKV, D), SENTINEL, dtype=dtype, device=dev).transpose(1, 2)
    return q, kn, vn, kc, torch.full_like(kc, SENTINEL), i32(KV_LENS), i32(CU), table


@pytest.mark.parametrize("layout", ["contiguous", "token-major", "page64", "page256"])
@STYLES
@pytest.mark.parametrize("D", [64, 128])
@DTYPES
def test_ragged_rope_append_equals_the_model(dtype, D, interleaved, layout):
    from photonic_flash_attention_amd import ops
    q, kn, vn, kc, vc, lens, cu, table = _ragged_case(dtype, D, layout, 100 + D)
    cos, sin = (t.to(device()) for t in _tables(D))
    kw = dict(cu_seqlens_q=cu, max_seqlen_q=MAXQ, rotary_interleaved=interleaved)
    q_out, mq, mk, mv = _run_and_compare(q, kn, vn, kc, vc, lens, cos, sin, table, **kw)
    written = 1 + 300 + 20 + 257                             # sequence 3 drops the K / V of 13 of its 33 rows ...
    assert int((mk != SENTINEL).any(-1).sum()) == written * HKV and int((mv != SENTINEL).any(-1).sum()) == written * HKV
    assert int((mq != SENTINEL).any(-1).sum()) == CU[-1] * H  # ... and none of their Q
    # a second launch is idempotent (out of place)
    again = torch.full_like(q, SENTINEL)
    ops.rope_append(kn, vn, kc, vc, cache_seqlens=lens, rotary_cos=cos, rotary_sin=sin, q=q, q_out=again, block_table=table, **kw)
    torch.cuda.synchronize()
    assert torch.equal(kc.cpu(), mk) and torch.equal(vc.cpu(), mv) and torch.equal(again, q_out)


@pytest.mark.parametrize("layout", ["contiguous", "page64"])
@STYLES
@pytest.mark.parametrize("D,R", [(128, 32), (64, 16)])
@DTYPES
def test_partial_rotation_copies_the_rest_of_the_head(dtype, D, R, interleaved, layout):
    q, kn, vn, kc, vc, lens, cu, table = _ragged_case(dtype, D, layout, 200 + R)
    cos, sin = (t.to(device()) for t in _tables(R))
    q_out, mq, mk, _ = _run_and_compare(q, kn, vn, kc, vc, lens, cos, sin, table, cu_seqlens_q=cu, max_seqlen_q=MAXQ, rotary_interleaved=interleaved)
    assert torch.equal(q_out[:CU[-1], :, R:], q[:CU[-1], :, R:]) and not torch.equal(q_out[:CU[-1], :, :R], q[:CU[-1], :, :R])


@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
@STYLES
@pytest.mark.parametrize("Sq,lens", [(1, [1, 64, 130]), (5, [130, 5, 3])], ids=["sq1", "sq5"])
def test_uniform_rope_append_on_views_of_a_fused_projection(Sq, lens, interleaved, paged):
    """B 3; q, k and v are strided views cut from one [B, Sq, (H + 2 Hkv) D] projection.  Sq 5 to a length of 130 with pages of 64
    crosses a page (keys 125 .. 129); 5 rows into a length of 3 drop the K / V of the first two."""
    dev, dtype, D = device(), torch.bfloat16, 64
    fused = torch.randn(3, Sq, (H + 2 * HKV) * D, generator=torch.Generator().manual_seed(7 + Sq)).to(dtype).to(dev)
    q = fused[..., :H * D].view(3, Sq, H, D).transpose(1, 2)
    kn = fused[..., H * D:(H + HKV) * D].view(3, Sq, HKV, D).transpose(1, 2)
    vn = fused[..., (H + HKV) * D:].view(3, Sq, HKV, D).transpose(1, 2)
    assert q.shape == (3, H, Sq, D) and kn.shape == vn.shape == (3, HKV, Sq, D) and not kn.is_contiguous()
    cos, sin = (t.to(dev) for t in _tables(D, 256))
    keep = fused.clone()
    if paged:
        table = i32([[5, 2, 7, 0], [1, 3, 4, 6], [8, 9, 10, 11]])
        kc = torch.full((13, 64, HKV, D), SENTINEL, dtype=dtype, device=dev).transpose(1, 2)
    else:
        table = None
        kc = torch.full((3, HKV, 256, D), SENTINEL, dtype=dtype, device=dev)
    _, _, mk, _ = _run_and_compare(q, kn, vn, kc, torch.full_like(kc, SENTINEL), i32(lens), cos, sin, table, rotary_interleaved=interleaved)
    assert torch.equal(fused, keep)                          # the inputs are only read
    assert int((mk != SENTINEL).any(-1).sum()) == sum(min(Sq, n) for n in lens) * HKV
    # without q_out the fresh buffer has the layout the attention calls prefer and the same bits
    from photonic_flash_attention_amd import ops
    kc2 = torch.full_like(kc, SENTINEL)
    fresh = ops.rope_append(kn, vn, kc2, torch.full_like(kc, SENTINEL), cache_seqlens=i32(lens), rotary_cos=cos, rotary_sin=sin, q=q,
                            rotary_interleaved=interleaved, block_table=table)
    torch.cuda.synchronize()
    assert fresh.shape == q.shape and fresh.transpose(1, 2).is_contiguous()
    mq = _model(q, kn, vn, kc2, kc2, i32(lens), cos, sin, table, rotary_interleaved=interleaved)[0]
    assert torch.equal(fresh.cpu(), mq)


@STYLES
@DTYPES
def test_in_place_equals_out_of_place_and_kv_only(dtype, interleaved):
    from photonic_flash_attention_amd import ops
    D = 128
    q, kn, vn, kc, vc, lens, cu, table = _ragged_case(dtype, D, "page64", 300)
    cos, sin = (t.to(device()) for t in _tables(D))
    kw = dict(cu_seqlens_q=cu, max_seqlen_q=MAXQ, rotary_interleaved=interleaved)
    q_out, _, mk, mv = _run_and_compare(q, kn, vn, kc, vc, lens, cos, sin, table, **kw)
    # in place
    qi, kc2, vc2 = q.clone(), torch.full_like(kc, SENTINEL), torch.full_like(kc, SENTINEL)
    assert ops.rope_append(kn, vn, kc2, vc2, cache_seqlens=lens, rotary_cos=cos, rotary_sin=sin, q=qi, q_out=qi, block_table=table, **kw) is qi
    torch.cuda.synchronize()
    assert torch.equal(qi[:CU[-1]], q_out[:CU[-1]]) and bool(torch.isnan(qi[CU[-1]:].float()).all())   # the spare rows stay as they were
    assert torch.equal(kc2.cpu(), mk) and torch.equal(vc2.cpu(), mv)
    # K / V only
    kc3, vc3 = torch.full_like(kc, SENTINEL), torch.full_like(kc, SENTINEL)
    assert _run_and_compare(None, kn, vn, kc3, vc3, lens, cos, sin, table, **kw)[0] is None
    assert torch.equal(kc3.cpu(), mk) and torch.equal(vc3.cpu(), mv)


@pytest.mark.parametrize("layout", ["contiguous", "page64"])
@STYLES
def test_pos_offsets_in_range_and_clamped_at_both_ends(interleaved, layout):
    """Offsets [100, -400, 7, 5000, -700]: sequence 0 at 876, sequence 2 brings no rows, sequence 4 at 43 .. 299; every row of sequence 1
    (keys 0 .. 299) is clamped to table row 0, every row of sequence 3 to row max_pos - 1.  Defined behaviour: no address leaves the
    tables (they are the whole allocation)."""
    dtype, D, R = torch.bfloat16, 64, 32
    q, kn, vn, kc, vc, lens, cu, table = _ragged_case(dtype, D, layout, 400)
    cos, sin = (t.to(device()) for t in _tables(R))
    offs = i32([100, -400, 7, 5000, -700])
    kw = dict(cu_seqlens_q=cu, max_seqlen_q=MAXQ, rotary_interleaved=interleaved)
    q_out = _run_and_compare(q, kn, vn, kc, vc, lens, cos, sin, table, pos_offsets=offs, **kw)[0]
    no_offs = _run_and_compare(q, kn, vn, torch.full_like(kc, SENTINEL), torch.full_like(kc, SENTINEL), lens, cos, sin, table, **kw)[0]
    assert not torch.equal(q_out[:1], no_offs[:1])
    # position 0 is the identity (cos 1, sin 0): sequence 1's Q comes back as it went in
    assert torch.equal(q_out[1:301], q[1:301])


@pytest.mark.parametrize("layout", ["contiguous", "page256"])
@STYLES
def test_identity_tables_equal_kv_append(interleaved, layout):
    from photonic_flash_attention_amd import ops
    dev, dtype, D = device(), torch.float16, 128
    q, kn, vn, kc, vc, lens, cu, table = _ragged_case(dtype, D, layout, 500)
    cos, sin = torch.ones(MAX_POS, D // 2, device=dev), torch.zeros(MAX_POS, D // 2, device=dev)
    q_out = _run_and_compare(q, kn, vn, kc, vc, lens, cos, sin, table, cu_seqlens_q=cu, max_seqlen_q=MAXQ, rotary_interleaved=interleaved)[0]
    ak, av = torch.full_like(kc, SENTINEL), torch.full_like(kc, SENTINEL)
    ops.kv_append(kn, vn, ak, av, cache_seqlens=lens, cu_seqlens_q=cu, max_seqlen_q=MAXQ, block_table=table)
    torch.cuda.synchronize()
    assert torch.equal(kc, ak) and torch.equal(vc, av) and torch.equal(q_out[:CU[-1]], q[:CU[-1]])


# ---- the rotary keywords of the attention calls -------------------------------------------------------------------------------------

FB, FSMAX, FD = 2, 256, 64


def _paged_copy(kc, vc, ids):
    """The contiguous caches [FB, Hkv, 256, D] as pools of 64-key pages under the table ``ids`` (one page unnamed)."""
    kp = torch.full((9, HKV, 64, FD), NAN, dtype=kc.dtype, device=kc.device)
    vp = torch.full_like(kp, NAN)
    for b in range(FB):
        for p, pg in enumerate(ids[b]):
            kp[pg], vp[pg] = kc[b, :, 64 * p:64 * p + 64], vc[b, :, 64 * p:64 * p + 64]
    return kp, vp


def _end_to_end(fn, q, kn, vn, kc, vc, lens, table, interleaved, offs, **ragged):
    """``fn(k_new=, v_new=, rotary_*=)`` against ``ops.rope_append`` + ``fn`` on the rotated Q -> (o, q_rot), the owned rows to check."""
    from photonic_flash_attention_amd import ops
    cos, sin = (t.to(device()) for t in _tables(FD, 256))
    rot = dict(rotary_cos=cos, rotary_sin=sin, rotary_interleaved=interleaved, pos_offsets=offs)
    rk, rv, q_before = kc.clone(), vc.clone(), q.clone()
    q_rot = ops.rope_append(kn, vn, rk, rv, cache_seqlens=lens, q=q, block_table=table, **rot, **ragged)
    o_ref, lse_ref = fn(q_rot, rk, rv, cache_seqlens=lens, block_table=table, return_lse=True, **ragged)
    o, lse = fn(q, kc, vc, cache_seqlens=lens, block_table=table, return_lse=True, k_new=kn, v_new=vn, **rot, **ragged)
    torch.cuda.synchronize()
    assert torch.equal(q.view(torch.int16), q_before.view(torch.int16)), "the caller's q was modified"
    assert torch.equal(kc.view(torch.int16), rk.view(torch.int16)) and torch.equal(vc.view(torch.int16), rv.view(torch.int16))   # NaN tails: compare bits
    return o, o_ref, lse, lse_ref, q_rot


@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
@STYLES
@pytest.mark.parametrize("entry,Sq", [("fa3_decode", 1), ("fa3_decode", 4), ("fa3_prefill_cache", 70)])
def test_uniform_attention_calls_rotate_and_append_first(entry, Sq, interleaved, paged):
    from photonic_flash_attention_amd import ops
    dev, dtype, lens = device(), torch.bfloat16, [100, 256]
    g = torch.Generator().manual_seed(600 + Sq)
    kc, vc = (torch.randn(FB, HKV, FSMAX, FD, generator=g).to(dtype).to(dev) for _ in range(2))
    for b in range(FB):                                      # valid keys below len_b - Sq, NaN from there on (the step's own rows included)
        kc[b, :, lens[b] - Sq:], vc[b, :, lens[b] - Sq:] = NAN, NAN
    q, kn, vn = (t.to(dev) for t in _rows(lambda h: (FB, h, Sq, FD), 601 + Sq, dtype))
    table = None
    if paged:
        ids = [[7, 2, 5, 0], [3, 8, 1, 6]]
        table = i32(ids)
        kc, vc = _paged_copy(kc, vc, ids)
    o, o_ref, lse, lse_ref, q_rot = _end_to_end(getattr(ops, entry), q, kn, vn, kc, vc, i32(lens), table, interleaved, i32([3, -20]))
    assert bool(torch.isfinite(o_ref.float()).all()) and not torch.equal(q_rot, q)
    assert torch.equal(o, o_ref) and torch.equal(lse, lse_ref)


@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
@STYLES
def test_ragged_attention_call_rotates_and_appends_first(interleaved, paged):
    """``fa3_prefill_varlen`` on the ragged fixture (D 64): caches of finite keys, the step's rows written by the call itself."""
    from photonic_flash_attention_amd import ops
    dev, dtype = device(), torch.bfloat16
    q, kn, vn, kc, vc, lens, cu, table = _ragged_case(dtype, FD, "page64" if paged else "contiguous", 700)
    g = torch.Generator(device="cpu").manual_seed(701)
    kc.copy_(torch.randn(kc.shape, generator=g).to(dtype))
    vc.copy_(torch.randn(vc.shape, generator=g).to(dtype))
    cos, sin = (t.to(dev) for t in _tables(FD))
    rot = dict(rotary_cos=cos, rotary_sin=sin, rotary_interleaved=interleaved)
    kw = dict(cu_seqlens_q=cu, max_seqlen_q=MAXQ, cache_seqlens=lens, block_table=table)
    rk, rv, q_before = kc.clone(), vc.clone(), q.clone()
    q_rot = ops.rope_append(kn, vn, rk, rv, q=q, **rot, **kw)
    o_ref, lse_ref = ops.fa3_prefill_varlen(q_rot, rk, rv, return_lse=True, **kw)
    o, lse = ops.fa3_prefill_varlen(q, kc, vc, return_lse=True, k_new=kn, v_new=vn, **rot, **kw)
    torch.cuda.synchronize()
    n = CU[-1]
    assert torch.equal(q.view(torch.int16), q_before.view(torch.int16)), "the caller's q was modified"
    assert torch.equal(kc, rk) and torch.equal(vc, rv)
    assert bool(torch.isfinite(o_ref[:n].float()).all())
    assert torch.equal(o[:n], o_ref[:n]) and torch.equal(lse[:, :n], lse_ref[:, :n])
    assert bool((o[301:301 + 13] == 0).all())               # sequence 3's rows in front of key 0


# ---- a whole step in a graph ----------------------------------------------------------------------------------------------------

def test_whole_rotary_step_replays_in_a_graph():
    """``write_step(q=, rotary_*=)`` + ``prefill_varlen`` captured once (a single chain on one stream) over a ``PagedKVCache`` with pages
    reserved ahead; three replays with different ``q_lens``, ``advance`` and in-place refreshes of ``cu_seqlens_q``, ``pos_offsets``, the
    inputs and the rotary tables in between, against an eager twin."""
    from photonic_flash_attention_amd import ops
    from photonic_flash_attention_amd.integration.pytorch import PagedKVCache
    dev, dtype, D, rows, bound = device(), torch.bfloat16, 64, 160, 130

    def make():
        c = PagedKVCache(num_pages=14, page_size=64, Hkv=HKV, D=D, dtype=dtype, device=dev, max_batch=3, max_pages_per_seq=4)
        c.k_pool.fill_(SENTINEL)
        c.v_pool.fill_(SENTINEL)
        for _ in range(3):
            c.reserve(c.allocate(), 256)
        return c

    cache, twin = make(), make()
    k_s = torch.full((rows, HKV, D), NAN, dtype=dtype, device=dev)
    v_s = torch.full_like(k_s, NAN)
    q_s = torch.zeros(rows, H, D, dtype=dtype, device=dev)
    o_s = torch.zeros(rows, H, D, dtype=dtype, device=dev)
    cu = torch.zeros(4, dtype=torch.int32, device=dev)       # no rows while warming up and capturing
    offs = torch.zeros(3, dtype=torch.int32, device=dev)
    cos, sin = (t.to(dev) for t in _tables(D, 512))
    rot = dict(rotary_cos=cos, rotary_sin=sin, pos_offsets=offs)

    def step():
        q_rot = cache.write_step(k_s, v_s, cu_seqlens_q=cu, max_seqlen_q=bound, q=q_s, **rot)
        return cache.prefill_varlen(q_rot, cu_seqlens_q=cu, max_seqlen_q=bound, out=o_s)[0]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert bool((cache.k_pool == SENTINEL).all())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o_g = step()

    g = torch.Generator().manual_seed(77)
    for n_step, (q_lens, step_offs) in enumerate((([5, 0, 70], [0, 0, 0]), ([1, 1, 1], [10, -2, 300]), ([0, 130, 2], [7, 100, 0]))):
        n = sum(q_lens)
        k, v, q = (torch.randn(n, heads, D, generator=g).to(dtype).to(dev) for heads in (HKV, HKV, H))
        k_s.fill_(NAN), v_s.fill_(NAN), o_s.fill_(SENTINEL)
        k_s[:n], v_s[:n], q_s[:n] = k, v, q
        at = [0]
        for x in q_lens:
            at.append(at[-1] + x)
        cu.copy_(torch.tensor(at, dtype=torch.int32))
        offs.copy_(torch.tensor(step_offs, dtype=torch.int32))
        if n_step == 2:                                      # other tables in the same storage
            c2, s2 = ops.rotary_tables(512, D, base=500000.0)
            cos.copy_(c2), sin.copy_(s2)
        cache.advance([0, 1, 2], q_lens)
        graph.replay()
        torch.cuda.synchronize()
        twin.advance([0, 1, 2], q_lens)
        q_e = torch.zeros_like(q_s)                          # the bound needs that many packed rows
        q_e[:n] = twin.write_step(k, v, q_lens, q=q, **rot)
        o_e = twin.prefill_varlen(q_e, q_lens, max_seqlen_q=bound)[0]
        torch.cuda.synchronize()
        assert torch.equal(cache.k_pool, twin.k_pool) and torch.equal(cache.v_pool, twin.v_pool), q_lens
        assert torch.equal(cache.cache_seqlens, twin.cache_seqlens) and torch.equal(cache.block_table, twin.block_table)
        assert bool(torch.isfinite(o_g[:n].float()).all()) and torch.equal(o_g[:n], o_e[:n]), q_lens
        assert bool((o_g[n:] == SENTINEL).all())
        assert not bool(torch.isnan(cache.k_pool.float()).any())
    assert [cache.length(s) for s in range(3)] == [6, 131, 73]

"""GPU tests of the device-side KV-cache append (``ops.kv_append`` / ``pfa_kv_append``, the ``k_new=, v_new=`` form of the three calls
over a KV cache, ``PagedKVCache.advance`` / ``write_step``).

A copy is bit-exact, so every comparison is ``torch.equal`` -- against the plain-torch model of the rule (``ops.kv_append`` on CPU
tensors, itself checked token by token in tests/test_kv_append_host.py) run on copies of the same cache or pool.  Every cache or
pool holds a sentinel before the call, and every packed row no sequence owns holds NaN: a stray write, a missing write and a read
of a foreign row all show in the whole-tensor comparison.

The ragged fixture is the one of tests/test_hip_prefill_varlen.py: B 5, Hkv 2, Smax 1024, ``q_lens = [1, 300, 0, 33, 257]``, lengths
after the step ``[777, 300, 512, 20, 1000]``, 640 packed rows (49 spare), ``max_seqlen_q = 300``: one row landing mid-page,
``len_b == Sq_b`` from key 0, an empty sequence, ``len_b < Sq_b`` (13 rows dropped, 20 written) and 257 rows crossing four 64-key
pages.  No destination falls into the first 256 keys of sequences 0 and 4 (776; 743 .. 999), so the paged layouts let the two share
those pages, as the sibling tests do.

Only legal arguments and in-range device data ever reach the GPU; out-of-range page ids and malformed ``cu_seqlens_q`` are
exercised on the CPU model (tests/test_kv_append_host.py)."""

from __future__ import annotations

import pytest
import torch

from kvcache_testlib import NAN, device, i32

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
B, HKV, SMAX, TOTAL, MAXQ = 5, 2, 1024, 640, 300
Q_LENS = [1, 300, 0, 33, 257]
KV_LENS = [777, 300, 512, 20, 1000]
CU = [0, 1, 301, 301, 334, 591]
SHARED = 256


def _rows(shape, seed, dtype, used=None):
    """Random K and V rows (CPU); rows at and past ``used`` of the first dim hold NaN."""
    g = torch.Generator().manual_seed(seed)
    k, v = torch.randn(shape, generator=g).to(dtype), torch.randn(shape, generator=g).to(dtype)
    if used is not None:
        k[used:], v[used:] = NAN, NAN
    return k, v


def _model(k_new, v_new, k_cache, v_cache, lens, table=None, **kw):
    """The CPU model on CPU copies of everything -> (k, v)."""
    from photonic_flash_attention_amd import ops
    mk, mv = k_cache.cpu().clone(), v_cache.cpu().clone()
    kw = {n: (t.cpu() if isinstance(t, torch.Tensor) else t) for n, t in kw.items()}
    ops.kv_append(k_new.cpu(), v_new.cpu(), mk, mv, cache_seqlens=lens.cpu(), block_table=None if table is None else table.cpu(), **kw)
    return mk, mv


def _run_and_compare(k_new, v_new, k_cache, v_cache, lens, table=None, **kw):
    """The kernel on the given device tensors against the model on copies: the WHOLE cache or pool, sentinels included."""
    from photonic_flash_attention_amd import ops
    mk, mv = _model(k_new, v_new, k_cache, v_cache, lens, table, **kw)
    assert ops.kv_append(k_new, v_new, k_cache, v_cache, cache_seqlens=lens, block_table=table, **kw) is None
    torch.cuda.synchronize()
    assert torch.equal(k_cache.cpu(), mk), "K differs from the model"
    assert torch.equal(v_cache.cpu(), mv), "V differs from the model"
    assert not bool(torch.isnan(k_cache.float()).any()) and not bool(torch.isnan(v_cache.float()).any()), "a row no sequence owns was read"
    return mk, mv


def _shuffled_table(page, seed):
    """Block table [B, SMAX / page] over shuffled pages, sequences 0 and 4 sharing their first 256 keys' pages -> (table, num_pages)."""
    per, shared = SMAX // page, SHARED // page
    n_pages = B * per - shared + 3                           # three pages nobody names
    perm = torch.randperm(n_pages, generator=torch.Generator().manual_seed(seed)).tolist()
    table, at = [], 0
    for b in range(B):
        own = per - shared if b == 4 else per
        table.append((table[0][:shared] if b == 4 else []) + perm[at:at + own])
        at += own
    return torch.tensor(table, dtype=torch.int32), n_pages


@pytest.mark.parametrize("layout", ["contiguous", "token-major", "page64", "page256"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_ragged_append_equals_the_model(dtype, D, layout):
    dev = device()
    kn, vn = (t.to(dev) for t in _rows((TOTAL, HKV, D), 100 + D, dtype, used=CU[-1]))
    lens, cu, table = i32(KV_LENS), i32(CU), None
    if layout == "contiguous":
        kc = torch.full((B, HKV, SMAX, D), SENTINEL, dtype=dtype, device=dev)
    elif layout == "token-major":                            # a flash-attn [B, Smax, Hkv, D] buffer as a view
        kc = torch.full((B, SMAX, HKV, D), SENTINEL, dtype=dtype, device=dev).transpose(1, 2)
    else:
        page = int(layout[4:])
        table, n_pages = _shuffled_table(page, page + D)
        table = table.to(dev)
        kc = torch.full((n_pages, page, HKV, D), SENTINEL, dtype=dtype, device=dev).transpose(1, 2)
    vc = torch.full_like(kc, SENTINEL)
    assert vc.stride() == kc.stride()
    mk, mv = _run_and_compare(kn, vn, kc, vc, lens, table, cu_seqlens_q=cu, max_seqlen_q=MAXQ)
    written = 1 + 300 + 20 + 257                             # sequence 3 drops 13 of its 33 rows
    assert int((mk != SENTINEL).any(-1).sum()) == written * HKV and int((mv != SENTINEL).any(-1).sum()) == written * HKV
    # a replay is idempotent
    from photonic_flash_attention_amd import ops
    ops.kv_append(kn, vn, kc, vc, cache_seqlens=lens, cu_seqlens_q=cu, max_seqlen_q=MAXQ, block_table=table)
    torch.cuda.synchronize()
    assert torch.equal(kc.cpu(), mk) and torch.equal(vc.cpu(), mv)


@pytest.mark.parametrize("view", ["bhsd", "transposed"])
@pytest.mark.parametrize("Sq,lens,D", [(1, [1, 64, 130], 64), (70, [130, 70, 40], 64), (70, [130, 256, 71], 96)], ids=["sq1", "sq70", "sq70-d96"])
def test_uniform_append_equals_the_model(Sq, lens, D, view):
    """B 3.  Sq 70 to a length of 130 with pages of 64 splits sequence 0's rows 4 / 64 / 2 over three pages; 70 rows into a length of
    40 drop the first 30; D 96 is a head dim the attention kernels do not take and the copy does."""
    dev, dtype = device(), torch.bfloat16
    if view == "bhsd":
        kn, vn = (t.to(dev) for t in _rows((3, HKV, Sq, D), 7 + Sq + D, dtype))
    else:
        kn, vn = (t.to(dev).transpose(1, 2) for t in _rows((3, Sq, HKV, D), 7 + Sq + D, dtype))
    assert kn.shape == (3, HKV, Sq, D)
    kc = torch.full((3, HKV, 256, D), SENTINEL, dtype=dtype, device=dev)
    _run_and_compare(kn, vn, kc, torch.full_like(kc, SENTINEL), i32(lens))
    table = i32([[5, 2, 7, 0], [1, 3, 4, 6], [8, 9, 10, 11]])
    kp = torch.full((13, 64, HKV, D), SENTINEL, dtype=dtype, device=dev).transpose(1, 2)
    mk, _ = _run_and_compare(kn, vn, kp, torch.full_like(kp, SENTINEL), i32(lens), table)
    if Sq == 70 and lens[0] == 130:
        assert [int((mk[p] != SENTINEL).any(-1)[0].sum()) for p in (5, 2, 7, 0)] == [4, 64, 2, 0]
    assert bool((mk[12] == SENTINEL).all())


@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
def test_rows_past_max_seqlen_q_are_neither_read_nor_written(paged):
    """300 rows with max_seqlen_q = 256: the first 256 land at len_b - 256 + i, where the attention call of that bound looks for them."""
    dev, dtype, D = device(), torch.bfloat16, 64
    kn, vn = (t.to(dev) for t in _rows((320, HKV, D), 55, dtype, used=300))
    kn[256:300], vn[256:300] = NAN, NAN                      # owned by the sequence, but past the bound
    lens, cu = i32([400]), i32([0, 300])
    if paged:
        table = i32([[6, 1, 4, 3, 0, 2, 7, 5]])
        kc = torch.full((9, 64, HKV, D), SENTINEL, dtype=dtype, device=dev).transpose(1, 2)
    else:
        table = None
        kc = torch.full((1, HKV, 512, D), SENTINEL, dtype=dtype, device=dev)
    mk, mv = _run_and_compare(kn, vn, kc, torch.full_like(kc, SENTINEL), lens, table, cu_seqlens_q=cu, max_seqlen_q=256)
    assert int((mk != SENTINEL).any(-1).sum()) == 256 * HKV
    if not paged:
        assert torch.equal(mk[0, :, 144:400].transpose(0, 1), kn[:256].cpu()) and torch.equal(mv[0, :, 144:400].transpose(0, 1), vn[:256].cpu())


# ---- the k_new=, v_new= form of the attention calls -----------------------------------------------------------------------------

FB, FH, FSMAX, FD = 2, 4, 256, 64


def _fused_fixture(sq_of, lens, seed):
    """Contiguous caches [2, Hkv, 256, D]: valid keys below ``len_b - Sq_b``, NaN from there on (the step's own rows included)."""
    dev, dtype = device(), torch.bfloat16
    kc, vc = (t.to(dev) for t in _rows((FB, HKV, FSMAX, FD), seed, dtype))
    for b in range(FB):
        kc[b, :, lens[b] - sq_of[b]:] = NAN
        vc[b, :, lens[b] - sq_of[b]:] = NAN
    return kc, vc


@pytest.mark.parametrize("entry,Sq", [("fa3_decode", 1), ("fa3_decode", 3), ("fa3_prefill_cache", 40)])
def test_uniform_attention_calls_append_first(entry, Sq):
    from photonic_flash_attention_amd import ops
    dev, dtype, lens = device(), torch.bfloat16, [100, 256]
    fn = getattr(ops, entry)
    kc, vc = _fused_fixture([Sq, Sq], lens, 300 + Sq)
    kn, vn = (t.to(dev) for t in _rows((FB, HKV, Sq, FD), 301 + Sq, dtype))
    q = torch.randn(FB, FH, Sq, FD, generator=torch.Generator().manual_seed(302)).to(dtype).to(dev)
    rk, rv = kc.clone(), vc.clone()
    for b in range(FB):                                      # the rows written with torch indexing, then the call as it was
        rk[b, :, lens[b] - Sq:lens[b]] = kn[b]
        rv[b, :, lens[b] - Sq:lens[b]] = vn[b]
    o_ref, lse_ref = fn(q, rk, rv, cache_seqlens=i32(lens), return_lse=True)
    o, lse = fn(q, kc, vc, cache_seqlens=i32(lens), return_lse=True, k_new=kn, v_new=vn)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(o_ref.float()).all())
    assert torch.equal(o, o_ref) and torch.equal(lse, lse_ref)
    assert torch.equal(kc.view(torch.int16), rk.view(torch.int16)) and torch.equal(vc.view(torch.int16), rv.view(torch.int16))   # NaN tails: compare bits
    with pytest.raises(ValueError, match="k_new / v_new need cache_seqlens"):
        fn(q, kc, vc, k_new=kn, v_new=vn)
    with pytest.raises(ValueError, match="go together"):
        fn(q, kc, vc, cache_seqlens=i32(lens), k_new=kn)


@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
def test_ragged_attention_call_appends_first(paged):
    from photonic_flash_attention_amd import ops
    dev, dtype = device(), torch.bfloat16
    q_lens, lens, cu = [3, 50], [100, 256], [0, 3, 53]
    kc, vc = _fused_fixture(q_lens, lens, 400)
    kn, vn = (t.to(dev) for t in _rows((64, HKV, FD), 401, dtype, used=53))
    q = torch.randn(64, FH, FD, generator=torch.Generator().manual_seed(402)).to(dtype).to(dev)
    table = None
    if paged:                                                # the same keys in a pool of 64-key pages, shuffled, one page unnamed
        ids = [[7, 2, 5, 0], [3, 8, 1, 6]]
        table = i32(ids)
        kp = torch.full((9, HKV, 64, FD), NAN, dtype=dtype, device=dev)
        vp = torch.full_like(kp, NAN)
        for b in range(FB):
            for p, pg in enumerate(ids[b]):
                kp[pg], vp[pg] = kc[b, :, 64 * p:64 * p + 64], vc[b, :, 64 * p:64 * p + 64]
        kc, vc = kp, vp
    rk, rv = kc.clone(), vc.clone()
    for b in range(FB):
        for i in range(q_lens[b]):
            pos = lens[b] - q_lens[b] + i
            slab, tok = (ids[b][pos // 64], pos % 64) if paged else (b, pos)
            rk[slab, :, tok], rv[slab, :, tok] = kn[cu[b] + i], vn[cu[b] + i]
    kw = dict(cu_seqlens_q=i32(cu), max_seqlen_q=50, cache_seqlens=i32(lens), block_table=table, return_lse=True)
    o_ref, lse_ref = ops.fa3_prefill_varlen(q, rk, rv, **kw)
    o, lse = ops.fa3_prefill_varlen(q, kc, vc, k_new=kn, v_new=vn, **kw)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(o_ref[:53].float()).all())
    assert torch.equal(o[:53], o_ref[:53]) and torch.equal(lse[:, :53], lse_ref[:, :53])
    assert torch.equal(kc.view(torch.int16), rk.view(torch.int16)) and torch.equal(vc.view(torch.int16), rv.view(torch.int16))


# ---- a whole step in a graph ----------------------------------------------------------------------------------------------------

def test_whole_step_replays_in_a_graph():
    """``write_step`` + ``prefill_varlen`` captured once (a single chain on one stream) over a ``PagedKVCache`` with pages reserved
    ahead; three replays with different ``q_lens``, ``advance`` and in-place refreshes in between, against an eager twin driven by
    ``append_varlen`` + ``prefill_varlen``."""
    from photonic_flash_attention_amd.integration.pytorch import PagedKVCache
    dev, dtype, H, D, rows, bound = device(), torch.bfloat16, 4, 64, 160, 130

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

    def step():
        cache.write_step(k_s, v_s, cu_seqlens_q=cu, max_seqlen_q=bound)
        return cache.prefill_varlen(q_s, cu_seqlens_q=cu, max_seqlen_q=bound, out=o_s)[0]

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
    for q_lens in ([5, 0, 70], [1, 1, 1], [0, 130, 2]):
        n = sum(q_lens)
        k, v, q = (torch.randn(n, heads, D, generator=g).to(dtype).to(dev) for heads in (HKV, HKV, H))
        k_s.fill_(NAN), v_s.fill_(NAN), o_s.fill_(SENTINEL)
        k_s[:n], v_s[:n], q_s[:n] = k, v, q
        at = [0]
        for x in q_lens:
            at.append(at[-1] + x)
        cu.copy_(torch.tensor(at, dtype=torch.int32))
        cache.advance([0, 1, 2], q_lens)
        graph.replay()
        torch.cuda.synchronize()
        twin.append_varlen([0, 1, 2], k, v, q_lens)
        o_e = twin.prefill_varlen(q_s.clone(), q_lens, max_seqlen_q=bound)[0]
        torch.cuda.synchronize()
        assert torch.equal(cache.k_pool, twin.k_pool) and torch.equal(cache.v_pool, twin.v_pool), q_lens
        assert torch.equal(cache.cache_seqlens, twin.cache_seqlens) and torch.equal(cache.block_table, twin.block_table)
        assert bool(torch.isfinite(o_g[:n].float()).all()) and torch.equal(o_g[:n], o_e[:n]), q_lens
        assert bool((o_g[n:] == SENTINEL).all())
    assert [cache.length(s) for s in range(3)] == [6, 131, 73]

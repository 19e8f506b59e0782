"""GPU tests of the page copy inside a paged KV cache's pools (``ops.page_copy`` / ``pfa_page_copy``) and of page sharing in
``PagedKVCache(copy_on_write=True)``: ``fork``, copy-on-write through ``advance`` + ``write_step``, ``common_prefix`` as the route into
``shared_prefix=``, and a captured step that replays through a fork and a free.

A copy is bit-exact, so every comparison of cache contents is ``torch.equal`` -- the kernel against the plain-torch model of the rule
(``ops.page_copy`` on CPU tensors, itself checked token by token in tests/test_page_copy_host.py) on copies of the same pools, a
cache that shares pages against a twin that holds every sequence in pages of its own.  The paged kernels give the same bits whatever
pages the keys lie in, so the attention outputs of the two caches are compared with ``torch.equal`` as well.  Pools hold a sentinel
outside their random pages: a stray write, a missing write and a wrong source all show in the whole-pool comparison.

Only legal arguments and documented device values (``-1`` for "no copy", ``src == dst``, row counts outside ``[0, page_size]``) reach
the GPU; page ids past the pool are exercised on the CPU model."""

from __future__ import annotations

import pytest
import torch

from kvcache_testlib import EPS, device, i32

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
HKV = 2


# ---- the kernel against the model -----------------------------------------------------------------------------------------------

def _pools(num_pages, page_size, D, random_pages, token_major, seed, dtype):
    """K and V pools (CPU) as ``[num_pages, Hkv, page_size, D]``-shaped views of head-major or token-major memory: random numbers in
    ``random_pages``, the sentinel everywhere else."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(2):
        pool = torch.full((num_pages, page_size, HKV, D) if token_major else (num_pages, HKV, page_size, D), SENTINEL, dtype=dtype)
        if token_major:
            pool = pool.transpose(1, 2)
        for pg in random_pages:
            pool[pg] = torch.randn(HKV, page_size, D, generator=g).to(dtype)
        out.append(pool)
    return out


def _to_dev(pool, token_major):
    """The same view of the same memory layout on the GPU."""
    return pool.transpose(1, 2).contiguous().to(device()).transpose(1, 2) if token_major else pool.contiguous().to(device())


@pytest.mark.parametrize("token_major", [False, True], ids=["head-major", "token-major"])
@pytest.mark.parametrize("page_size", [64, 256])
@pytest.mark.parametrize("D", [64, 96, 128])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_kernel_equals_the_model_on_the_whole_pools(dtype, D, page_size, token_major):
    """Five legal pairs between -1 entries and one ``src == dst``, with whole pages and with row counts 0, 1, 63, page_size and
    page_size + 136 (clamped); at page_size 256 and D 128 a page is 8 workgroups, at page_size 64 and D 96 a partly filled one."""
    from photonic_flash_attention_amd import ops
    num_pages = 13 if D == 128 else 11 if D == 96 else 12
    kp, vp = _pools(num_pages, page_size, D, (0, 1, 2, 3, 4), token_major, D + page_size, dtype)
    pairs = [(0, 5), (-1, -1), (1, 6), (2, 7), (3, 3), (3, 8), (-1, 10), (4, 9), (9, -1)]
    wide = torch.full((len(pairs), 4), -1, dtype=torch.int32)                 # the pair list as a strided view: pairs_stride 4
    wide[:, :2] = torch.tensor(pairs, dtype=torch.int32)
    rows = [0, 40, 1, 63, 17, page_size, 64, page_size + 136, 3]
    assert kp.stride() == _to_dev(kp, token_major).stride()
    for pair_t, row_l in ((torch.tensor(pairs, dtype=torch.int32), None), (wide[:, :2], rows), (wide[:, :2], None)):
        mk, mv = kp.clone(), vp.clone()
        row_t = None if row_l is None else torch.tensor(row_l, dtype=torch.int32)
        ops.page_copy(mk, mv, pair_t, rows=row_t)                                               # the model
        assert not torch.equal(mk, kp) and bool((mk[10:] == SENTINEL).all())
        dk, dv = _to_dev(kp, token_major), _to_dev(vp, token_major)
        dpairs = pair_t.to(device()) if pair_t.is_contiguous() else wide.to(device())[:, :2]
        drows = None if row_t is None else row_t.to(device())
        ops.page_copy(dk, dv, dpairs, rows=drows)
        torch.cuda.synchronize()
        assert torch.equal(dk.cpu(), mk) and torch.equal(dv.cpu(), mv), (row_l, dpairs.stride())
        ops.page_copy(dk, dv, dpairs, rows=drows)                                               # a replay is idempotent
        torch.cuda.synchronize()
        assert torch.equal(dk.cpu(), mk) and torch.equal(dv.cpu(), mv)


def test_an_empty_pair_list_launches_nothing_and_empty_pairs_write_nothing():
    from photonic_flash_attention_amd import ops
    kp, vp = _pools(9, 64, 64, (0, 1), False, 9, torch.bfloat16)
    dk, dv = kp.to(device()), vp.to(device())
    ops.page_copy(dk, dv, i32([[0, 1]])[:0])
    ops.page_copy(dk, dv, torch.full((3, 2), -1, dtype=torch.int32, device=device()), rows=i32([-1, -1, -1]))     # a cache's idle table
    ops.page_copy(dk, dv, i32([[1, 1], [0, 0]]))
    torch.cuda.synchronize()
    assert torch.equal(dk.cpu(), kp) and torch.equal(dv.cpu(), vp)


# ---- fork through the kernels ---------------------------------------------------------------------------------------------------

H, D, PAGE = 4, 64, 64


def _cache(cow, **kw):
    from photonic_flash_attention_amd.integration.pytorch import PagedKVCache
    base = dict(num_pages=12, page_size=PAGE, Hkv=HKV, D=D, dtype=torch.bfloat16, device=device(), max_batch=3, max_pages_per_seq=4)
    base.update(kw)
    c = PagedKVCache(**base, copy_on_write=cow)
    c.k_pool.fill_(SENTINEL)
    c.v_pool.fill_(SENTINEL)
    return c


def _randn(g, *shape):
    return torch.randn(*shape, generator=g).to(torch.bfloat16).to(device())


def _same_keys(cache, twin, slots):
    for s in slots:
        (k, v), (tk, tv) = cache.gather(s), twin.gather(s)
        assert torch.equal(k, tk) and torch.equal(v, tv), s


@pytest.mark.parametrize("first", ["child", "parent"])
@pytest.mark.parametrize("rows", [1, 3], ids=["decode", "prefill3"])
@pytest.mark.parametrize("n_tokens", [None, 70])
def test_fork_then_a_step_through_the_kernels(n_tokens, rows, first):
    """A parent of 100 keys, a fork (whole, or of its first 70 keys), then one step of ``rows`` tokens for child and parent with
    different K / V through ``advance`` + ``write_step`` (page copy + append kernels) and the attention kernel -- against a twin that
    holds the two sequences in pages of their own, built by plain ``append``.  Whoever comes first in ``advance`` copies the shared
    tail page; the other then writes into it in place, behind the copy on the stream."""
    g = torch.Generator().manual_seed(100 + rows + (n_tokens or 0))
    hist_k, hist_v = _randn(g, 1, HKV, 100, D), _randn(g, 1, HKV, 100, D)
    new_k, new_v = _randn(g, 2 * rows, HKV, D), _randn(g, 2 * rows, HKV, D)          # packed: the parent's rows, then the child's
    q = _randn(g, 2, rows, H, D).transpose(1, 2)
    n = 100 if n_tokens is None else n_tokens

    cache = _cache(True)
    p = cache.allocate()
    cache.append(p, hist_k, hist_v)
    ch = cache.fork(p, n_tokens)
    assert (p, ch) == (0, 1) and cache.pages(ch) == (0, 1) and cache.page_refcount(1) == 2
    cache.advance([ch, p] if first == "child" else [p, ch], [rows, rows])
    mover = ch if first == "child" else p
    assert cache.cow_pairs[mover].tolist() == [1, 2] and cache.cow_rows.tolist()[mover] == (n if mover == ch else 100) % PAGE
    assert cache.pages(mover) == (0, 2) and cache.page_refcount(1) == cache.page_refcount(2) == 1
    cache.write_step(new_k, new_v, [rows, rows], [p, ch])

    twin = _cache(False)
    assert (twin.allocate(), twin.allocate()) == (0, 1)
    twin.append([0, 1], torch.cat([hist_k, hist_k]), torch.cat([hist_v, hist_v]))
    if n < 100:                                                # the child's shorter history: a fresh twin slot with n keys
        twin.free(1)
        assert twin.allocate() == 1
        twin.append(1, hist_k[:, :, :n], hist_v[:, :, :n])
    twin.append([0, 1], new_k.view(2, rows, HKV, D).transpose(1, 2), new_v.view(2, rows, HKV, D).transpose(1, 2))

    call = "decode" if rows == 1 else "prefill"
    o, lse = getattr(cache, call)(q, [0, 1], return_lse=True)
    to, tlse = getattr(twin, call)(q, [0, 1], return_lse=True)
    torch.cuda.synchronize()
    assert [cache.length(s) for s in (0, 1)] == [100 + rows, n + rows] == [twin.length(s) for s in (0, 1)]
    _same_keys(cache, twin, (0, 1))
    assert bool(torch.isfinite(o.float()).all()) and torch.equal(o, to) and torch.equal(lse, tlse)
    assert torch.equal(cache.k_pool[0], twin.k_pool[0]) and bool((cache.k_pool[3:] == SENTINEL).all())      # the full page: never written


# ---- shared_prefix from the class -----------------------------------------------------------------------------------------------

def _reference(q, k, v):
    """fp64 attention of one decode row q [H, D] over keys k / v [Hkv, n, D] -> (o [H, D], lse [H], ||p_row||_2 [H, 1])."""
    grp = q.shape[0] // k.shape[0]
    kd, vd = k.double().repeat_interleave(grp, dim=0), v.double().repeat_interleave(grp, dim=0)
    s = (kd @ q.double()[:, :, None])[..., 0] * q.shape[1] ** -0.5
    m = s.amax(-1, keepdim=True)
    e = torch.exp(s - m)
    pn = e / e.sum(-1, keepdim=True)
    return (pn[:, None, :] @ vd)[:, 0], (m + torch.log(e.sum(-1, keepdim=True)))[:, 0], pn.norm(dim=-1, keepdim=True)


def test_shared_prefix_comes_from_the_cache_class():
    """Three forks of a 256-key parent, each 40 keys of its own further: ``common_prefix`` names the 256 shared keys, and the
    shared-prefix decode through the class is, bit for bit, the call on a caller-built table over the same pages.  That result and the
    plain call both meet the per-element bound tests/test_hip_attn_merge.py holds a shared-prefix step and the plain paged call to,
    against fp64 attention over the gathered keys: ``eps |ref| + 3 eps max|v| ||p_row||_2 + 2e-6`` (one rounding of the output, the
    rounding of P in front of PV, the fp32 accumulation), the LSE within 2e-3."""
    from photonic_flash_attention_amd import ops
    g = torch.Generator().manual_seed(256)
    cache = _cache(True, num_pages=10, max_batch=4, max_pages_per_seq=6)
    p = cache.allocate()
    cache.append(p, _randn(g, 1, HKV, 256, D), _randn(g, 1, HKV, 256, D))
    kids = [cache.fork(p) for _ in range(3)]
    assert kids == [1, 2, 3] and cache.free_pages == 6 and [cache.page_refcount(pg) for pg in range(4)] == [4] * 4
    cache.append(kids, _randn(g, 3, HKV, 40, D), _randn(g, 3, HKV, 40, D))
    P = cache.common_prefix(kids)
    assert P == 256 and cache.free_pages == 3 and all(cache.pages(s)[:4] == (0, 1, 2, 3) for s in kids)
    q = _randn(g, 3, 1, H, D).transpose(1, 2)
    o, lse = cache.decode(q, kids, shared_prefix=P, return_lse=True)
    table, lens = cache.block_table[1:4].clone(), cache.cache_seqlens[1:4].clone()
    assert table[:, :4].tolist() == [[0, 1, 2, 3]] * 3 and lens.tolist() == [296] * 3
    o_t, lse_t = ops.fa3_decode(q, cache.k_pool.transpose(1, 2), cache.v_pool.transpose(1, 2), cache_seqlens=lens, block_table=table,
                                shared_prefix=256, return_lse=True)
    o_p, lse_p = cache.decode(q, kids, return_lse=True)
    torch.cuda.synchronize()
    assert torch.equal(o, o_t) and torch.equal(lse, lse_t)
    for b, s in enumerate(kids):
        k, v = cache.gather(s)
        ro, rlse, pn = _reference(q[b, :, 0], k, v)
        bound = EPS[torch.bfloat16] * ro.abs() + 3 * EPS[torch.bfloat16] * float(v.abs().max()) * pn + 2e-6
        for what, (oo, ll) in (("shared prefix", (o, lse)), ("plain", (o_p, lse_p))):
            err = (oo[b, :, 0].double() - ro).abs()
            lerr = float((ll[b, :, 0].double() - rlse).abs().max())
            print(f"{what} slot {s}: O max err {float(err.max()):.3e} (worst err - bound {float((err - bound).max()):.3e}), LSE max err {lerr:.3e}")
            assert bool((err <= bound).all()), (what, s, float((err - bound).max()))
            assert lerr <= 2e-3, (what, s, lerr)


# ---- one graph through a fork and a free ----------------------------------------------------------------------------------------

def test_a_captured_step_replays_through_fork_and_free():
    """``write_step`` + ``decode`` over all slots captured once (a single chain on one stream) on a ``copy_on_write`` cache with pages
    reserved ahead; replays after ``advance``, after ``fork`` + ``advance`` of both, and after ``free(parent)`` + ``advance(child)``,
    against an eager twin that shares nothing."""
    dev, dtype = device(), torch.bfloat16
    g = torch.Generator().manual_seed(99)
    hist_k, hist_v = _randn(g, 1, HKV, 100, D), _randn(g, 1, HKV, 100, D)
    cache, twin = _cache(True), _cache(False)
    for c in (cache, twin):
        assert c.allocate() == 0
        c.append(0, hist_k, hist_v)
    cache.reserve(0, 256)
    k_s = torch.zeros(3, HKV, D, dtype=dtype, device=dev)
    v_s = torch.zeros_like(k_s)
    q_s = torch.zeros(3, H, 1, D, dtype=dtype, device=dev)
    cu = torch.zeros(4, dtype=torch.int32, device=dev)        # no rows while warming up and capturing

    def step():
        cache.write_step(k_s, v_s, cu_seqlens_q=cu, max_seqlen_q=1)
        return cache.decode(q_s, return_lse=True)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    before = cache.k_pool.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o_g, lse_g = step()
    torch.cuda.synchronize()
    assert torch.equal(cache.k_pool, before)

    def replay(live, q_lens):
        """One token for every slot with q_lens 1: into the static inputs, replay, the same step eagerly on the twin, compare."""
        n = sum(q_lens)
        k, v = _randn(g, n, HKV, D), _randn(g, n, HKV, D)
        k_s.zero_(), v_s.zero_()
        k_s[:n], v_s[:n] = k, v
        q_s.copy_(_randn(g, 3, H, 1, D))
        at = [0]
        for x in q_lens:
            at.append(at[-1] + x)
        cu.copy_(torch.tensor(at, dtype=torch.int32))
        graph.replay()
        torch.cuda.synchronize()
        twin.append_varlen(live, k, v, [1] * n)
        o_e, lse_e = twin.decode(q_s.clone(), return_lse=True)
        torch.cuda.synchronize()
        _same_keys(cache, twin, live)
        assert [cache.length(s) for s in live] == [twin.length(s) for s in live]
        assert bool(torch.isfinite(o_g.float()).all())
        assert torch.equal(o_g[live], o_e[live]) and torch.equal(lse_g[live], lse_e[live]), live

    cache.advance([0], [1])
    replay([0], [1, 0, 0])
    # a fork: the child shares both pages; child and parent step together, the child copies the tail page inside the graph
    assert cache.fork(0) == 1 and twin.allocate() == 1
    twin.append(1, *(t[None] for t in twin.gather(0)))
    cache.advance([1, 0], [1, 1])
    assert cache.cow_pairs.tolist() == [[-1, -1], [1, 4], [-1, -1]] and cache.cow_rows.tolist() == [-1, 37, -1]
    replay([0, 1], [1, 1, 0])
    assert cache.pages(1) == (0, 4) and cache.pages(0)[:2] == (0, 1)
    # the parent goes: its reserved pages and its tail page return, the shared full page stays with the child
    cache.free(0)
    twin.free(0)
    assert cache.page_refcount(0) == 1 and cache.page_refcount(1) == 0
    cache.advance([1], [1])
    assert cache.cow_pairs.tolist() == [[-1, -1]] * 3
    replay([1], [0, 1, 0])
    assert cache.length(1) == 103 and bool((o_g[0] == 0).all()) and bool((o_g[2] == 0).all())      # unallocated slots: length 0

"""CPU-side tests (no GPU, CPU tensors) of page sharing in ``PagedKVCache``: ``copy_on_write=False`` is the cache it was, and with
``copy_on_write=True`` the reference counts, ``fork``, the copy of a shared tail page in ``_grow`` (through ``append``,
``append_varlen`` and ``advance`` + ``write_step``), the pending table ``cow_pairs`` / ``cow_rows`` and its resets, the refusals and
``common_prefix``.

On CPU tensors ``ops.page_copy`` and ``ops.kv_append`` run their plain-torch models, which the GPU tests hold the kernels to.  Token t
of a sequence carries the value the test gives it in every element, pools start at a sentinel, and every comparison is ``torch.equal``:
a copy is bit-exact."""

from __future__ import annotations

import pytest
import torch

from photonic_flash_attention_amd.integration.pytorch import PagedCacheFull, PagedKVCache

SENTINEL = -7.0


def _cache(cow=True, **kw):
    base = dict(num_pages=8, page_size=64, Hkv=1, D=8, dtype=torch.bfloat16, device="cpu", max_batch=4, max_pages_per_seq=4)
    base.update(kw)
    c = PagedKVCache(**base, copy_on_write=cow) if cow is not None else PagedKVCache(**base)
    c.k_pool.fill_(SENTINEL)
    c.v_pool.fill_(SENTINEL)
    return c


def _toks(lo, n, Hkv=1, D=8):
    """n tokens valued lo, lo + 1, ... (keep them at or below 256: exact in bf16) as append's ``[1, Hkv, n, D]`` K and V = -K."""
    k = torch.arange(lo, lo + n, dtype=torch.float32).reshape(1, 1, n, 1).expand(1, Hkv, n, D).to(torch.bfloat16)
    return k, -k


def _packed(*runs):
    """append_varlen's packed ``[total, 1, 8]`` K and V = -K from ``(lo, n)`` runs."""
    k = torch.cat([torch.arange(lo, lo + n, dtype=torch.float32) for lo, n in runs]).reshape(-1, 1, 1).expand(-1, 1, 8).to(torch.bfloat16)
    return k.contiguous(), (-k).contiguous()


def _keys(c, slot):
    """The slot's keys as a list of token values, after checking that every element of a token agrees and V = -K."""
    k, v = c.gather(slot)
    assert torch.equal(k, k[:, :, :1].expand_as(k)) and torch.equal(v, -k)
    return k[0, :, 0].tolist()


def _counts(c):
    return [c.page_refcount(p) for p in range(c.num_pages)]


def _state(c):
    return (c.k_pool.clone(), c.v_pool.clone(), c.block_table.clone(), c.cache_seqlens.clone(),
            [c.pages(s) if c._live[s] else None for s in range(c.max_batch)], [c.length(s) if c._live[s] else None for s in range(c.max_batch)],
            list(c._free_pages), _counts(c))


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a[:4], b[:4])) and a[4:] == b[4:]


# ---- copy_on_write=False is the cache it was -------------------------------------------------------------------------------------

@pytest.mark.parametrize("cow", [None, False])
def test_default_off_is_the_cache_it_was(cow):
    """A script of allocate / append / release_behind_window / free: the block table, the lengths and the free list after every
    step, and the pools at the end, are the values the class gave before it could share pages (recorded from that version)."""
    c = _cache(cow, max_batch=3)
    assert c.cow_pairs is None and c.cow_rows is None
    snaps = []

    def snap():
        snaps.append((c.block_table.tolist(), c.cache_seqlens.tolist(), list(c._free_pages)))

    a, b = c.allocate(70), c.allocate()
    snap()
    c.append(a, *_toks(0, 100))
    c.append(b, *_toks(100, 65))
    snap()
    assert c.release_behind_window(a, 30) == 1
    snap()
    e = c.allocate(64)
    snap()
    c.free(a)
    snap()
    c.append(b, *_toks(165, 64))
    snap()
    c.free(b)
    snap()
    d = c.allocate(3 * 64)
    snap()
    assert (a, b, e, d) == (0, 1, 2, 0)
    assert snaps == [
        ([[0, 1, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]], [0, 0, 0], [7, 6, 5, 4, 3, 2]),
        ([[0, 1, 0, 0], [2, 3, 0, 0], [0, 0, 0, 0]], [100, 65, 0], [7, 6, 5, 4]),
        ([[-1, 1, 0, 0], [2, 3, 0, 0], [0, 0, 0, 0]], [100, 65, 0], [7, 6, 5, 4, 0]),
        ([[-1, 1, 0, 0], [2, 3, 0, 0], [0, 0, 0, 0]], [100, 65, 0], [7, 6, 5, 4]),
        ([[-1, 1, 0, 0], [2, 3, 0, 0], [0, 0, 0, 0]], [0, 65, 0], [7, 6, 5, 4, 1]),
        ([[-1, 1, 0, 0], [2, 3, 1, 0], [0, 0, 0, 0]], [0, 129, 0], [7, 6, 5, 4]),
        ([[-1, 1, 0, 0], [2, 3, 1, 0], [0, 0, 0, 0]], [0, 0, 0], [7, 6, 5, 4, 1, 3, 2]),
        ([[2, 3, 1, 0], [2, 3, 1, 0], [0, 0, 0, 0]], [0, 0, 0], [7, 6, 5, 4]),
    ]
    want = torch.full((8, 64), SENTINEL)
    want[0] = torch.arange(0, 64)
    want[1, 0], want[1, 1:36] = 228, torch.arange(65, 100)     # slot 1's key 128 over slot 0's freed page
    want[2], want[3] = torch.arange(100, 164), torch.arange(164, 228)
    want_v = torch.where(want == SENTINEL, want, -want)       # V = -K where a token was written
    want, want_v = (t.to(torch.bfloat16)[:, :, None, None].expand(8, 64, 1, 8) for t in (want, want_v))
    assert torch.equal(c.k_pool, want) and torch.equal(c.v_pool, want_v)
    with pytest.raises(ValueError, match="copy_on_write=True"):
        c.fork(d)
    assert _counts(c) == [1, 1, 1, 1, 0, 0, 0, 0]               # slot 2 holds page 0, slot 0 pages 2, 3, 1


def test_copy_on_write_is_the_last_constructor_keyword():
    import inspect
    params = list(inspect.signature(PagedKVCache.__init__).parameters.values())
    assert params[-1].name == "copy_on_write" and params[-1].default is False


# ---- fork ------------------------------------------------------------------------------------------------------------------------

def _parent(n, **kw):
    c = _cache(**kw)
    p = c.allocate()
    if n:
        c.append(p, *_toks(0, n))
    return c, p


def test_fork_at_an_unaligned_length_copies_the_tail_page_on_the_first_write():
    c, p = _parent(100)
    assert c.pages(p) == (0, 1) and _counts(c)[:3] == [1, 1, 0] and c.free_pages == 6
    assert c.cow_pairs.tolist() == [[-1, -1]] * 4 and c.cow_rows.tolist() == [-1] * 4 and c.cow_pairs.dtype == c.cow_rows.dtype == torch.int32
    pool_before = c.k_pool.clone()
    ch = c.fork(p)
    assert ch == 1 and c.pages(ch) == (0, 1) and c.length(ch) == 100 and c.free_pages == 6      # no page taken, nothing moved
    assert _counts(c)[:3] == [2, 2, 0] and torch.equal(c.k_pool, pool_before)
    assert c.block_table[ch, :2].tolist() == [0, 1] and c.cache_seqlens.tolist() == [100, 100, 0, 0]
    assert _keys(c, ch) == _keys(c, p) == list(range(100))
    # the child's first token: a fresh page with the tail page's 36 filled rows, the parent's page untouched
    c.append(ch, *_toks(200, 1))
    assert c.pages(ch) == (0, 2) and c.pages(p) == (0, 1) and _counts(c)[:4] == [2, 1, 1, 0] and c.free_pages == 5
    assert c.block_table[ch, :2].tolist() == [0, 2] and c.block_table[p, :2].tolist() == [0, 1]
    assert torch.equal(c.k_pool[1], pool_before[1]) and torch.equal(c.k_pool[0], pool_before[0])
    assert c.k_pool[2, :, 0, 0].tolist() == list(range(64, 100)) + [200] + [SENTINEL] * 27                # rows == 36, then the token
    assert _keys(c, ch) == list(range(100)) + [200] and _keys(c, p) == list(range(100))
    # the parent's page is its own again: it appends in place
    c.append(p, *_toks(150, 2))
    assert c.pages(p) == (0, 1) and _counts(c)[:4] == [2, 1, 1, 0] and c.free_pages == 5
    assert _keys(c, p) == list(range(100)) + [150, 151] and _keys(c, ch) == list(range(100)) + [200]
    assert c.cow_pairs.tolist() == [[-1, -1]] * 4 and c.cow_rows.tolist() == [-1] * 4                      # append runs its copies itself


def test_fork_at_a_page_boundary_and_at_zero_copy_nothing():
    c, p = _parent(128, max_batch=5)
    ch = c.fork(p)
    assert c.pages(ch) == (0, 1) and _counts(c)[:3] == [2, 2, 0]
    before = c.k_pool.clone()
    c.append(ch, *_toks(200, 1))
    c.append(p, *_toks(210, 1))
    assert c.pages(ch) == (0, 1, 2) and c.pages(p) == (0, 1, 3) and _counts(c)[:5] == [2, 2, 1, 1, 0]      # full pages stay shared
    assert torch.equal(c.k_pool[:2], before[:2]) and c.k_pool[2, 1:].eq(SENTINEL).all() and c.k_pool[3, 1:].eq(SENTINEL).all()
    assert _keys(c, ch) == list(range(128)) + [200] and _keys(c, p) == list(range(128)) + [210]
    # fork of an empty sequence, and n_tokens=0 of a long one
    e = c.allocate(64)                                                                               # one page reserved, no keys
    z, z2 = c.fork(e), c.fork(p, 0)
    assert c.pages(z) == () and c.pages(z2) == () and c.length(z) == c.length(z2) == 0
    assert c.page_refcount(c.pages(e)[0]) == 1                                                       # a reserved page is never shared
    assert _counts(c)[:5] == [2, 2, 1, 1, 1]
    with pytest.raises(PagedCacheFull, match="slots"):
        c.fork(p)
    c.free(z2)
    c.append(z, *_toks(30, 3))
    assert _keys(c, z) == [30, 31, 32] and c.pages(z) == (5,)


def test_fork_with_n_tokens():
    c, p = _parent(100, max_batch=5)
    a, b = c.fork(p, n_tokens=64), c.fork(p, 70)
    assert c.pages(a) == (0,) and c.pages(b) == (0, 1) and (c.length(a), c.length(b)) == (64, 70)
    assert _counts(c)[:3] == [3, 2, 0] and c.cache_seqlens.tolist() == [100, 64, 70, 0, 0]
    assert _keys(c, a) == list(range(64)) and _keys(c, b) == list(range(70))
    c.append(a, *_toks(200, 1))                                   # behind a full page: a fresh page, no copy
    assert c.pages(a) == (0, 2) and c.k_pool[2, :, 0, 0].tolist() == [200] + [SENTINEL] * 63
    c.append(b, *_toks(210, 1))                                   # 6 rows of the tail page are b's: rows == 6
    assert c.pages(b) == (0, 3) and c.k_pool[3, :, 0, 0].tolist() == list(range(64, 70)) + [210] + [SENTINEL] * 57
    assert _keys(c, b) == list(range(70)) + [210] and _keys(c, p) == list(range(100)) and _counts(c)[:5] == [3, 1, 1, 1, 0]
    # the parent forked below its length copies too while the child still holds the page: whoever writes first
    d = c.fork(p, 70)
    c.append(p, *_toks(220, 1))
    assert c.pages(p) == (0, 4) and c.pages(d) == (0, 1) and _counts(c)[:6] == [4, 1, 1, 1, 1, 0]
    assert c.k_pool[4, :, 0, 0].tolist() == list(range(64, 100)) + [220] + [SENTINEL] * 27
    c.append(d, *_toks(230, 1))                                   # the page is d's alone now: in place, over the parent's old key 70
    assert c.pages(d) == (0, 1) and _keys(c, d) == list(range(70)) + [230] and _keys(c, p) == list(range(100)) + [220]
    for bad in (-1, 102, 1.0, True, "3"):
        with pytest.raises(ValueError, match="n_tokens"):
            c.fork(p, bad)
    with pytest.raises(ValueError, match="not allocated"):
        c.fork(4)


def test_fork_carries_released_entries_over():
    c, p = _parent(200)
    assert c.release_behind_window(p, 50) == 2                    # pages 0, 1 behind key 151
    ch = c.fork(p)
    assert c.pages(ch) == (-1, -1, 2, 3) and c.block_table[ch].tolist() == [-1, -1, 2, 3] and _counts(c)[:4] == [0, 0, 2, 2]
    c.append(ch, *_toks(250, 1))
    assert c.pages(ch) == (-1, -1, 2, 0) and c.k_pool[0, :9, 0, 0].tolist() == list(range(192, 200)) + [250]    # page 0 went back last
    c.free(ch)
    c.free(p)
    assert c.free_pages == 8 and _counts(c) == [0] * 8


# ---- pool accounting -------------------------------------------------------------------------------------------------------------

def test_pages_survive_until_the_last_holder_lets_go():
    c, p = _parent(100)
    kids = [c.fork(p) for _ in range(3)]
    assert _counts(c)[:2] == [4, 4] and c.free_pages == 6
    c.free(p)
    assert _counts(c)[:2] == [3, 3] and c.free_pages == 6 and all(_keys(c, s) == list(range(100)) for s in kids)
    c.free(kids[0])
    c.free(kids[2])
    assert _counts(c)[:2] == [1, 1] and c.free_pages == 6 and _keys(c, kids[1]) == list(range(100))
    assert list(c._free_pages) == [7, 6, 5, 4, 3, 2]
    c.free(kids[1])
    assert _counts(c) == [0] * 8 and list(c._free_pages) == [7, 6, 5, 4, 3, 2, 1, 0]     # in free's order: the last page first
    assert c.allocate(64) == 0 and c.pages(0) == (0,)


def test_release_behind_window_keeps_a_shared_page_alive():
    c, p = _parent(200)
    ch = c.fork(p)
    assert c.release_behind_window(ch, 50) == 2                   # "entries this slot let go"
    assert c.pages(ch) == (-1, -1, 2, 3) and c.pages(p) == (0, 1, 2, 3) and _counts(c)[:4] == [1, 1, 2, 2] and c.free_pages == 4
    assert c.block_table[ch].tolist() == [-1, -1, 2, 3] and _keys(c, p) == list(range(200))
    assert c.release_behind_window(ch, 50) == 0
    assert c.release_behind_window(p, 50) == 2                    # the last holder: now they go back, in that call's order
    assert _counts(c)[:4] == [0, 0, 2, 2] and list(c._free_pages) == [7, 6, 5, 4, 1, 0]


def test_pool_full_on_a_copy_on_write_page_changes_nothing():
    c, p = _parent(100, num_pages=3)
    ch = c.fork(p)
    other = c.allocate(64)                                        # takes the last free page
    assert c.free_pages == 0
    before = _state(c)
    with pytest.raises(PagedCacheFull, match="needs 1 more pages"):
        c.append(ch, *_toks(200, 1))                              # needs no page for its length, one for the copy
    assert _same(_state(c), before)
    with pytest.raises(PagedCacheFull):
        c.advance([p], [1])
    with pytest.raises(PagedCacheFull):
        c.append_varlen([other, ch], *_packed((0, 10), (200, 1)), [10, 1])       # all or nothing across slots
    assert _same(_state(c), before) and c.cow_pairs.tolist() == [[-1, -1]] * 4
    # two holders of one tail page in one call: the first copies, the last keeps the page -- one fresh page, not two
    c.free(other)
    c.append_varlen([ch, p], *_packed((200, 1), (210, 1)), [1, 1])
    assert c.pages(ch) == (0, 2) and c.pages(p) == (0, 1) and c.free_pages == 0
    assert _keys(c, ch) == list(range(100)) + [200] and _keys(c, p) == list(range(100)) + [210]
    # a slot that gains nothing copies nothing
    d = c.fork(p, 70)
    c.advance([d], [0])
    assert c.pages(d) == (0, 1) and c.cow_pairs.tolist() == [[-1, -1]] * 4


# ---- advance + write_step --------------------------------------------------------------------------------------------------------

def test_advance_then_write_step_equals_append_varlen_through_forks():
    one, two = _cache(), _cache()
    empty_pairs, empty_rows = [[-1, -1]] * 4, [-1] * 4
    for c in (one, two):
        assert c.allocate() == 0
        c.append(0, *_toks(0, 100))

    def step(slots, runs, want_pairs, want_rows):
        lens = [n for _, n in runs]
        k, v = _packed(*runs)
        one.append_varlen(slots, k, v, lens)
        two.advance(slots, lens)
        assert two.cow_pairs.tolist() == want_pairs and two.cow_rows.tolist() == want_rows
        two.write_step(k, v, lens, slots)
        assert _same(_state(one), _state(two)), (slots, lens)
        assert two.cow_pairs.tolist() == want_pairs                                   # write_step leaves the table alone

    assert one.fork(0) == two.fork(0) == 1
    step([1, 0], [(200, 1), (210, 3)], [[-1, -1], [1, 2], [-1, -1], [-1, -1]], [-1, 36, -1, -1])    # the child copies, the parent keeps
    step([0, 1], [(220, 1), (230, 1)], empty_pairs, empty_rows)                                     # nothing shared: reset by advance
    assert one.fork(1, 70) == two.fork(1, 70) == 2 and one.fork(0) == two.fork(0) == 3
    assert two.cow_pairs.tolist() == empty_pairs
    # slot 1 (tail page 2, at 102) is held by slot 2 below its length; slot 0 (tail page 1, at 104) by slot 3
    step([3, 2, 0, 1], [(110, 30), (250, 1), (0, 0), (160, 2)], [[-1, -1], [-1, -1], [2, 5], [1, 3]], [-1, -1, 6, 40])
    assert _keys(two, 3) == list(range(100)) + [210, 211, 212, 220] + list(range(110, 140))
    assert _keys(two, 2) == list(range(70)) + [250] and _keys(two, 1) == list(range(100)) + [200, 230, 160, 161]
    # every tail page is its slot's own now: nothing pending; a replay-style device cu_seqlens_q over all slots
    k, v = _packed((100, 1), (110, 1), (120, 1), (130, 1))
    one.append_varlen([0, 1, 2, 3], k, v, [1, 1, 1, 1])
    two.advance([0, 1, 2, 3], [1, 1, 1, 1])
    assert two.cow_pairs.tolist() == empty_pairs and two.cow_rows.tolist() == empty_rows
    two.write_step(k, v, cu_seqlens_q=torch.tensor([0, 1, 2, 3, 4], dtype=torch.int32), max_seqlen_q=1)
    assert _same(_state(one), _state(two))


@pytest.mark.parametrize("call", ["append", "append_varlen", "fork", "free", "release_behind_window", "swap_pages", "advance"])
def test_every_ownership_call_resets_the_pending_table(call):
    c, p = _parent(100)
    ch = c.fork(p)
    c.advance([ch], [1])
    assert c.cow_pairs.tolist() == [[-1, -1], [1, 2], [-1, -1], [-1, -1]] and c.cow_rows.tolist() == [-1, 36, -1, -1]
    pairs, rows = c.cow_pairs, c.cow_rows
    c.write_step(*_packed((200, 1)), [1], [ch])
    if call == "append":
        c.append(p, *_toks(210, 1))
    elif call == "append_varlen":
        c.append_varlen([p], *_packed((210, 1)), [1])
    elif call == "fork":
        c.fork(p)
    elif call == "free":
        c.free(p)
    elif call == "release_behind_window":
        assert c.release_behind_window(ch, 10) == 1
    elif call == "swap_pages":
        c.reserve(ch, 192)
        c.swap_pages(ch, 1, 2)
    else:
        c.advance([p], [1])
    assert c.cow_pairs is pairs and c.cow_rows is rows                                # the same storage for the cache's lifetime
    assert c.cow_pairs.tolist() == [[-1, -1]] * 4 and c.cow_rows.tolist() == [-1] * 4
    assert _keys(c, ch)[:101] == list(range(100)) + [200] if call != "release_behind_window" else c.pages(ch)[0] == -1


def test_write_step_runs_page_copy_over_the_caches_own_pending_table(monkeypatch):
    from photonic_flash_attention_amd.integration.pytorch import paged_cache
    calls = []
    monkeypatch.setattr(paged_cache.ops, "page_copy", lambda *a, **kw: calls.append(("page_copy", a, kw)))
    monkeypatch.setattr(paged_cache.ops, "kv_append", lambda *a, **kw: calls.append(("kv_append", a, kw)))
    c, p = _parent(100)
    k, v = _packed((200, 2))
    c.advance([p], [2])
    c.write_step(k, v, [2], [p])
    (n1, (kp, vp, pairs), kw), (n2, _, _) = calls
    assert (n1, n2) == ("page_copy", "kv_append")                                     # the copy goes first
    assert pairs is c.cow_pairs and kw == {"rows": c.cow_rows}                        # capturable: the cache's own tensors
    assert kp.shape == (8, 1, 64, 8) and kp.data_ptr() == c.k_pool.data_ptr() and vp.data_ptr() == c.v_pool.data_ptr()
    del calls[:]
    c.write_step(k, v, [0], [p])                                                      # no rows: no launch at all
    assert not calls
    off = _cache(False)
    off.allocate()
    off.advance([0], [2])
    off.write_step(k, v, [2], [0])
    assert [n for n, _, _ in calls] == ["kv_append"]                                  # copy_on_write=False: no extra launch


# ---- refusals and common_prefix --------------------------------------------------------------------------------------------------

def test_swap_pages_refuses_a_shared_page():
    c, p = _parent(100)
    c.reserve(p, 192)
    ch = c.fork(p)
    for i, j in ((0, 2), (2, 1), (1, 1)):
        with pytest.raises(ValueError, match="shared with another slot"):
            c.swap_pages(p, i, j)
    c.append(ch, *_toks(200, 1))                                  # page 1 is the parent's alone again
    before = _keys(c, p)
    c.swap_pages(p, 1, 2)
    assert c.pages(p) == (0, 2, 1) and _keys(c, p) == before and _keys(c, ch) == list(range(100)) + [200]
    with pytest.raises(ValueError, match="shared with another slot"):
        c.swap_pages(ch, 0, 1)


def test_common_prefix():
    c, p = _parent(200, num_pages=12, max_batch=6, max_pages_per_seq=6)
    a, b = c.fork(p), c.fork(p, 130)
    assert c.common_prefix([p, a]) == 192 and c.common_prefix([p, a, b]) == 128 and c.common_prefix([b]) == 128
    assert c.common_prefix([p]) == 192 and c.common_prefix((a, p)) == 192
    c.append(a, *_toks(210, 1))                                   # a's tail page is copied: the full pages stay common
    c.append(b, *_toks(220, 70))                                  # b fills its third page with keys of its own
    assert c.length(b) == 200 and c.common_prefix([p, a]) == 192 and c.common_prefix([p, b]) == 128 and c.common_prefix([a, b]) == 128
    aligned = c.fork(p, 128)
    assert c.common_prefix([aligned, p]) == 128 and c.common_prefix([aligned]) == 128
    short = c.fork(p, 100)
    assert c.common_prefix([p, short]) == 64 and c.common_prefix([short]) == 64
    c.free(short)
    other = c.allocate()
    c.append(other, *_toks(0, 200))                               # the same keys in other pages
    assert c.common_prefix([p, other]) == 0 and c.common_prefix([other, a, p]) == 0
    assert c.release_behind_window(a, 100) == 1                   # a's first page is gone: nothing in common is readable
    assert c.common_prefix([p, a]) == 0 and c.common_prefix([a]) == 0 and c.common_prefix([p, b]) == 128
    c.free(other)
    empty = c.allocate()
    assert c.common_prefix([p, empty]) == 0 and c.common_prefix([empty]) == 0
    with pytest.raises(ValueError, match="not allocated"):
        c.common_prefix([p, 5])
    with pytest.raises(ValueError, match="no slots"):
        c.common_prefix([])

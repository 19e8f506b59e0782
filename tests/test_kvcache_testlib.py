"""CPU tests of tests/kvcache_testlib.py, the reference and the checks every KV-cache GPU test relies on: the vectorised fp64
reference against a loop that spells the visibility rule out key by key, the two checks against outputs they must reject, the page
scatter against a gather through its own table, and the guard, the runner and the bit-equality helpers driven by a stand-in kernel
(``reference()`` on the caches it is handed, rounded) and by stand-ins that are wrong in one way each."""

from __future__ import annotations

import itertools
import math
import types

import pytest
import torch

from kvcache_testlib import (EPS, FP8, INF, NAN, NANB, b8, both, check_against_cache, check_lse, check_out, contiguous_of, guard, i32,
                             ragged_equals_uniform, reference, run_and_check, scatter, scatter_fp8, seq_rows, share_prefix_pages, window_lo)

B, H, HKV, SQ, SMAX, D = 2, 4, 2, 3, 9, 8


def _inputs(dtype=torch.float64, seed=0):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, H, SQ, D, generator=g, dtype=torch.float64).to(dtype)
    k = torch.randn(B, HKV, SMAX, D, generator=g, dtype=torch.float64).to(dtype)
    v = torch.randn(B, HKV, SMAX, D, generator=g, dtype=torch.float64).to(dtype)
    return q, k, v


def _mask():
    km = torch.ones(B, SMAX, dtype=torch.bool)
    km[1, 0] = km[1, 4] = False
    return km


def _naive(q, k, v, seqlens, key_mask, causal, window):
    """Row by row: explicit ``if`` visibility, ``math.exp`` sums in Python floats (fp64)."""
    scale = D ** -0.5
    o = torch.zeros(B, H, SQ, D, dtype=torch.float64)
    lse = torch.full((B, H, SQ), -INF, dtype=torch.float64)
    pnorm = torch.zeros(B, H, SQ, 1, dtype=torch.float64)
    ql, kl, vl = q.tolist(), k.tolist(), v.tolist()
    for b, h, i in itertools.product(range(B), range(H), range(SQ)):
        n = SMAX if seqlens is None else seqlens[b]
        hk = h // (H // HKV)
        seen, scores = [], []
        for j in range(SMAX):
            if j >= n:
                continue
            if causal and j > i + n - SQ:
                continue
            if window is not None and j <= i + n - SQ - window:
                continue
            if key_mask is not None and not bool(key_mask[b, j]):
                continue
            seen.append(j)
            scores.append(sum(ql[b][h][i][d] * kl[b][hk][j][d] for d in range(D)) * scale)
        if not seen:
            continue
        m = max(scores)
        w = [math.exp(s - m) for s in scores]
        total = sum(w)
        for d in range(D):
            o[b, h, i, d] = sum(wj / total * vl[b][hk][j][d] for wj, j in zip(w, seen))
        lse[b, h, i] = m + math.log(total)
        pnorm[b, h, i, 0] = math.sqrt(sum((wj / total) ** 2 for wj in w))
    return o, lse, pnorm


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("seqlens", [None, [9, 5], [2, 0]], ids=["full", "9-5", "2-0"])
def test_reference_agrees_with_a_naive_loop(seqlens, masked):
    """1e-12: both sides are fp64 sums of at most 9 terms of magnitude O(1), four orders above their rounding."""
    q, k, v = _inputs()
    key_mask = _mask() if masked else None
    sl = None if seqlens is None else torch.tensor(seqlens, dtype=torch.int32)
    for causal, window in [(False, None)] + [(True, w) for w in (None, 1, 2, 4)]:
        o, lse, pn = reference(q, k, v, seqlens=sl, key_mask=key_mask, causal=causal, window=window)
        no, nlse, npn = _naive(q, k, v, seqlens, key_mask, causal, window)
        what = (seqlens, masked, causal, window)
        assert o.dtype == lse.dtype == pn.dtype == torch.float64 and pn.shape == (B, H, SQ, 1)
        empty = nlse == -INF
        assert torch.equal(lse == -INF, empty) and torch.equal(torch.isfinite(lse), ~empty), what
        assert bool((o[empty] == 0).all()) and bool((pn[empty] == 0).all()), what
        assert float((o - no).abs().max()) <= 1e-12, what
        assert float((lse - nlse)[~empty].abs().max() if bool((~empty).any()) else 0.0) <= 1e-12, what
        assert float((pn - npn).abs().max()) <= 1e-12, what
        if seqlens == [2, 0]:
            assert bool(empty[1].all()) and bool(empty[0, :, 0].all()) == causal, what       # Sq 3 over 2 keys: row 0 sees key j <= -1
    with pytest.raises(AssertionError):
        reference(q, k, v, causal=False, window=2)


def _passing():
    """bf16 inputs with rows that see no key, the reference, and outputs that pass: ``got = ref.to(bf16)``.  One rounding moves an element
    by at most 2 eps |ref|, and with at most 9 keys ||p_row||_2 >= 1/3 and |ref| <= max|v|, so the bound is at least 2 eps |ref|."""
    q, k, v = _inputs(torch.bfloat16, seed=1)
    ref, rlse, pn = reference(q, k, v, seqlens=torch.tensor([9, 2], dtype=torch.int32))
    vmax = float(v.abs().max())
    bound = EPS[torch.bfloat16] * ref.abs() + 3 * EPS[torch.bfloat16] * vmax * pn + 2e-6
    assert bool((rlse[1, :, 0] == -INF).all()) and bool(torch.isfinite(rlse[0]).all())
    return ref, rlse, pn, vmax, bound, ref.to(torch.bfloat16), rlse.float()


def test_the_checks_pass_a_correctly_rounded_output():
    ref, rlse, pn, vmax, _, got, lse = _passing()
    check_out(got, ref, pn, vmax, torch.bfloat16, "bf16")
    check_out(ref.float(), ref, pn, vmax, torch.bfloat16, "fp32")
    check_lse(got, lse, rlse, "lse")


def test_check_out_rejects_what_it_must():
    ref, _, pn, vmax, bound, got, _ = _passing()
    # the element of batch 0 with the smallest |ref|: there the bound is far above one bf16 rounding, so the move survives it
    at = (0,) + tuple(int(x) for x in torch.unravel_index(ref[0].abs().argmin(), ref[0].shape))
    moved = got.clone()
    moved[at] = (ref[at] + 2 * bound[at]).to(torch.bfloat16)
    with pytest.raises(AssertionError, match="over the bound"):
        check_out(moved, ref, pn, vmax, torch.bfloat16)
    nan = got.clone()
    nan[at] = NAN
    with pytest.raises(AssertionError, match="non-finite"):
        check_out(nan, ref, pn, vmax, torch.bfloat16)
    off = ref.float()
    off[at] += 2e-3
    with pytest.raises(AssertionError):
        check_out(off, ref, pn, vmax, torch.bfloat16)
    nan32 = ref.float()
    nan32[at] = NAN
    with pytest.raises(AssertionError, match="non-finite"):
        check_out(nan32, ref, pn, vmax, torch.bfloat16)


def test_check_lse_rejects_what_it_must():
    _, rlse, _, _, _, got, lse = _passing()
    off = lse.clone()
    off[0, 1, 2] += 3e-3                                   # a finite row
    with pytest.raises(AssertionError):
        check_lse(got, off, rlse)
    finite = lse.clone()
    finite[1, 0, 0] = 0.0                                  # the reference has -inf here
    with pytest.raises(AssertionError, match="finite LSE"):
        check_lse(got, finite, rlse)
    missing = lse.clone()
    missing[0, 0, 0] = -INF                                # and a finite value here
    with pytest.raises(AssertionError, match="finite LSE"):
        check_lse(got, missing, rlse)
    nan = lse.clone()
    nan[1, 0, 0] = NAN
    with pytest.raises(AssertionError, match="NaN"):
        check_lse(got, nan, rlse)
    nonzero = got.clone()
    nonzero[1, 0, 0, 3] = 2.0 ** -20                       # a row with no key
    with pytest.raises(AssertionError, match="not exactly zero"):
        check_lse(nonzero, lse, rlse)


@pytest.mark.parametrize("layout", ["phsd", "hpsd", "slice"])
def test_scatter_then_contiguous_of_round_trips(layout):
    Bc, Hkv, Smax, Dc, page = 2, 2, 128, 8, 64
    g = torch.Generator().manual_seed(3)
    k = torch.randn(Bc, Hkv, Smax, Dc, generator=g).to(torch.bfloat16)
    v = torch.randn(Bc, Hkv, Smax, Dc, generator=g).to(torch.bfloat16)
    kp, vp, table = scatter(k, v, page, seed=4, layout=layout)
    assert kp.shape == vp.shape == (Bc * 2 + 5, Hkv, page, Dc) and table.shape == (Bc, 2) and table.dtype == torch.int32
    assert kp.is_contiguous() == (layout == "hpsd")
    named = sorted(table.flatten().tolist())
    assert len(set(named)) == Bc * 2 and 0 <= named[0] and named[-1] < kp.shape[0]
    for pool in (kp, vp):
        for p in range(pool.shape[0]):
            assert bool(torch.isnan(pool[p]).all()) == (p not in named)
            assert bool(torch.isnan(pool[p]).any()) == (p not in named)

    def gather(s):
        return tuple(pool[table[s].long()].permute(1, 0, 2, 3).reshape(Hkv, Smax, Dc) for pool in (kp, vp))

    cache = types.SimpleNamespace(max_batch=Bc, Hkv=Hkv, D=Dc, k_pool=kp, device=k.device, gather=gather)
    k2, v2 = contiguous_of(cache, Smax)
    assert torch.equal(k2.view(torch.int16), k.view(torch.int16)) and torch.equal(v2.view(torch.int16), v.view(torch.int16))


# --- the guard, the scatter's options, the runner: a second tiny shape with room for the 64-key boundary --------------------------------

SMAX2, PAGE = 192, 64
LENS2 = [150, 192]


def _caches(dtype=torch.bfloat16, seed=5, Sq=SQ):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, H, Sq, D, generator=g).to(dtype)
    k = torch.randn(B, HKV, SMAX2, D, generator=g).to(dtype)
    v = torch.randn(B, HKV, SMAX2, D, generator=g).to(dtype)
    return q, k, v


@pytest.mark.parametrize("sqs", [SQ, [SQ, 40]], ids=["sq3", "sq3-40"])
@pytest.mark.parametrize("W", [None, 10, 20, 21, 84, 1000])
def test_guard_puts_nan_where_the_rule_says(W, sqs):
    """lens 150 and 192, Sq 3: W 10 puts lo_0 = 138 inside a tile (floor 128), W 20 on a boundary (128), W 21 one below it (127 -> 64),
    W 84 on 64, W 1000 is larger than the cache (0)."""
    _, k, v = _caches()
    kn, vn = guard(k, v, LENS2, sqs, W)
    want = torch.zeros(B, SMAX2, dtype=torch.bool)
    for b in range(B):
        sq = sqs if isinstance(sqs, int) else sqs[b]
        for j in range(SMAX2):
            below = W is not None and j < max(0, LENS2[b] - sq - W + 1) // 64 * 64
            want[b, j] = j >= LENS2[b] or below
    for src, got in ((k, kn), (v, vn)):
        assert torch.equal(torch.isnan(got), want[:, None, :, None].expand_as(got))
        assert torch.equal(got[~torch.isnan(got)], src[~torch.isnan(got)]) and not bool(torch.isnan(src).any())
    if W == 10 and sqs == SQ:
        assert bool(want[0, 127]) and not bool(want[0, 128]) and window_lo(LENS2, SQ, W) == [138, 180]


def _gather(pool, table):
    """[num_pages,Hkv,page,D] through [B,pages] (a -1 clamped to page 0) -> [B,Hkv,pages*page,D]."""
    Bc, pages = table.shape
    return pool[table.clamp_min(0).long()].permute(0, 2, 1, 3, 4).reshape(Bc, pool.shape[1], pages * pool.shape[2], pool.shape[3])


def test_scatter_leaves_page_zero_unnamed_and_releases_the_pages_below_a_window():
    _, k, v = _caches()
    lo = window_lo(LENS2, SQ, 10)                                      # [138, 180]: two released pages each
    kp0, _, table0 = scatter(k, v, PAGE, seed=7, first=1)
    kp, vp, table = scatter(k, v, PAGE, seed=7, first=1, lo=lo)
    assert kp.shape[0] == 1 + B * 3 + 5 and 0 not in table0.flatten().tolist() and len(set(table0.flatten().tolist())) == B * 3
    assert torch.equal(_gather(kp0, table0).view(torch.int16), k.view(torch.int16))
    for pool in (kp, vp):
        assert bool(torch.isnan(pool[0]).all())
    for b in range(B):
        n = lo[b] // PAGE
        assert n == 2 and table[b, :n].tolist() == [-1] * n and torch.equal(table[b, n:], table0[b, n:])
        for pool in (kp, vp):
            assert bool(torch.isnan(pool[table0[b, :n].long()]).all())
    live = _gather(kp, table)[:, :, 2 * PAGE:]
    assert torch.equal(live.view(torch.int16), k[:, :, 2 * PAGE:].view(torch.int16))


@pytest.mark.parametrize("layout", ["phsd", "hpsd"])
def test_scatter_fp8_round_trips_bytes_and_names_page_zero_behind_each_length(layout):
    g = torch.Generator().manual_seed(8)
    k8, v8 = (torch.randint(0, 256, (B, HKV, SMAX2, D), generator=g, dtype=torch.uint8).view(FP8) for _ in range(2))
    lens = [100, 9]
    for seed in range(4):                                              # some seeds put keys on page 0 first: they move to a spare page
        kp, vp, table = scatter_fp8(k8, v8, PAGE, seed, lens, layout)
        assert kp.dtype == FP8 and kp.is_contiguous() == (layout == "hpsd")
        for src, pool in ((k8, kp), (v8, vp)):
            assert bool((b8(pool)[0] == NANB).all())
            got = _gather(b8(pool), table)
            for b, n in enumerate(lens):
                used = -(-n // PAGE)
                assert table[b, used:].tolist() == [0] * (3 - used) and 0 not in table[b, :used].tolist()
                assert torch.equal(got[b, :, :used * PAGE], b8(src)[b, :, :used * PAGE])


def test_share_prefix_pages_names_the_pages_once_and_frees_the_copies():
    _, k, v = _caches()
    kp, vp, table = scatter(k, v, PAGE, seed=9)
    before, kp0 = table.clone(), kp.clone()
    share_prefix_pages(kp, vp, table, 0, 1, 2)
    assert torch.equal(table[1, :2], table[0, :2]) and torch.equal(table[0], before[0]) and torch.equal(table[1, 2:], before[1, 2:])
    kept = torch.ones(kp.shape[0], dtype=torch.bool)
    kept[before[1, :2].long()] = False
    for pool in (kp, vp):
        assert bool(torch.isnan(pool[~kept]).all())
    assert torch.equal(kp[kept].view(torch.int16), kp0[kept].view(torch.int16))


def _standin(use_lens=True, use_window=True, use_table=True, dead_lse=-INF, dtype=None):
    """A "kernel": ``reference()`` on the caches it is handed, rounded to the output dtype.  What it promises not to read -- keys at and
    past len_b, and below floor64(lo_b) under a window -- it zeroes first, so NaN there stays out; whatever else it is handed goes in.
    The mutants: use_lens=False ignores the lengths, use_window=False the window, use_table=False reads the pool's pages in order;
    dead_lse is the LSE of a row with no key; dtype overrides the output's."""
    def call(q, k, v, *, cache_seqlens=None, causal=True, return_lse=False, window=None, key_mask=None, out_dtype=None, block_table=None):
        if block_table is not None:
            rows = block_table if use_table else torch.arange(block_table.numel()).reshape(block_table.shape)
            k, v = _gather(k, rows), _gather(v, rows)
        sl = cache_seqlens if use_lens else None
        w = window if use_window else None
        j = torch.arange(k.shape[2])
        n = sl.long() if sl is not None else torch.full((q.shape[0],), k.shape[2])
        lo = torch.tensor(window_lo(n.tolist(), q.shape[2], w)) // 64 * 64
        read = ((j[None] < n[:, None]) & (j[None] >= lo[:, None]))[:, None, :, None]
        o, lse, _ = reference(q, torch.where(read, k, 0), torch.where(read, v, 0), seqlens=sl, key_mask=key_mask, causal=causal, window=w)
        lse = torch.where(torch.isneginf(lse), torch.full_like(lse, dead_lse), lse)
        return o.to(dtype or out_dtype or q.dtype), lse.float()

    return call


def test_run_and_check_passes_the_standin_and_raises_on_the_mutants():
    q, k, v = _caches()
    small = _inputs(torch.bfloat16, seed=1)                            # 9 keys: a correctly rounded bf16 output is inside the bound (``_passing``)
    o, lse = run_and_check(_standin(), *small, [9, 2])
    assert o.dtype == torch.bfloat16 and bool((lse[1, :, 0] == -INF).all())
    run_and_check(_standin(), *small, None, causal=False)
    run_and_check(_standin(), *small, torch.tensor([9, 5], dtype=torch.int32), key_mask=_mask(), guarded=False)
    for W in (None, 10, 21, 1000):
        run_and_check(_standin(), q, k, v, LENS2, window=W, out_dtype=torch.float32)
    with pytest.raises(AssertionError, match="non-finite"):            # 1: the NaN tail reaches the output
        run_and_check(_standin(use_lens=False), q, k, v, LENS2, out_dtype=torch.float32)
    run_and_check(_standin(use_lens=False), q, k, v, [SMAX2, SMAX2], out_dtype=torch.float32)      # ... and full caches hide that mutant
    with pytest.raises(AssertionError, match="non-finite"):            # 2: the keys below the window's boundary are read
        run_and_check(_standin(use_window=False), q, k, v, LENS2, window=10, out_dtype=torch.float32)
    with pytest.raises(AssertionError):                                # 2, unguarded: the keys are finite, the output is wrong
        run_and_check(_standin(use_window=False), q, k, v, LENS2, window=10, out_dtype=torch.float32, guarded=False)
    with pytest.raises(AssertionError, match="finite LSE"):            # 3: a finite LSE on a row with no key
        run_and_check(_standin(dead_lse=0.0), *small, [9, 2])
    with pytest.raises(AssertionError, match="the output is"):         # 4: the wrong dtype
        run_and_check(_standin(dtype=torch.float32), *small, [9, 2])
    with pytest.raises(AssertionError, match="the output is"):
        run_and_check(_standin(dtype=torch.bfloat16), q, k, v, LENS2, out_dtype=torch.float32)


def test_run_and_check_applies_with_ref_and_a_given_reference():
    q, k, v = _caches()
    sl = torch.tensor(LENS2, dtype=torch.int32)
    ref = reference(q, k, v, seqlens=sl)
    run_and_check(_standin(), q, k, v, LENS2, out_dtype=torch.float32, ref=ref)
    half = lambda r: (r[0] / 2, r[1], r[2])
    with pytest.raises(AssertionError):
        run_and_check(_standin(), q, k, v, LENS2, out_dtype=torch.float32, ref=ref, with_ref=half)

    def halved(*a, **kw):
        o, lse = _standin()(*a, **kw)
        return o / 2, lse
    run_and_check(halved, q, k, v, LENS2, out_dtype=torch.float32, with_ref=half)


def test_both_raises_on_a_paged_call_that_ignores_the_table():
    q, k, v = _caches()
    kn, vn = guard(k, v, LENS2)
    kp, vp, table = scatter(kn, vn, PAGE, seed=3)
    assert table.flatten().tolist() != list(range(table.numel()))
    kw = dict(cache_seqlens=i32(LENS2, q.device), out_dtype=torch.float32)
    op, lp = both(_standin(), q, kn, vn, kp, vp, table, **kw)
    oc, lc = _standin()(q, kn, vn, return_lse=True, **kw)
    assert torch.equal(op, oc) and torch.equal(lp, lc)
    with pytest.raises(AssertionError):
        both(_standin(use_table=False), q, kn, vn, kp, vp, table, **kw)


def test_ragged_equals_uniform_raises_on_one_ulp_and_on_a_swapped_row():
    _, k, v = _caches()
    kn, vn = guard(k, v, LENS2)
    cu = [0, 3, 8]
    g = torch.Generator().manual_seed(11)
    q = torch.randn(8, H, D, generator=g).to(torch.bfloat16)
    o, lse = torch.empty(8, H, D, dtype=torch.bfloat16), torch.empty(H, 8)
    for b in range(B):
        ob, lb = _standin()(seq_rows(q, cu, b), kn[b:b + 1], vn[b:b + 1], cache_seqlens=i32(LENS2[b:b + 1], q.device), return_lse=True)
        o[cu[b]:cu[b + 1]], lse[:, cu[b]:cu[b + 1]] = ob[0].permute(1, 0, 2), lb[0]
    ragged_equals_uniform(_standin(), o, lse, q, kn, vn, cu, LENS2)
    mid = lambda t: torch.cat([t[:1], torch.full_like(t[:1], NAN), t[1:]])       # a sequence without rows in between: it is skipped
    ragged_equals_uniform(_standin(), o, lse, q, mid(kn), mid(vn), [0, 3, 3, 8], [LENS2[0], 7, LENS2[1]])
    ulp = o.clone()
    ulp.view(torch.int16)[5, 1, 2] += 1
    assert float((ulp.float() - o.float()).abs().max()) > 0
    with pytest.raises(AssertionError, match="sequence 1: O differs"):
        ragged_equals_uniform(_standin(), ulp, lse, q, kn, vn, cu, LENS2)
    l_ulp = lse.clone()
    l_ulp.view(torch.int32)[0, 1] += 1
    with pytest.raises(AssertionError, match="sequence 0: LSE differs"):
        ragged_equals_uniform(_standin(), o, l_ulp, q, kn, vn, cu, LENS2)
    swapped = o.clone()
    swapped[2] = o[3]                                                   # the first row of sequence 1 in the last row of sequence 0
    with pytest.raises(AssertionError, match="sequence 0: O differs"):
        ragged_equals_uniform(_standin(), swapped, lse, q, kn, vn, cu, LENS2)


def test_check_against_cache_on_a_cpu_paged_cache():
    from photonic_flash_attention_amd.integration.pytorch import PagedKVCache
    cache = PagedKVCache(num_pages=8, page_size=PAGE, Hkv=HKV, D=D, dtype=torch.bfloat16, device="cpu", max_batch=B, max_pages_per_seq=3)
    g = torch.Generator().manual_seed(12)
    for s, n in enumerate([100, 70]):
        assert cache.allocate() == s
        cache.append(s, *(torch.randn(1, HKV, n, D, generator=g).to(torch.bfloat16) for _ in range(2)))
    q = torch.randn(B, H, SQ, D, generator=g).to(torch.bfloat16)
    kc, vc = contiguous_of(cache, SMAX2)
    o, lse = _standin()(q, kc, vc, cache_seqlens=cache.cache_seqlens, return_lse=True, out_dtype=torch.float32)
    check_against_cache(cache, q, o, lse, SMAX2)
    cache.k_pool[cache.pages(0)[0], :, 0] *= -30.0                      # one cached key of sequence 0, which every row sees
    with pytest.raises(AssertionError):
        check_against_cache(cache, q, o, lse, SMAX2)

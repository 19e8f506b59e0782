"""GPU tests of the forward over a KV cache with the keys split over workgroups (``ops.fa3_prefill_cache(key_splits=)`` /
``pfa_fa3_prefill_split``) and of ``prefix_key_splits=`` on the shared-prefix step.

The fp64 reference, its bounds, the NaN poisoning (every cache holds NaN at and past each length, every pool page no table entry names
is NaN) and the shared-prefix step are those of tests/kvcache_testlib.py, as tests/test_hip_prefill_cache.py and
tests/test_hip_attn_merge.py use them.  The split path carries P as hi + lo and rounds the output once, in the merge, so it sits inside
what those bounds already allow.  Paged against contiguous, one split against none, the split rule against ``attn_merge`` of plain
calls on the key slices, and graph replays against eager calls need no tolerance: ``torch.equal``.

Only in-range page ids and legal arguments ever reach the device; refusals are tested on the host (tests/test_prefill_split_host.py)."""

from __future__ import annotations

import functools

import pytest
import torch

from kvcache_testlib import (NAN, both, both_prefix_caches, capture, check_lse, check_out, device, gen, guard, i32, prefix_problem, problem,
                             reference, run_and_check, scatter, share_prefix_pages)

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _case(B, H, Hkv, Sq, Smax, D, dtype, seed, lens, causal):
    """One problem and its fp64 reference, built once and shared by every split count: (q, k, v, reference)."""
    q, k, v = problem(B, H, Hkv, Sq, Smax, D, dtype, seed)
    sl = i32(list(lens)) if lens is not None else None
    return q, k, v, reference(q, k, v, seqlens=sl, causal=causal)


def _run_and_check(case, lens, key_splits, **kw):
    """The split call on the NaN-tailed caches against fp64 on the clean ones.  lens: tuple or None (then nothing is poisoned)."""
    from photonic_flash_attention_amd import ops
    q, k, v, ref = case
    return run_and_check(ops.fa3_prefill_cache, q, k, v, lens, ref=ref, key_splits=key_splits, **kw)


# --- against fp64 --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key_splits", [2, 3, 8])
@pytest.mark.parametrize("Sq", [1, 65, 257, 300])
@pytest.mark.parametrize("D", [64, 128])
def test_against_fp64(D, Sq, key_splits):
    lens = (Sq + 1000, Sq + 17)          # the second sequence has fewer tiles than splits: whole splits are empty, -inf parts of the merge
    for dtype in (torch.bfloat16, torch.float16):
        for causal in (True, False):
            case = _case(2, 8, 2, Sq, 2048, D, dtype, Sq + D, lens, causal)
            for out_dtype in (None, torch.float32):
                _run_and_check(case, lens, key_splits, causal=causal, out_dtype=out_dtype)


@pytest.mark.parametrize("H,Hkv", [(4, 4), (16, 1)])
def test_head_groups_against_fp64(H, Hkv):
    Sq = 300
    lens = (Sq + 1000, Sq + 17)
    for dtype, D in ((torch.bfloat16, 128), (torch.float16, 64)):
        _run_and_check(_case(2, H, Hkv, Sq, 2048, D, dtype, H + Sq, lens, True), lens, 3)
        _run_and_check(_case(2, H, Hkv, Sq, 2048, D, dtype, H + Sq, lens, False), lens, 4, causal=False, out_dtype=torch.float32)


# --- edges ---------------------------------------------------------------------------------------------------------------------------

def test_zero_length():
    for causal in (True, False):
        lens = (0, 300 + 64)
        for out_dtype in (None, torch.float32):
            o, lse = _run_and_check(_case(2, 8, 2, 300, 2048, 128, torch.bfloat16, 60, lens, causal), lens, 4, causal=causal, out_dtype=out_dtype)
            assert bool((o[0] == 0).all()) and bool((lse[0] == float("-inf")).all())
    o, lse = _run_and_check(_case(2, 8, 2, 300, 2048, 128, torch.bfloat16, 60, (0, 0), True), (0, 0), 8)
    assert bool((o == 0).all()) and bool((lse == float("-inf")).all())


def test_length_below_the_row_count_leaves_the_leading_rows_zero():
    Sq = 300
    for D, dtype in ((128, torch.bfloat16), (64, torch.float16)):
        for lens in ((Sq + 500, 100), (37, Sq + 1)):
            for out_dtype in (None, torch.float32):
                o, lse = _run_and_check(_case(2, 8, 2, Sq, 2048, D, dtype, 50 + D, lens, True), lens, 4, out_dtype=out_dtype)
                b, n = (1, 100) if lens[1] == 100 else (0, 37)
                assert bool((o[b, :, :Sq - n] == 0).all()) and bool((lse[b, :, :Sq - n] == float("-inf")).all())
                assert bool(torch.isfinite(lse[b, :, Sq - n:]).all()) and bool(torch.isfinite(lse[1 - b]).all())
            _run_and_check(_case(2, 8, 2, Sq, 2048, D, dtype, 50 + D, lens, False), lens, 3, causal=False)


@pytest.mark.parametrize("page", [64, 256])
def test_lengths_next_to_tile_and_split_boundaries(page):
    """Sq = 40 is one q block of n = ceil(len / 64) tiles; with 4 splits per = ceil(n / 4): 511 / 512 / 513 keys are per * 64 * 4 - 1, + 0 and
    the first length with a larger per, 127 / 128 / 129 the same one octave down, 1023 / 1024 / 1025 one up."""
    from photonic_flash_attention_amd import ops
    Sq = 40
    for lens in ((63, 65), (64, 127), (128, 129), (511, 513), (512, 1025), (1023, 1024)):
        sl = i32(list(lens))
        for causal in (True, False):
            case = _case(2, 8, 2, Sq, 2048, 128, torch.bfloat16, 80 + page, lens, causal)
            o, lse = _run_and_check(case, lens, 4, causal=causal)
            kn, vn = guard(case[1], case[2], lens)
            kp, vp, table = scatter(kn, vn, page, seed=page)
            op, lp = ops.fa3_prefill_cache(case[0], kp, vp, block_table=table, cache_seqlens=sl, causal=causal, return_lse=True, key_splits=4)
            torch.cuda.synchronize()
            assert torch.equal(op, o) and torch.equal(lp, lse), lens


@pytest.mark.parametrize("D", [64, 128])
def test_full_cache_and_no_lengths(D):
    Smax = 1024
    for causal in (True, False):
        o1, l1 = _run_and_check(_case(2, 8, 2, 257, Smax, D, torch.bfloat16, 70 + D, (Smax, Smax), causal), (Smax, Smax), 3, causal=causal)
        o2, l2 = _run_and_check(_case(2, 8, 2, 257, Smax, D, torch.bfloat16, 70 + D, None, causal), None, 3, causal=causal)
        assert torch.equal(o1, o2) and torch.equal(l1, l2)


# --- the split rule, bit for bit -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,lens", [(2, (1000, 40)), (4, (1000, 300)), (4, (2048, 65))])
def test_the_split_rule_is_attn_merge_of_plain_calls_on_the_key_slices(N, lens):
    """Full attention over a contiguous cache: split s of a sequence of n = ceil(len / 64) tiles owns the keys [64 s per, 64 min(n,
    (s + 1) per)), per = ceil(n / N), and its partial result is the unsplit kernel's fp32 result on that slice with the length
    clamp(len - start, 0, slice).  An empty split (the second sequence's last ones) is a plain call of length 0."""
    from photonic_flash_attention_amd import ops
    Sq = 300
    for D, dtype in ((128, torch.bfloat16), (64, torch.float16)):
        q, k, v = problem(2, 8, 2, Sq, 2048, D, dtype, seed=N + D)
        kn, vn = guard(k, v, lens)
        empty = 0
        for out_dtype in (dtype, torch.float32):
            o, lse = ops.fa3_prefill_cache(q, kn, vn, cache_seqlens=i32(list(lens)), causal=False, out_dtype=out_dtype, return_lse=True,
                                           key_splits=N)
            for b, n_keys in enumerate(lens):
                n = -(-n_keys // 64)
                per = -(-n // N)
                outs, lses = [], []
                for s in range(N):
                    start, end = s * per * 64, min((s + 1) * per, n) * 64
                    if end <= start:                 # an empty range: nothing is fetched, the part is O = 0, LSE = -inf
                        start, end, length, empty = 0, 64, 0, empty + 1
                    else:
                        length = min(max(n_keys - start, 0), end - start)
                    po, pl = ops.fa3_prefill_cache(q[b:b + 1], kn[b:b + 1, :, start:end], vn[b:b + 1, :, start:end], cache_seqlens=i32([length]),
                                                   causal=False, out_dtype=torch.float32, return_lse=True)
                    outs.append(po)
                    lses.append(pl)
                mo, ml = ops.attn_merge(outs, lses, out_dtype=out_dtype, return_lse=True)
                torch.cuda.synchronize()
                assert bool(torch.isfinite(o[b].float()).all())
                assert torch.equal(o[b:b + 1], mo), (b, float((o[b:b + 1].double() - mo.double()).abs().max()))
                assert torch.equal(lse[b:b + 1], ml), b
        assert empty > 0                             # the lens do leave a split without a tile


# --- paged == contiguous -------------------------------------------------------------------------------------------------------------

def _both(*a, **kw):
    from photonic_flash_attention_amd import ops
    return both(ops.fa3_prefill_cache, *a, **kw)


@pytest.mark.parametrize("page", [64, 128, 256])
@pytest.mark.parametrize("D", [64, 128])
def test_paged_equals_contiguous(page, D):
    """Pages in random order; with pages of 128 and 256 keys (2 and 4 tiles) the splits of 3, 5 and 8 begin in the middle of a page."""
    for dtype in (torch.bfloat16, torch.float16):
        for Sq in (65, 300):
            q, k, v = problem(2, 8, 2, Sq, 2048, D, dtype, seed=page + D + Sq)
            lens = [Sq + 1000, Sq + 17]
            kn, vn = guard(k, v, lens)
            kp, vp, table = scatter(kn, vn, page, seed=page + Sq)
            for causal, N in ((True, 3), (True, 8), (False, 5)):
                for out_dtype in (None, torch.float32):
                    _both(q, kn, vn, kp, vp, table, cache_seqlens=i32(lens), causal=causal, out_dtype=out_dtype, key_splits=N)
        kp, vp, table = scatter(k, v, page, seed=page)
        _both(q, k, v, kp, vp, table, key_splits=3)                    # no lengths: every page is read


def test_two_sequences_sharing_prefix_pages():
    page, Sq = 128, 200
    q, k, v = problem(3, 8, 2, Sq, 2048, 128, torch.bfloat16, seed=10)
    k[1, :, :5 * page] = k[0, :, :5 * page]          # batches 0 and 1 have a common 640-key prefix
    v[1, :, :5 * page] = v[0, :, :5 * page]
    lens = [2048, 5 * page + Sq + 7, 900]
    kn, vn = guard(k, v, lens)
    kp, vp, table = scatter(kn, vn, page, seed=4)
    share_prefix_pages(kp, vp, table, 0, 1, 5)       # ... held once: both tables name the same pages, the duplicate copies are gone
    ref = reference(q, k, v, seqlens=i32(lens))
    for N in (3, 8):
        o, lse = _both(q, kn, vn, kp, vp, table, cache_seqlens=i32(lens), key_splits=N)
        check_out(o, ref[0], ref[2], float(v.abs().max()), q.dtype)
        check_lse(o, lse, ref[1])


# --- identity, determinism, views ----------------------------------------------------------------------------------------------------

def test_one_split_is_the_plain_call():
    from photonic_flash_attention_amd import ops
    q, k, v = problem(2, 8, 2, 300, 2048, 128, torch.bfloat16, seed=13)
    lens = [2048, 700]
    kn, vn = guard(k, v, lens)
    kp, vp, table = scatter(kn, vn, 128, seed=5)
    for caches in (dict(), dict(block_table=table)):
        kk, vv = (kp, vp) if caches else (kn, vn)
        for out_dtype in (None, torch.float32):
            for causal in (True, False):
                kw = dict(cache_seqlens=i32(lens), causal=causal, out_dtype=out_dtype, return_lse=True, **caches)
                plain = ops.fa3_prefill_cache(q, kk, vv, **kw)
                none = ops.fa3_prefill_cache(q, kk, vv, key_splits=None, **kw)
                one = ops.fa3_prefill_cache(q, kk, vv, key_splits=1, **kw)
                torch.cuda.synchronize()
                assert bool(torch.isfinite(plain[0]).all())
                assert torch.equal(plain[0], one[0]) and torch.equal(plain[1], one[1])
                assert torch.equal(plain[0], none[0]) and torch.equal(plain[1], none[1])
    # a shape the plan leaves alone (B * H * ceil(Sq / 256) >= 512) takes the same road
    q, k, v = problem(64, 8, 2, 40, 128, 64, torch.float16, seed=14)
    auto = ops.fa3_prefill_cache(q, k, v, return_lse=True, key_splits="auto")
    plain = ops.fa3_prefill_cache(q, k, v, return_lse=True)
    torch.cuda.synchronize()
    assert torch.equal(auto[0], plain[0]) and torch.equal(auto[1], plain[1])


def test_outputs_are_bitwise_reproducible():
    from photonic_flash_attention_amd import ops
    q, k, v = problem(2, 8, 2, 300, 2048, 128, torch.bfloat16, seed=12)
    lens = [2048, 1500]
    kn, vn = guard(k, v, lens)
    kp, vp, table = scatter(kn, vn, 64, seed=7)
    for out_dtype in (None, torch.float32):
        for N in (5, "auto"):
            runs = [ops.fa3_prefill_cache(q, kp, vp, block_table=table, cache_seqlens=i32(lens), out_dtype=out_dtype, return_lse=True,
                                          key_splits=N) for _ in range(2)]
            torch.cuda.synchronize()
            assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
            assert bool(torch.isfinite(runs[0][0]).all())


def test_strided_views_of_q_cache_and_out():
    from photonic_flash_attention_amd import ops
    dev = device()
    B, H, Hkv, Sq, Smax, D = 2, 8, 2, 200, 1024, 128
    g = gen(11)
    qkv = torch.randn(B, Sq, 3, H, D, generator=g, device=dev).to(torch.bfloat16)       # a fused projection
    q = qkv[:, :, 0].permute(0, 2, 1, 3)
    big_k = torch.randn(B, Hkv, Smax + 96, D, generator=g, device=dev).to(torch.bfloat16)
    big_v = torch.randn(B, Hkv, Smax + 96, D, generator=g, device=dev).to(torch.bfloat16)
    lens = [Sq + 700, Sq + 1]
    for b, n in enumerate(lens):                     # the tails stay NaN inside the larger buffer
        big_k[b, :, n:] = NAN
        big_v[b, :, n:] = NAN
    k, v = big_k[:, :, :Smax], big_v[:, :, :Smax]    # the first Smax positions of a larger preallocated cache
    assert not q.is_contiguous() and not k.is_contiguous()
    sl = i32(lens)
    ref = reference(q, torch.nan_to_num(k), torch.nan_to_num(v), seqlens=sl)
    vmax = float(torch.nan_to_num(v).abs().max())
    o, lse = ops.fa3_prefill_cache(q, k, v, cache_seqlens=sl, return_lse=True, key_splits=3)
    torch.cuda.synchronize()
    check_out(o, ref[0], ref[2], vmax, q.dtype)
    check_lse(o, lse, ref[1])
    # out= given, with strides of its own: a slice of a wider [B, Sq, H, 2 D] buffer, untouched outside the slice
    wide = torch.full((B, Sq, H, 2 * D), 7.0, dtype=torch.bfloat16, device=dev)
    out = wide[..., D:].permute(0, 2, 1, 3)
    o2, _ = ops.fa3_prefill_cache(q, k, v, cache_seqlens=sl, out=out, key_splits=3)
    torch.cuda.synchronize()
    assert o2.data_ptr() == out.data_ptr() and torch.equal(o2, o) and bool((wide[..., :D] == 7.0).all())
    # flash-attn style [B, Smax, Hkv, D] cache passed transposed
    kt, vt = k.transpose(1, 2).contiguous().transpose(1, 2), v.transpose(1, 2).contiguous().transpose(1, 2)
    o3, l3 = ops.fa3_prefill_cache(q, kt, vt, cache_seqlens=sl, return_lse=True, key_splits=3)
    torch.cuda.synchronize()
    assert torch.equal(o3, o) and torch.equal(l3, lse)


# --- graph capture -------------------------------------------------------------------------------------------------------------------

def test_split_step_replays_in_a_graph():
    """Append + split launch + merge captured once on a paged cache; replayed while the lengths grow across a tile (100 -> 130 keys: 2 ->
    3 tiles) and a split boundary (255 -> 257: per 1 -> 2 with 4 splits), pages move and q changes: each replay equals the eager call."""
    from photonic_flash_attention_amd import ops
    dev, dtype, B, H, Hkv, D, page, n_pages, Sq = device(), torch.bfloat16, 2, 8, 2, 128, 64, 24, 70
    g = torch.Generator().manual_seed(89)

    def rnd(*shape):
        return torch.randn(*shape, generator=g).to(dev, dtype)

    q_s, kn_s, vn_s = rnd(B, Sq, H, D).permute(0, 2, 1, 3), rnd(B, Hkv, Sq, D), rnd(B, Hkv, Sq, D)
    kp, vp = rnd(n_pages, Hkv, page, D), rnd(n_pages, Hkv, page, D)
    o_s = torch.empty(B, Sq, H, D, dtype=dtype, device=dev).permute(0, 2, 1, 3)

    def table_of(seed):
        return torch.randperm(n_pages, generator=torch.Generator().manual_seed(seed))[:B * 8].reshape(B, 8).to(torch.int32)

    all_lens = ([100, 255], [130, 257], [300, 512])
    lens_s = torch.tensor(all_lens[0], dtype=torch.int32, device=dev)
    table_s = table_of(0).to(dev)

    def step(q, kn, vn, k, v, lens, table, out):
        return ops.fa3_prefill_cache(q, k, v, cache_seqlens=lens, block_table=table, k_new=kn, v_new=vn, key_splits=4, out=out, return_lse=True)

    graph, (o_g, lse_g) = capture(lambda: step(q_s, kn_s, vn_s, kp, vp, lens_s, table_s, o_s))
    assert o_g is o_s
    for n, lens in enumerate(all_lens):
        if n:                                                   # everything the graph reads from the device changes
            q_s.copy_(rnd(B, Sq, H, D).permute(0, 2, 1, 3))
            kn_s.copy_(rnd(B, Hkv, Sq, D))
            vn_s.copy_(rnd(B, Hkv, Sq, D))
            kp.copy_(rnd(n_pages, Hkv, page, D))
            vp.copy_(rnd(n_pages, Hkv, page, D))
            lens_s.copy_(torch.tensor(lens, dtype=torch.int32))
            table_s.copy_(table_of(n))
        ke, ve = kp.clone(), vp.clone()
        o_e, lse_e = step(q_s.clone(), kn_s.clone(), vn_s.clone(), ke, ve, lens_s.clone(), table_s.clone(), None)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(o_g, o_e) and torch.equal(lse_g, lse_e), n
        assert torch.equal(kp, ke) and torch.equal(vp, ve), n
        assert bool(torch.isfinite(o_g.float()).all())
    # and the eager result is the right one: fp64 on the gathered caches of the last step
    kc = torch.stack([kp[table_s[b].long()].permute(1, 0, 2, 3).reshape(Hkv, 8 * page, D) for b in range(B)])
    vc = torch.stack([vp[table_s[b].long()].permute(1, 0, 2, 3).reshape(Hkv, 8 * page, D) for b in range(B)])
    ref = reference(q_s, kc, vc, seqlens=lens_s)
    check_out(o_g, ref[0], ref[2], float(vc.abs().max()), dtype)
    check_lse(o_g, lse_g, ref[1])


# --- shared prefix -------------------------------------------------------------------------------------------------------------------

PRIVATE = tuple(100 + (37 * b) % 101 for b in range(40))        # 100 .. 200 private keys


def test_prefix_key_splits_on_the_shared_prefix_step():
    """80 and 120 rows against a 1024-key prefix: the prefix pass is fa3_prefill_cache over one sequence, now split over its keys."""
    from photonic_flash_attention_amd import ops
    pr = prefix_problem(40, 2, 128, PRIVATE, 1024 + 256, torch.bfloat16, P=1024)
    both_prefix_caches(ops.fa3_decode, pr, "decode B40 Sq2 prefix_key_splits=4", prefix_key_splits=4)
    pr3 = prefix_problem(40, 3, 128, PRIVATE, 1024 + 256, torch.bfloat16, P=1024)
    both_prefix_caches(ops.fa3_prefill_cache, pr3, "prefill B40 Sq3 prefix_key_splits=auto", prefix_key_splits="auto")
    both_prefix_caches(ops.fa3_prefill_cache, pr3, "prefill B40 Sq3 prefix_key_splits=8", prefix_key_splits=8)


def test_prefix_key_splits_reaches_the_prefix_pass_only_past_64_rows(monkeypatch):
    from photonic_flash_attention_amd import ops
    seen = []
    real = ops.fa3_prefill_cache

    def spy(*a, **kw):
        seen.append((tuple(a[0].shape), kw.get("key_splits"), kw.get("shared_prefix")))
        return real(*a, **kw)

    monkeypatch.setattr(ops, "fa3_prefill_cache", spy)
    pr = prefix_problem(40, 2, 128, PRIVATE, 1024 + 256, torch.bfloat16, P=1024)
    kw = dict(cache_seqlens=pr["lens"], block_table=pr["table"], shared_prefix=1024, return_lse=True)
    with_none = ops.fa3_decode(pr["q"], pr["kp"], pr["vp"], prefix_key_splits=None, **kw)
    assert seen == [((1, 8, 80, 128), None, None)]
    del seen[:]
    without = ops.fa3_decode(pr["q"], pr["kp"], pr["vp"], **kw)
    assert seen == [((1, 8, 80, 128), None, None)]
    del seen[:]
    ops.fa3_decode(pr["q"], pr["kp"], pr["vp"], prefix_key_splits=4, **kw)
    assert seen == [((1, 8, 80, 128), 4, None)]
    torch.cuda.synchronize()
    assert torch.equal(with_none[0], without[0]) and torch.equal(with_none[1], without[1])
    # 64 rows or fewer: the decode kernel splits by itself, the argument is validated and otherwise unused
    del seen[:]
    small = prefix_problem(4, 3, 64, (3, 64, 65, 130), 320, torch.bfloat16)
    skw = dict(cache_seqlens=small["lens"], shared_prefix=128, return_lse=True)
    a = ops.fa3_decode(small["q"], small["kc"], small["vc"], prefix_key_splits=8, **skw)
    b = ops.fa3_decode(small["q"], small["kc"], small["vc"], **skw)
    torch.cuda.synchronize()
    assert seen == [] and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_shared_prefix_step_with_a_split_prefix_pass_replays_in_a_graph():
    """Append + split prefix pass + its merge + own-keys pass + final merge captured once; replayed after q, the new rows and the
    lengths changed: each replay equals the eager call bit for bit."""
    from photonic_flash_attention_amd import ops
    pr = prefix_problem(40, 2, 128, PRIVATE, 1024 + 256, torch.bfloat16, P=1024)
    dev, dtype = device(), torch.bfloat16
    g = torch.Generator().manual_seed(90)

    def rnd(*shape):
        return torch.randn(*shape, generator=g).to(dev, dtype)

    q_s, kn_s, vn_s = rnd(40, 2, 8, 128).permute(0, 2, 1, 3), rnd(40, 2, 2, 128), rnd(40, 2, 2, 128)
    kp, vp, lens_s, table_s = pr["kp"].clone(), pr["vp"].clone(), pr["lens"].clone(), pr["table"].clone()
    o_s = torch.empty(40, 2, 8, 128, dtype=dtype, device=dev).permute(0, 2, 1, 3)

    def step(q, kn, vn, k, v, lens, out):
        return ops.fa3_decode(q, k, v, cache_seqlens=lens, block_table=table_s, k_new=kn, v_new=vn, shared_prefix=1024, prefix_key_splits=4,
                              out=out, return_lse=True)

    graph, (o_g, lse_g) = capture(lambda: step(q_s, kn_s, vn_s, kp, vp, lens_s, o_s))
    for n in range(3):
        if n:
            q_s.copy_(rnd(40, 2, 8, 128).permute(0, 2, 1, 3))
            kn_s.copy_(rnd(40, 2, 2, 128))
            vn_s.copy_(rnd(40, 2, 2, 128))
            lens_s.copy_(pr["lens"] - 7 * n)                      # still behind the prefix: at least 100 - 14 private keys, 2 rows
        ke, ve = kp.clone(), vp.clone()
        o_e, lse_e = step(q_s.clone(), kn_s.clone(), vn_s.clone(), ke, ve, lens_s.clone(), None)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(o_g, o_e) and torch.equal(lse_g, lse_e), n
        assert torch.equal(kp.view(torch.int16), ke.view(torch.int16)) and torch.equal(vp.view(torch.int16), ve.view(torch.int16)), n
        assert bool(torch.isfinite(o_g.float()).all()) and bool(torch.isfinite(lse_g).all())

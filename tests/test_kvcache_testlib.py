"""CPU tests of tests/kvcache_testlib.py, the reference and the checks every KV-cache GPU test relies on: the vectorised fp64
reference against a loop that spells the visibility rule out key by key, the two checks against outputs they must reject, and the page
scatter against a gather through its own table."""

from __future__ import annotations

import itertools
import math
import types

import pytest
import torch

from kvcache_testlib import EPS, INF, NAN, check_lse, check_out, contiguous_of, reference, scatter

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

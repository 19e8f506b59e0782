"""CPU tests of tests/probe_testlib.py, the exact visibility probes of tests/test_hip_cache_probes.py and
tests/test_hip_dense_probes.py: the visibility helpers against the references the suite already has, the two facts the probes rest on
(``float32(ln 2) * float32(log2 e) == 1.0f``; the builder's exactness assertion), the 16-bit half ulp, and ``check_probe`` driven by a
stand-in kernel and by stand-ins that are wrong in one way each.

The stand-in runs the calls' arithmetic in fp32 torch, tile by tile: 64-key tiles, a split's tiles dealt to 4 "waves" that each keep a
running ``(m, l, O)`` in log2 units with the deferred rescale of the MFMA kernels (the maximum moves only on a jump above 8), the waves
joined, and N splits joined in natural-log units through ``ops._attn_merge_model``.  It passes both probes at every tolerance."""

from __future__ import annotations

import math

import numpy as np
import pytest
import torch

import dense_testlib
import kvcache_testlib
from kvcache_testlib import INF
from photonic_flash_attention_amd._models import _attn_merge_model
from probe_testlib import (BITS, COL_ONE, COL_SEQ, COL_UNSEEN, LN2, LOG2E, U, cache_visible, check_probe, count, dense_visible, expected,
                           half_ulp16, probe_v, stair, unseen_keys)

TILE, WAVES, THR = 64, 4, 8.0


# --- the stand-in ------------------------------------------------------------------------------------------------------------------------

def _wave_pass(s, v, tiles):
    """One wave's running (m, l, O) over its tiles: s [R,S] fp32 scores in log2 units (-inf: hidden), v [S,D] fp32."""
    R = s.shape[0]
    m = torch.full((R,), -INF)
    l = torch.zeros(R)
    O = torch.zeros(R, v.shape[1])
    for idx in tiles:
        st = s[:, idx]
        mt = torch.maximum(m, st.amax(-1))
        move = (mt - m > THR) | torch.isneginf(m)                     # the deferred rescale: a jump of 8 or less leaves m where it is
        m_new = torch.where(move, mt, m)
        f = torch.where(torch.isneginf(m), torch.zeros_like(m), torch.exp2(m - m_new))
        p = torch.where(torch.isneginf(st), torch.zeros_like(st), torch.exp2(st - torch.where(torch.isneginf(m_new), 0.0, m_new)[:, None]))
        l = l * f + p.sum(-1)
        O = O * f[:, None] + p @ v[idx]
        m = m_new
    return m, l, O


def _join(parts):
    """Waves -> one (m, l, O), the maximum exact."""
    m = torch.stack([p[0] for p in parts]).amax(0)
    l = torch.zeros_like(m)
    O = torch.zeros_like(parts[0][2])
    for mw, lw, Ow in parts:
        f = torch.where(torch.isneginf(mw), torch.zeros_like(mw), torch.exp2(mw - torch.where(torch.isneginf(m), 0.0, m)))
        l = l + lw * f
        O = O + Ow * f[:, None]
    return m, l, O


def standin(q, k, v, vis, scale, *, nsplit=1, out_dtype=torch.float32, sinks=None, mutant=None):
    """-> (o [B,H,Sq,D] of out_dtype, lse [B,H,Sq] fp32).  mutant: None, "boundary_twice" (the last key of split 0 also in split 1),
    "tile_skipped" (tile 1 of the last split), "sink_every_split", "truncate" (the 16-bit store), "lse_off" (+1e-4)."""
    B, H, Sq, D = q.shape
    Hkv, S = k.shape[1], k.shape[2]
    g = H // Hkv
    c = float(np.float32(LN2 if scale is None else scale) * np.float32(LOG2E))
    n_tiles = -(-S // TILE)
    per = -(-n_tiles // nsplit)
    o = torch.zeros(B, H, Sq, D)
    lse = torch.zeros(B, H, Sq)
    for b in range(B):
        for h in range(H):
            s = (q[b, h].float() @ k[b, h // g].float().T) * c
            s = s.masked_fill(~vis[b, h], -INF)
            vv = v[b, h // g].float()
            outs, lses = [], []
            for sp in range(nsplit):
                tiles = [torch.arange(t * TILE, min(S, (t + 1) * TILE)) for t in range(sp * per, min(n_tiles, (sp + 1) * per))]
                if mutant == "boundary_twice" and sp == 1:
                    tiles[0] = torch.cat([tiles[0][:1] - 1, tiles[0]])
                if mutant == "tile_skipped" and sp == nsplit - 1:
                    del tiles[1]
                m, l, O = _join([_wave_pass(s, vv, tiles[w::WAVES]) for w in range(WAVES)])
                if sinks is not None and (sp == 0 or mutant == "sink_every_split") and math.isfinite(float(sinks[h])):
                    s2 = torch.full_like(m, float(np.float32(float(sinks[h])) * np.float32(LOG2E)))
                    none = torch.isneginf(m)
                    l = torch.where(none, torch.ones_like(l), l + torch.exp2(s2 - torch.where(none, 0.0, m)))
                    m = torch.where(none, s2, m)
                some = l > 0
                outs.append(torch.where(some[:, None], O / torch.where(some, l, 1.0)[:, None], torch.zeros_like(O))[None, None])
                lses.append(torch.where(some, (m + torch.log2(torch.where(some, l, 1.0))) * np.float32(LN2), -INF)[None, None].float())
            if nsplit == 1:
                o[b, h], lse[b, h] = outs[0][0, 0], lses[0][0, 0]
            else:
                ob, lb = torch.empty(1, 1, Sq, D), torch.empty(1, 1, Sq)
                _attn_merge_model(outs, lses, ob, lb)
                o[b, h], lse[b, h] = ob[0, 0], lb[0, 0]
    if mutant == "lse_off":
        lse = lse + 1e-4
    if mutant == "truncate" and out_dtype != torch.float32:
        bits = 16 if out_dtype == torch.bfloat16 else 13                # fp32 -> toward zero; exact for fp16 normals
        t = (o.view(torch.int32) >> bits << bits).view(torch.float32)
        return t.to(out_dtype), lse
    return o.to(out_dtype), lse


# --- the facts the probes rest on ------------------------------------------------------------------------------------------------------

def test_ln2_times_log2e_is_one_in_fp32():
    assert np.float32(LN2) * np.float32(LOG2E) == np.float32(1.0)
    assert np.float32(np.float64(np.float32(LN2)) * LOG2E) == np.float32(1.0)          # the double product rounded to fp32
    assert np.float32(LN2 * LOG2E) == np.float32(1.0)


def test_stair_asserts_that_every_fp32_sum_is_exact():
    stair(1, 2, 1, 1, 16384, 64, torch.bfloat16, {5: 3, 9000: 9})                      # 2^9 * 2^14 < 2^24
    with pytest.raises(AssertionError, match="no longer exact"):
        stair(1, 2, 1, 1, 32768, 64, torch.bfloat16, {5: 3, 9000: 9})
    with pytest.raises(AssertionError, match="no longer exact"):
        stair(1, 2, 1, 1, 1024, 64, torch.bfloat16, {5: -7, 900: 9})
    pr = stair(2, 4, 2, 3, 128, 64, torch.float16, [{7: 5}, {100: -2}])
    assert pr["scale"] == LN2 and pr["steps"][0, :, 7].tolist() == [5, 5] and pr["steps"][1, :, 100].tolist() == [-2, -2]
    assert bool((pr["q"][..., 0] == 1).all()) and bool((pr["q"][..., 1:] == 0).all()) and float(pr["k"][1, 0, 100, 0]) == -2.0
    assert bool(torch.isfinite(pr["k"]).all()) and float(pr["k"][..., 1:].abs().max()) > 0
    assert bool((count(2, 4, 2, 3, 128, 64, torch.float16)["q"] == 0).all())


def test_probe_v_columns():
    vis = cache_visible(2, 4, 1, 256, [200, 70], window=50)
    v = probe_v(2, 2, 256, 64, torch.bfloat16, unseen_keys(vis, 2))
    assert bool(((v == 0) | (v == 1)).all())
    for j in (0, 1, 77, 255):
        assert sum(int(v[1, 1, j, t]) << t for t in range(BITS)) == j
        assert bool((v[1, 1, j, BITS:2 * BITS] == 1 - v[1, 1, j, :BITS]).all())
    assert bool((v[..., COL_ONE] == 1).all()) and bool((v[..., COL_UNSEEN + 1:] == 0).all())
    assert [sum(int(v[b, hk, 9, COL_SEQ + t]) << t for t in range(8)) for b in range(2) for hk in range(2)] == [0, 1, 2, 3]
    assert v[0, 0, :, COL_UNSEEN].nonzero().flatten().tolist() == list(range(150)) + list(range(200, 256))
    e = expected(vis, v)
    assert bool((e["C"][..., COL_UNSEEN] == 0).all()) and e["n"][:, 0, 0].tolist() == [50, 50]


def test_half_ulp16_and_why_the_bf16_bound_is_not_eps_times_ref():
    """EPS[bf16] = 2^-9 is half of bf16's unit roundoff: 257/512 rounds (to nearest) to 0.5, 2^-8 |ref| away."""
    ref = torch.tensor([257.0 / 512, 1.0, 0.75, 3.0, 0.0, 2.0 ** -20], dtype=torch.float64)
    assert half_ulp16(ref, torch.bfloat16).tolist() == [2.0 ** -9, 2.0 ** -8, 2.0 ** -9, 2.0 ** -7, 0.0, 2.0 ** -28]
    assert half_ulp16(ref, torch.float16).tolist() == [2.0 ** -12, 2.0 ** -11, 2.0 ** -12, 2.0 ** -10, 0.0, 2.0 ** -25]
    err = abs(float(ref[:1].to(torch.bfloat16)) - float(ref[0]))
    assert err == 2.0 ** -9 and err > kvcache_testlib.EPS[torch.bfloat16] * float(ref[0]) * (1 + 2.0 ** -10) + 16 * U
    g = torch.Generator().manual_seed(0)
    x = (torch.rand(4096, generator=g) * 4).double()                   # fp32 values: one rounding on the way to 16 bits
    for dt in (torch.bfloat16, torch.float16):
        assert bool(((x.to(dt).double() - x).abs() <= half_ulp16(x, dt)).all())
        assert bool((half_ulp16(x, dt) <= 2 * kvcache_testlib.EPS[dt] * x).all())
    assert bool((half_ulp16(x, torch.float16) <= kvcache_testlib.EPS[torch.float16] * x).all())


# --- the visibility helpers against the references ---------------------------------------------------------------------------------------

def _ref_vis(B, H, Sq, S, lens, **kw):
    """Who ``kvcache_testlib.reference`` lets a row see: the keys whose one-hot V column comes back non-zero."""
    q = torch.zeros(B, H, Sq, 8, dtype=torch.float64)
    k = torch.zeros(B, 1, S, 8, dtype=torch.float64)
    p = kvcache_testlib.reference(q, k, torch.eye(S, dtype=torch.float64).expand(B, 1, S, S), seqlens=torch.tensor(lens), **kw)[0]
    return p > 0


def test_cache_visible_against_the_reference():
    B, H, Sq, S = 4, 2, 5, 40
    lens = [40, 17, 3, 0]
    km = torch.rand(B, S, generator=torch.Generator().manual_seed(1)) > 0.3
    km[1] = False
    for causal, window, mask in [(False, None, None), (True, None, None), (True, 1, None), (True, 4, None), (True, 100, None),
                                 (True, None, km), (True, 6, km), (False, None, km)]:
        got = cache_visible(B, H, Sq, S, lens, causal=causal, window=window, key_mask=mask)
        assert torch.equal(got, _ref_vis(B, H, Sq, S, lens, causal=causal, window=window, key_mask=mask)), (causal, window)
    assert torch.equal(cache_visible(1, 1, 2, 8), _ref_vis(1, 1, 2, 8, [8]))
    assert not bool(cache_visible(B, H, Sq, S, lens)[2, :, :2].any()) and not bool(cache_visible(B, H, Sq, S, lens)[3].any())


def test_cache_visible_tree_words_against_tree_visible():
    B, Sq, S = 5, 8, 48
    lens = torch.tensor([48, 20, 8, 5, 30])
    g = torch.Generator().manual_seed(2)
    words = torch.randint(-2 ** 63, 2 ** 63 - 1, (B, Sq), generator=g, dtype=torch.int64)
    words[1] = torch.tensor([(1 << (i + 1)) - 1 for i in range(Sq)])       # the chain
    words[2] = -1                                                       # all ones; no prefix (len == Sq)
    words[4, 3] = 0                                                     # an empty word behind a prefix
    words[4, 4] = -2 ** 63                                              # bit 63 alone
    km = torch.rand(B, S, generator=g) > 0.2
    want = kvcache_testlib.tree_visible(words, lens, Sq, S)
    got = cache_visible(B, 3, Sq, S, lens.tolist(), tree=words)
    assert torch.equal(got, want[:, None].expand(B, 3, Sq, S))
    assert torch.equal(cache_visible(B, 3, Sq, S, lens.tolist(), tree=words, key_mask=km), (want & km[:, None])[:, None].expand(B, 3, Sq, S))
    assert torch.equal(got[1], cache_visible(B, 3, Sq, S, lens.tolist())[1]) and torch.equal(got[2], cache_visible(B, 3, Sq, S, lens.tolist(), causal=False)[2])


def test_dense_visible_against_dense_testlib():
    B, H, Sq, Sk = 3, 2, 9, 13
    g = torch.Generator().manual_seed(3)
    km = torch.rand(B, Sk, generator=g) > 0.3
    km[2] = False
    m3 = torch.rand(B, Sq, Sk, generator=g) > 0.4
    m4 = torch.rand(B, H, Sq, Sk, generator=g) > 0.4
    m4[0, 1, 4] = False
    for causal in (False, True):
        for lens in (None, [0, 1, 13], [5, 40, 12]):
            assert torch.equal(dense_visible(B, H, Sq, Sk, causal=causal, seqlens=lens), dense_testlib.visible(B, H, Sq, Sk, causal=causal, seqlens=lens))
            assert torch.equal(dense_visible(B, H, Sq, Sk, causal=causal, seqlens=lens, key_mask=km),
                               dense_testlib.visible(B, H, Sq, Sk, causal=causal, seqlens=lens, keep=km[:, None, None, :]))
        assert torch.equal(dense_visible(B, H, Sq, Sk, causal=causal, mask=m3), dense_testlib.visible(B, H, Sq, Sk, causal=causal, keep=m3[:, None]))
        assert torch.equal(dense_visible(B, H, Sq, Sk, causal=causal, mask=m4.to(torch.uint8)), dense_testlib.visible(B, H, Sq, Sk, causal=causal, keep=m4))
    assert torch.equal(dense_visible(B, H, Sq, Sk, mask=m4[:1, :, :1]), dense_testlib.visible(B, H, Sq, Sk, keep=m4[:1, :, :1]))


def test_expected_against_the_fp64_reference():
    """``expected`` (counts and powers of two) against ``kvcache_testlib.reference`` / ``with_sink`` on the same operands: 1e-12."""
    B, H, Hkv, Sq, S, D = 2, 4, 2, 5, 200, 64
    lens = [200, 3]
    vis = cache_visible(B, H, Sq, S, lens, window=70)
    v = probe_v(B, Hkv, S, D, torch.float64, unseen_keys(vis, Hkv))
    sinks = torch.tensor([0.0, -INF, 0.0, -INF])
    for pr in (count(B, H, Hkv, Sq, S, D, torch.float64), stair(B, H, Hkv, Sq, S, D, torch.float64, {131: 9, 150: 3, 199: -4, 129: 12})):
        ref = kvcache_testlib.reference(pr["q"], pr["k"], v, seqlens=torch.tensor(lens), window=70, scale=pr["scale"])
        for e, r in ((expected(vis, v, pr["steps"]), ref), (expected(vis, v, pr["steps"], sinks), kvcache_testlib.with_sink(ref, sinks))):
            assert float((e["ref_o"] - r[0]).abs().max()) <= 1e-12
            assert torch.equal(torch.isneginf(e["ref_lse"]), torch.isneginf(r[1]))
            fin = torch.isfinite(r[1])
            assert float((e["ref_lse"] - r[1])[fin].abs().max()) <= 1e-12
            assert bool(e["dead"][1, :, :2].all()) and not bool(e["dead"][0].any())
    half = expected(vis, v, None, None, torch.tensor([0.5, 0.25]))
    assert torch.equal(half["ref_o"][:, :2] * 2, expected(vis, v)["ref_o"][:, :2]) and torch.equal(half["ref_o"][:, 2:] * 4, expected(vis, v)["ref_o"][:, 2:])


# --- check_probe: the honest stand-in passes, every mutant is rejected by the check meant for it ---------------------------------------

B, H, HKV, SQ, S, D = 2, 2, 1, 40, 1024, 64
LENS = [1024, 777]
W = 300
SINKS = torch.tensor([0.0, -INF])
# steps (CPU stand-in: tiles of 64, 4 waves, 2 splits of 8 tiles): +3 early (deferred), 9 in a late tile of wave 1 (rescale), 12 in
# split 1 / wave 2, 1 and 6 on the two newest keys of sequence 1, and under the window of 300 over sequence 0 (row 0's first key is
# 1024 - 40 + 1 - 300 = 685): 2 on that key, 13 on the one just outside it, 684
STEPS = [{10: 3, 330: 9, 700: 12, 1023: 5, 685: 2, 684: 13}, {10: 3, 330: 9, 700: 12, 776: 6, 775: 1}]


def _problem(kind, dtype, window=None):
    vis = cache_visible(B, H, SQ, S, LENS, window=window)
    v = probe_v(B, HKV, S, D, dtype, unseen_keys(vis, HKV))
    pr = count(B, H, HKV, SQ, S, D, dtype) if kind == "count" else stair(B, H, HKV, SQ, S, D, dtype, STEPS)
    return pr, v, vis


@pytest.mark.parametrize("kind", ["count", "stair"])
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["o32", "bf16", "fp16"])
def test_the_honest_standin_passes_both_probes(kind, out_dtype):
    dtype = torch.bfloat16 if out_dtype == torch.float32 else out_dtype
    for window in (None, W):
        pr, v, vis = _problem(kind, dtype, window)
        for nsplit, sinks in ((1, None), (2, None), (5, SINKS), (1, SINKS)):
            o, lse = standin(pr["q"], pr["k"], v, vis, pr["scale"], nsplit=nsplit, out_dtype=out_dtype, sinks=sinks)
            ro, rl = check_probe(o, lse, expected(vis, v, pr["steps"], sinks), out_dtype, f"{kind} W {window} splits {nsplit}", kind == "count",
                                     merged=nsplit > 1)
            assert ro <= 1 and rl <= 1


def _run(kind, vis_kernel=None, out_dtype=torch.float32, window=None, sinks=None, swap_page=False, **kw):
    """The stand-in on ``vis_kernel`` (what the mutant lets the rows see) against the expectation of the true rule."""
    pr, v, vis = _problem(kind, torch.bfloat16 if out_dtype == torch.float32 else out_dtype, window)
    k2, v2 = pr["k"], v
    if swap_page:                                                       # keys 128 .. 191 of sequence 0 come from sequence 1's page
        k2, v2 = pr["k"].clone(), v.clone()
        k2[0, :, 128:192], v2[0, :, 128:192] = pr["k"][1, :, 128:192], v[1, :, 128:192]
    o, lse = standin(pr["q"], k2, v2, vis if vis_kernel is None else vis_kernel(vis.clone()), pr["scale"], out_dtype=out_dtype, sinks=sinks, **kw)
    return check_probe(o, lse, expected(vis, v, pr["steps"], sinks), out_dtype, "mutant", kind == "count", merged=kw.get("nsplit", 1) > 1)


def _newest_hidden(vis):
    vis[1, :, :, LENS[1] - 1] = False                                   # in sequence 1 only
    return vis


def _window_too_wide(vis):
    for i in range(16, 32):                                             # the second row block of sequence 0 only
        vis[0, :, i, LENS[0] - SQ + i + 1 - W - 1] = True
    return vis


def _diagonal_off(vis):
    for i in range(SQ - 32, SQ - 1):                                    # the last 32 rows see the key behind their diagonal
        vis[0, :, i, LENS[0] - SQ + i + 1] = True
    return vis


def test_the_single_key_mutants_are_named_with_key_and_direction():
    with pytest.raises(AssertionError, match=rf"\(1, 0, {SQ - 1}\): 777 keys expected, 776 found -- the counts differ; key {LENS[1] - 1} is missing"):
        _run("count", _newest_hidden)
    with pytest.raises(AssertionError, match=rf"\(0, 0, 16\): 300 keys expected, 301 found .* key {1024 - 40 + 16 - 300} is extra"):
        _run("count", _window_too_wide, window=W)
    with pytest.raises(AssertionError, match=r"\(0, 0, 0\): 985 keys expected, 986 found .* key 511 is extra"):
        _run("count", nsplit=2, mutant="boundary_twice")
    with pytest.raises(AssertionError, match=rf"\(0, 0, {SQ - 32}\): .* key {1024 - 32 + 1} is extra"):
        _run("count", _diagonal_off)


def test_the_other_mutants_are_rejected_by_the_check_meant_for_them():
    with pytest.raises(AssertionError, match=r"\(0, 0, 0\): 985 keys expected, 921 found -- the counts differ; columns"):
        _run("count", nsplit=2, mutant="tile_skipped")
    with pytest.raises(AssertionError, match=rf"the counts differ; columns off: \[{COL_SEQ}\]"):
        _run("count", swap_page=True)                                   # the same keys of another sequence: only its number shows
    with pytest.raises(AssertionError, match=r"\(0, 0, 0\): 986 keys expected, 990 found -- the counts differ"):
        _run("count", nsplit=5, sinks=SINKS, mutant="sink_every_split")
    for dt in (torch.bfloat16, torch.float16):
        with pytest.raises(AssertionError, match="O over the tolerance"):
            _run("stair", out_dtype=dt, mutant="truncate")
    with pytest.raises(AssertionError, match="LSE over the tolerance"):
        _run("stair", mutant="lse_off")
    with pytest.raises(AssertionError, match="LSE over the tolerance"):  # ... in count mode too: at 985 keys exp(1e-4) moves the count by 0.1
        _run("count", mutant="lse_off")
    with pytest.raises(AssertionError, match="986 found -- the counts differ"):     # a 16-bit O carries no count; the LSE's does
        _run("count", out_dtype=torch.bfloat16, nsplit=2, mutant="boundary_twice")


def test_the_stair_probe_rejects_the_visibility_mutants_too():
    for mutate, kw in ((_newest_hidden, {}), (_window_too_wide, dict(window=W)), (_diagonal_off, {})):
        with pytest.raises(AssertionError, match="over the tolerance"):
            _run("stair", mutate, **kw)
    for mutant, kw in (("boundary_twice", dict(nsplit=2)), ("tile_skipped", dict(nsplit=2)), ("sink_every_split", dict(nsplit=5, sinks=SINKS))):
        with pytest.raises(AssertionError, match="over the tolerance"):
            _run("stair", mutant=mutant, **kw)


def test_check_probe_rejects_dead_rows_that_are_not_dead_and_non_finite_output():
    lens = [1024, 20]                                                   # sequence 1: 20 rows of 40 see nothing
    vis = cache_visible(B, H, SQ, S, lens)
    v = probe_v(B, HKV, S, D, torch.bfloat16, unseen_keys(vis, HKV))
    pr = count(B, H, HKV, SQ, S, D, torch.bfloat16)
    for sinks in (None, SINKS):
        e = expected(vis, v, None, sinks)
        o, lse = standin(pr["q"], pr["k"], v, vis, None, sinks=sinks)
        check_probe(o, lse, e, torch.float32, "dead rows", True)
        assert bool(e["dead"][1, :, :20].all()) and float(e["ref_lse"][1, 0, 0]) == (0.0 if sinks is not None else -INF)
        assert float(e["ref_lse"][1, 1, 0]) == -INF
        bad = o.clone()
        bad[1, 1, 3, 5] = 2.0 ** -30
        with pytest.raises(AssertionError, match=r"\(1, 1, 3\).* a row with no visible key"):
            check_probe(bad, lse, e, torch.float32, "", True)
        bad = lse.clone()
        bad[1, 1, 3] = 0.0
        with pytest.raises(AssertionError, match=r"\(1, 1, 3\).* a row with no visible key"):
            check_probe(o, bad, e, torch.float32, "", True)
        bad = lse.clone()
        bad[0, 0, 0] = -INF
        with pytest.raises(AssertionError, match="non-finite LSE"):
            check_probe(o, bad, e, torch.float32, "", True)
        bad = o.clone()
        bad[0, 0, 0, 63] = float("nan")
        with pytest.raises(AssertionError, match="non-finite output"):
            check_probe(bad, lse, e, torch.float32, "", True)
    with pytest.raises(AssertionError, match="the output is"):
        check_probe(o.to(torch.bfloat16), lse, e, torch.float32)

"""GPU tests of ``ops.norm_rope_append`` (``pfa_norm_rope_append``: QK-norm, rotary and the FP8 store fused into the KV-cache append) and
of the ``q_norm_weight=`` keywords of the calls over a KV cache.  Every comparison is bit for bit against the CPU model
(``_models._norm_rope_append_model``, itself held to fp64 by tests/test_norm_rope_append_host.py) over whole buffers prefilled with NaN,
which also proves that nothing else was written.

Shapes: H 3 / Hkv 1, so a row has 5 * G items and waves and workgroups straddle rows and the Q / K / V head kinds; D 64 (G 4) and 128
(G 8); pages of 64 keys.  Ragged: an empty sequence, one with more rows than keys (rows at pos < 0) and one cut by ``max_seqlen_q`` whose
step crosses a page boundary -- with ``drop`` into a page id >= num_pages, while the second sequence's page is -1.  Uniform: 12 rows, two
sequences with pos < 0, one crossing key 64.  ``pos_offsets`` pushes the last sequence past ``max_pos``."""

from __future__ import annotations

import itertools

import pytest
import torch

from kvcache_testlib import capture, device, i32
from photonic_flash_attention_amd import ops

pytestmark = pytest.mark.gpu

H, HKV, PAGE, NP, MAX_POS, SQ = 3, 1, 64, 8, 100, 12
CU, MAX_SQ, OFFS = [0, 0, 7, 40], 20, [0, 2, 60]
LENS = {True: [5, 3, 140], False: [5, 3, 70]}                     # ragged: keys 120 .. 139 cross 128; uniform: keys 58 .. 69 cross 64
WEIGHTS = ("fp32", "16-bit", "q only", "k only", "none")
NAN = float("nan")


def bits(t):
    return t.view(torch.uint8 if t.element_size() == 1 else torch.int16)


def cases():
    """Every instantiation (16-bit type x G x ragged x paged x pairing x quantising store) once; the run-time choices cycle over them."""
    for n, (dtype, D, ragged, paged, il, fp8) in enumerate(itertools.product((torch.bfloat16, torch.float16), (64, 128), (False, True),
                                                                             (False, True), (False, True), (False, True))):
        weights, R = WEIGHTS[n % 5], (0, 32, D)[n % 3]
        if R == 0 and (il or weights == "none"):
            R = 32
        yield pytest.param(dtype, D, ragged, paged, il, fp8, R, weights, weights != "none" and n // 2 % 2 == 1, n % 3 == 0, n % 4 < 2,
                           id=f"{n}-{str(dtype)[6:]}-d{D}-r{R}-{'ragged' if ragged else 'uniform'}-{'paged' if paged else 'contig'}"
                              f"{'-il' if il else ''}{'-fp8' if fp8 else ''}-{weights.replace(' ', '_')}")


def problem(dtype, D, ragged, paged, fp8, R, weights, drop, seed):
    """CPU tensors: (k, v, caches, keywords with q).  The caches hold NaN (FP8: NaN bytes) everywhere."""
    g = torch.Generator().manual_seed(seed)
    shape = (lambda h: (40, h, D)) if ragged else (lambda h: (3, SQ, h, D))
    q, k, v = (torch.randn(shape(h), generator=g).to(dtype) for h in (H, HKV, HKV))
    if not ragged:
        q, k, v = (t.transpose(1, 2) for t in (q, k, v))          # [B, H, Sq, D] views of [B, Sq, H, D] buffers
    cdt = torch.uint8 if fp8 else dtype
    fill = 0x7f if fp8 else NAN
    if paged:                                                     # flash-attn style pools [NP, page, Hkv, D], passed transposed
        caches = [torch.full((NP, PAGE, HKV, D), fill, dtype=cdt).transpose(1, 2) for _ in range(2)]
    else:
        caches = [torch.full((3, 3 * PAGE, HKV, D), fill, dtype=cdt).transpose(1, 2) for _ in range(2)]
    kw = dict(q=q, cache_seqlens=torch.tensor(LENS[ragged], dtype=torch.int32))
    if ragged:
        kw.update(cu_seqlens_q=torch.tensor(CU, dtype=torch.int32), max_seqlen_q=MAX_SQ)
    if paged:
        kw["block_table"] = torch.tensor([[1, 2, 0], [-1 if drop else 3, 4, 0], [6, 5, NP + 1 if drop else 7]], dtype=torch.int32)
    if R:
        cos, sin = ops.rotary_tables(MAX_POS, R)
        kw.update(rotary_cos=cos, rotary_sin=sin, pos_offsets=torch.tensor(OFFS, dtype=torch.int32))
    wq, wk = torch.rand(D, generator=g) + 0.5, torch.randn(D, generator=g)
    if weights == "16-bit":
        wq, wk = wq.to(dtype), wk.to(dtype)
    if weights not in ("none", "k only"):
        kw["q_weight"] = wq
    if weights not in ("none", "q only"):
        kw["k_weight"] = wk
    if fp8:
        kw.update(k_descale=torch.rand(3, HKV, generator=g) + 0.5, v_descale=torch.rand(3, HKV, generator=g) + 0.5)
    return k, v, caches, kw


def to_dev(x, dev):
    """A tensor on ``dev`` with the strides it has (a FP8 cache as its view); anything else as it is."""
    if not torch.is_tensor(x):
        return x
    y = torch.empty_strided(x.shape, x.stride(), dtype=x.dtype, device=dev)
    y.copy_(x)
    return y


def run(k, v, caches, kw, dev, inplace, **flags):
    """``norm_rope_append`` on copies of the tensors on ``dev`` -> (q_out, k cache, v cache)."""
    fp8 = "k_descale" in kw
    k, v, kc, vc = (to_dev(t, dev) for t in (k, v, *caches))
    kw = {n: to_dev(x, dev) for n, x in kw.items()}
    q_out = kw["q"] if inplace else torch.full_like(kw["q"], NAN)
    got = ops.norm_rope_append(k, v, kc.view(ops.FP8) if fp8 else kc, vc.view(ops.FP8) if fp8 else vc, q_out=q_out, **kw, **flags)
    assert got is q_out
    return got, kc, vc


@pytest.mark.parametrize("dtype,D,ragged,paged,il,fp8,R,weights,unit,inplace,drop", cases())
def test_kernel_equals_the_cpu_model_bit_for_bit_over_whole_buffers(dtype, D, ragged, paged, il, fp8, R, weights, unit, inplace, drop):
    k, v, caches, kw = problem(dtype, D, ragged, paged, fp8, R, weights, drop, seed=D + R)
    flags = dict(unit_offset=unit, rotary_interleaved=il)
    want = run(k, v, caches, kw, torch.device("cpu"), inplace, **flags)
    got = run(k, v, caches, kw, device(), inplace, **flags)
    torch.cuda.synchronize()
    for name, a, b in zip(("q_out", "k cache", "v cache"), got, want):
        assert torch.equal(bits(a).cpu(), bits(b)), f"{name}: {int((bits(a).cpu() != bits(b)).sum())} elements differ"
    assert int((bits(want[1]) != bits(caches[0])).sum()) > 0                                         # the case wrote keys


@pytest.mark.parametrize("ragged,paged,il", [(True, True, False), (False, False, True)])
def test_without_weights_it_is_rope_append_bit_for_bit(ragged, paged, il):
    k, v, caches, kw = problem(torch.bfloat16, 128, ragged, paged, False, 64, "none", True, seed=5)
    outs = []
    for fn in (ops.norm_rope_append, ops.rope_append):
        kd, vd, kc, vc = (to_dev(t, device()) for t in (k, v, *caches))
        kwd = {n: to_dev(x, device()) for n, x in kw.items()}
        outs.append((fn(kd, vd, kc, vc, q_out=torch.full_like(kwd["q"], NAN), rotary_interleaved=il, **kwd), kc, vc))
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(*outs))


@pytest.mark.parametrize("dtype,D,R,il,per_sequence", [(torch.bfloat16, 128, 64, False, True), (torch.float16, 64, 64, True, False),
                                                       (torch.bfloat16, 64, 32, False, False)])
def test_fp8_bytes_equal_the_quantising_append_of_what_the_16_bit_call_stores(dtype, D, R, il, per_sequence):
    dev, lens = device(), [40, 12, 70]
    k, v, _, kw = problem(dtype, D, False, False, False, R, "fp32", False, seed=9)
    k, v = k.clone(), v.clone()
    k[1, 0, 3, 5] = v[2, 0, 7, 9] = NAN                                                              # a NaN stays NaN
    kw = {n: to_dev(x, dev) for n, x in dict(kw, cache_seqlens=torch.tensor(lens, dtype=torch.int32)).items()}
    k, v = to_dev(k, dev), to_dev(v, dev)
    c16 = [torch.full((3, HKV, 3 * PAGE, D), NAN, dtype=dtype, device=dev) for _ in range(2)]
    fused, split = ([torch.full((3, HKV, 3 * PAGE, D), 0x7f, dtype=torch.uint8, device=dev).view(ops.FP8) for _ in range(2)] for _ in range(2))
    g = torch.Generator().manual_seed(3)
    kd, vd = ((torch.rand((3, HKV) if per_sequence else (HKV,), generator=g) + 0.5).to(dev) for _ in range(2))
    q16 = ops.norm_rope_append(k, v, *c16, rotary_interleaved=il, **kw)
    q8 = ops.norm_rope_append(k, v, *fused, rotary_interleaved=il, k_descale=kd, v_descale=vd, **kw)
    k16 = torch.stack([c16[0][b, :, n - SQ:n] for b, n in enumerate(lens)])                          # the K rows the 16-bit call stored
    ops.kv_append(k16, v, *split, cache_seqlens=kw["cache_seqlens"], k_descale=kd, v_descale=vd)
    torch.cuda.synchronize()
    assert torch.equal(bits(q8), bits(q16))
    for a, b in zip(fused, split):
        assert torch.equal(bits(a), bits(b)) and int((bits(a) != 0x7f).sum()) > 1000
    assert int(bits(fused[0])[1, 0, 3, 5]) & 0x7f == 0x7f and int(bits(fused[1])[2, 0, lens[2] - SQ + 7, 9]) & 0x7f == 0x7f


@pytest.mark.parametrize("ragged", [False, True])
def test_cache_calls_with_the_norm_keywords_equal_the_same_calls_on_the_ops_outputs(ragged):
    dev = device()
    k, v, caches, kw = problem(torch.bfloat16, 128, ragged, True, False, 64, "fp32", False, seed=11)
    k, v = to_dev(k, dev), to_dev(v, dev)
    kw = {n: to_dev(x, dev) for n, x in kw.items()}
    q, wq, wk = kw.pop("q"), kw.pop("q_weight"), kw.pop("k_weight")
    one, two = ([torch.zeros_like(to_dev(c, dev)) for c in caches] for _ in range(2))
    call = ops.fa3_prefill_varlen if ragged else ops.fa3_decode
    outs = [torch.zeros_like(q) for _ in range(2)] if ragged else [None, None]                       # packed rows no sequence covers stay
    o1, l1 = call(q, *one, k_new=k, v_new=v, q_norm_weight=wq, k_norm_weight=wk, qk_norm_unit_offset=True, return_lse=True, out=outs[0], **kw)
    q2 = ops.norm_rope_append(k, v, *two, q=q, q_weight=wq, k_weight=wk, unit_offset=True, **kw)
    rest = {n: x for n, x in kw.items() if n not in ("rotary_cos", "rotary_sin", "pos_offsets")}
    o2, l2 = call(q2, *two, return_lse=True, out=outs[1], **rest)
    torch.cuda.synchronize()
    rows = slice(0, CU[2] + MAX_SQ) if ragged else slice(None)
    assert torch.equal(bits(o1), bits(o2)) and torch.equal(l1[..., rows], l2[..., rows]) and all(torch.equal(bits(a), bits(b)) for a, b in zip(one, two))
    assert bool(torch.isfinite(o1[CU[1]:CU[1] + 7] if ragged else o1).all())


def test_a_captured_step_replays_after_lengths_table_weights_and_inputs_change():
    dev = device()
    k, v, caches, kw = problem(torch.bfloat16, 128, False, True, False, 64, "fp32", False, seed=13)
    k, v = to_dev(k, dev), to_dev(v, dev)
    kw = {n: to_dev(x, dev) for n, x in kw.items()}
    q = kw.pop("q")
    pools = [torch.zeros_like(to_dev(c, dev)) for c in caches]
    rest = {n: x for n, x in kw.items() if n in ("cache_seqlens", "block_table")}

    def step(kc, vc):
        q2 = ops.norm_rope_append(k, v, kc, vc, q=q, **kw)
        return (q2,) + ops.fa3_decode(q2, kc, vc, return_lse=True, **rest)

    graph, res = capture(lambda: step(*pools))
    g = torch.Generator(device=dev).manual_seed(17)
    for lens, table in (([30, 64, 150], [[2, 1, 0], [3, 4, 0], [5, 6, 7]]), ([12, 100, 129], [[7, 1, 0], [3, 2, 0], [4, 6, 5]])):
        kw["cache_seqlens"].copy_(i32(lens))
        kw["block_table"].copy_(i32(table))
        for t in (q, k, v, kw["q_weight"], kw["k_weight"]):
            t.copy_(torch.randn(t.shape, generator=g, device=dev).to(t.dtype))
        for p in pools:
            p.zero_()
        graph.replay()
        eager_pools = [torch.zeros_like(p) for p in pools]
        eager = step(*eager_pools)
        torch.cuda.synchronize()
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(res[:2] + tuple(pools), eager[:2] + tuple(eager_pools)))
        assert torch.equal(res[2], eager[2]) and bool(torch.isfinite(res[1]).all())

"""CPU-side tests (no GPU) of QK-norm, rotary and the FP8 store fused into the KV-cache append (``pfa_norm_rope_append*``, declared in
``include/pfa_hip_norm_rope_append.h`` and bound by ``_capi_norm_rope_append``; ``ops.norm_rope_append``; the ``q_norm_weight=`` keywords
of the three calls over a KV cache and of ``PagedKVCache.write_step``): the struct against its mirror, every rung of the check ladder and
its precedence over the later ones, the plain-torch model against fp64 under the forward bound of tests/qk_norm_testlib.py and against
the models it is composed of, and the refusals."""

from __future__ import annotations

import pytest
import torch

import qk_norm_testlib as Q
from capi_testlib import ALIGN, DTYPE, FLAGS, HEAD_DIM, NULL, OK, SHAPE, SIZE, STRIDE, built_lib
from photonic_flash_attention_amd import _capi, _capi_norm_rope_append as nra, ops
from photonic_flash_attention_amd.integration.pytorch.paged_cache import PagedKVCache
from test_capi_conformance import mirrors_of, prototype_mismatches, read_header, struct_mismatches

H, HKV, PAGE = 3, 1, 64
FP8_ON = dict(kv_dtype=3, k_descale=0x7000, v_descale=0x7400)


def args(**over):
    """A valid ragged, paged ``pfa_norm_rope_append_args``: B 3, H 3 / Hkv 1, D 64, rot_dim 32, both weights fp32, a 16-bit pool."""
    d = over.get("D", 64)
    base = dict(q=0x100000, q_out=0x200000, k_new=0x300000, v_new=0x400000, k_cache=0x1000000, v_cache=0x2000000, cos=0x500000, sin=0x600000,
                cu_seqlens_q=0x9000, cache_seqlens=0x9100, pos_offsets=0x9200, q_weight=0x700000, k_weight=0x710000, block_table=0xA000,
                block_table_stride_b=4, page_size=PAGE, num_pages=20, B=3, H=H, Hkv=HKV, total_new=40, max_seqlen_q=16, Smax=4 * PAGE, D=d,
                rot_dim=32, max_pos=128, dtype=0, weight_dtype=2, kv_dtype=0, cs_stride=16, eps=1e-6)
    for pre, h in (("q", H), ("qo", H), ("kn", HKV), ("vn", HKV), ("k", HKV), ("v", HKV)):
        base.update({f"{pre}_stride_s": h * d, f"{pre}_stride_h": d})
    base.update(k_stride_b=PAGE * HKV * d, v_stride_b=PAGE * HKV * d)
    return nra.make_norm_rope_append_args(**dict(base, **over))


# the rungs of the header's "Field rules", in the order their errors are reported (the size rule is checked apart)
RULES = [
    (dict(flags=4), FLAGS), (dict(reserved1=1), FLAGS), (dict(q=0, q_out=0, H=0), FLAGS),             # ... q_weight without q
    (dict(flags=2, q_weight=0, k_weight=0), FLAGS),                                                  # unit offset without a weight
    (dict(rot_dim=0, cos=0, sin=0, q_weight=0, k_weight=0), FLAGS),                                  # nothing to do: pfa_kv_append
    (dict(block_table=0), FLAGS), (dict(qo_stride_b=64), FLAGS),
    (dict(k_new=0), NULL), (dict(cache_seqlens=0), NULL), (dict(q_out=0), NULL), (dict(v_descale=0x7400), NULL), (dict(sin=0), NULL),
    (dict(rot_dim=0), NULL),
    (dict(B=0), SHAPE), (dict(max_pos=0), SHAPE), (dict(eps=-1.0), SHAPE), (dict(page_size=32), SHAPE), (dict(max_seqlen_q=41), SHAPE),
    (dict(D=256), HEAD_DIM), (dict(D=32), HEAD_DIM), (dict(rot_dim=24), HEAD_DIM), (dict(rot_dim=80), HEAD_DIM),
    (dict(dtype=2), DTYPE), (dict(weight_dtype=1), DTYPE), (dict(kv_dtype=1), DTYPE), (dict(kv_dtype=0, k_descale=0x7000, v_descale=0x7400), DTYPE),
    (dict(kv_dtype=3), DTYPE),                                                                       # an FP8 cache without descales
    (dict(q_stride_s=196), STRIDE), (dict(k_stride_s=-64), STRIDE), (dict(cs_stride=8), STRIDE), (dict(FP8_ON, v_stride_h=72), STRIDE),
    (dict(FP8_ON, ds_sb=-1), STRIDE),
    (dict(q=0x100008), ALIGN), (dict(k_weight=0x710004), ALIGN), (dict(pos_offsets=0x9202), ALIGN), (dict(FP8_ON, k_descale=0x7002), ALIGN),
    (dict(total_new=1 << 30, max_seqlen_q=1 << 30), SHAPE),                                          # the grid
]


@pytest.fixture(scope="module")
def lib():
    built_lib()
    return nra.load()


def test_struct_prototypes_and_exports_match_the_binding(lib, tmp_path):
    structs, protos, layout = read_header("pfa_hip_norm_rope_append.h", str(tmp_path))
    assert struct_mismatches(structs, layout, mirrors_of(nra), dict(pfa_norm_rope_append_args=376)) == []
    assert prototype_mismatches(protos, nra._PROTOTYPES, dict(mirrors_of(_capi), **mirrors_of(nra))) == []
    assert sorted(nra.EXPORTS) == ["pfa_norm_rope_append", "pfa_norm_rope_append_check", "pfa_norm_rope_append_describe"] == sorted(protos)
    assert all(getattr(lib, n) is not None for n in nra.EXPORTS) and not set(nra.EXPORTS) & set(_capi.EXPORTS)
    assert (nra.PFA_NRA_INTERLEAVED, nra.PFA_NRA_UNIT_OFFSET) == (1, 2)


def test_check_ladder_every_rung_and_its_precedence(lib):
    check = lambda a: lib.pfa_norm_rope_append_check(a)
    assert check(args()) == OK and check(None) == NULL and check(args(size=8, flags=4)) == SIZE
    for over in (dict(q=0, q_out=0, H=0, q_weight=0), dict(FP8_ON), dict(FP8_ON, ds_sb=HKV), dict(rot_dim=0, cos=0, sin=0), dict(k_weight=0),
                 dict(D=128, rot_dim=128, cs_stride=64), dict(flags=3, weight_dtype=0), dict(cu_seqlens_q=0, q_stride_b=16 * H * 64, total_new=48)):
        assert check(args(**over)) == OK, over
    pairs = 0
    for i, (first, status) in enumerate(RULES):
        assert check(args(**first)) == status, first
        assert lib.pfa_norm_rope_append(args(**first), None) == status                              # ... before anything is enqueued
        for later, _ in RULES[i + 1:]:
            if not set(first) & set(later):
                assert check(args(**first, **later)) == status, (first, later)                      # of two broken rules the earlier wins
                pairs += 1
    assert pairs > 500


# ---- the model: a ragged paged fixture -- an empty sequence, one with more rows than keys (pos < 0), one cut by max_seqlen_q ------------

CU, LENS, MAX_SQ, OFFS, MAX_POS = [0, 0, 7, 40], [5, 3, 100], 20, [0, 2, 60], 128


def problem(D, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(40, h, D, generator=g).to(dtype) for h in (H, HKV, HKV))
    table = torch.tensor([[1, 2], [3, 4], [6, 5]], dtype=torch.int32)
    kw = dict(cache_seqlens=torch.tensor(LENS, dtype=torch.int32), cu_seqlens_q=torch.tensor(CU, dtype=torch.int32), max_seqlen_q=MAX_SQ,
              block_table=table, pos_offsets=torch.tensor(OFFS, dtype=torch.int32))
    return q, k, v, kw, (torch.rand(D, generator=g) + 0.5, torch.randn(D, generator=g))


def pools(D, dtype):
    if dtype == ops.FP8:
        return tuple(torch.full((8, HKV, PAGE, D), 0x7f, dtype=torch.uint8).view(ops.FP8) for _ in range(2))
    return tuple(torch.full((8, HKV, PAGE, D), float("nan"), dtype=dtype) for _ in range(2))


def bits(t):
    return t.view(torch.uint8 if t.element_size() == 1 else torch.int16)


@pytest.mark.parametrize("D,R,dtype,interleaved,unit", [(64, 32, torch.bfloat16, False, False), (128, 128, torch.float16, True, True),
                                                        (128, 0, torch.bfloat16, False, True)])
def test_model_against_fp64_within_the_forward_bound_of_qk_norm(D, R, dtype, interleaved, unit):
    q, k, v, kw, (wq, wk) = problem(D, dtype)
    cos, sin = ops.rotary_tables(MAX_POS, R) if R else (None, None)
    kp, vp = pools(D, dtype)
    q_out = torch.full_like(q, float("nan"))
    got = ops.norm_rope_append(k, v, kp, vp, q=q, q_out=q_out, q_weight=wq, k_weight=wk, unit_offset=unit, rotary_cos=cos, rotary_sin=sin,
                               rotary_interleaved=interleaved, **(kw if R else dict(kw, pos_offsets=None)))
    assert got is q_out
    worst, written = 0.0, torch.zeros(40, dtype=torch.bool)
    for b, n in enumerate(LENS):
        sq = min(CU[b + 1] - CU[b], MAX_SQ)
        if sq < 1:
            continue
        pos = torch.arange(n - sq, n)
        c = s = None
        if R:
            at = (pos + OFFS[b]).clamp(0, MAX_POS - 1)
            c, s = cos[at][None, None].double(), sin[at][None, None].double()
        rows = slice(CU[b], CU[b] + sq)
        written[rows] = True
        worst = max(worst, Q.forward_ratio(q_out[rows].transpose(0, 1)[None], q[rows].transpose(0, 1)[None], wq, 1e-6, unit, c, s, interleaved))
        keep = pos >= 0                                                                             # rows in front of key 0 are dropped
        page = kw["block_table"][b, pos[keep] // PAGE].long()
        k_got, v_got = kp[page, :, pos[keep] % PAGE], vp[page, :, pos[keep] % PAGE]                  # [rows, Hkv, D]
        ck, sk = (None, None) if c is None else (c[:, :, keep], s[:, :, keep])
        worst = max(worst, Q.forward_ratio(k_got.transpose(0, 1)[None], k[rows][keep].transpose(0, 1)[None], wk, 1e-6, unit, ck, sk, interleaved))
        assert torch.equal(bits(v_got), bits(v[rows][keep]))
    print(f"worst ratio to the forward bound {worst:.3f}")
    assert worst <= 1.0
    assert bool(torch.isnan(q_out[~written]).all()) and int((~torch.isnan(kp[:, 0, :, 0])).sum()) == 0 + 3 + 20     # nothing else is written


@pytest.mark.parametrize("interleaved", [False, True])
def test_model_without_weights_is_the_rope_append_model_bit_for_bit(interleaved):
    q, k, v, kw, _ = problem(64, torch.bfloat16, 1)
    cos, sin = ops.rotary_tables(MAX_POS, 32)
    outs = []
    for fn in (ops.norm_rope_append, ops.rope_append):
        kp, vp = pools(64, torch.bfloat16)
        outs.append((fn(k, v, kp, vp, q=q, q_out=torch.full_like(q, float("nan")), rotary_cos=cos, rotary_sin=sin,
                        rotary_interleaved=interleaved, **kw), kp, vp))
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(*outs))


def test_model_with_descales_is_quantize_kv_of_the_16_bit_models_cache_byte_for_byte():
    q, k, v, kw, (wq, wk) = problem(64, torch.float16, 2)
    k[10, 0, 3] = v[11, 0, 5] = float("nan")
    cos, sin = ops.rotary_tables(MAX_POS, 32)
    common = dict(kw, q=q, q_weight=wq, k_weight=wk, rotary_cos=cos, rotary_sin=sin)
    c16, c8 = pools(64, torch.float16), pools(64, ops.FP8)
    kd, vd = torch.rand(HKV) + 0.5, torch.rand(HKV) + 0.5
    q16 = ops.norm_rope_append(k, v, *c16, q_out=torch.full_like(q, float("nan")), **common)
    q8 = ops.norm_rope_append(k, v, *c8, q_out=torch.full_like(q, float("nan")), k_descale=kd, v_descale=vd, **common)
    assert torch.equal(bits(q16), bits(q8))
    for got, c, d in zip(c8, c16, (kd, vd)):
        assert torch.equal(bits(got), bits(ops.quantize_kv(c, d))) and int((bits(got) != 0x7f).sum()) > 1000


def test_refusals_of_the_cache_calls_and_write_step():
    bf = torch.bfloat16
    q, k, v, kw, (wq, wk) = problem(64, bf)
    q4, k4, lens = q[:4].view(1, 4, H, 64).transpose(1, 2), k[:4].view(1, 4, HKV, 64).transpose(1, 2), kw["cache_seqlens"][:1]
    kc, k8, ones = torch.zeros(1, HKV, 128, 64, dtype=bf), torch.zeros(1, HKV, 128, 64).to(ops.FP8), torch.ones(HKV)
    calls = ((ops.fa3_decode, (q4, kc, kc), (q4, k8, k8), dict(k_new=k4, v_new=k4)),
             (ops.fa3_prefill_cache, (q4, kc, kc), (q4, k8, k8), dict(k_new=k4, v_new=k4)),
             (ops.fa3_prefill_varlen, (q[:4], kc, kc), (q[:4], k8, k8), dict(k_new=k[:4], v_new=k[:4], cu_seqlens_q=kw["cu_seqlens_q"][:2] * 0,
                                                                           max_seqlen_q=4)))
    for fn, pos, pos8, new in calls:
        ragged = {n: x for n, x in new.items() if n not in ("k_new", "v_new")}
        with pytest.raises(ValueError, match="need k_new, v_new and cache_seqlens"):
            fn(*pos, cache_seqlens=lens, q_norm_weight=wq, k_norm_weight=wq, **ragged)
        with pytest.raises(ValueError, match="qk_norm_unit_offset needs"):
            fn(*pos, cache_seqlens=lens, qk_norm_unit_offset=True, **new)
        with pytest.raises(ValueError, match="q_norm_weight / k_norm_weight is not supported with an FP8"):
            fn(*pos8, cache_seqlens=lens, k_norm_weight=wq, k_descale=ones, v_descale=ones, **new)
    cache = PagedKVCache(4, PAGE, HKV, 64, dtype=bf, device="cpu", max_pages_per_seq=2)
    cache8 = PagedKVCache(4, PAGE, HKV, 64, dtype=ops.FP8, device="cpu", max_pages_per_seq=2, k_descale=ones, v_descale=ones)
    for c in (cache, cache8):
        c.allocate(0)
        c.advance([0], [4])
    with pytest.raises(ValueError, match="rotary is not fused into the quantising append"):
        cache8.write_step(k[:4], k[:4], [4], [0], k_norm_weight=wq)
    with pytest.raises(ValueError, match="qk_norm_unit_offset needs"):
        cache.write_step(k[:4], k[:4], [4], [0], qk_norm_unit_offset=True)

"""Host-side (no GPU) tests of the latent cache of a serving step (include/pfa_hip_mla_cache.h): the check codes of
``pfa_mla_decode_q8`` and ``pfa_mla_append`` in their documented order, the describe names and the workspace against the 16-bit call's,
``ops.mla_decode`` over an FP8 cache on CPU tensors against the fp64 reference on the exactly dequantised cache (the library's bounds:
the quantisation is in the reference's input), ``ops.mla_append`` on CPU tensors against direct indexing, and the ``ValueError``s."""

from __future__ import annotations

import ctypes as C

import pytest
import torch

from capi_testlib import ALIGN, DTYPE, FLAGS, NULL, OK, SHAPE, SIZE, STRIDE, name_of, ref
from capi_testlib import lib as base_lib  # noqa: F401  (the fixture)
from kvcache_testlib import FP8, NANB, b8, check_lse, check_out, reference
from photonic_flash_attention_amd import _capi_mla, _capi_mla_cache, ops

BF = torch.bfloat16


@pytest.fixture(scope="module")
def lib(base_lib):  # noqa: F811
    _capi_mla.load()
    return _capi_mla_cache.load()


def _decode(paged=False, **over):
    """tests/test_mla_decode_host.py's valid block over a cache of one-byte elements: B 2, H 16, Sq 2, Smax 4096."""
    base = dict(q=0x1000, kv_cache=0x1000000, o=0x4000, lse=0x8000, cache_seqlens=0x5000, B=2, H=16, Sq=2, Smax=4096, softmax_scale=0.07,
                q_stride_b=2 * 16 * 576, q_stride_s=16 * 576, q_stride_h=576, o_stride_b=2 * 16 * 512, o_stride_s=16 * 512, o_stride_h=512,
                kv_stride_b=4096 * 576, kv_stride_s=576, workspace=0x4000000, workspace_bytes=1 << 40)
    if paged:
        base.update(kv_stride_b=128 * 576, block_table=0x9000, block_table_stride_b=32, page_size=128, num_pages=100)
    return _capi_mla.make_mla_decode_args(**{**base, **over})


def _append(**over):
    """A valid ragged block: B 5, 640 packed rows of which a sequence has at most 300, k_pe a column slice of a [640, 576] buffer."""
    base = dict(kv_c=0x1000, k_pe=0x3000, kv_cache=0x1000000, cache_seqlens=0x5000, cu_seqlens_q=0x9000, B=5, Smax=4096, total_new=640,
                max_seqlen_q=300, kvc_stride_s=512, kpe_stride_s=576, kv_stride_b=4096 * 576, kv_stride_s=576)
    return _capi_mla_cache.make_mla_append_args(**{**base, **over})


def _quant(**over):
    return _capi_mla_cache.make_mla_kv_quant(**{"kv_descale": 0x7000, "descale_stride_b": 1, **over})


# in the order the errors are reported: each row breaks one rule and every rule in front of it holds.  (block, quant) overrides; a quant
# of None is the NULL block
QUANT_RULES = [(None, NULL), ({"size": 8}, SIZE), ({"flags": 1}, FLAGS), ({"reserved": 1}, FLAGS), ({"kv_dtype": 0}, DTYPE),
               ({"kv_descale": 0}, NULL), ({"kv_descale": 0x7002}, ALIGN), ({"descale_stride_b": -1}, STRIDE)]
DECODE_RULES = [({}, {}, OK), ({"size": 8}, None, SIZE)] + [({"flags": 1}, q, want) for q, want in QUANT_RULES] + [
    ({"flags": 1}, {"descale_stride_b": 0}, FLAGS), ({"kv_stride_s": 584, "flags": 1}, {}, STRIDE), ({"kv_stride_b": 4096 * 576 + 8}, {}, STRIDE),
    ({"kv_cache": 0x1000008, "flags": 1}, {}, ALIGN), ({"reserved": 1}, {}, FLAGS), ({"q": 0}, {}, NULL), ({"Sq": 65}, {}, SHAPE),
    ({"dtype_in": 2}, {}, DTYPE), ({"q_stride_h": 580}, {}, STRIDE), ({"kv_stride_s": 560}, {}, STRIDE), ({"lse": 0x8002}, {}, ALIGN),
    ({"page_size": 64}, {}, FLAGS), ({"workspace": 0}, {}, NULL), ({"workspace": 0x4000008}, {}, ALIGN)]
APPEND_RULES = [({}, {}, OK), ({}, None, OK), ({"size": 8}, None, SIZE)] + [({"flags": 1}, q, want) for q, want in QUANT_RULES[1:]] + [
    ({"flags": 1}, {}, FLAGS), ({"reserved1": 1}, None, FLAGS), ({"k_pe": 0}, None, NULL), ({"cache_seqlens": 0}, {}, NULL),
    ({"total_new": 0}, None, SHAPE), ({"dtype": 2}, None, DTYPE), ({"kpe_stride_s": 580}, None, STRIDE), ({"kv_stride_s": 584}, None, OK),
    ({"kv_stride_s": 584}, {}, STRIDE), ({"kv_stride_s": 568}, None, STRIDE), ({"k_pe": 0x3008}, None, ALIGN),
    ({"cu_seqlens_q": 0x9002}, None, ALIGN), ({"page_size": 64}, None, FLAGS), ({"kvc_stride_b": 512}, None, FLAGS),
    ({"max_seqlen_q": 641}, None, SHAPE), ({"cu_seqlens_q": 0, "max_seqlen_q": 129}, {}, SHAPE), ({"cu_seqlens_q": 0, "max_seqlen_q": 128}, {}, OK)]


def _ids(rules):
    return [f"{next(iter(o), 'valid')}-{n}" for n, (o, _, _) in enumerate(rules)]


@pytest.mark.parametrize("over,quant,want", DECODE_RULES, ids=_ids(DECODE_RULES))
def test_decode_q8_check_codes_in_order(lib, over, quant, want):
    assert lib.pfa_mla_decode_q8_check(C.byref(_decode(**over)), ref(None if quant is None else _quant(**quant))) == want


@pytest.mark.parametrize("over,quant,want", APPEND_RULES, ids=_ids(APPEND_RULES))
def test_append_check_codes_in_order(lib, over, quant, want):
    assert lib.pfa_mla_append_check(C.byref(_append(**over)), ref(None if quant is None else _quant(**quant))) == want


def test_null_blocks(lib):
    assert lib.pfa_mla_decode_q8_check(None, C.byref(_quant())) == NULL and lib.pfa_mla_append_check(None, None) == NULL
    assert lib.pfa_mla_decode_q8_workspace_bytes(None, C.byref(_quant())) == 0 and lib.pfa_mla_decode_q8_workspace_bytes(C.byref(_decode()), None) == 0


@pytest.mark.parametrize("dtype_in,dtype_out,Smax,H,paged,want", [
    (0, 0, 4096, 16, False, "mla_decode_q8_bf16_o16+combine"), (1, 2, 4096, 128, True, "mla_decode_q8_fp16_o32+combine_paged"),
    (1, 1, 128, 16, False, "mla_decode_q8_fp16_o16"), (0, 2, 128, 24, True, "mla_decode_q8_bf16_o32_paged")])
def test_decode_q8_names_grid_and_workspace_are_the_16_bit_calls(lib, dtype_in, dtype_out, Smax, H, paged, want):
    a, q = _decode(paged, dtype_in=dtype_in, dtype_out=dtype_out, Smax=Smax, H=H), _quant()
    n, name, ns = name_of(lib.pfa_mla_decode_q8_describe, a, C.byref(q), nsplit=True)
    n16, name16, ns16 = name_of(lib.pfa_mla_decode_describe, a, nsplit=True)
    assert name == want and name16 == want.replace("_q8", "") and (n, ns) == (n16, ns16)
    assert lib.pfa_mla_decode_q8_workspace_bytes(C.byref(a), C.byref(q)) == lib.pfa_mla_decode_workspace_bytes(C.byref(a))
    assert (lib.pfa_mla_decode_workspace_bytes(C.byref(a)) > 0) == (ns > 1)


@pytest.mark.parametrize("over,quant,want,groups", [
    ({}, None, "mla_append_varlen", 5 * 85), ({}, {}, "mla_append_q8_bf16_varlen", 5 * 43), ({"dtype": 1}, {}, "mla_append_q8_fp16_varlen", 5 * 43),
    ({"cu_seqlens_q": 0, "max_seqlen_q": 1}, None, "mla_append", 5),
    (dict(kv_stride_b=128 * 576, block_table=0x9000, block_table_stride_b=32, page_size=128, num_pages=100), {}, "mla_append_q8_bf16_varlen_paged", 5 * 43)])
def test_append_names_and_the_grid_from_host_shapes(lib, over, quant, want, groups):
    n, name = name_of(lib.pfa_mla_append_describe, _append(**over), ref(None if quant is None else _quant(**quant)))[:2]
    assert (name, n) == (want, groups)                                        # B * ceil(max_seqlen_q * (72 | 36) / 256)


def _cpu_cache(B=4, Smax=128, seed=11):
    """q, a latent cache quantised with per-sequence absmax descales (no powers of two), as FP8 and exactly dequantised in fp64."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, 3, 5, 576, generator=g).to(BF).permute(0, 2, 1, 3)
    kv = torch.randn(B, Smax, 576, generator=g) * torch.tensor([0.5, 1.0, 3.0, 7.0])[:B, None, None]
    d = kv.abs().amax(dim=(1, 2)) / 448
    kv8 = ops.quantize_kv(kv[:, None], d[:, None])[:, 0]
    return q, kv8, d, ops.dequantize_kv(kv8[:, None], d[:, None], torch.float64)[:, 0]


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("paged", [False, True])
def test_the_cpu_fp8_model_against_fp64_on_the_dequantised_cache(causal, paged):
    q, kv8, d, kv64 = _cpu_cache()
    lens = torch.tensor([0, 2, 70, 128], dtype=torch.int32)
    kn = b8(kv8).clone()
    for b, n in enumerate(lens.tolist()):
        kn[b, n:] = NANB
    table = None
    if paged:                                    # pages of 64 keys in reverse order behind an unnamed page of NaN bytes
        table = torch.arange(8, 0, -1, dtype=torch.int32).reshape(4, 2)
        pool = torch.full((9, 64, 576), NANB, dtype=torch.uint8)
        pool[table.flatten().long()] = kn.reshape(8, 64, 576)
        kn = pool
    o, lse = ops.mla_decode(q, kn.view(FP8), cache_seqlens=lens, softmax_scale=0.07, causal=causal, block_table=table, return_lse=True, kv_descale=d)
    ro, rlse, pn = reference(q, kv64[:, None], kv64[:, None, :, :512], seqlens=lens, causal=causal, scale=0.07)
    assert o.shape == (4, 5, 3, 512) and o.dtype == q.dtype
    check_out(o, ro, pn, float(kv64.abs().max()), q.dtype, "cpu fp8 model")
    check_lse(o, lse, rlse, "cpu fp8 model")


@pytest.mark.parametrize("fp8", [False, True], ids=["16-bit", "fp8"])
def test_the_append_model_against_direct_indexing(fp8):
    """Ragged rows, one sequence with len_b < Sq_b (its first rows fall in front of key 0), one table entry outside the pool."""
    g = torch.Generator().manual_seed(5)
    cu, lens, page = [0, 3, 3, 8, 70], [130, 9, 2, 64], 64       # Sq_b 3, 0, 5, 62: sequence 2 keeps its last two rows
    rows = torch.randn(70, 576, generator=g).to(BF)
    d = torch.tensor([0.5, 0.013, 1.7, 0.3]) if fp8 else None
    table = (torch.randperm(12, generator=g)[:12].to(torch.int32)).reshape(4, 3)
    table[0, 2] = 12                                              # sequence 0's rows at keys 128, 129: dropped
    pool = torch.full((12, page, 576), 0x55, dtype=torch.uint8).view(FP8) if fp8 else torch.full((12, page, 576), -7.0, dtype=BF)
    want = pool.clone()
    for b in range(4):
        sq = cu[b + 1] - cu[b]
        for i in range(max(0, sq - lens[b]), sq):
            pos, x = lens[b] - sq + i, rows[cu[b] + i]
            if table[b, pos // page] < 12:
                want[table[b, pos // page], pos % page] = ops.quantize_kv(x[None, None, None], d[b].reshape(1))[0, 0, 0] if fp8 else x
    ops.mla_append(rows[:, :512], rows[:, 512:], pool, cache_seqlens=torch.tensor(lens, dtype=torch.int32),
                   cu_seqlens_q=torch.tensor(cu, dtype=torch.int32), max_seqlen_q=62, block_table=table, kv_descale=d)
    assert torch.equal(pool.view(torch.uint8 if fp8 else torch.int16), want.view(torch.uint8 if fp8 else torch.int16))


@pytest.mark.parametrize("what,change", [
    ("needs kv_descale", lambda q, kv, d, kw: (q, kv, kw)),
    ("kv_descale goes with", lambda q, kv, d, kw: (q, kv.to(BF), {**kw, "kv_descale": d})),
    ("kv_descale must be", lambda q, kv, d, kw: (q, kv, {**kw, "kv_descale": d[:3]})),
    ("kv_descale must be", lambda q, kv, d, kw: (q, kv, {**kw, "kv_descale": d.double()})),
    ("kv_descale must be", lambda q, kv, d, kw: (q, kv, {**kw, "kv_descale": d[:, None]})),
    ("multiple of 16", lambda q, kv, d, kw: (q, torch.empty(4, 128, 584, dtype=torch.uint8).view(FP8)[..., :576], {**kw, "kv_descale": d})),
    ("dtype", lambda q, kv, d, kw: (q.float(), kv, {**kw, "kv_descale": d}))])
def test_value_errors_before_anything_runs(what, change):
    q, kv8, d, _ = _cpu_cache()
    q, kv, kw = change(q, kv8, d, dict(cache_seqlens=torch.tensor([1, 2, 3, 4], dtype=torch.int32), softmax_scale=0.07))
    with pytest.raises(ValueError, match=what):
        ops.mla_decode(q, kv, **kw)
    if kv.dtype == FP8 and q.dtype == BF:        # the append's refusals of the same cache and descale
        with pytest.raises(ValueError, match=what):
            ops.mla_append(torch.zeros(4, 1, 512, dtype=BF), torch.zeros(4, 1, 64, dtype=BF), kv, cache_seqlens=kw["cache_seqlens"],
                           kv_descale=kw.get("kv_descale"))

"""Host-side (no GPU) tests of the MLA decode over a latent KV cache (include/pfa_hip_mla.h): the check's codes in their order, the
describe names, the workspace against the split count, ``ops.mla_decode`` on CPU tensors (the plain-torch specification) against the fp64
reference of tests/kvcache_testlib.py, and the ``ValueError``s."""

from __future__ import annotations

import ctypes as C

import pytest
import torch

from capi_testlib import ALIGN, DTYPE, FLAGS, NULL, OK, SHAPE, SIZE, STRIDE, name_of
from capi_testlib import lib as base_lib  # noqa: F401  (the fixture)
from kvcache_testlib import check_lse, check_out, reference
from photonic_flash_attention_amd import _capi_mla, ops


@pytest.fixture(scope="module")
def lib(base_lib):  # noqa: F811
    return _capi_mla.load()


def _args(paged=False, **over):
    """A valid block: B 2, H 16, Sq 2, Smax 4096, bf16, [B, Sq, H, .] q and o, a contiguous cache or a pool of 100 pages of 128 keys."""
    base = dict(q=0x1000, kv_cache=0x1000000, o=0x4000, lse=0x8000, cache_seqlens=0x5000, B=2, H=16, Sq=2, Smax=4096, softmax_scale=0.07,
                q_stride_b=2 * 16 * 576, q_stride_s=16 * 576, q_stride_h=576, o_stride_b=2 * 16 * 512, o_stride_s=16 * 512, o_stride_h=512,
                kv_stride_b=4096 * 576, kv_stride_s=576, workspace=0x4000000, workspace_bytes=1 << 40)
    if paged:
        base.update(kv_stride_b=128 * 576, block_table=0x9000, block_table_stride_b=32, page_size=128, num_pages=100)
    return _capi_mla.make_mla_decode_args(**{**base, **over})


# in the order the errors are reported: each row breaks one rule and every rule in front of it holds
RULES = [({}, OK), ({"size": 8}, SIZE), ({"flags": 1}, FLAGS), ({"reserved": 1}, FLAGS), ({"kv_cache": 0}, NULL), ({"cache_seqlens": 0}, NULL),
         ({"Sq": 65}, SHAPE), ({"H": 0}, SHAPE), ({"softmax_scale": 0.0}, SHAPE), ({"dtype_in": 2}, DTYPE), ({"dtype_out": 1}, DTYPE),
         ({"q_stride_h": 580}, STRIDE), ({"o_stride_h": 514}, STRIDE), ({"kv_stride_s": 568}, STRIDE), ({"kv_stride_s": 1 << 27}, STRIDE),
         ({"kv_cache": 0x1000008}, ALIGN), ({"lse": 0x8002}, ALIGN), ({"page_size": 64}, FLAGS), ({"workspace": 0}, NULL),
         ({"workspace_bytes": 100}, NULL), ({"workspace": 0x4000008}, ALIGN)]


@pytest.mark.parametrize("over,want", RULES, ids=[f"{next(iter(o), 'valid')}-{n}" for n, (o, _) in enumerate(RULES)])
def test_check_codes_in_order(lib, over, want):
    assert lib.pfa_mla_decode_check(C.byref(_args(**over))) == want


def test_null_block_and_paging_rules(lib):
    assert lib.pfa_mla_decode_check(None) == NULL and lib.pfa_mla_decode_workspace_bytes(None) == 0
    assert lib.pfa_mla_decode_check(C.byref(_args(paged=True))) == OK
    for over, want in (({"page_size": 96}, SHAPE), ({"block_table": 0x9002}, ALIGN), ({"num_pages": 0}, SHAPE), ({"Smax": 4000}, SHAPE)):
        assert lib.pfa_mla_decode_check(C.byref(_args(paged=True, **over))) == want


@pytest.mark.parametrize("dtype_in,dtype_out,Smax,H,paged,want", [
    (0, 0, 4096, 16, False, "mla_decode_bf16_o16+combine"), (1, 2, 4096, 128, True, "mla_decode_fp16_o32+combine_paged"),
    (1, 1, 128, 16, False, "mla_decode_fp16_o16"), (0, 2, 128, 24, True, "mla_decode_bf16_o32_paged")])
def test_describe_names_and_workspace_follow_the_split_count(lib, dtype_in, dtype_out, Smax, H, paged, want):
    a = _args(paged, dtype_in=dtype_in, dtype_out=dtype_out, Smax=Smax, H=H)
    n, name, ns = name_of(lib.pfa_mla_decode_describe, a, nsplit=True)
    nrb = -(-a.Sq * H // 16)
    assert name == want and ("+combine" in want) == (ns > 1)
    assert n == -(-a.B * ns // 8) * 8 * nrb                                   # (b, split) pairs in whole groups of 8, times the row blocks
    assert lib.pfa_mla_decode_workspace_bytes(C.byref(a)) == (ns * a.B * H * a.Sq * (512 + 2) * 4 if ns > 1 else 0)


def _cpu_problem(B=4, H=5, Sq=3, Smax=128, dtype=torch.bfloat16):
    g = torch.Generator().manual_seed(11)
    q = torch.randn(B, Sq, H, 576, generator=g).to(dtype).permute(0, 2, 1, 3)
    return q, torch.randn(B, Smax, 576, generator=g).to(dtype)


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("paged", [False, True])
def test_the_cpu_model_against_fp64_on_a_ragged_batch(causal, paged):
    q, kv = _cpu_problem()
    lens = torch.tensor([0, 2, 70, 128], dtype=torch.int32)
    kn = kv.clone()
    for b, n in enumerate(lens.tolist()):
        kn[b, n:] = float("nan")
    table = None
    if paged:                                    # pages of 64 keys in reverse order behind an unnamed page of NaN
        table = torch.arange(8, 0, -1, dtype=torch.int32).reshape(4, 2)
        pool = torch.full((9, 64, 576), float("nan"), dtype=kv.dtype)
        pool[table.flatten().long()] = kn.reshape(8, 64, 576)
        kn = pool
    o, lse = ops.mla_decode(q, kn, cache_seqlens=lens, softmax_scale=0.07, causal=causal, block_table=table, return_lse=True)
    ro, rlse, pn = reference(q, kv[:, None], kv[:, None, :, :512], seqlens=lens, causal=causal, scale=0.07)
    assert o.shape == (4, 5, 3, 512) and o.dtype == q.dtype
    check_out(o, ro, pn, float(kv.abs().max()), q.dtype, "cpu model")
    check_lse(o, lse, rlse, "cpu model")


@pytest.mark.parametrize("what,change", [
    ("576", lambda q, kv, kw: (q[..., :512], kv, kw)), ("576", lambda q, kv, kw: (q, kv[..., :512], kw)),
    ("dtype", lambda q, kv, kw: (q, kv.half(), kw)), ("dtype", lambda q, kv, kw: (q.float(), kv.float(), kw)),
    ("Sq", lambda q, kv, kw: (q.repeat(1, 1, 33, 1), kv, kw)), ("shape mismatch", lambda q, kv, kw: (q, kv[:3], kw)),
    ("softmax_scale", lambda q, kv, kw: (q, kv, {**kw, "softmax_scale": 0.0})),
    ("cache_seqlens", lambda q, kv, kw: (q, kv, {**kw, "cache_seqlens": kw["cache_seqlens"][:2]})),
    ("output dtype", lambda q, kv, kw: (q, kv, {**kw, "out_dtype": torch.float16})),
    ("multiple of 64", lambda q, kv, kw: (q, kv[:, :96], {**kw, "block_table": torch.zeros(4, 1, dtype=torch.int32)})),
    ("block_table", lambda q, kv, kw: (q, kv, {**kw, "block_table": torch.zeros(4, 1, dtype=torch.int64)}))])
def test_value_errors_before_anything_runs(what, change):
    q, kv = _cpu_problem()
    q, kv, kw = change(q, kv, dict(cache_seqlens=torch.tensor([1, 2, 3, 4], dtype=torch.int32), softmax_scale=0.07))
    with pytest.raises(ValueError, match=what):
        ops.mla_decode(q, kv, **kw)
    with pytest.raises(TypeError):               # cache_seqlens and softmax_scale have no default
        ops.mla_decode(q, kv)

"""Host-side (no GPU) tests of the non-absorbed MLA prefill over packed sequences (include/pfa_hip_mla_prefill.h): the check's codes in
their order, the describe names and the grid, ``ops.mla_prefill`` on CPU tensors (the plain-torch specification) against the fp64
reference of tests/kvcache_testlib.py per sequence, and the ``ValueError``s."""

from __future__ import annotations

import ctypes as C

import pytest
import torch

from capi_testlib import ALIGN, DTYPE, FLAGS, NULL, OK, SHAPE, SIZE, STRIDE, name_of
from capi_testlib import lib as base_lib  # noqa: F401  (the fixture)
from kvcache_testlib import check_lse, check_out, reference
from photonic_flash_attention_amd import _capi_mla_prefill, ops


@pytest.fixture(scope="module")
def lib(base_lib):  # noqa: F811
    return _capi_mla_prefill.load()


def _args(**over):
    """A valid block: B 3, H 16, 1000 packed rows of at most 600, 900 packed keys of at most 700, bf16, k_nope and v the halves of one
    [total_k, H, 256] buffer, one rotary key row per token."""
    base = dict(q=0x100000, k_nope=0x200000, v=0x200100, k_rope=0x300000, o=0x400000, lse=0x500000, cu_seqlens_q=0x600000, cu_seqlens_k=0x700000,
                q_stride_s=16 * 192, q_stride_h=192, kn_stride_s=16 * 256, kn_stride_h=256, v_stride_s=16 * 256, v_stride_h=256,
                kr_stride_s=64, kr_stride_h=0, o_stride_s=16 * 128, o_stride_h=128, B=3, H=16, rope_heads=1, total_q=1000, total_k=900,
                max_seqlen_q=600, max_seqlen_k=700, causal=1, softmax_scale=0.07)
    return _capi_mla_prefill.make_mla_prefill_args(**{**base, **over})


# in the order the errors are reported: each row breaks one rule and every rule in front of it holds
RULES = [({}, OK), ({"size": 8}, SIZE), ({"flags": 1}, FLAGS), ({"reserved": 1}, FLAGS), ({"k_rope": 0}, NULL), ({"cu_seqlens_k": 0}, NULL),
         ({"H": 0}, SHAPE), ({"rope_heads": 2}, SHAPE), ({"max_seqlen_q": 1001}, SHAPE), ({"max_seqlen_k": 0}, SHAPE),
         ({"softmax_scale": 0.0}, SHAPE), ({"dtype_in": 2}, DTYPE), ({"dtype_out": 1}, DTYPE), ({"q_stride_h": 196}, STRIDE),
         ({"o_stride_h": 130}, STRIDE), ({"kr_stride_s": 56}, STRIDE), ({"kn_stride_s": 1 << 27}, STRIDE), ({"q_stride_s": 184}, STRIDE),
         ({"v": 0x200108}, ALIGN), ({"lse": 0x500002}, ALIGN), ({"B": 1 << 27, "H": 64}, SHAPE)]


@pytest.mark.parametrize("over,want", RULES, ids=[f"{next(iter(o), 'valid')}-{n}" for n, (o, _) in enumerate(RULES)])
def test_check_codes_in_order(lib, over, want):
    assert lib.pfa_mla_prefill_check(C.byref(_args(**over))) == want


def test_null_block_and_a_rope_head_stride_only_matters_with_h_heads(lib):
    assert lib.pfa_mla_prefill_check(None) == NULL
    assert lib.pfa_mla_prefill_check(C.byref(_args(kr_stride_h=3))) == OK
    assert lib.pfa_mla_prefill_check(C.byref(_args(rope_heads=16, kr_stride_s=1024, kr_stride_h=3))) == STRIDE


@pytest.mark.parametrize("dtype_in,dtype_out,causal,rope_heads,max_q,want", [
    (0, 0, 1, 1, 600, "mla_prefill_bf16_o16_causal_rope1"), (1, 2, 0, 16, 256, "mla_prefill_fp16_o32_full_ropeH"),
    (1, 1, 1, 16, 257, "mla_prefill_fp16_o16_causal_ropeH"), (0, 2, 0, 1, 1, "mla_prefill_bf16_o32_full_rope1")])
def test_describe_names_and_the_grid_from_host_shapes(lib, dtype_in, dtype_out, causal, rope_heads, max_q, want):
    a = _args(dtype_in=dtype_in, dtype_out=dtype_out, causal=causal, rope_heads=rope_heads, max_seqlen_q=max_q, kr_stride_s=1024, kr_stride_h=64)
    n, name, _ = name_of(lib.pfa_mla_prefill_describe, a)
    assert name == want and n == a.B * a.H * -(-max_q // _capi_mla_prefill.BLOCK_M)
    assert _capi_mla_prefill.describe_mla_prefill(a) == (want, n)


SEQS = [(5, 0), (0, 17), (3, 70), (40, 9), (33, 33)]         # (Lq, Lk): no key, no row, a chunk over a context, Lk < Lq, square


def _cpu_problem(rope_heads=1, H=3, dtype=torch.bfloat16):
    """Packed q, k_nope, k_rope, v with three spare rows behind cu[B] -> (q, k_nope, k_rope, v, cu_q, cu_k)."""
    g = torch.Generator().manual_seed(12)
    cu = torch.tensor([[0, 0]] + SEQS).cumsum(0).to(torch.int32)
    tq, tk = int(cu[-1, 0]) + 3, int(cu[-1, 1]) + 3
    q = torch.randn(tq, H, 192, generator=g).to(dtype)
    kv = torch.randn(tk, H, 256, generator=g).to(dtype)
    return q, kv[..., :128], torch.randn(tk, rope_heads, 64, generator=g).to(dtype), kv[..., 128:], cu[:, 0].contiguous(), cu[:, 1].contiguous()


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("rope_heads", [1, 3])
def test_the_cpu_model_against_fp64_per_sequence(causal, rope_heads):
    q, kn, kr, v, cu_q, cu_k = _cpu_problem(rope_heads)
    o, lse = ops.mla_prefill(q, kn, kr, v, cu_seqlens_q=cu_q, cu_seqlens_k=cu_k, max_seqlen_q=40, max_seqlen_k=70, softmax_scale=0.07,
                             causal=causal, return_lse=True, out=torch.full((q.shape[0], 3, 128), 7.0, dtype=q.dtype))
    assert o.dtype == q.dtype and lse.shape == (3, q.shape[0]) and bool((o[int(cu_q[-1]):] == 7).all())       # spare rows: not written
    for b, (nq, nk) in enumerate(SEQS):
        if nq == 0:
            continue
        rq, rk = slice(int(cu_q[b]), int(cu_q[b + 1])), slice(int(cu_k[b]), int(cu_k[b]) + max(nk, 1))      # (the reference wants a key row)
        k = torch.cat([kn[rk], kr[rk].expand(-1, 3, 64)], dim=-1)
        ro, rlse, pn = reference(q[rq].transpose(0, 1)[None], k.transpose(0, 1)[None], v[rk].transpose(0, 1)[None],
                                 seqlens=torch.tensor([nk]), causal=causal, scale=0.07)
        check_out(o[rq].transpose(0, 1)[None], ro, pn, float(v.abs().max()), q.dtype, f"cpu model seq {b}")
        check_lse(o[rq].transpose(0, 1)[None], lse[:, rq][None], rlse, f"cpu model seq {b}")


@pytest.mark.parametrize("what,change", [
    ("last dims", lambda t, kw: ((t[0][..., :128],) + t[1:], kw)), ("last dims", lambda t, kw: (t[:2] + (t[2][..., :32], t[3]), kw)),
    ("shape mismatch", lambda t, kw: (t[:3] + (t[3][:, :2],), kw)), ("shape mismatch", lambda t, kw: (t[:2] + (t[2].expand(-1, 2, -1), t[3]), kw)),
    ("dtype", lambda t, kw: (t[:3] + (t[3].half(),), kw)), ("dtype", lambda t, kw: (tuple(x.float() for x in t), kw)),
    ("softmax_scale", lambda t, kw: (t, {**kw, "softmax_scale": float("inf")})),
    ("cu_seqlens_k", lambda t, kw: (t, {**kw, "cu_seqlens_k": kw["cu_seqlens_k"].long()})),
    ("both be", lambda t, kw: (t, {**kw, "cu_seqlens_q": kw["cu_seqlens_q"][:3].contiguous()})),
    ("max_seqlen_q", lambda t, kw: (t, {**kw, "max_seqlen_q": 0})), ("max_seqlen_k", lambda t, kw: (t, {**kw, "max_seqlen_k": 1 << 20})),
    ("k_rope: needs", lambda t, kw: (t[:2] + (t[2].repeat(1, 1, 2)[..., ::2], t[3]), kw)),
    ("output dtype", lambda t, kw: (t, {**kw, "out_dtype": torch.float16})), ("out must", lambda t, kw: (t, {**kw, "out": torch.empty(3, 3, 128)})),
    ("not both", lambda t, kw: (t, {**kw, "k": t[0]})), ("k must", lambda t, kw: ((t[0], None, None, t[3]), {**kw, "k": t[1]}))])
def test_value_errors_before_anything_runs(what, change):
    q, kn, kr, v, cu_q, cu_k = _cpu_problem(rope_heads=1)
    t, kw = change((q, kn, kr, v), dict(cu_seqlens_q=cu_q, cu_seqlens_k=cu_k, max_seqlen_q=40, max_seqlen_k=70, softmax_scale=0.07))
    with pytest.raises(ValueError, match=what):
        ops.mla_prefill(*t, **kw)
    with pytest.raises(TypeError):               # the cu_seqlens, the bounds and softmax_scale have no default
        ops.mla_prefill(q, kn, kr, v)

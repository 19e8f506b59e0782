"""CPU-side tests (no GPU) of the merge of partial attention results (``pfa_attn_merge*``, ABI v9 additive) and of ``shared_prefix=``:
every validation rule and the order the rules are reported in, the launch
description, the plain-torch model of the rule (``ops.attn_merge`` on CPU tensors: the executable specification the GPU tests compare
the kernel with) against the rule in fp64 (``merge_ref64`` of tests/kvcache_testlib.py), its exactness property, and the
``ValueError``s ``shared_prefix`` raises before anything is enqueued."""

from __future__ import annotations

import ctypes as C
import inspect
import os

import pytest
import torch

from capi_testlib import ALIGN, DTYPE, FLAGS, HEAD_DIM, NULL, SHAPE, SIZE, STRIDE, lib  # noqa: F401
from capi_testlib import attn_merge_args as _args
from conftest import REPO
from kvcache_testlib import merge_ref64
from photonic_flash_attention_amd import _capi, ops

BF16, FP16, FP32 = 0, 1, 2
INF, NAN = float("inf"), float("nan")


def _set(a, field, n, value):
    getattr(a, field)[n] = value
    return a


def _check(lib, a):
    return lib.pfa_attn_merge_check(C.byref(a))


def test_the_part_limit_is_eight():
    header = open(os.path.join(REPO, "include", "pfa_hip.h")).read()
    assert "#define PFA_MERGE_MAX_PARTS 8" in header and _capi.PFA_MERGE_MAX_PARTS == 8


def test_attn_merge_argument_validation(lib):
    assert _check(lib, _args()) == 0
    assert lib.pfa_attn_merge_check(None) == NULL
    bad = _args()
    bad.size = 16
    assert _check(lib, bad) == SIZE
    other = _args()
    other.size = C.sizeof(_capi.PfaKvAppendArgs)
    assert _check(lib, other) == SIZE
    cases = [
        (dict(flags=1), FLAGS), (dict(flags=0x100), FLAGS), (dict(reserved0=1), FLAGS), (dict(reserved1=-1), FLAGS),
        (dict(o=0), NULL),
        (dict(n_parts=1), SHAPE), (dict(n_parts=0), SHAPE), (dict(n_parts=-2), SHAPE), (dict(_n=8, n_parts=9), SHAPE),
        (dict(B=0), SHAPE), (dict(H=0), SHAPE), (dict(Sq=0), SHAPE), (dict(Sq=-1), SHAPE),
        (dict(D=0), HEAD_DIM), (dict(D=4), HEAD_DIM), (dict(D=100), HEAD_DIM), (dict(D=264), HEAD_DIM), (dict(D=512), HEAD_DIM),
        (dict(dtype_part=3), DTYPE), (dict(dtype_part=-1), DTYPE), (dict(dtype_out=3), DTYPE), (dict(dtype_out=7), DTYPE),
        (dict(dtype_part=BF16, dtype_out=FP16), DTYPE), (dict(dtype_part=FP16, dtype_out=BF16), DTYPE),
        (dict(o_stride_b=5 * 512 + 2), STRIDE), (dict(o_stride_h=129), STRIDE), (dict(o_stride_s=513), STRIDE),
        (dict(dtype_out=BF16, o_stride_s=512 + 4), STRIDE),                                   # a 16-bit output wants multiples of 8
        (dict(o=0x9000008), ALIGN), (dict(lse_out=0x8002), ALIGN),
        (dict(B=1 << 15, Sq=1 << 10, H=64, D=256), SHAPE),                                    # 2^31 + items: past the grid and the index
        (dict(B=1 << 30, Sq=1 << 30, H=1 << 30), SHAPE),                                      # the product does not wrap
    ]
    for over, want in cases:
        assert _check(lib, _args(**over)) == want, over
    # per-part fields, of every part that counts
    for n in range(3):
        assert _check(lib, _set(_args(), "o_part", n, 0)) == NULL and _check(lib, _set(_args(), "lse_part", n, 0)) == NULL
        for f in ("op_stride_b", "op_stride_h", "op_stride_s"):
            assert _check(lib, _set(_args(), f, n, 130)) == STRIDE, (f, n)
            assert _check(lib, _set(_args(dtype_part=BF16), f, n, 132)) == STRIDE, (f, n)     # 16-bit parts: multiples of 8
            assert _check(lib, _set(_args(), f, n, 132)) == 0                                 # fp32 parts: of 4
        assert _check(lib, _set(_args(), "o_part", n, 0x100008)) == ALIGN
        assert _check(lib, _set(_args(), "lse_part", n, 0x10002)) == ALIGN
    # ... and of no other: entries at and past n_parts are ignored
    assert _check(lib, _set(_set(_args(), "o_part", 3, 0x3), "op_stride_s", 7, 1)) == 0
    # the launch refuses what the check refuses, before it touches a device
    assert lib.pfa_attn_merge(C.byref(_args(D=100)), None) == HEAD_DIM and lib.pfa_attn_merge(None, None) == NULL


def test_attn_merge_rules_are_reported_in_the_documented_order(lib):
    """STRUCT_SIZE, FLAGS, NULL, SHAPE, HEAD_DIM, DTYPE, STRIDE, ALIGN, then the grid limit: of two violated rules the earlier wins."""
    ladder = [("size", dict(), SIZE), ("flags", dict(flags=2), FLAGS), ("null", dict(o=0), NULL), ("shape", dict(H=0), SHAPE),
              ("head_dim", dict(D=12), HEAD_DIM), ("dtype", dict(dtype_out=5), DTYPE), ("stride", dict(o_stride_h=2), STRIDE),
              ("align", dict(lse_out=0x8001), ALIGN)]
    for i, (first, over_i, want) in enumerate(ladder):
        for later, over_j, _ in ladder[i + 1:]:
            a = _args(**dict(over_j, **over_i))
            if first == "size":
                a.size += 8
            assert _check(lib, a) == want, (first, later)
    # a missing part is reported before a part count out of range, and that before the head dim
    assert _check(lib, _set(_args(n_parts=9), "lse_part", 7, 0)) == NULL
    assert _check(lib, _args(_n=8, n_parts=9, D=12)) == SHAPE
    # the grid limit comes last: behind an unaligned base
    big = dict(B=1 << 15, Sq=1 << 10, H=64, D=256)
    assert _check(lib, _args(**big)) == SHAPE and _check(lib, _args(o=0x9000004, **big)) == ALIGN
    assert _check(lib, _args(o_stride_s=3, **big)) == STRIDE


def test_attn_merge_accepted_variants(lib):
    for ok in (dict(D=8), dict(D=64), dict(D=96), dict(D=256), dict(_n=2), dict(_n=8), dict(B=1), dict(Sq=1), dict(H=1), dict(lse_out=0),
               dict(dtype_out=BF16), dict(dtype_out=FP16), dict(dtype_part=BF16, dtype_out=BF16), dict(dtype_part=BF16, dtype_out=FP32),
               dict(dtype_part=FP16, dtype_out=FP16), dict(dtype_part=FP16, dtype_out=FP32),
               dict(lp_stride_b=[5, 20, 20], lp_stride_h=[15, 5, 5]),                           # a [1, H, B * Sq] LSE among [B, H, Sq] ones
               dict(lp_stride_b=[1, 3, 7], lp_stride_h=[1, 1, 1], lp_stride_s=[0, -1, 9]),     # LSE strides are free
               dict(B=1, Sq=1 << 20, H=64, D=128)):                                             # 2^30 items
        assert _check(lib, _args(**ok)) == 0, ok


@pytest.mark.parametrize("B,H,Sq,D", [(3, 4, 5, 128), (3, 4, 5, 8), (1, 1, 1, 8), (7, 3, 11, 72), (32, 32, 1, 128), (2, 5, 300, 256)])
def test_attn_merge_describe_counts_workgroups_from_host_shapes(lib, B, H, Sq, D):
    items = B * Sq * H * (D // 8)
    a = _args(B=B, H=H, Sq=Sq, D=D)
    name, wgs = _capi.describe_attn_merge(a)
    assert wgs == -(-items // 256) and name == f"attn_merge_fp32_fp32_d{D}_n3"
    a.o, a.lse_out = 0xA000000, 0
    _set(_set(a, "o_part", 1, 0x7000000), "lp_stride_h", 2, 999)                                # pointers and LSE strides change nothing
    assert _capi.describe_attn_merge(a) == (name, wgs)


def test_attn_merge_describe_names(lib):
    a = _args()                                               # 3 * 5 * 4 * 16 = 960 items: the fourth workgroup is partly empty
    assert 960 % 256 != 0 and _capi.describe_attn_merge(a) == ("attn_merge_fp32_fp32_d128_n3", 4)
    assert _capi.describe_attn_merge(_args(_n=2, dtype_part=BF16, dtype_out=BF16, D=64))[0] == "attn_merge_bf16_bf16_d64_n2"
    assert _capi.describe_attn_merge(_args(_n=8, dtype_part=FP16, dtype_out=FP32, D=256))[0] == "attn_merge_fp16_fp32_d256_n8"
    assert _capi.describe_attn_merge(_args(_n=5, dtype_out=FP16, D=8))[0] == "attn_merge_fp32_fp16_d8_n5"
    with pytest.raises(_capi.PfaError):
        _capi.describe_attn_merge(_args(D=100))
    buf = C.create_string_buffer(8)                           # truncated, NUL terminated
    assert lib.pfa_attn_merge_describe(C.byref(a), buf, 8) == 4 and buf.value == b"attn_me"
    assert lib.pfa_attn_merge_describe(C.byref(a), None, 0) == 4


# ---- the CPU model against fp64 -------------------------------------------------------------------------------------------------

def _parts(N, B, H, Sq, D, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    offs = [0.0, 5.0, -5.0, 120.0, -120.0, 0.0, 5.0, -5.0]
    outs = [torch.randn(B, Sq, H, D, generator=g).to(dtype).permute(0, 2, 1, 3) for _ in range(N)]
    lses = [3 * torch.randn(B, H, Sq, generator=g) + offs[n] for n in range(N)]
    return outs, lses


@pytest.mark.parametrize("dtype,odt", [(torch.float32, torch.float32), (torch.float32, torch.bfloat16), (torch.bfloat16, torch.bfloat16),
                                       (torch.float16, torch.float32), (torch.float16, torch.float16)])
@pytest.mark.parametrize("N", [2, 3, 8])
def test_cpu_attn_merge_matches_fp64(N, dtype, odt):
    outs, lses = _parts(N, 3, 4, 5, 64, dtype, 100 + N)
    lses[1] = lses[1].permute(1, 0, 2).contiguous().view(1, 4, 15).view(4, 3, 5).transpose(0, 1)   # the prefix pass's [1, H, B * Sq] layout
    o, lse = ops.attn_merge(outs, lses, out_dtype=odt, return_lse=True)
    ref_o, ref_lse = merge_ref64(outs, lses)
    assert o.dtype == odt and o.shape == (3, 4, 5, 64) and lse.shape == (3, 4, 5) and lse.dtype == torch.float32
    bound = 1e-5 * torch.stack([t.double().abs() for t in outs]).max(dim=0).values
    if odt != torch.float32:
        bound = bound + (2.0 ** -8 if odt == torch.bfloat16 else 2.0 ** -11) * ref_o.abs()
    assert bool(((o.double() - ref_o).abs() <= bound).all())
    assert bool(((lse.double() - ref_lse).abs() <= 4e-6 * ref_lse.abs().clamp_min(1.0)).all())
    # into a caller's buffer, without the LSE
    buf = torch.full((3, 5, 4, 64), 9.0, dtype=odt).permute(0, 2, 1, 3)
    o2, none = ops.attn_merge(outs, lses, out=buf)
    assert o2 is buf and none is None and torch.equal(buf, o)


def test_cpu_attn_merge_inf_nan_and_exactness():
    outs, lses = _parts(3, 2, 2, 6, 16, torch.float32, 7)
    lses[0][0, 0, 1] = -INF
    outs[0][0, 0, 1] = NAN                                   # a skipped part's O does not reach the result
    for l in lses:
        l[0, 1, 2] = -INF                                    # a row with no visible key anywhere
    outs[2][0, 1, 2] = NAN
    lses[1][1, 0, 3] = NAN                                   # a NaN LSE
    o, lse = ops.attn_merge(outs, lses, return_lse=True)
    clean = torch.ones(2, 2, 6, dtype=torch.bool)
    clean[0, 1, 2] = clean[1, 0, 3] = False
    assert bool(torch.isfinite(o[clean]).all()) and bool(torch.isfinite(lse[clean]).all())
    assert bool((o[0, 1, 2] == 0).all()) and float(lse[0, 1, 2]) == -INF
    assert bool(torch.isnan(o[1, 0, 3]).all()) and bool(torch.isnan(lse[1, 0, 3]))
    ref_o, ref_lse = merge_ref64([t[:, :, :2] for t in outs[1:]], [t[:, :, :2] for t in lses[1:]])
    assert bool(((o[0, 0, 1].double() - ref_o[0, 0, 1]).abs() <= 1e-5 * max(float(t[0, 0, 1].abs().max()) for t in outs[1:])).all())
    # one finite part among -inf parts comes back bit for bit, wherever it stands
    finite = 3 * torch.randn(2, 2, 6, generator=torch.Generator().manual_seed(8)) + 40
    for where in range(3):
        ls = [torch.full((2, 2, 6), -INF) for _ in range(3)]
        ls[where] = finite
        os_ = [torch.full_like(outs[0], NAN) for _ in range(3)]
        os_[where] = outs[1]
        o, lse = ops.attn_merge(os_, ls, return_lse=True)
        assert torch.equal(o, outs[1]) and torch.equal(lse, finite)
        o16, _ = ops.attn_merge(os_, ls, out_dtype=torch.bfloat16)
        assert torch.equal(o16, outs[1].to(torch.bfloat16))


def test_attn_merge_refusals():
    outs, lses = _parts(2, 2, 3, 4, 16, torch.bfloat16, 3)
    ops.attn_merge(outs, lses)
    with pytest.raises(ValueError, match="2 .. 8 parts"):
        ops.attn_merge(outs[:1], lses[:1])
    with pytest.raises(ValueError, match="2 .. 8 parts"):
        ops.attn_merge(outs * 5, lses * 5)
    with pytest.raises(ValueError, match="2 .. 8 parts"):
        ops.attn_merge(outs, lses[:1])
    with pytest.raises(ValueError, match="one shape and one dtype"):
        ops.attn_merge([outs[0], outs[1].float()], lses)
    with pytest.raises(ValueError, match="one shape and one dtype"):
        ops.attn_merge([outs[0], outs[1][:1]], lses)
    with pytest.raises(ValueError, match="one shape and one dtype"):
        ops.attn_merge([t.double() for t in outs], lses)
    with pytest.raises(ValueError, match="lses must be fp32"):
        ops.attn_merge(outs, [lses[0], lses[1].double()])
    with pytest.raises(ValueError, match="lses must be fp32"):
        ops.attn_merge(outs, [lses[0], lses[1].transpose(1, 2)])
    with pytest.raises(ValueError, match="head dim 12"):
        ops.attn_merge([t[..., :12] for t in outs], lses)
    with pytest.raises(ValueError, match="output dtype"):
        ops.attn_merge(outs, lses, out_dtype=torch.float16)            # bf16 parts: bf16 or fp32
    with pytest.raises(ValueError, match="output dtype"):
        ops.attn_merge(outs, lses, out_dtype=torch.float64)
    with pytest.raises(ValueError, match="out must be"):
        ops.attn_merge(outs, lses, out=torch.zeros(2, 3, 4, 8, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="out must be"):
        ops.attn_merge(outs, lses, out=torch.zeros(2, 3, 4, 16), out_dtype=torch.bfloat16)
    assert ops.attn_merge(outs, lses, out=torch.zeros(2, 3, 4, 16))[0].dtype == torch.float32   # out's dtype is the default


# ---- shared_prefix: what is refused before anything is enqueued -----------------------------------------------------------------

def _decode_operands(paged=False):
    bf = torch.bfloat16
    q = torch.zeros(2, 4, 1, 64, dtype=bf)
    lens = torch.tensor([300, 400], dtype=torch.int32)
    if paged:
        pool = torch.zeros(12, 2, 128, 64, dtype=bf)
        return q, pool, pool.clone(), dict(cache_seqlens=lens, block_table=torch.zeros(2, 4, dtype=torch.int32))
    k = torch.zeros(2, 2, 512, 64, dtype=bf)
    return q, k, k.clone(), dict(cache_seqlens=lens)


@pytest.mark.parametrize("fn", [ops.fa3_decode, ops.fa3_prefill_cache])
def test_shared_prefix_refusals(fn):
    sig = inspect.signature(fn).parameters["shared_prefix"]
    assert sig.default is None and sig.kind is inspect.Parameter.KEYWORD_ONLY
    q, k, v, kw = _decode_operands()
    for bad in (0, -64, 32, 100, 65, 64 + 32):
        with pytest.raises(ValueError, match="positive multiple of 64"):
            fn(q, k, v, shared_prefix=bad, **kw)
    for bad in (64.0, "64", True):
        with pytest.raises(ValueError, match="host integer"):
            fn(q, k, v, shared_prefix=bad, **kw)
    for bad in (512, 576, 1 << 20):
        with pytest.raises(ValueError, match="below the cache capacity 512"):
            fn(q, k, v, shared_prefix=bad, **kw)
    with pytest.raises(ValueError, match="shared_prefix needs cache_seqlens"):
        fn(q, k, v, shared_prefix=128)
    with pytest.raises(ValueError, match="key_mask or window"):
        fn(q, k, v, shared_prefix=128, window=256, **kw)
    with pytest.raises(ValueError, match=r"cache_seqlens must be a \[B\] tensor"):
        fn(q, k, v, shared_prefix=128, cache_seqlens=kw["cache_seqlens"][:1])
    # a good P gets as far as the calls' own "no CPU path"
    with pytest.raises(ValueError, match="device tensors"):
        fn(q, k, v, shared_prefix=128, **kw)
    # with a block table: a multiple of the page size, below max_pages * page_size
    q, kp, vp, kw = _decode_operands(paged=True)
    for bad in (64, 192, 320):
        with pytest.raises(ValueError, match="multiple of the page size 128"):
            fn(q, kp, vp, shared_prefix=bad, **kw)
    with pytest.raises(ValueError, match="below the cache capacity 512"):
        fn(q, kp, vp, shared_prefix=512, **kw)
    with pytest.raises(ValueError, match="positive multiple of 64"):
        fn(q, kp, vp, shared_prefix=100, **kw)


def test_shared_prefix_refuses_a_key_mask():
    q, k, v, kw = _decode_operands()
    with pytest.raises(ValueError, match="key_mask or window"):
        ops.fa3_decode(q, k, v, shared_prefix=128, key_mask=torch.ones(2, 512, dtype=torch.bool), **kw)
    with pytest.raises(ValueError, match="key_mask or window"):
        ops.fa3_decode(q, k, v, shared_prefix=128, key_mask=torch.ones(2, 512, dtype=torch.bool))   # in front of the missing lengths
    with pytest.raises(ValueError, match="at most 64 query rows"):
        ops.fa3_decode(torch.zeros(2, 4, 65, 64, dtype=torch.bfloat16), k, v, shared_prefix=128, **kw)

"""CPU-side tests (no GPU) of the rotary embedding fused into the KV-cache append (``pfa_rope_append*``, ABI v9 additive):
every validation rule in the order the header states, the launch description, the refusals of
``ops.rope_append`` and of the attention calls' rotary keywords, and the plain-torch model of the rule (``ops.rope_append`` on CPU
tensors: the executable specification the GPU tests compare the kernel with).

The model is checked four ways: bit for bit against a loop over rows, heads and pairs written here with scalar fp32 arithmetic
(every clamp, drop and bad page id included), bit for bit against Hugging Face's ``x * cos + rotate_half(x) * sin`` evaluated in fp32,
against fp64 within the bound one final rounding plus three fp32 roundings allow, and against ``ops.kv_append`` with identity tables.
Every cache, pool and ``q_out`` holds a sentinel before a call and every packed row no sequence owns holds NaN."""

from __future__ import annotations

import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

from capi_testlib import ALIGN, DTYPE, FLAGS, HEAD_DIM, NULL, SHAPE, SIZE, STRIDE, lib  # noqa: F401
from capi_testlib import rope_append_args as _args, rope_append_paged as _pargs, rope_append_uniform as _uargs
from conftest import REPO
from photonic_flash_attention_amd import _capi, ops

SENTINEL, NAN = -7.0, float("nan")
IL = _capi.PFA_ROPE_INTERLEAVED


def _check(lib, a):
    return lib.pfa_rope_append_check(C.byref(a))


def test_the_interleaved_flag_and_the_abi_history_entry():
    header = open(os.path.join(REPO, "include", "pfa_hip.h")).read()
    assert "#define PFA_ROPE_INTERLEAVED 0x1u" in header and "v9, additive: pfa_rope_append*" in header
    assert IL == 1


# every rule of the header's "Field rules", in the order the errors are reported (the size rule is checked apart)
RULES = [
    (dict(reserved0=1), FLAGS), (dict(reserved1=-1), FLAGS),
    (dict(k_new=0), NULL), (dict(v_new=0), NULL), (dict(k_cache=0), NULL), (dict(v_cache=0), NULL), (dict(cache_seqlens=0), NULL),
    (dict(B=0), SHAPE), (dict(Hkv=0), SHAPE), (dict(Smax=0), SHAPE), (dict(total_new=0), SHAPE), (dict(max_seqlen_q=0), SHAPE),
    (dict(D=4), HEAD_DIM), (dict(D=100), HEAD_DIM), (dict(D=264), HEAD_DIM),
    (dict(dtype=2), DTYPE), (dict(dtype=-1), DTYPE),
    (dict(kn_stride_s=2 * 128 + 4), STRIDE), (dict(vn_stride_h=132), STRIDE), (dict(k_stride_b=4096 * 256 + 2), STRIDE),
    (dict(v_stride_h=129), STRIDE), (dict(k_stride_s=-256), STRIDE), (dict(v_stride_s=-256), STRIDE),
    (dict(k_new=0x1008), ALIGN), (dict(v_new=0x3004), ALIGN), (dict(k_cache=0x1000008), ALIGN), (dict(v_cache=0x2000002), ALIGN),
    (dict(cache_seqlens=0x5001), ALIGN),
    (dict(page_size=64), FLAGS), (dict(num_pages=3), FLAGS), (dict(block_table_stride_b=4), FLAGS),      # paging fields without a table
    (dict(cu_seqlens_q=0x9002), ALIGN),
    (dict(kn_stride_b=8), FLAGS), (dict(vn_stride_b=4096), FLAGS),                       # ragged rows have no batch stride
    (dict(max_seqlen_q=641), SHAPE), (dict(total_new=299), SHAPE),                       # ragged: max_seqlen_q > total_new
    # the rotary rules
    (dict(flags=2), FLAGS), (dict(flags=0x101), FLAGS),
    (dict(cos=0), NULL), (dict(sin=0), NULL),
    (dict(q_out=0), NULL), (dict(q=0), NULL),
    (dict(H=0), SHAPE), (dict(H=-2), SHAPE),
    (dict(q=0, q_out=0, H=4), FLAGS),
    (dict(max_pos=0), SHAPE), (dict(max_pos=-1), SHAPE),
    (dict(D=8, rot_dim=8), HEAD_DIM), (dict(D=24), HEAD_DIM), (dict(D=72), HEAD_DIM), (dict(rot_dim=24), HEAD_DIM), (dict(rot_dim=0), HEAD_DIM),
    (dict(rot_dim=8), HEAD_DIM), (dict(rot_dim=144), HEAD_DIM),
    (dict(q_stride_s=4 * 128 + 4), STRIDE), (dict(q_stride_h=132), STRIDE), (dict(qo_stride_s=3), STRIDE), (dict(qo_stride_h=129), STRIDE),
    (dict(cs_stride=34), STRIDE), (dict(cs_stride=28), STRIDE),
    (dict(q=0x100008), ALIGN), (dict(q_out=0x200002), ALIGN), (dict(cos=0x400004), ALIGN), (dict(sin=0x500008), ALIGN),
    (dict(pos_offsets=0x6002), ALIGN),
    (dict(q_stride_b=8), FLAGS), (dict(qo_stride_b=4096), FLAGS),                       # ragged rows have no batch stride
    (dict(B=1 << 24, total_new=1 << 20, max_seqlen_q=1 << 12), SHAPE),                  # more workgroups than a grid holds
    (dict(H=1 << 10, Hkv=1 << 9, total_new=1 << 30, max_seqlen_q=1 << 20), SHAPE),          # a sequence's items past 32 bits
]


def test_rope_append_argument_validation_in_order(lib):
    assert _check(lib, _args()) == 0 and _check(lib, _uargs()) == 0 and _check(lib, _pargs()) == 0
    assert lib.pfa_rope_append_check(None) == NULL
    bad = _args(k_new=0)
    bad.size = 16
    assert _check(lib, bad) == SIZE                                                       # before every other rule
    other = _args()
    other.size = C.sizeof(_capi.PfaKvAppendArgs)
    assert _check(lib, other) == SIZE
    for over, want in RULES:
        assert _check(lib, _args(**over)) == want, over
    # the order: of two broken rules the one stated first is reported
    pairs = 0
    for i, (first, want) in enumerate(RULES):
        for later, _ in RULES[i + 1:]:
            if set(first) & set(later) or {**first, **later}.get("q", 1) == {**first, **later}.get("q_out", 1) == 0:
                continue                                     # the same field twice; q and q_out both NULL are one legal form
            assert _check(lib, _args(**first, **later)) == want, (first, later)
            pairs += 1
    assert pairs > 1500
    uniform = [
        (dict(total_new=1499), SHAPE), (dict(B=6), SHAPE), (dict(max_seqlen_q=301), SHAPE),  # B * max_seqlen_q > total_new
        (dict(kn_stride_b=300 * 256 + 4), STRIDE), (dict(q_stride_b=3), STRIDE), (dict(qo_stride_b=300 * 512 + 4), STRIDE),
    ]
    for over, want in uniform:
        assert _check(lib, _uargs(**over)) == want, over
    paged = [
        (dict(page_size=96), SHAPE), (dict(page_size=0), SHAPE), (dict(num_pages=0), SHAPE), (dict(Smax=33 * 128), SHAPE),
        (dict(block_table_stride_b=31), SHAPE), (dict(block_table=0x8002), ALIGN), (dict(block_table=0), FLAGS),
    ]
    for over, want in paged:
        assert _check(lib, _pargs(**over)) == want, over
        assert _check(lib, _pargs(flags=2, **over)) == want, over                         # the paging rules come before the rotary ones
    # every rule pfa_kv_append shares returns what pfa_kv_append returns for it
    shared = {f for f, _ in _capi.PfaKvAppendArgs._fields_} - {"size", "flags"}
    for over, want in RULES:
        if set(over) <= shared and "D" not in over:
            a = _args(**over)
            kv = _capi.make_kv_append_args(**{f: getattr(a, f) for f in shared})
            if lib.pfa_kv_append_check(C.byref(kv)) != 0:
                assert lib.pfa_kv_append_check(C.byref(kv)) == want, over
    # the launch refuses what the check refuses, before it touches a device
    assert lib.pfa_rope_append(C.byref(_args(rot_dim=24)), None) == HEAD_DIM and lib.pfa_rope_append(None, None) == NULL


def test_rope_append_accepted_variants(lib):
    for ok in (dict(D=16, rot_dim=16), dict(D=64), dict(D=96, rot_dim=48 + 16), dict(D=256, rot_dim=256, cs_stride=128), dict(rot_dim=16),
               dict(rot_dim=128, cs_stride=64), dict(rot_dim=32, cs_stride=16), dict(cs_stride=36), dict(cs_stride=4096),
               dict(dtype=1), dict(flags=IL), dict(flags=IL, dtype=1), dict(pos_offsets=0), dict(max_pos=1), dict(H=1), dict(H=64),
               dict(q=0, q_out=0, H=0), dict(q_out=0x100000),                                # K / V only; in place
               dict(Hkv=1), dict(Smax=1), dict(B=1), dict(max_seqlen_q=640), dict(max_seqlen_q=1), dict(total_new=1, max_seqlen_q=1),
               dict(q_stride_s=8 * 128, q_stride_h=128, kn_stride_s=8 * 128, vn_stride_s=8 * 128),   # q, k, v inside a fused projection
               dict(k_stride_h=4096 * 128, k_stride_s=128, k_stride_b=2 * 4096 * 128)):       # an [B, Hkv, Smax, D] buffer
        assert _check(lib, _args(**ok)) == 0, ok
    for ok in (dict(), dict(max_seqlen_q=1, total_new=5), dict(q_stride_b=0, qo_stride_b=0, kn_stride_b=0, vn_stride_b=0), dict(flags=IL),
               dict(q=0, q_out=0, H=0, q_stride_b=0, qo_stride_b=0),
               dict(q_stride_h=300 * 128, q_stride_s=128, q_stride_b=4 * 300 * 128)):         # [B, H, Sq, D] rows
        assert _check(lib, _uargs(**ok)) == 0, ok
    for ok in (dict(), dict(_page=64), dict(_page=1024), dict(num_pages=1), dict(D=64), dict(flags=IL), dict(cu_seqlens_q=0, total_new=1500)):
        assert _check(lib, _pargs(**ok)) == 0, ok


@pytest.mark.parametrize("max_seqlen_q", [1, 3, 300, 2048])
@pytest.mark.parametrize("B,H,Hkv,D", [(5, 4, 2, 128), (64, 32, 8, 128), (3, 1, 1, 64), (2, 0, 2, 96), (1, 3, 3, 16)])
def test_rope_append_describe_counts_workgroups_from_host_shapes(lib, B, H, Hkv, D, max_seqlen_q):
    want = B * -(-max_seqlen_q * (H + 2 * Hkv) * (D // 16) // 256)
    noq = dict(q=0, q_out=0) if H == 0 else {}
    for make in (_args, _pargs, _uargs):
        a = make(B=B, H=H, Hkv=Hkv, D=D, rot_dim=16, total_new=B * 4096, max_seqlen_q=max_seqlen_q, **noq)
        name, wgs = _capi.describe_rope_append(a)
        assert wgs == want
        # device-side inputs change neither the name nor the count
        a.cache_seqlens, a.k_new, a.cos, a.sin, a.pos_offsets = 0x6000, 0x7000, 0x600000, 0x700000, 0
        if H:
            a.q, a.q_out = 0x300000, 0x300000
        if make is not _uargs:
            a.cu_seqlens_q = 0xA000
        if make is _pargs:
            a.block_table = 0xB000
        assert _capi.describe_rope_append(a) == (name, wgs)
        # and neither do total_new, the tables' length or the cache's capacity
        a.total_new, a.max_pos = B * 8192, 17
        if make is not _pargs:
            a.Smax = 8192
        assert _capi.describe_rope_append(a) == (name, wgs)


def test_rope_append_describe_names(lib):
    assert _capi.describe_rope_append(_args())[0] == "rope_append_bf16_d128_r64_varlen"
    assert _capi.describe_rope_append(_pargs(flags=IL))[0] == "rope_append_bf16_d128_r64_il_varlen_paged"
    assert _capi.describe_rope_append(_uargs(rot_dim=128, cs_stride=64))[0] == "rope_append_bf16_d128_r128"
    assert _capi.describe_rope_append(_uargs(flags=IL, dtype=1))[0] == "rope_append_fp16_d128_r64_il"
    assert _capi.describe_rope_append(_pargs(cu_seqlens_q=0, total_new=1500, dtype=1, D=96, rot_dim=32))[0] == "rope_append_fp16_d96_r32_paged"
    with pytest.raises(_capi.PfaError):
        _capi.describe_rope_append(_args(rot_dim=24))
    buf = C.create_string_buffer(8)                       # truncated, NUL terminated
    wgs = 5 * -(-300 * 8 * 8 // 256)
    assert lib.pfa_rope_append_describe(C.byref(_args()), buf, 8) == wgs and buf.value == b"rope_ap"
    assert lib.pfa_rope_append_describe(C.byref(_args()), None, 0) == wgs


# ---- refusals of the Python layer ------------------------------------------------------------------------------------------------

def test_rope_append_refusals():
    bf = torch.bfloat16
    kn, q = torch.zeros(640, 2, 64, dtype=bf), torch.zeros(640, 4, 64, dtype=bf)
    k = torch.zeros(5, 2, 512, 64, dtype=bf)
    lens = torch.tensor([100, 300, 0, 20, 400], dtype=torch.int32)
    cu = torch.tensor([0, 1, 301, 301, 334, 591], dtype=torch.int32)
    cos, sin = ops.rotary_tables(512, 64)
    ok = dict(cache_seqlens=lens, cu_seqlens_q=cu, max_seqlen_q=300, rotary_cos=cos, rotary_sin=sin)

    def call(kn_=kn, k_=k, **kw):
        return ops.rope_append(kn_, kn_.clone(), k_, k_.clone(), **dict(ok, **kw))

    assert call() is None and call(q=q).shape == q.shape                                  # the CPU model takes it
    inplace = q.clone()
    assert call(q=inplace, q_out=inplace) is inplace
    with pytest.raises(TypeError):
        ops.rope_append(kn, kn.clone(), k, k.clone(), cache_seqlens=lens, cu_seqlens_q=cu, max_seqlen_q=300, rotary_cos=cos)   # one table missing
    with pytest.raises(ValueError, match="fp32"):
        call(rotary_cos=cos.to(bf), rotary_sin=sin.to(bf))
    with pytest.raises(ValueError, match="fp32"):
        call(rotary_sin=sin.double())
    with pytest.raises(ValueError, match="fp32"):
        call(rotary_sin=None)
    with pytest.raises(ValueError, match=r"rot_dim / 2\]"):
        call(rotary_sin=sin[:, :16])
    with pytest.raises(ValueError, match=r"rot_dim / 2\]"):
        call(rotary_cos=cos[0], rotary_sin=sin[0])
    with pytest.raises(ValueError, match="rot_dim 24"):
        call(rotary_cos=cos[:, :12].contiguous(), rotary_sin=sin[:, :12].contiguous())
    with pytest.raises(ValueError, match="rot_dim 128"):                                  # more than the head dim
        call(rotary_cos=torch.zeros(512, 64), rotary_sin=torch.zeros(512, 64))
    with pytest.raises(ValueError, match="row strides equal"):
        call(rotary_cos=torch.zeros(512, 64)[:, :32])
    with pytest.raises(ValueError, match="last dim must be contiguous"):
        call(rotary_cos=torch.zeros(512, 64)[:, ::2], rotary_sin=torch.zeros(512, 64)[:, ::2])
    k72, kn72 = torch.zeros(5, 2, 512, 72, dtype=bf), torch.zeros(640, 2, 72, dtype=bf)
    with pytest.raises(ValueError, match="head dim 72"):
        call(kn72, k72)
    with pytest.raises(ValueError, match="shape mismatch: q"):
        call(q=q[:600])
    with pytest.raises(ValueError, match="shape mismatch: q"):
        call(q=q[:, :, :32])
    with pytest.raises(ValueError, match="shape mismatch: q"):
        call(q=q[None])
    with pytest.raises(ValueError, match="shape mismatch: q"):
        call(q=q[:, :0])
    with pytest.raises(ValueError, match="k_new's dtype"):
        call(q=q.half())
    with pytest.raises(ValueError, match="q_out must have q's shape and dtype"):
        call(q=q, q_out=q[:, :2].clone())
    with pytest.raises(ValueError, match="q_out without q"):
        call(q_out=q.clone())
    with pytest.raises(ValueError, match="pos_offsets"):
        call(pos_offsets=torch.zeros(5, dtype=torch.int64))
    with pytest.raises(ValueError, match="pos_offsets"):
        call(pos_offsets=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="pos_offsets"):
        call(pos_offsets=[0] * 5)
    # kv_append's own refusals, by the same code
    with pytest.raises(ValueError, match="needs max_seqlen_q"):
        call(max_seqlen_q=None)
    with pytest.raises(ValueError, match="must lie in 1 .. 640"):
        call(max_seqlen_q=641)
    with pytest.raises(ValueError, match=r"cache_seqlens must be a \[B\] tensor"):
        call(cache_seqlens=lens[:4])
    # uniform: q is [B, H, Sq, D]
    un, uq = torch.zeros(5, 2, 7, 64, dtype=bf), torch.zeros(5, 4, 7, 64, dtype=bf)
    out = ops.rope_append(un, un.clone(), k, k.clone(), cache_seqlens=lens, rotary_cos=cos, rotary_sin=sin, q=uq)
    assert out.shape == uq.shape and out.stride() == (7 * 4 * 64, 64, 4 * 64, 1)           # a view of a [B, Sq, H, D] buffer
    with pytest.raises(ValueError, match="shape mismatch: q"):
        ops.rope_append(un, un.clone(), k, k.clone(), cache_seqlens=lens, rotary_cos=cos, rotary_sin=sin, q=uq.transpose(1, 2))
    with pytest.raises(ValueError, match="shape mismatch: q"):
        ops.rope_append(un, un.clone(), k, k.clone(), cache_seqlens=lens, rotary_cos=cos, rotary_sin=sin, q=uq[:, :, :6])


def test_rotary_tables():
    cos, sin = ops.rotary_tables(4096, 128)
    assert cos.shape == sin.shape == (4096, 64) and cos.dtype == sin.dtype == torch.float32 and cos.is_contiguous()
    inv = 10000.0 ** (-torch.arange(0, 128, 2, dtype=torch.float64) / 128)
    ang = torch.arange(4096, dtype=torch.float64)[:, None] * inv
    assert torch.equal(cos, ang.cos().float()) and torch.equal(sin, ang.sin().float())
    assert bool((cos[0] == 1).all()) and bool((sin[0] == 0).all())
    c2, _ = ops.rotary_tables(8, 16, base=500000.0)
    assert c2.shape == (8, 8) and float(c2[1, 7]) == float(np.float32(np.cos(500000.0 ** (-14 / 16))))
    for bad in ((0, 16), (8, 0), (8, 15)):
        with pytest.raises(ValueError):
            ops.rotary_tables(*bad)


def test_attention_calls_refuse_incomplete_rotary_arguments():
    """Refused before anything else is looked at, CPU tensors included; without the keywords the calls are what they were."""
    bf = torch.bfloat16
    q, k, kn = torch.zeros(2, 4, 1, 64, dtype=bf), torch.zeros(2, 2, 256, 64, dtype=bf), torch.zeros(2, 2, 1, 64, dtype=bf)
    lens = torch.tensor([5, 9], dtype=torch.int32)
    cos, sin = ops.rotary_tables(256, 64)
    calls = [(ops.fa3_decode, (q, k, k.clone()), {}), (ops.fa3_prefill_cache, (q, k, k.clone()), {}),
             (ops.fa3_prefill_varlen, (q[:, :, 0], k, k.clone()), dict(cu_seqlens_q=torch.tensor([0, 1, 2], dtype=torch.int32), max_seqlen_q=1))]
    for fn, pos, kw in calls:
        new = dict(k_new=kn if fn is not ops.fa3_prefill_varlen else kn[:, :, 0], v_new=kn if fn is not ops.fa3_prefill_varlen else kn[:, :, 0])
        with pytest.raises(ValueError, match="go together"):
            fn(*pos, cache_seqlens=lens, rotary_cos=cos, **new, **kw)
        with pytest.raises(ValueError, match="go together"):
            fn(*pos, cache_seqlens=lens, rotary_sin=sin, **new, **kw)
        with pytest.raises(ValueError, match="need k_new, v_new and cache_seqlens"):
            fn(*pos, cache_seqlens=lens, rotary_cos=cos, rotary_sin=sin, **kw)
        with pytest.raises(ValueError, match="need k_new, v_new and cache_seqlens"):
            fn(*pos, cache_seqlens=lens, rotary_cos=cos, rotary_sin=sin, k_new=new["k_new"], **kw)
        if fn is not ops.fa3_decode:                          # the decode says so in its own words, as it did
            with pytest.raises(ValueError, match="need k_new, v_new and cache_seqlens"):
                fn(*pos, rotary_cos=cos, rotary_sin=sin, **new, **kw)
        with pytest.raises(ValueError, match="fp32"):
            fn(*pos, cache_seqlens=lens, rotary_cos=cos.to(bf), rotary_sin=sin.to(bf), **new, **kw)
        with pytest.raises(ValueError, match="need rotary_cos and rotary_sin"):
            fn(*pos, cache_seqlens=lens, rotary_interleaved=True, **new, **kw)
        with pytest.raises(ValueError, match="need rotary_cos and rotary_sin"):
            fn(*pos, cache_seqlens=lens, pos_offsets=lens, **new, **kw)
        with pytest.raises(ValueError, match="device tensors"):                          # no rotary: no CPU path, as before
            fn(*pos, cache_seqlens=lens, **kw)
        sig = inspect.signature(fn).parameters
        assert sig["rotary_cos"].default is None and sig["rotary_sin"].default is None and sig["pos_offsets"].default is None
        assert sig["rotary_interleaved"].default is False and sig["rotary_cos"].kind is inspect.Parameter.KEYWORD_ONLY
    sig = inspect.signature(ops.rope_append).parameters
    assert [n for n in sig][:4] == ["k_new", "v_new", "k_cache", "v_cache"]
    assert [n for n, p in sig.items() if p.kind is inspect.Parameter.KEYWORD_ONLY] == [
        "cache_seqlens", "rotary_cos", "rotary_sin", "q", "q_out", "rotary_interleaved", "pos_offsets", "cu_seqlens_q", "max_seqlen_q", "block_table"]


# ---- the CPU model against a loop over rows, heads and pairs ---------------------------------------------------------------------

Q_LENS, KV_LENS, CU = [1, 300, 0, 33, 257], [777, 300, 512, 20, 1000], [0, 1, 301, 301, 334, 591]
H, HKV, D, MAX_POS = 4, 2, 64, 1024


def _ragged(seed=11, dtype=torch.bfloat16, total=640, used=591):
    g = torch.Generator().manual_seed(seed)
    q, kn, vn = (torch.randn(total, h, D, generator=g).to(dtype) for h in (H, HKV, HKV))
    for t in (q, kn, vn):
        t[used:] = NAN                                      # the spare rows behind cu[B]
    return q, kn, vn


def _tables(R, seed=3):
    """Tables of random angles (any values serve the rule), wider than ``half`` so that the row stride is not the row length."""
    g = torch.Generator().manual_seed(seed)
    ang = (torch.rand(MAX_POS, R // 2 + 4, generator=g, dtype=torch.float64) - 0.5) * 20
    return ang.cos().float()[:, :R // 2], ang.sin().float()[:, :R // 2]


def _rotate_scalar(x, c, s, R, interleaved):
    """One head's row ``x`` (np.float32 [D]) at table rows ``c`` / ``s`` (np.float32 [R / 2]) -> np.float32 [D]: scalar fp32 arithmetic,
    each product and the add / subtract an operation of its own."""
    y = x.copy()
    half = R // 2
    for j in range(half):
        i1, i2 = (2 * j, 2 * j + 1) if interleaved else (j, j + half)
        x1, x2, cj, sj = x[i1], x[i2], c[j], s[j]
        a, b = x1 * cj, x2 * sj
        y[i1] = a - b
        a, b = x2 * cj, x1 * sj
        y[i2] = a + b
    return y


def _loop(q, q_out, k_new, v_new, k_cache, v_cache, cos, sin, lens, cu, maxq, offs, interleaved, table=None):
    """The rule one token, one head and one pair at a time on [.., Hkv, S, D]-shaped caches / pools and packed rows."""
    paged = table is not None
    ps, npages = k_cache.shape[2], k_cache.shape[0]
    Smax = table.shape[1] * ps if paged else k_cache.shape[2]
    total, max_pos, R = k_new.shape[0], cos.shape[0], 2 * cos.shape[1]
    qf, kf, cf, sf = q.float().numpy(), k_new.float().numpy(), cos.numpy(), sin.numpy()
    assert qf.dtype == kf.dtype == cf.dtype == sf.dtype == np.float32
    for b, n in enumerate(lens):
        len_b = min(max(n, 0), Smax)
        s = min(max(cu[b], 0), total)
        e = min(max(cu[b + 1], s), total)
        sq = min(e - s, maxq)
        for i in range(sq):
            pos = len_b - sq + i
            p = min(max(pos + (offs[b] if offs is not None else 0), 0), max_pos - 1)
            for h in range(q.shape[1]):
                q_out[s + i, h] = torch.from_numpy(_rotate_scalar(qf[s + i, h], cf[p], sf[p], R, interleaved)).to(q.dtype)
            if pos < 0:
                continue
            slab, tok = b, pos
            if paged:
                slab, tok = int(table[b, pos // ps]), pos % ps
                if not 0 <= slab < npages:
                    continue
            for h in range(k_new.shape[1]):
                k_cache[slab, h, tok] = torch.from_numpy(_rotate_scalar(kf[s + i, h], cf[p], sf[p], R, interleaved)).to(q.dtype)
            v_cache[slab, :, tok] = v_new[s + i]


def _both(q, kn, vn, kc, vc, cos, sin, lens, cu, maxq, offs, interleaved, table=None):
    """Run the model and the loop on copies and compare everything they write -> the model's (q_out, k, v)."""
    mq, lq = torch.full_like(q, SENTINEL), torch.full_like(q, SENTINEL)
    mk, mv, lk, lv = kc.clone(), vc.clone(), kc.clone(), vc.clone()
    got = ops.rope_append(kn, vn, mk, mv, cache_seqlens=torch.tensor(lens, dtype=torch.int32), rotary_cos=cos, rotary_sin=sin, q=q, q_out=mq,
                          rotary_interleaved=interleaved, pos_offsets=None if offs is None else torch.tensor(offs, dtype=torch.int32),
                          cu_seqlens_q=torch.tensor(cu, dtype=torch.int32), max_seqlen_q=maxq, block_table=table)
    assert got is mq
    _loop(q, lq, kn, vn, lk, lv, cos, sin, lens, cu, maxq, offs, interleaved, table)
    assert torch.equal(mq, lq) and torch.equal(mk, lk) and torch.equal(mv, lv)
    for t in (mq, mk, mv):
        assert not bool(torch.isnan(t.float()).any())       # no row that no sequence owns was read
    return mq, mk, mv


# sequence 0 sits in the middle of the table, 1 is clamped at position 0 (rows 0 .. 299 at offset -400), 3 at max_pos - 1
OFFS = [100, -400, 7, 5000, -700]


@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
@pytest.mark.parametrize("R", [64, 16])
@pytest.mark.parametrize("interleaved", [False, True], ids=["half", "interleaved"])
def test_model_equals_the_scalar_loop_on_the_ragged_fixture(interleaved, R, paged):
    q, kn, vn = _ragged()
    cos, sin = _tables(R)
    assert cos.stride(0) == R // 2 + 4
    table = None
    if paged:
        per = 1024 // 64
        perm = torch.randperm(5 * per + 3, generator=torch.Generator().manual_seed(R)).to(torch.int32)
        table = perm[:5 * per].reshape(5, per).clone()
        table[4, 12], table[4, 13] = -1, 5 * per + 3        # keys 768 .. 895 of sequence 4: page ids outside the pool
        kc = torch.full((5 * per + 3, HKV, 64, D), SENTINEL, dtype=torch.bfloat16)
    else:
        kc = torch.full((5, HKV, 1024, D), SENTINEL, dtype=torch.bfloat16)
    mq, mk, mv = _both(q, kn, vn, kc, kc.clone(), cos, sin, KV_LENS, CU, 300, OFFS, interleaved, table)
    # (e) V, and K / Q elements at and past R, are exact copies
    assert torch.equal(mq[:591, :, R:], q[:591, :, R:]) and bool((mq[591:] == SENTINEL).all())
    if R < D:
        assert not torch.equal(mq[:591, :, :R], q[:591, :, :R])
    # V lands exactly where ops.kv_append puts it, and K there too, its elements past R untouched
    ak, av = kc.clone(), kc.clone()
    ops.kv_append(kn, vn, ak, av, cache_seqlens=torch.tensor(KV_LENS, dtype=torch.int32), cu_seqlens_q=torch.tensor(CU, dtype=torch.int32),
                  max_seqlen_q=300, block_table=table)
    assert torch.equal(mv, av) and torch.equal(mk[..., R:], ak[..., R:])
    assert torch.equal((mk != SENTINEL).any(-1), (ak != SENTINEL).any(-1))
    written = 1 + 300 + 20 + 257 - (128 if paged else 0)    # sequence 3 drops 13 of its 33 rows; the bad page ids drop 128
    assert int((mk != SENTINEL).any(-1).sum()) == written * HKV
    # clamped positions: sequence 1 rotates every row at table row 0, sequence 3 at the last one
    one = torch.full_like(q[:1], SENTINEL)
    for rows, p in ((slice(1, 301), 0), (slice(301, 334), MAX_POS - 1)):
        for r in (rows.start, rows.stop - 1):
            _loop(q[r:r + 1], one, kn[r:r + 1], vn[r:r + 1], torch.zeros(1, HKV, 64, D, dtype=torch.bfloat16), torch.zeros(1, HKV, 64, D, dtype=torch.bfloat16),
                  cos[p:p + 1], sin[p:p + 1], [1], [0, 1], 1, None, interleaved)
            assert torch.equal(mq[r], one[0])


def test_model_clamps_malformed_cu_and_lengths_as_specified():
    q, kn, vn = _ragged(seed=31, total=64, used=64)
    cos, sin = _tables(32, seed=5)
    kc = torch.full((4, HKV, 128, D), SENTINEL, dtype=torch.bfloat16)
    # cu[0] < 0 -> 0; cu[2] < cu[1] -> an empty sequence at s_b = 20; cu[4] > total -> total; a length past Smax and a negative one.
    # Sequences 0 (rows 0 .. 19) and 2 (rows 8 .. 39) overlap: each rotates the caller's rows at its own positions, and of the q_out
    # rows both cover the later sequence's stay (model and loop run the sequences in order; on a device either may).
    for il in (False, True):
        mq, mk, mv = _both(q, kn, vn, kc, kc.clone(), cos, sin, [10, 500, -3, 128], [-5, 20, 8, 40, 90], 64, [3, 0, 900, -2000], il)
        assert bool((mk[1] == SENTINEL).all()) and bool((mk[2] == SENTINEL).all())   # empty; 32 rows at length 0: all dropped
        assert int((mk[0] != SENTINEL).any(-1).sum()) == 10 * HKV and int((mk[3] != SENTINEL).any(-1).sum()) == 24 * HKV
        assert torch.equal(mv[3, :, 104:128].transpose(0, 1), vn[40:64]) and torch.equal(mk[3, :, 104:128, 32:].transpose(0, 1), kn[40:64, :, 32:])
        assert not bool((mq == SENTINEL).any())             # rows 0 .. 63 are all covered, the dropped ones' Q included


# ---- (b) Hugging Face's formula ---------------------------------------------------------------------------------------------------

def _rotate_half(x):
    x1, x2 = x[..., :x.shape[-1] // 2], x[..., x.shape[-1] // 2:]
    return torch.cat((-x2, x1), dim=-1)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("R", [64, 32])
def test_model_equals_the_hugging_face_formula_in_fp32(R, dtype):
    g = torch.Generator().manual_seed(R)
    B, Sq, lens = 3, 5, [130, 5, 64]
    q, kn, vn = (torch.randn(B, h, Sq, D, generator=g).to(dtype) for h in (H, HKV, HKV))
    cos, sin = ops.rotary_tables(256, R)
    kc = torch.full((B, HKV, 256, D), SENTINEL, dtype=dtype)
    vc = kc.clone()
    out = ops.rope_append(kn, vn, kc, vc, cache_seqlens=torch.tensor(lens, dtype=torch.int32), rotary_cos=cos, rotary_sin=sin, q=q)
    for b in range(B):
        pos = torch.arange(lens[b] - Sq, lens[b])
        cf, sf = torch.cat((cos[pos], cos[pos]), -1), torch.cat((sin[pos], sin[pos]), -1)      # [Sq, R], HF's layout
        for x, y in ((q[b], out[b]), (kn[b], kc[b, :, lens[b] - Sq:lens[b]])):
            xr = x[..., :R].float()
            want = (xr * cf + _rotate_half(xr) * sf).to(dtype)
            assert torch.equal(y[..., :R], want) and torch.equal(y[..., R:], x[..., R:])
        assert torch.equal(vc[b, :, lens[b] - Sq:lens[b]], vn[b])


# ---- (c) against fp64 -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("interleaved", [False, True], ids=["half", "interleaved"])
@pytest.mark.parametrize("dtype,eps", [(torch.bfloat16, 2.0 ** -8), (torch.float16, 2.0 ** -11)], ids=["bf16", "fp16"])
@pytest.mark.parametrize("R", [16, 64, 128])
def test_model_against_fp64_within_the_rounding_bound(R, dtype, eps, interleaved):
    """|y - y64| <= eps |y64| + 2^-22 (|x1| + |x2|) + 2^-24: the final round-to-nearest (half an ulp of the dtype, or of its smallest
    subnormal) plus three fp32 roundings of terms no larger than |x1| + |x2| (|cos|, |sin| <= 1)."""
    g = torch.Generator().manual_seed(R + interleaved)
    Dh, Sq, lens = 128, 256, [256, 4096]                    # positions 0 .. 255 and 3840 .. 4095
    q, kn = (torch.randn(2, h, Sq, Dh, generator=g).to(dtype) for h in (H, HKV))
    cos, sin = ops.rotary_tables(4096, R)
    kc = torch.zeros(2, HKV, 4096, Dh, dtype=dtype)
    out = ops.rope_append(kn, kn.clone(), kc, kc.clone(), cache_seqlens=torch.tensor(lens, dtype=torch.int32), rotary_cos=cos, rotary_sin=sin,
                          q=q, rotary_interleaved=interleaved)
    worst = 0.0
    for b in range(2):
        pos = torch.arange(lens[b] - Sq, lens[b])
        c, s = cos[pos].double(), sin[pos].double()         # the same fp32 tables
        for x, y in ((q[b], out[b]), (kn[b], kc[b, :, lens[b] - Sq:lens[b]])):
            xr, yr = x[..., :R].double(), y[..., :R].double()
            sel = (lambda t: (t[..., 0::2], t[..., 1::2])) if interleaved else (lambda t: (t[..., :R // 2], t[..., R // 2:]))
            (x1, x2), (y1, y2) = sel(xr), sel(yr)
            slack = 2.0 ** -22 * (x1.abs() + x2.abs()) + 2.0 ** -24
            for got, want in ((y1, x1 * c - x2 * s), (y2, x2 * c + x1 * s)):
                ratio = (got - want).abs() / (eps * want.abs() + slack)
                worst = max(worst, float(ratio.max()))
    print(f"worst ratio to the bound: {worst:.4f}")
    assert worst <= 1.0


# ---- (d) identity tables ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("interleaved", [False, True], ids=["half", "interleaved"])
def test_model_with_identity_tables_is_kv_append(interleaved):
    q, kn, vn = _ragged(seed=17)
    cos, sin = torch.ones(MAX_POS, 32), torch.zeros(MAX_POS, 32)
    kc = torch.full((5, HKV, 1024, D), SENTINEL, dtype=torch.bfloat16)
    rk, rv, ak, av = kc.clone(), kc.clone(), kc.clone(), kc.clone()
    kw = dict(cache_seqlens=torch.tensor(KV_LENS, dtype=torch.int32), cu_seqlens_q=torch.tensor(CU, dtype=torch.int32), max_seqlen_q=300)
    out = ops.rope_append(kn, vn, rk, rv, rotary_cos=cos, rotary_sin=sin, q=q, q_out=torch.full_like(q, SENTINEL),
                          rotary_interleaved=interleaved, **kw)
    ops.kv_append(kn, vn, ak, av, **kw)
    assert torch.equal(rk, ak) and torch.equal(rv, av)
    assert torch.equal(out[:591], q[:591]) and bool((out[591:] == SENTINEL).all())
    # K / V only; and in place equals out of place
    rk2, rv2 = kc.clone(), kc.clone()
    cos, sin = _tables(64)
    assert ops.rope_append(kn, vn, rk2, rv2, rotary_cos=cos, rotary_sin=sin, rotary_interleaved=interleaved, **kw) is None
    rk3, rv3, qi = kc.clone(), kc.clone(), q.clone()
    fresh = ops.rope_append(kn, vn, rk3, rv3, rotary_cos=cos, rotary_sin=sin, q=q, q_out=torch.full_like(q, SENTINEL),
                            rotary_interleaved=interleaved, **kw)
    assert ops.rope_append(kn, vn, kc.clone(), kc.clone(), rotary_cos=cos, rotary_sin=sin, q=qi, q_out=qi, rotary_interleaved=interleaved, **kw) is qi
    assert torch.equal(rk2, rk3) and torch.equal(rv2, rv3) and torch.equal(qi[:591], fresh[:591])
    assert bool(torch.isnan(qi[591:].float()).all())        # the spare rows were left alone


# ---- PagedKVCache.write_step ------------------------------------------------------------------------------------------------------

def test_write_step_with_rotary_equals_append_varlen_of_rotated_rows():
    from photonic_flash_attention_amd.integration.pytorch import PagedKVCache

    def cache():
        c = PagedKVCache(num_pages=12, page_size=64, Hkv=HKV, D=D, dtype=torch.bfloat16, device="cpu", max_batch=3, max_pages_per_seq=4)
        for _ in range(3):
            c.allocate()
        return c

    one, two = cache(), cache()
    cos, sin = ops.rotary_tables(512, 32)
    g = torch.Generator().manual_seed(9)
    offs = torch.tensor([0, 40, -3], dtype=torch.int32)
    for lens in ([100, 1, 65], [0, 130, 27], [1, 1, 1]):
        n = sum(lens)
        q, k, v = (torch.randn(n, h, D, generator=g).to(torch.bfloat16) for h in (H, HKV, HKV))
        starts = [one.length(s) for s in range(3)]
        pos = torch.cat([torch.arange(at, at + x) + int(o) for at, x, o in zip(starts, lens, offs)]).clamp(0, 511)
        one.append_varlen([0, 1, 2], ops._rope_rotate(k, cos[pos], sin[pos], False), v, lens)
        two.advance([0, 1, 2], lens)
        out = two.write_step(k, v, lens, q=q, rotary_cos=cos, rotary_sin=sin, pos_offsets=offs)
        assert torch.equal(one.k_pool, two.k_pool) and torch.equal(one.v_pool, two.v_pool)
        assert torch.equal(out, ops._rope_rotate(q, cos[pos], sin[pos], False))
        assert two.write_step(k, v, lens, rotary_cos=cos, rotary_sin=sin, pos_offsets=offs) is None     # K / V only; idempotent
        assert torch.equal(one.k_pool, two.k_pool)
    with pytest.raises(ValueError, match="need rotary_cos and rotary_sin"):
        two.write_step(k, v, [1, 1, 1], q=q)
    with pytest.raises(ValueError, match="need rotary_cos and rotary_sin"):
        two.write_step(k, v, [1, 1, 1], rotary_interleaved=True)
    with pytest.raises(ValueError, match="go together"):
        two.write_step(k, v, [1, 1, 1], rotary_cos=cos)
    sig = inspect.signature(PagedKVCache.write_step).parameters
    assert sig["q"].default is None and sig["rotary_cos"].default is None and sig["rotary_interleaved"].default is False

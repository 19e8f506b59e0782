"""CPU-side tests (no GPU) of the rotary embedding for the training calls (``pfa_rotary*``, ABI v9 additive, declared in
``include/pfa_hip_rotary.h`` and bound by ``_capi_rotary``; ``ops.apply_rotary``; the ``rotary_*=`` keywords of ``ops.fa3_attention`` and
``ops.fa3_varlen_attention``; ``rotary=`` on the modules): every validation rule in the order the header
states (the header against its binding is tests/test_capi_conformance.py's), the launch description, the plain-torch model (``ops.apply_rotary`` on CPU tensors: the executable specification the GPU
tests compare the kernel with) against fp64 pair by pair, forward and conjugate, and the refusals of ``ops`` and of the modules."""

from __future__ import annotations

import ctypes as C
import inspect

import pytest
import torch

from capi_testlib import ALIGN, DTYPE, FLAGS, HEAD_DIM, NULL, OK, SHAPE, SIZE, STRIDE, built_lib, name_of
from photonic_flash_attention_amd import _capi, _capi_rotary, _models, ops
from photonic_flash_attention_amd.core.flash_attention_3 import FlashAttention3
from photonic_flash_attention_amd.integration.pytorch.modules import PhotonicFlashAttention, PhotonicMultiHeadAttention

IL, CONJ = _capi_rotary.PFA_ROTARY_INTERLEAVED, _capi_rotary.PFA_ROTARY_CONJUGATE
NAN = float("nan")


def rotary_args(**over):
    """A valid dense ``pfa_rotary_args`` with K, out of place: B 3, H 4 / Hkv 2, S 67, D 64, rot_dim 32, [B, S, H, D] buffers, tables
    of 128 positions."""
    d, s, h0, h1 = (over.get(n, v) for n, v in (("D", 64), ("S", 67), ("H0", 4), ("H1", 2)))
    base = dict(x0=0x100000, x0_out=0x200000, x1=0x300000, x1_out=0x400000, cos=0x500000, sin=0x600000, pos_offsets=0x7000,
                B=3, S=s, H0=h0, H1=h1, D=d, rot_dim=min(32, d), max_pos=128, dtype=0, cs_stride=min(32, d) // 2)
    for pre, h in (("x0", h0), ("x0o", h0), ("x1", h1), ("x1o", h1)):
        base.update({f"{pre}_stride_b": s * max(h, 1) * d, f"{pre}_stride_s": max(h, 1) * d, f"{pre}_stride_h": d})
    base.update(over)
    return _capi_rotary.make_rotary_args(**base)


def packed_args(**over):
    """The packed call of the ragged fixture: B 5, 640 rows of which a sequence has at most 300."""
    return rotary_args(**{**dict(cu_seqlens=0x9000, B=5, S=300, total=640), **over})


def inplace_args(**over):
    return rotary_args(**{**dict(x0_out=0x100000, x1_out=0x300000), **over})


@pytest.fixture(scope="module")
def lib():
    built_lib()
    return _capi_rotary.load()


def _check(lib, a):
    return lib.pfa_rotary_check(C.byref(a))


# every rule of the header's "Field rules", in the order the errors are reported (the size rule is checked apart)
RULES = [
    (dict(flags=4), FLAGS), (dict(flags=0x101), FLAGS),
    (dict(position_ids=0x8000), FLAGS),                                                 # together with the default block's pos_offsets
    (dict(x1_out=0x300000), FLAGS), (dict(x0_out=0x100000), FLAGS),                     # one tensor in place, the other not
    (dict(x0=0), NULL), (dict(x0_out=0), NULL), (dict(cos=0), NULL), (dict(sin=0), NULL),
    (dict(x1=0), NULL), (dict(x1_out=0), NULL), (dict(H1=0), NULL),                     # x1 / x1_out both NULL exactly when H1 = 0
    (dict(B=0), SHAPE), (dict(S=0), SHAPE), (dict(H0=0), SHAPE), (dict(H1=-1), SHAPE), (dict(max_pos=0), SHAPE), (dict(max_pos=-1), SHAPE),
    (dict(D=8, rot_dim=8), HEAD_DIM), (dict(D=24), HEAD_DIM), (dict(D=72), HEAD_DIM), (dict(D=272), HEAD_DIM), (dict(rot_dim=24), HEAD_DIM),
    (dict(rot_dim=0), HEAD_DIM), (dict(rot_dim=8), HEAD_DIM), (dict(rot_dim=80), HEAD_DIM),
    (dict(dtype=2), DTYPE), (dict(dtype=-1), DTYPE),
    (dict(x0_stride_s=4 * 64 + 4), STRIDE), (dict(x0_stride_h=65), STRIDE), (dict(x0o_stride_s=3), STRIDE), (dict(x0o_stride_h=68), STRIDE),
    (dict(x1_stride_s=2 * 64 + 2), STRIDE), (dict(x1_stride_h=60), STRIDE), (dict(x1o_stride_s=1), STRIDE), (dict(x1o_stride_h=-4), STRIDE),
    (dict(x0_stride_b=67 * 256 + 4), STRIDE), (dict(x1o_stride_b=7), STRIDE),
    (dict(cs_stride=18), STRIDE), (dict(cs_stride=12), STRIDE),
    (dict(x0=0x100008), ALIGN), (dict(x0_out=0x200002), ALIGN), (dict(x1=0x300004), ALIGN), (dict(x1_out=0x400001), ALIGN),
    (dict(cos=0x500004), ALIGN), (dict(sin=0x600008), ALIGN), (dict(pos_offsets=0x7002), ALIGN),
    (dict(B=1 << 24, S=1 << 12), SHAPE),                                                # more workgroups than a grid holds
    (dict(H0=1 << 10, H1=1 << 9, S=1 << 20), SHAPE),                                    # a sequence's items past 32 bits
]


def test_argument_validation_in_order(lib):
    assert _check(lib, rotary_args()) == OK and _check(lib, packed_args()) == OK and _check(lib, inplace_args()) == OK
    assert lib.pfa_rotary_check(None) == NULL
    bad = rotary_args(x0=0, flags=4)
    bad.size = 16
    assert _check(lib, bad) == SIZE                                                       # before every other rule
    for over, want in RULES:
        assert _check(lib, rotary_args(**over)) == want, over
    # the order: of two broken rules the one stated first is reported
    pairs = 0
    for i, (first, want) in enumerate(RULES):
        for later, _ in RULES[i + 1:]:
            both = {**first, **later}
            if set(first) & set(later):
                continue                                     # the same field twice
            if "H1" in both and ({"x1", "x1_out"} & set(both)):
                continue                                     # x1 and H1 spoilt together can make the legal Q-only form
            if {"x0", "x0_out", "x1", "x1_out"} & set(first) and {"x0", "x0_out", "x1", "x1_out"} & set(later):
                continue                                     # two pointers moved can land in (or leave) the in-place form
            assert _check(lib, rotary_args(**both)) == want, (first, later)
            pairs += 1
    assert pairs > 1000
    packed = [(dict(total=0), SHAPE), (dict(total=299), SHAPE), (dict(S=641), SHAPE), (dict(cu_seqlens=0x9002), ALIGN),
              (dict(x0_stride_b=3, x1o_stride_b=-1), OK),                                 # packed rows have no batch stride: not looked at
              (dict(position_ids=0x8000, pos_offsets=0), OK), (dict(position_ids=0x8002, pos_offsets=0), ALIGN)]
    for over, want in packed:
        assert _check(lib, packed_args(**over)) == want, over
    inplace = [(dict(x0o_stride_s=512), STRIDE), (dict(x0o_stride_h=128), STRIDE), (dict(x1o_stride_s=256), STRIDE), (dict(x1o_stride_h=128), STRIDE),
               (dict(x0o_stride_b=8), STRIDE), (dict(x1o_stride_b=8), STRIDE)]           # the same tensor has the same strides
    for over, want in inplace:
        assert _check(lib, inplace_args(**over)) == want, over
    assert _check(lib, inplace_args(cu_seqlens=0x9000, B=5, S=300, total=640, x0o_stride_b=8)) == OK
    # the launch refuses what the check refuses, before it touches a device
    assert lib.pfa_rotary(C.byref(rotary_args(rot_dim=24)), None) == HEAD_DIM and lib.pfa_rotary(None, None) == NULL


def test_accepted_variants(lib):
    q_only = dict(x1=0, x1_out=0, H1=0)
    for ok in (dict(D=16), dict(D=96, rot_dim=64, cs_stride=32), dict(D=256, rot_dim=256, cs_stride=128), q_only, dict(rot_dim=16, cs_stride=8),
               dict(rot_dim=64, cs_stride=32), dict(cs_stride=20), dict(cs_stride=4096), dict(dtype=1), dict(flags=IL), dict(flags=CONJ),
               dict(flags=IL | CONJ, dtype=1), dict(pos_offsets=0), dict(pos_offsets=0, position_ids=0x8000, pid_stride_b=67, pid_stride_s=1),
               dict(max_pos=1), dict(H0=1), dict(H0=64), dict(B=1), dict(S=1),
               dict(x0_stride_b=4 * 67 * 64, x0_stride_h=67 * 64, x0_stride_s=64),            # a contiguous [B, H, S, D] tensor
               dict(x0_stride_s=8 * 64, x1_stride_s=8 * 64)):                                 # q and k inside a fused projection
        assert _check(lib, rotary_args(**ok)) == OK, ok
        if "x0_stride_s" not in ok:
            assert _check(lib, inplace_args(**ok)) == OK, ok
    for ok in (dict(), q_only, dict(S=1), dict(S=640), dict(total=300), dict(flags=IL), dict(D=256, rot_dim=256, cs_stride=128), dict(D=16)):
        assert _check(lib, packed_args(**ok)) == OK, ok


@pytest.mark.parametrize("S", [1, 5, 67, 300, 4096])
@pytest.mark.parametrize("B,H0,H1,D,R", [(3, 4, 2, 64, 32), (4, 16, 16, 128, 128), (2, 32, 8, 64, 64), (1, 3, 0, 16, 16), (5, 1, 1, 256, 48), (2, 8, 2, 96, 64)])
def test_describe_counts_workgroups_from_host_shapes(lib, B, H0, H1, D, R, S):
    noq = dict(x1=0, x1_out=0) if H1 == 0 else {}
    shape = dict(B=B, H0=H0, H1=H1, D=D, rot_dim=R, cs_stride=R // 2, S=S, **noq)
    for make, kw in ((rotary_args, {}), (packed_args, dict(total=B * 4096))):
        for inplace, per_head in ((False, D // 16), (True, R // 16)):      # in place only the rotated units are items
            a = make(**shape, **kw)
            if inplace:
                a.x0_out, a.x1_out = a.x0, a.x1
            name, wgs = _capi_rotary.describe_rotary(a)
            assert wgs == B * -(-S * (H0 + H1) * per_head // 256), (name, wgs)
            assert name.endswith("_inplace") == inplace
            # device-side inputs change neither the name nor the count, and neither do the tables' length and the packed rows held
            a.cos, a.sin, a.pos_offsets, a.max_pos = 0x700000, 0x800000, 0, 17
            if make is packed_args:
                a.cu_seqlens, a.total = 0xA000, B * 8192
            assert _capi_rotary.describe_rotary(a) == (name, wgs)


def test_describe_names(lib):
    d = _capi_rotary.describe_rotary
    assert d(rotary_args())[0] == "rotary_bf16" and d(rotary_args()) == ("rotary_bf16", 3 * 7)      # 67 * 24 items: seven workgroups a sequence
    assert d(inplace_args()) == ("rotary_bf16_inplace", 3 * 4)                                       # 67 * 12 items
    assert d(packed_args(flags=IL))[0] == "rotary_bf16_packed_interleaved"
    assert d(rotary_args(flags=CONJ, dtype=1))[0] == "rotary_fp16_conj"
    assert d(inplace_args(cu_seqlens=0x9000, B=5, S=300, total=640, flags=IL | CONJ, dtype=1))[0] == "rotary_fp16_packed_interleaved_conj_inplace"
    with pytest.raises(_capi.PfaError):
        d(rotary_args(rot_dim=24))
    buf = C.create_string_buffer(8)                       # truncated, NUL terminated
    assert lib.pfa_rotary_describe(C.byref(rotary_args()), buf, 8) == 21 and buf.value == b"rotary_"
    assert lib.pfa_rotary_describe(C.byref(rotary_args()), None, 0) == 21
    assert name_of(lib.pfa_rotary_describe, rotary_args(x0=0))[0] == NULL


# ---- the model against fp64, pair by pair -----------------------------------------------------------------------------------------

def _pairs(t, R, interleaved):
    return (t[..., 0:R:2], t[..., 1:R:2]) if interleaved else (t[..., :R // 2], t[..., R // 2:R])


def _rotate64(x, c, s, R, interleaved):
    """The rotation of ``x`` [B, H, S, D] in fp64 with the table rows ``c`` / ``s`` [S, R / 2] (the fp32 values widened)."""
    x1, x2 = _pairs(x, R, interleaved)
    y1, y2 = x1 * c - x2 * s, x2 * c + x1 * s
    out = x.clone()
    if interleaved:
        out[..., 0:R:2], out[..., 1:R:2] = y1, y2
    else:
        out[..., :R // 2], out[..., R // 2:R] = y1, y2
    return out


def _worst_ratio(got, want, x, R, interleaved, dtype):
    """max over pairs of |y - y64| / bound, with the issue's bound: bf16 2^-8 |y64| + 2^-22 (|x1| + |x2|); fp16 2^-11 |y64| + 2^-25 in place
    of the first term.  Half a unit in the last place of the result, and three fp32 roundings of terms no larger than |x1| + |x2|."""
    x1, x2 = (t.abs() for t in _pairs(x.double(), R, interleaved))
    slack = 2.0 ** -22 * (x1 + x2)
    worst = 0.0
    for g, w in zip(_pairs(got.double(), R, interleaved), _pairs(want, R, interleaved)):
        first = 2.0 ** -8 * w.abs() if dtype == torch.bfloat16 else 2.0 ** -11 * w.abs() + 2.0 ** -25
        worst = max(worst, float(((g - w).abs() / (first + slack)).max()))
    return worst


@pytest.mark.parametrize("interleaved", [False, True], ids=["half", "interleaved"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("R", [16, 64, 128])
def test_model_and_its_conjugate_against_fp64_within_the_rounding_bound(R, dtype, interleaved):
    g = torch.Generator().manual_seed(R + interleaved)
    B, S, D = 2, 96, 128
    q, k = (torch.randn(B, h, S, D, generator=g).to(dtype) for h in (4, 2))
    cos, sin = ops.rotary_tables(4096, R)
    offs = torch.tensor([0, 4000], dtype=torch.int32)      # positions 0 .. 95 and 4000 .. 4095
    kw = dict(rotary_cos=cos, rotary_sin=sin, rotary_interleaved=interleaved, pos_offsets=offs)
    qo, ko = ops.apply_rotary(q, k, **kw)
    dq, dk = ops.apply_rotary(q, k, conjugate=True, **kw)  # q and k standing in for the incoming gradients
    worst = 0.0
    for x, y, dx in ((q, qo, dq), (k, ko, dk)):
        assert torch.equal(y[..., R:], x[..., R:]) and torch.equal(dx[..., R:], x[..., R:])
        for b in range(B):
            pos = torch.arange(S) + int(offs[b])
            c, s = cos[pos].double(), sin[pos].double()   # the same fp32 tables, widened
            x64 = x[b:b + 1].double().requires_grad_(True)
            y64 = _rotate64(x64, c, s, R, interleaved)
            worst = max(worst, _worst_ratio(y[b:b + 1], y64.detach(), x[b:b + 1], R, interleaved, dtype))
            # the conjugate: the fp64 autograd gradient of the fp64 rotation at dout = x
            (g64,) = torch.autograd.grad(y64, x64, x[b:b + 1].double())
            worst = max(worst, _worst_ratio(dx[b:b + 1], g64, x[b:b + 1], R, interleaved, dtype))
    print(f"worst ratio to the bound: {worst:.4f}")
    assert 0.0 < worst <= 1.0


def test_mutants_of_the_rotation_miss_the_bound():
    # a fused multiply-add is inside the bound (it is closer to fp64), a wrong sign or the other pairing is far outside
    g = torch.Generator().manual_seed(2)
    x = torch.randn(1, 2, 32, 64, generator=g).bfloat16()
    cos, sin = ops.rotary_tables(64, 64)
    pos = torch.arange(32)
    want = _rotate64(x.double(), cos[pos].double(), sin[pos].double(), 64, False)
    good = ops.apply_rotary(x, rotary_cos=cos, rotary_sin=sin)
    assert _worst_ratio(good, want, x, 64, False, torch.bfloat16) <= 1.0
    for mutant in (ops.apply_rotary(x, rotary_cos=cos, rotary_sin=sin, conjugate=True), ops.apply_rotary(x, rotary_cos=cos, rotary_sin=sin, rotary_interleaved=True)):
        assert _worst_ratio(mutant, want, x, 64, False, torch.bfloat16) > 10.0


def test_model_positions_packed_rows_and_the_in_place_form():
    g = torch.Generator().manual_seed(7)
    cu = torch.tensor([0, 1, 301, 301, 334, 591], dtype=torch.int32)
    q, k = (torch.randn(640, h, 64, generator=g).bfloat16() for h in (4, 2))
    for t in (q, k):
        t[591:] = NAN                                      # the spare rows behind cu[B]
    cos, sin = ops.rotary_tables(128, 32)
    kw = dict(rotary_cos=cos, rotary_sin=sin, cu_seqlens=cu)
    qi, ki = q.clone(), k.clone()
    got = ops.apply_rotary(qi, ki, max_seqlen=256, inplace=True, **kw)
    assert got[0] is qi and got[1] is ki
    # rows 257 .. 300 (the 300-row sequence's rows past max_seqlen) and everything at and past rot_dim are untouched
    assert torch.equal(qi[257:301], q[257:301]) and torch.equal(qi[:591, :, 32:], q[:591, :, 32:]) and bool(torch.isnan(qi[591:].float()).all())
    pos = torch.cat([torch.arange(n) for n in (1, 256)]).clamp(max=127)      # rows at and past 128 rotate at 127
    want = _models._rope_rotate(q[:257], cos[pos], sin[pos], False)
    assert torch.equal(qi[:257], want) and not torch.equal(qi[129:257], q[129:257])
    assert torch.equal(ki[:257], _models._rope_rotate(k[:257], cos[pos], sin[pos], False))
    # position_ids, not monotonic, against offsets that give the same positions; both together are refused
    ids = torch.zeros(640, dtype=torch.int32)
    ids[1:301] = torch.arange(300, 0, -1, dtype=torch.int32) - 150                     # 150 .. -149: clamped at both ends of the table
    a = ops.apply_rotary(q, max_seqlen=300, position_ids=ids, **kw)
    p = ids[1:301].to(torch.int64).clamp(0, 127)
    assert torch.equal(a[1:301], _models._rope_rotate(q[1:301], cos[p], sin[p], False))
    off = torch.tensor([5, -3, 0, 127, 200], dtype=torch.int32)
    b = ops.apply_rotary(q, max_seqlen=300, pos_offsets=off, **kw)
    p = (torch.arange(33) + 127).clamp(0, 127)
    assert torch.equal(b[301:334], _models._rope_rotate(q[301:334], cos[p], sin[p], False))
    assert torch.equal(b[1:4], _models._rope_rotate(q[1:4], cos[[0, 0, 0]], sin[[0, 0, 0]], False))      # -3, -2, -1 clamp to 0
    # the conjugate undoes the rotation up to rounding, and autograd's gradient IS the conjugate model on dout
    x = q[:591].clone().requires_grad_(True)
    y = ops.apply_rotary(x, rotary_cos=cos, rotary_sin=sin, cu_seqlens=cu, max_seqlen=300, pos_offsets=off)
    dout = torch.randn(591, 4, 64, generator=g).bfloat16()
    keep = dout.clone()
    y.backward(dout)
    want = ops.apply_rotary(dout, rotary_cos=cos, rotary_sin=sin, cu_seqlens=cu, max_seqlen=300, pos_offsets=off, conjugate=True)
    assert torch.equal(x.grad, want) and torch.equal(dout, keep)                        # incoming gradients are not modified


# ---- refusals of the Python layer ------------------------------------------------------------------------------------------------

def test_apply_rotary_refusals():
    bf = torch.bfloat16
    q, k = torch.zeros(2, 4, 7, 64, dtype=bf), torch.zeros(2, 2, 7, 64, dtype=bf)
    cos, sin = ops.rotary_tables(64, 32)
    ok = dict(rotary_cos=cos, rotary_sin=sin)
    out = ops.apply_rotary(q, k, **ok)
    assert isinstance(out, tuple) and out[0].shape == q.shape and out[0].stride() == (7 * 4 * 64, 64, 4 * 64, 1)      # a [B, S, H, D] buffer
    assert ops.apply_rotary(q, **ok).shape == q.shape
    with pytest.raises(TypeError):
        ops.apply_rotary(q, k, rotary_cos=cos)
    with pytest.raises(ValueError, match="bf16 / fp16 operands"):
        ops.apply_rotary(q.float(), **ok)
    with pytest.raises(ValueError, match="fp32"):
        ops.apply_rotary(q, rotary_cos=cos.to(bf), rotary_sin=sin.to(bf))
    with pytest.raises(ValueError, match="fp32"):
        ops.apply_rotary(q, rotary_cos=cos, rotary_sin=sin.double())
    with pytest.raises(ValueError, match="head dim 72"):
        ops.apply_rotary(torch.zeros(2, 4, 7, 72, dtype=bf), **ok)
    with pytest.raises(ValueError, match="head dim 264"):
        ops.apply_rotary(torch.zeros(2, 4, 7, 264, dtype=bf), **ok)
    with pytest.raises(ValueError, match="rot_dim 24"):
        ops.apply_rotary(q, rotary_cos=cos[:, :12].contiguous(), rotary_sin=sin[:, :12].contiguous())
    with pytest.raises(ValueError, match="rot_dim 128"):
        ops.apply_rotary(q, rotary_cos=torch.zeros(64, 64), rotary_sin=torch.zeros(64, 64))
    for bad in (k[:, :, :6], k[:1], k[..., :32], torch.zeros(2, 2, 9, 64, dtype=bf)):
        with pytest.raises(ValueError, match="make two calls"):
            ops.apply_rotary(q, bad, **ok)
    with pytest.raises(ValueError, match="q's dtype"):
        ops.apply_rotary(q, k.half(), **ok)
    with pytest.raises(ValueError, match=r"\[B, H, S, D\]"):
        ops.apply_rotary(q[0], **ok)
    with pytest.raises(ValueError, match="max_seqlen goes with cu_seqlens"):
        ops.apply_rotary(q, max_seqlen=7, **ok)
    with pytest.raises(ValueError, match="exclude each other"):
        ops.apply_rotary(q, pos_offsets=torch.zeros(2, dtype=torch.int32), position_ids=torch.zeros(2, 7, dtype=torch.int32), **ok)
    for bad in (torch.zeros(2, dtype=torch.int64), torch.zeros(3, dtype=torch.int32), [0, 0]):
        with pytest.raises(ValueError, match="pos_offsets"):
            ops.apply_rotary(q, pos_offsets=bad, **ok)
    for bad in (torch.zeros(2, 7, dtype=torch.int64), torch.zeros(2, 6, dtype=torch.int32), torch.zeros(14, dtype=torch.int32)):
        with pytest.raises(ValueError, match="position_ids"):
            ops.apply_rotary(q, position_ids=bad, **ok)
    grad = q.clone().requires_grad_(True)
    with pytest.raises(ValueError, match="requires grad"):
        ops.apply_rotary(grad, inplace=True, **ok)
    with pytest.raises(ValueError, match="requires grad"):
        ops.apply_rotary(q.clone(), k.clone().requires_grad_(True), inplace=True, **ok)
    with torch.no_grad():
        assert ops.apply_rotary(grad, inplace=True, **ok) is grad
    with pytest.raises(ValueError, match="inplace=True"):
        ops.apply_rotary(torch.zeros(2, 4, 7, 128, dtype=bf)[..., ::2], inplace=True, **ok)
    # packed
    pq, cu = torch.zeros(10, 4, 64, dtype=bf), torch.tensor([0, 4, 10], dtype=torch.int32)
    assert ops.apply_rotary(pq, cu_seqlens=cu, max_seqlen=6, **ok).shape == pq.shape
    for bad in (dict(max_seqlen=None), dict(max_seqlen=11), dict(max_seqlen=0), dict(max_seqlen=True)):
        with pytest.raises(ValueError, match="max_seqlen"):
            ops.apply_rotary(pq, **{**dict(cu_seqlens=cu, max_seqlen=6), **bad}, **ok)
    for bad in (cu.long(), cu[:1], cu[None], [0, 4, 10]):
        with pytest.raises(ValueError, match="cu_seqlens must be"):
            ops.apply_rotary(pq, cu_seqlens=bad, max_seqlen=6, **ok)
    with pytest.raises(ValueError, match="make two calls"):
        ops.apply_rotary(pq, torch.zeros(9, 2, 64, dtype=bf), cu_seqlens=cu, max_seqlen=6, **ok)
    with pytest.raises(ValueError, match="position_ids"):
        ops.apply_rotary(pq, cu_seqlens=cu, max_seqlen=6, position_ids=torch.zeros(2, 5, dtype=torch.int32), **ok)
    sig = inspect.signature(ops.apply_rotary).parameters
    assert list(sig) == ["q", "k", "rotary_cos", "rotary_sin", "rotary_interleaved", "cu_seqlens", "max_seqlen", "pos_offsets", "position_ids",
                         "conjugate", "inplace"]
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for n, p in sig.items() if n not in ("q", "k")) and sig["k"].default is None


def test_attention_calls_refuse_bad_rotary_arguments_before_anything_is_enqueued():
    bf = torch.bfloat16
    q, k = torch.zeros(2, 4, 5, 64, dtype=bf), torch.zeros(2, 2, 5, 64, dtype=bf)
    qv, kv = torch.zeros(6, 4, 64, dtype=bf), torch.zeros(6, 2, 64, dtype=bf)
    cu = torch.tensor([0, 3, 6], dtype=torch.int32)
    cos, sin = ops.rotary_tables(64, 64)
    calls = [(lambda **kw: ops.fa3_attention(q, k, k, **kw)), (lambda **kw: ops.fa3_attention(q, k, k, sinks=torch.zeros(4), **kw)),
             (lambda **kw: ops.fa3_varlen_attention(qv, kv, kv, cu, cu, 3, 3, **kw)),
             (lambda **kw: ops.fa3_varlen_attention(qv, kv, kv, cu, cu, 3, 3, sinks=torch.zeros(4), **kw))]
    for call in calls:
        with pytest.raises(ValueError, match="go together"):
            call(rotary_cos=cos)
        with pytest.raises(ValueError, match="go together"):
            call(rotary_sin=sin)
        for alone in (dict(rotary_interleaved=True), dict(pos_offsets=cu[:2]), dict(position_ids=torch.zeros(2, 5, dtype=torch.int32))):
            with pytest.raises(ValueError, match="need rotary_cos and rotary_sin"):
                call(**alone)
        with pytest.raises(ValueError, match="fp32"):
            call(rotary_cos=cos.to(bf), rotary_sin=sin.to(bf))
        with pytest.raises(ValueError, match="rot_dim 128"):
            call(rotary_cos=torch.zeros(64, 64), rotary_sin=torch.zeros(64, 64))
        with pytest.raises(ValueError, match="exclude each other"):
            call(rotary_cos=cos, rotary_sin=sin, pos_offsets=cu[:2], position_ids=torch.zeros(2, 5, dtype=torch.int32))
    with pytest.raises(ValueError, match="bf16 / fp16 operands"):                        # fp32 operands are not rotated
        ops.fa3_attention(q.float(), k.float(), k.float(), rotary_cos=cos, rotary_sin=sin)
    for fn in (ops.fa3_attention, ops.fa3_varlen_attention):
        sig = inspect.signature(fn).parameters
        assert list(sig)[-5:] == ["rotary_cos", "rotary_sin", "rotary_interleaved", "pos_offsets", "position_ids"]
        assert all(sig[n].kind is inspect.Parameter.KEYWORD_ONLY for n in list(sig)[-5:])
        assert [sig[n].default for n in list(sig)[-5:]] == [None, None, False, None, None]


def test_modules_hold_tables_outside_the_state_dict_and_refuse_what_rotary_cannot_do():
    for cls in (FlashAttention3, PhotonicFlashAttention, PhotonicMultiHeadAttention):
        torch.manual_seed(5)
        plain = cls(64, 4)
        torch.manual_seed(5)
        off = cls(64, 4, rotary=False)
        torch.manual_seed(5)
        on = cls(64, 4, rotary=True, rotary_base=500000.0, rotary_max_position=96)
        pre = "" if cls is FlashAttention3 else "gpu_attention."
        keys = [pre + n for n in ("qkv_proj.weight", "qkv_proj.bias", "out_proj.weight", "out_proj.bias")]
        assert list(plain.state_dict()) == keys == list(off.state_dict()) == list(on.state_dict())
        for k in keys:                                                   # the option draws nothing from the generator
            assert torch.equal(plain.state_dict()[k], on.state_dict()[k]) and torch.equal(plain.state_dict()[k], off.state_dict()[k])
        on.load_state_dict(plain.state_dict())                           # a checkpoint made without the option loads with it, and back
        plain.load_state_dict(on.state_dict())
        core, core_off = (m if cls is FlashAttention3 else m.gpu_attention for m in (on, off))
        assert core.rotary and not core_off.rotary and not hasattr(core_off, "rotary_cos")
        assert [n for n, _ in core_off.named_buffers()] == [] and [n for n, _ in core.named_buffers()] == ["rotary_cos", "rotary_sin"]
        want = ops.rotary_tables(96, 16, 500000.0)
        assert torch.equal(core.rotary_cos, want[0]) and torch.equal(core.rotary_sin, want[1]) and core.rotary_cos.dtype == torch.float32
    with pytest.raises(ValueError, match="rotary does not combine with attention dropout"):
        FlashAttention3(64, 4, dropout=0.1, rotary=True)
    with pytest.raises(ValueError, match="multiple of 16"):
        FlashAttention3(96, 4, rotary=True)
    m = FlashAttention3(64, 4, rotary=True)
    with pytest.raises(RuntimeError, match="MI355X only"):
        m(torch.zeros(1, 8, 64))
    # (the seam refuses on what it is asked for and the operands' dtype, before it looks at the data)
    m_cuda = type("Q", (), {"is_cuda": True, "requires_grad": False, "dtype": torch.float32})()
    with pytest.raises(NotImplementedError, match="need_weights together with rotary"):
        m._flash_attention_forward(m_cuda, m_cuda, m_cuda, None, True)
    with pytest.raises(ValueError, match='fp32_attention="bf16"'):
        m._flash_attention_forward(m_cuda, m_cuda, m_cuda, None, False)

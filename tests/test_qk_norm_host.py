"""CPU-side tests (no GPU) of QK-norm fused with the rotary embedding of the training calls (``pfa_qk_norm*`` / ``pfa_qk_norm_bwd*``, ABI v9
additive, declared in ``include/pfa_hip_qk_norm.h`` and bound by ``_capi_qk_norm``; ``ops.qk_norm``; the ``q_norm_weight=`` keywords of
``ops.fa3_attention`` and ``ops.fa3_varlen_attention``; ``qk_norm=`` on the modules): every validation
rule in the order the header states (pairwise: of two broken rules the earlier wins), the launch descriptions, the workspace, the
plain-torch models (``ops.qk_norm`` on CPU tensors: the executable specification the GPU tests compare the kernels with) against fp64
element by element under the bounds derived in tests/qk_norm_testlib.py, mutants of the rule that must each miss those bounds, and the
refusals of ``ops`` and of the modules.

Worst ratios to the bounds seen here (printed by the tests): forward 0.996, dx 0.994 (a 16-bit result next to a power of two is half
a unit in the last place, 2^-8 of its size, from fp64 by the final rounding alone), dw 0.007."""

from __future__ import annotations

import ctypes as C
import inspect

import pytest
import torch

import qk_norm_testlib as Q
from capi_testlib import ALIGN, DTYPE, FLAGS, HEAD_DIM, NULL, OK, SHAPE, SIZE, STRIDE, built_lib, name_of
from photonic_flash_attention_amd import _capi, _capi_qk_norm, ops
from photonic_flash_attention_amd.core.flash_attention_3 import FlashAttention3
from photonic_flash_attention_amd.core.hybrid_router import HybridFlashAttention
from photonic_flash_attention_amd.integration.pytorch.modules import PhotonicFlashAttention, PhotonicMultiHeadAttention

IL, UNIT = _capi_qk_norm.PFA_QKNORM_INTERLEAVED, _capi_qk_norm.PFA_QKNORM_UNIT_OFFSET
EPS = 1e-6


def _shape(over):
    return tuple(over.get(n, v) for n, v in (("D", 64), ("S", 67), ("H0", 4), ("H1", 2)))


def fwd_args(**over):
    """A valid dense ``pfa_qk_norm_args`` with K, out of place: B 3, H 4 / Hkv 2, S 67, D 64, rot_dim 32, [B, S, H, D] buffers, fp32
    weights, tables of 128 positions."""
    d, s, h0, h1 = _shape(over)
    base = dict(x0=0x100000, x0_out=0x200000, x1=0x300000, x1_out=0x400000, w0=0x700000, w1=0x710000, cos=0x500000, sin=0x600000,
                pos_offsets=0x7000, B=3, S=s, H0=h0, H1=h1, D=d, rot_dim=32, max_pos=128, dtype=0, w_dtype=2, cs_stride=16, eps=EPS)
    for pre, h in (("x0", h0), ("x0o", h0), ("x1", h1), ("x1o", h1)):
        base.update({f"{pre}_stride_b": s * max(h, 1) * d, f"{pre}_stride_s": max(h, 1) * d, f"{pre}_stride_h": d})
    base.update(over)
    return _capi_qk_norm.make_qk_norm_args(**base)


def bwd_args(**over):
    """The ``pfa_qk_norm_bwd_args`` of the same problem, with a workspace large enough for any shape here."""
    d, s, h0, h1 = _shape(over)
    base = dict(x0=0x100000, dy0=0x200000, dx0=0x300000, w0=0x700000, dw0=0x720000, x1=0x400000, dy1=0x800000, dx1=0x900000, w1=0x710000,
                dw1=0x730000, cos=0x500000, sin=0x600000, pos_offsets=0x7000, workspace=0x4000000, workspace_bytes=1 << 40,
                B=3, S=s, H0=h0, H1=h1, D=d, rot_dim=32, max_pos=128, dtype=0, w_dtype=2, cs_stride=16, eps=EPS)
    for pre, h in (("x0", h0), ("dy0", h0), ("dx0", h0), ("x1", h1), ("dy1", h1), ("dx1", h1)):
        base.update({f"{pre}_stride_b": s * max(h, 1) * d, f"{pre}_stride_s": max(h, 1) * d, f"{pre}_stride_h": d})
    base.update(over)
    return _capi_qk_norm.make_qk_norm_bwd_args(**base)


PACKED = dict(cu_seqlens=0x9000, B=5, S=300, total=640)
INPLACE = dict(x0_out=0x100000, x1_out=0x300000)


@pytest.fixture(scope="module")
def lib():
    built_lib()
    return _capi_qk_norm.load()


# every rule of the header's "Field rules", in the order the errors are reported (the size rule is checked apart)
COMMON_TAIL = [
    (dict(B=0), SHAPE), (dict(S=0), SHAPE), (dict(H0=0), SHAPE), (dict(H1=-1), SHAPE), (dict(max_pos=0), SHAPE), (dict(max_pos=-1), SHAPE),
    (dict(eps=-1.0), SHAPE), (dict(eps=float("inf")), SHAPE), (dict(eps=float("nan")), SHAPE),
    (dict(D=16), HEAD_DIM), (dict(D=32), HEAD_DIM), (dict(D=96), HEAD_DIM), (dict(D=256), HEAD_DIM), (dict(D=72), HEAD_DIM),
    (dict(rot_dim=24), HEAD_DIM), (dict(rot_dim=8), HEAD_DIM), (dict(rot_dim=80), HEAD_DIM), (dict(rot_dim=-16), HEAD_DIM),
    (dict(dtype=2), DTYPE), (dict(dtype=-1), DTYPE), (dict(w_dtype=1), DTYPE), (dict(w_dtype=3), DTYPE),          # an fp32 x is refused
]
FWD_RULES = [
    (dict(flags=4), FLAGS), (dict(flags=0x101), FLAGS),
    (dict(position_ids=0x8000), FLAGS),                                                 # together with the default block's pos_offsets
    (dict(x1_out=0x300000), FLAGS), (dict(x0_out=0x100000), FLAGS),                     # one tensor in place, the other not
    (dict(x0=0), NULL), (dict(x0_out=0), NULL), (dict(w0=0), NULL),
    (dict(x1=0), NULL), (dict(x1_out=0), NULL), (dict(w1=0), NULL), (dict(H1=0), NULL), # x1 / x1_out / w1 all NULL exactly when H1 = 0
    (dict(cos=0), NULL), (dict(sin=0), NULL), (dict(rot_dim=0), NULL),                  # cos / sin both NULL exactly when rot_dim = 0
] + COMMON_TAIL + [
    (dict(x0_stride_s=4 * 64 + 4), STRIDE), (dict(x0_stride_h=65), STRIDE), (dict(x0o_stride_s=3), STRIDE), (dict(x0o_stride_h=68), STRIDE),
    (dict(x1_stride_s=2 * 64 + 2), STRIDE), (dict(x1_stride_h=60), STRIDE), (dict(x1o_stride_s=1), STRIDE), (dict(x1o_stride_h=-4), STRIDE),
    (dict(x0_stride_b=67 * 256 + 4), STRIDE), (dict(x1o_stride_b=7), STRIDE),
    (dict(cs_stride=18), STRIDE), (dict(cs_stride=12), STRIDE),
    (dict(x0=0x100008), ALIGN), (dict(x0_out=0x200002), ALIGN), (dict(x1=0x300004), ALIGN), (dict(x1_out=0x400001), ALIGN),
    (dict(w0=0x700008), ALIGN), (dict(w1=0x710004), ALIGN), (dict(cos=0x500004), ALIGN), (dict(sin=0x600008), ALIGN),
    (dict(pos_offsets=0x7002), ALIGN),
    (dict(B=1 << 24, S=1 << 12), SHAPE),                                                # more workgroups than a grid holds
    (dict(H0=1 << 10, H1=1 << 9, S=1 << 20), SHAPE),                                    # a sequence's items past 32 bits
]
BWD_RULES = [
    (dict(flags=4), FLAGS), (dict(flags=0x101), FLAGS), (dict(position_ids=0x8000), FLAGS),
    (dict(dx0=0x100000), FLAGS), (dict(dx0=0x200000), FLAGS), (dict(dx1=0x400000), FLAGS), (dict(dx1=0x800000), FLAGS),      # in place
    (dict(x0=0), NULL), (dict(dy0=0), NULL), (dict(dx0=0), NULL), (dict(w0=0), NULL), (dict(dw0=0), NULL), (dict(workspace=0), NULL),
    (dict(x1=0), NULL), (dict(dy1=0), NULL), (dict(dx1=0), NULL), (dict(w1=0), NULL), (dict(dw1=0), NULL), (dict(H1=0), NULL),
    (dict(cos=0), NULL), (dict(sin=0), NULL), (dict(rot_dim=0), NULL),
] + COMMON_TAIL + [
    (dict(x0_stride_s=4 * 64 + 4), STRIDE), (dict(dy0_stride_h=65), STRIDE), (dict(dx0_stride_s=3), STRIDE), (dict(x1_stride_h=60), STRIDE),
    (dict(dy1_stride_s=1), STRIDE), (dict(dx1_stride_h=-4), STRIDE), (dict(dy0_stride_b=67 * 256 + 4), STRIDE), (dict(dx1_stride_b=7), STRIDE),
    (dict(cs_stride=18), STRIDE), (dict(cs_stride=12), STRIDE),
    (dict(x0=0x100008), ALIGN), (dict(dy0=0x200002), ALIGN), (dict(dx0=0x300004), ALIGN), (dict(x1=0x400001), ALIGN), (dict(dy1=0x800008), ALIGN),
    (dict(dx1=0x900008), ALIGN), (dict(w0=0x700008), ALIGN), (dict(w1=0x710004), ALIGN), (dict(cos=0x500004), ALIGN), (dict(sin=0x600008), ALIGN),
    (dict(dw0=0x720002), ALIGN), (dict(dw1=0x730001), ALIGN), (dict(workspace=0x4000002), ALIGN), (dict(pos_offsets=0x7002), ALIGN),
    (dict(B=1 << 26, S=1 << 12), SHAPE),                                                # more stage-1 workgroups than a grid holds
    (dict(H0=1 << 10, H1=1 << 9, S=1 << 20), SHAPE),                                    # a sequence's items past 32 bits
    (dict(workspace_bytes=2 * 3 * 3 * 64 * 4 - 1), NULL),                               # one byte short of T * B * ceil(67 / 32) * D floats
]
FWD_PTRS, BWD_PTRS = {"x0", "x0_out", "x1", "x1_out"}, {"x0", "dy0", "dx0", "x1", "dy1", "dx1"}
FWD_K, BWD_K = {"x1", "x1_out", "w1"}, {"x1", "dy1", "dx1", "w1", "dw1"}


def _pairwise(check, make, rules, ptrs, k_fields):
    pairs = 0
    for i, (first, want) in enumerate(rules):
        for later, _ in rules[i + 1:]:
            both = {**first, **later}
            if set(first) & set(later):
                continue                                     # the same field twice
            if "H1" in both and (k_fields & set(both)):
                continue                                     # x1 and H1 spoilt together can make the legal Q-only form
            if ptrs & set(first) and ptrs & set(later):
                continue                                     # two pointers moved can land in (or leave) an in-place form
            if "rot_dim" in both and ({"cos", "sin"} & set(both)):
                continue                                     # rot_dim 0 and a NULL table together are one half of the legal norm-only form
            assert check(make(**both)) == want, (first, later)
            pairs += 1
    return pairs


def test_forward_argument_validation_in_order_pairwise(lib):
    def check(a):
        return lib.pfa_qk_norm_check(C.byref(a))
    assert check(fwd_args()) == OK and check(fwd_args(**PACKED)) == OK and check(fwd_args(**INPLACE)) == OK
    assert lib.pfa_qk_norm_check(None) == NULL
    bad = fwd_args(x0=0, flags=4)
    bad.size = 16
    assert check(bad) == SIZE                                                              # before every other rule
    for over, want in FWD_RULES:
        assert check(fwd_args(**over)) == want, over
    assert _pairwise(check, fwd_args, FWD_RULES, FWD_PTRS, FWD_K) > 1500
    packed = [(dict(total=0), SHAPE), (dict(total=299), SHAPE), (dict(S=641), SHAPE), (dict(cu_seqlens=0x9002), ALIGN),
              (dict(x0_stride_b=3, x1o_stride_b=-1), OK),                                 # packed rows have no batch stride: not looked at
              (dict(position_ids=0x8000, pos_offsets=0), OK), (dict(position_ids=0x8002, pos_offsets=0), ALIGN)]
    for over, want in packed:
        assert check(fwd_args(**{**PACKED, **over})) == want, over
    inplace = [(dict(x0o_stride_s=512), STRIDE), (dict(x0o_stride_h=128), STRIDE), (dict(x1o_stride_s=256), STRIDE), (dict(x1o_stride_h=128), STRIDE),
               (dict(x0o_stride_b=8), STRIDE), (dict(x1o_stride_b=8), STRIDE)]           # the same tensor has the same strides
    for over, want in inplace:
        assert check(fwd_args(**{**INPLACE, **over})) == want, over
    assert check(fwd_args(**INPLACE, **PACKED, x0o_stride_b=8)) == OK
    # the launch refuses what the check refuses, before it touches a device
    assert lib.pfa_qk_norm(C.byref(fwd_args(rot_dim=24)), None) == HEAD_DIM and lib.pfa_qk_norm(None, None) == NULL


def test_backward_argument_validation_in_order_pairwise(lib):
    def check(a):
        return lib.pfa_qk_norm_bwd_check(C.byref(a))
    assert check(bwd_args()) == OK and check(bwd_args(**PACKED)) == OK and lib.pfa_qk_norm_bwd_check(None) == NULL
    bad = bwd_args(x0=0, flags=4)
    bad.size = 16
    assert check(bad) == SIZE
    for over, want in BWD_RULES:
        assert check(bwd_args(**over)) == want, over
    assert _pairwise(check, bwd_args, BWD_RULES, BWD_PTRS, BWD_K) > 1500
    for over, want in [(dict(total=0), SHAPE), (dict(S=641), SHAPE), (dict(cu_seqlens=0x9002), ALIGN), (dict(dy0_stride_b=3, dx1_stride_b=-1), OK),
                       (dict(workspace_bytes=2 * 5 * 10 * 64 * 4), OK), (dict(workspace_bytes=2 * 5 * 10 * 64 * 4 - 1), NULL)]:
        assert check(bwd_args(**{**PACKED, **over})) == want, over
    assert lib.pfa_qk_norm_bwd(C.byref(bwd_args(D=96)), None) == HEAD_DIM and lib.pfa_qk_norm_bwd(None, None) == NULL


def test_accepted_variants(lib):
    q_only = dict(x1=0, x1_out=0, w1=0, H1=0)
    norm_only = dict(rot_dim=0, cos=0, sin=0, pos_offsets=0, max_pos=0, cs_stride=0)
    for ok in (dict(D=128), dict(D=128, rot_dim=128, cs_stride=64), q_only, norm_only, {**q_only, **norm_only}, dict(rot_dim=16, cs_stride=8),
               dict(rot_dim=64, cs_stride=32), dict(cs_stride=20), dict(cs_stride=4096), dict(dtype=1, w_dtype=1), dict(dtype=1), dict(w_dtype=0),
               dict(flags=IL), dict(flags=UNIT), dict(flags=IL | UNIT), dict(eps=0.0), dict(eps=1e-5), dict(pos_offsets=0),
               dict(pos_offsets=0, position_ids=0x8000, pid_stride_b=67, pid_stride_s=1), dict(max_pos=1), dict(H0=1), dict(H0=64), dict(B=1),
               dict(S=1), dict(x0_stride_b=4 * 67 * 64, x0_stride_h=67 * 64, x0_stride_s=64), dict(x0_stride_s=8 * 64, x1_stride_s=8 * 64)):
        assert lib.pfa_qk_norm_check(C.byref(fwd_args(**ok))) == OK, ok
        if "x0_stride_s" not in ok:
            assert lib.pfa_qk_norm_check(C.byref(fwd_args(**{**INPLACE, **ok}))) == OK, ok
        bok = {("dx1" if k == "x1_out" else k): v for k, v in ok.items()}
        if "H1" in ok:
            bok.update(dy1=0, dw1=0)
        assert lib.pfa_qk_norm_bwd_check(C.byref(bwd_args(**bok))) == OK, ok


@pytest.mark.parametrize("S", [1, 5, 67, 300, 4096])
@pytest.mark.parametrize("B,H0,H1,D,R", [(3, 4, 2, 64, 32), (4, 16, 16, 128, 128), (2, 32, 8, 64, 64), (1, 3, 0, 64, 0), (5, 1, 1, 128, 48)])
def test_describe_counts_workgroups_and_the_workspace_from_host_shapes(lib, B, H0, H1, D, R, S):
    rows = ops.QKNORM_BWD_ROWS
    assert rows == 32
    shape = dict(B=B, H0=H0, H1=H1, D=D, rot_dim=R, cs_stride=R // 2, S=S)
    if R == 0:
        shape.update(cos=0, sin=0, pos_offsets=0)
    for kw in ({}, dict(cu_seqlens=0x9000, total=B * 4096)):
        a = fwd_args(**shape, **kw, **(dict(x1=0, x1_out=0, w1=0) if H1 == 0 else {}))
        b = bwd_args(**shape, **kw, **(dict(x1=0, dy1=0, dx1=0, w1=0, dw1=0) if H1 == 0 else {}))
        (name, wgs), (bname, bwgs) = _capi_qk_norm.describe_qk_norm(a), _capi_qk_norm.describe_qk_norm_bwd(b)
        assert wgs == B * -(-S * (H0 + H1) * (D // 16) // 256), (name, wgs)
        assert bwgs == (2 if H1 else 1) * B * -(-S // rows) and bname.endswith(f"_r{rows}+dw"), (bname, bwgs)
        assert _capi_qk_norm.bwd_workspace_bytes(b) == bwgs * D * 4
        # device-side inputs change neither the names nor the counts nor the bytes; a block without any pointer still has its bytes
        for blk in (a, b):
            blk.pos_offsets, blk.max_pos = 0, 17
            if kw:
                blk.cu_seqlens, blk.total = 0xA000, B * 8192
        b.workspace = b.x0 = b.dw0 = 0
        assert _capi_qk_norm.describe_qk_norm(a) == (name, wgs) and _capi_qk_norm.bwd_workspace_bytes(b) == bwgs * D * 4
    for refused in (dict(D=96), dict(B=0), dict(S=0), dict(H0=0), dict(H1=-1), dict(cu_seqlens=0x9000, total=0), dict(B=1 << 26, S=1 << 12)):
        assert _capi_qk_norm.bwd_workspace_bytes(bwd_args(**refused)) == 0, refused
    short = bwd_args()
    short.size = 16
    assert _capi_qk_norm.bwd_workspace_bytes(short) == 0 and lib.pfa_qk_norm_bwd_workspace_bytes(None) == 0


def test_describe_names(lib):
    d, db = _capi_qk_norm.describe_qk_norm, _capi_qk_norm.describe_qk_norm_bwd
    assert d(fwd_args()) == ("qk_norm_bf16_d64_rot_w32", 3 * 7)                            # 67 * 24 items: seven workgroups a sequence
    assert d(fwd_args(**INPLACE)) == ("qk_norm_bf16_d64_rot_w32_inplace", 3 * 7)           # in place every unit changes all the same
    assert d(fwd_args(**PACKED, flags=IL))[0] == "qk_norm_bf16_d64_packed_interleaved_rot_w32"
    assert d(fwd_args(flags=UNIT, dtype=1, w_dtype=1, D=128))[0] == "qk_norm_fp16_d128_rot_unit"
    assert d(fwd_args(rot_dim=0, cos=0, sin=0, pos_offsets=0, flags=IL | UNIT, w_dtype=0))[0] == "qk_norm_bf16_d64_interleaved_unit"
    assert db(bwd_args()) == ("qk_norm_bwd_bf16_d64_rot_w32_r32+dw", 2 * 3 * 3)
    assert db(bwd_args(**PACKED, flags=IL | UNIT, dtype=1, w_dtype=1, D=128))[0] == "qk_norm_bwd_fp16_d128_packed_interleaved_rot_unit_r32+dw"
    with pytest.raises(_capi.PfaError):
        d(fwd_args(rot_dim=24))
    with pytest.raises(_capi.PfaError):
        db(bwd_args(dx0=0x100000))
    buf = C.create_string_buffer(8)                       # truncated, NUL terminated
    assert lib.pfa_qk_norm_describe(C.byref(fwd_args()), buf, 8) == 21 and buf.value == b"qk_norm"
    assert lib.pfa_qk_norm_describe(C.byref(fwd_args()), None, 0) == 21 and lib.pfa_qk_norm_bwd_describe(C.byref(bwd_args()), None, 0) == 18
    assert name_of(lib.pfa_qk_norm_describe, fwd_args(x0=0))[0] == NULL and name_of(lib.pfa_qk_norm_bwd_describe, bwd_args(dw0=0))[0] == NULL


# ---- the models against fp64, element by element ---------------------------------------------------------------------------------------

def _problem(D, R, dtype, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    B, S = 2, 40
    q, k, gq, gk = ((scale * torch.randn(B, h, S, D, generator=g)).to(dtype) for h in (3, 2, 3, 2))
    wq, wk = (1.0 + 0.5 * torch.randn(D, generator=g) for _ in range(2))
    offs = torch.tensor([0, 4000], dtype=torch.int32)
    tabs = ops.rotary_tables(4096, R) if R else (None, None)
    return q, k, gq, gk, wq, wk, offs, tabs


CASES = [(64, 0), (64, 32), (64, 64), (128, 0), (128, 48), (128, 128)]


@pytest.mark.parametrize("interleaved", [False, True], ids=["half", "interleaved"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("D,R", CASES)
def test_forward_model_against_fp64_within_the_rounding_bound(D, R, dtype, interleaved):
    """The bound is ``2^-8 |y| + K 2^-24 (|n1| + |n2|)`` (fp16: ``2^-11 |y| + 2^-25 + ...``) with K = 20 fp32 roundings on the longest
    path, counted in tests/qk_norm_testlib.py: 12 in the sum tree at D 128, eps, sqrt, divide, two scale products, the unit offset, a
    rotation product and its add."""
    unit = bool((D + R) // 16 % 2)
    q, k, _, _, wq, wk, offs, (cos, sin) = _problem(D, R, dtype, D + R + interleaved)
    if dtype == torch.float16:
        wq, wk = wq.half(), wk.half()                    # weights of the tensors' dtype
    kw = dict(rotary_cos=cos, rotary_sin=sin, rotary_interleaved=interleaved, pos_offsets=offs) if R else {}
    qo, ko = ops.qk_norm(q, k, q_weight=wq, k_weight=wk, eps=EPS, unit_offset=unit, **kw)
    worst = 0.0
    for x, y, w in ((q, qo, wq), (k, ko, wk)):
        for (xb, yb), c, s in Q.each_sequence([x, y], cos, sin, offsets=offs):
            worst = max(worst, Q.forward_ratio(yb, xb, w, EPS, unit, c, s, interleaved))
    print(f"worst ratio to the bound: {worst:.4f}")
    assert 0.0 < worst <= 1.0


@pytest.mark.parametrize("interleaved", [False, True], ids=["half", "interleaved"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("D,R", CASES)
def test_backward_model_against_fp64_autograd_within_the_rounding_bounds(D, R, dtype, interleaved):
    """dx: ``2^-8 |dx| + K' 2^-24 r (A_j + |xh_j| sum(A |xh|) / D)`` with K' = 66; dw: ``(N + 19) 2^-24 sum |g| |xh|`` over N = rows x
    heads terms.  Both constants are counted in tests/qk_norm_testlib.py.  The reference is torch.autograd on the fp64 RMSNorm + rotation:
    it guards the formula itself."""
    unit = bool((D + R) // 16 % 2)
    q, k, gq, gk, wq, wk, offs, (cos, sin) = _problem(D, R, dtype, 100 + D + R + interleaved)
    geo = ops._qk_norm_geometry(q, k, wq, wk, EPS, cos, sin, None, None, offs if R else None, None)
    dxs, dws = ops._qk_norm_bwd_call([q, k], [gq, gk], [wq, wk], geo, EPS, unit, cos, sin, interleaved, None, offs if R else None, None)
    worst_dx = worst_dw = 0.0
    for x, dy, dx, w, dw in ((q, gq, dxs[0], wq, dws[0]), (k, gk, dxs[1], wk, dws[1])):
        for (xb, dyb, dxb), c, s in Q.each_sequence([x, dy, dx], cos, sin, offsets=offs):
            dx64, _ = Q.backward64(xb, dyb, w, EPS, unit, c, s, interleaved)
            bound, _ = Q.backward_bounds(xb, dyb, w, EPS, unit, c, s, interleaved, dx64, dtype)
            worst_dx = max(worst_dx, float(((dxb.double() - dx64).abs() / bound).max()))
            # the closed form the kernels evaluate is autograd's gradient
            closed = Q.backward_mutant64(xb, dyb, w, EPS, unit, c, s, interleaved, None)
            assert float((closed - dx64).abs().max()) <= 1e-12 * float(dx64.abs().max())
        want, bound = Q.dw_reference(x, dy, w, EPS, unit, cos, sin, interleaved, offsets=offs)
        worst_dw = max(worst_dw, float(((dw.double() - want).abs() / bound).max()))
        assert dw.dtype == torch.float32 and float(want.abs().max()) > 0
    print(f"worst ratios to the bounds: dx {worst_dx:.4f}, dw {worst_dw:.4f}")
    assert 0.0 < worst_dx <= 1.0 and 0.0 < worst_dw <= 1.0


@pytest.mark.parametrize("mutant", ["no_eps", "mean_over_R", "weight_first", "unit"])
def test_mutants_of_the_forward_miss_the_bound(mutant):
    # tiny x for the eps mutant: mean(x^2) is then of eps's size; everywhere else unit-size data
    q, _, _, _, wq, _, offs, (cos, sin) = _problem(64, 32, torch.bfloat16, 7, scale=1e-3 if mutant == "no_eps" else 1.0)
    good = ops.qk_norm(q, q_weight=wq, eps=EPS, rotary_cos=cos, rotary_sin=sin, pos_offsets=offs)
    for flag in (False, True):
        if flag:
            good = ops.qk_norm(q, q_weight=wq, eps=EPS, unit_offset=True, rotary_cos=cos, rotary_sin=sin, pos_offsets=offs)
        worst_good = worst_bad = 0.0
        for (xb, yb), c, s in Q.each_sequence([q, good], cos, sin, offsets=offs):
            worst_good = max(worst_good, Q.forward_ratio(yb, xb, wq, EPS, flag, c, s, False))
            bad, _ = Q.forward64(xb.double(), wq.double(), EPS, flag, c, s, False, mutant=mutant)
            worst_bad = max(worst_bad, Q.forward_ratio(bad.to(q.dtype), xb, wq, EPS, flag, c, s, False))
        assert worst_good <= 1.0 < worst_bad, (mutant, flag, worst_good, worst_bad)
        assert worst_bad > 10.0


@pytest.mark.parametrize("mutant", ["sign", "no_c"])
def test_mutants_of_the_backward_miss_the_bound(mutant):
    q, _, gq, _, wq, _, offs, (cos, sin) = _problem(64, 32, torch.bfloat16, 9)
    worst = 0.0
    for (xb, dyb), c, s in Q.each_sequence([q, gq], cos, sin, offsets=offs):
        dx64, _ = Q.backward64(xb, dyb, wq, EPS, False, c, s, False)
        bound, _ = Q.backward_bounds(xb, dyb, wq, EPS, False, c, s, False, dx64, q.dtype)
        bad = Q.backward_mutant64(xb, dyb, wq, EPS, False, c, s, False, mutant).to(q.dtype)
        worst = max(worst, float(((bad.double() - dx64).abs() / bound).max()))
    assert worst > 10.0, (mutant, worst)


def test_model_positions_packed_rows_the_in_place_form_and_autograd():
    g = torch.Generator().manual_seed(7)
    cu = torch.tensor([0, 1, 301, 301, 334, 591], dtype=torch.int32)
    q, k = (torch.randn(640, h, 64, generator=g).bfloat16() for h in (4, 2))
    for t in (q, k):
        t[591:] = float("nan")                             # the spare rows behind cu[B]
    wq, wk = (1.0 + 0.5 * torch.randn(64, generator=g) for _ in range(2))
    cos, sin = ops.rotary_tables(128, 32)
    kw = dict(q_weight=wq, k_weight=wk, rotary_cos=cos, rotary_sin=sin, cu_seqlens=cu)
    qi, ki = q.clone(), k.clone()
    got = ops.qk_norm(qi, ki, max_seqlen=256, inplace=True, **kw)
    assert got[0] is qi and got[1] is ki
    # rows 257 .. 300 (the 300-row sequence's rows past max_seqlen) are untouched, the spare rows stay NaN, everything else changed
    assert torch.equal(qi[257:301], q[257:301]) and bool(torch.isnan(qi[591:].float()).all()) and not bool(torch.isnan(qi[:591].float()).any())
    fresh = ops.qk_norm(q, k, max_seqlen=256, **kw)
    assert torch.equal(fresh[0][:257], qi[:257]) and torch.equal(fresh[1][301:590], ki[301:590])      # row 590 is the 257th of its sequence
    # the fused call is the norm alone followed by the rotation only up to the rounding in between: they differ, by less than 2 ulp
    normed = ops.qk_norm(q, q_weight=wq, cu_seqlens=cu, max_seqlen=300)
    two_step = ops.apply_rotary(normed, rotary_cos=cos, rotary_sin=sin, cu_seqlens=cu, max_seqlen=300)
    fused = ops.qk_norm(q, q_weight=wq, rotary_cos=cos, rotary_sin=sin, cu_seqlens=cu, max_seqlen=300)
    assert torch.equal(fused[:591, :, 32:], normed[:591, :, 32:]) and not torch.equal(fused[:591], two_step[:591])
    # autograd's four gradients ARE the backward model's, and the incoming gradients are not modified
    x, y, a, b = (t.clone().requires_grad_(True) for t in (q[:591], k[:591], wq, wk))
    off = torch.tensor([5, -3, 0, 127, 200], dtype=torch.int32)
    qo, ko = ops.qk_norm(x, y, q_weight=a, k_weight=b, rotary_cos=cos, rotary_sin=sin, cu_seqlens=cu, max_seqlen=300, pos_offsets=off)
    dq, dk = torch.randn(591, 4, 64, generator=g).bfloat16(), torch.randn(591, 2, 64, generator=g).bfloat16()
    keep = dq.clone()
    torch.autograd.backward((qo, ko), (dq, dk))
    geo = ops._qk_norm_geometry(q[:591], k[:591], wq, wk, 1e-6, cos, sin, cu, 300, off, None)
    dxs, dws = ops._qk_norm_bwd_call([q[:591], k[:591]], [dq, dk], [wq, wk], geo, 1e-6, False, cos, sin, False, cu, off, None)
    assert torch.equal(x.grad, dxs[0]) and torch.equal(y.grad, dxs[1]) and torch.equal(a.grad, dws[0]) and torch.equal(b.grad, dws[1])
    assert torch.equal(dq, keep)
    # a 16-bit weight gets its gradient in its own dtype
    b16 = wq.bfloat16().requires_grad_(True)
    ops.qk_norm(q[:591], q_weight=b16, cu_seqlens=cu, max_seqlen=300).backward(dq)
    assert b16.grad.dtype == torch.bfloat16 and bool(torch.isfinite(b16.grad.float()).all())


# ---- refusals of the Python layer ------------------------------------------------------------------------------------------------

def test_qk_norm_refusals():
    bf = torch.bfloat16
    q, k = torch.zeros(2, 4, 7, 64, dtype=bf), torch.zeros(2, 2, 7, 64, dtype=bf)
    w = torch.ones(64)
    cos, sin = ops.rotary_tables(64, 32)
    out = ops.qk_norm(q, k, q_weight=w, k_weight=w)
    assert isinstance(out, tuple) and out[0].shape == q.shape and out[0].stride() == (7 * 4 * 64, 64, 4 * 64, 1)      # a [B, S, H, D] buffer
    assert ops.qk_norm(q, q_weight=w.to(bf), rotary_cos=cos, rotary_sin=sin).shape == q.shape
    with pytest.raises(TypeError):
        ops.qk_norm(q, k)
    with pytest.raises(ValueError, match="bf16 / fp16 operands"):
        ops.qk_norm(q.float(), q_weight=w)
    for d in (16, 32, 96, 256):
        with pytest.raises(ValueError, match=f"head dim {d}"):
            ops.qk_norm(torch.zeros(2, 4, 7, d, dtype=bf), q_weight=torch.ones(d))
    with pytest.raises(ValueError, match="go together"):
        ops.qk_norm(q, q_weight=w, rotary_cos=cos)
    with pytest.raises(ValueError, match="k and k_weight go together"):
        ops.qk_norm(q, k, q_weight=w)
    with pytest.raises(ValueError, match="k and k_weight go together"):
        ops.qk_norm(q, q_weight=w, k_weight=w)
    with pytest.raises(ValueError, match="need rotary_cos and rotary_sin"):
        ops.qk_norm(q, q_weight=w, pos_offsets=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="exclude each other"):
        ops.qk_norm(q, q_weight=w, rotary_cos=cos, rotary_sin=sin, pos_offsets=torch.zeros(2, dtype=torch.int32),
                    position_ids=torch.zeros(2, 7, dtype=torch.int32))
    with pytest.raises(ValueError, match="fp32"):
        ops.qk_norm(q, q_weight=w, rotary_cos=cos.to(bf), rotary_sin=sin.to(bf))
    with pytest.raises(ValueError, match="rot_dim 24"):
        ops.qk_norm(q, q_weight=w, rotary_cos=cos[:, :12].contiguous(), rotary_sin=sin[:, :12].contiguous())
    for bad in (torch.ones(63), torch.ones(64, 1), torch.ones(64, dtype=torch.float16), torch.ones(64, dtype=torch.float64), [1.0] * 64):
        with pytest.raises(ValueError, match="norm weight"):
            ops.qk_norm(q, q_weight=bad)
    with pytest.raises(ValueError, match="share a dtype"):
        ops.qk_norm(q, k, q_weight=w, k_weight=w.to(bf))
    for bad in (-1e-6, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="eps"):
            ops.qk_norm(q, q_weight=w, eps=bad)
    with pytest.raises(ValueError, match="make two calls"):
        ops.qk_norm(q, k[:, :, :6], q_weight=w, k_weight=w)
    with pytest.raises(ValueError, match="max_seqlen goes with cu_seqlens"):
        ops.qk_norm(q, q_weight=w, max_seqlen=7)
    for leaf in (dict(q=q.clone().requires_grad_(True)), dict(q_weight=w.clone().requires_grad_(True))):
        with pytest.raises(ValueError, match="requires grad"):
            ops.qk_norm(**{**dict(q=q.clone(), q_weight=w), **leaf}, inplace=True)
    with torch.no_grad():
        grad = q.clone().requires_grad_(True)
        assert ops.qk_norm(grad, q_weight=w, inplace=True) is grad
    with pytest.raises(ValueError, match="inplace=True"):
        ops.qk_norm(torch.zeros(2, 4, 7, 128, dtype=bf)[..., ::2], q_weight=w, inplace=True)
    sig = inspect.signature(ops.qk_norm).parameters
    assert list(sig) == ["q", "k", "q_weight", "k_weight", "eps", "unit_offset", "rotary_cos", "rotary_sin", "rotary_interleaved", "cu_seqlens",
                         "max_seqlen", "pos_offsets", "position_ids", "inplace"]
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for n, p in sig.items() if n not in ("q", "k")) and sig["k"].default is None
    assert (sig["eps"].default, sig["unit_offset"].default, sig["inplace"].default) == (1e-6, False, False)


def test_attention_calls_refuse_bad_qk_norm_arguments_before_anything_is_enqueued():
    bf = torch.bfloat16
    q, k = torch.zeros(2, 4, 5, 64, dtype=bf), torch.zeros(2, 2, 5, 64, dtype=bf)
    qv, kv = torch.zeros(6, 4, 64, dtype=bf), torch.zeros(6, 2, 64, dtype=bf)
    cu = torch.tensor([0, 3, 6], dtype=torch.int32)
    w = torch.ones(64)
    calls = [(lambda **kw: ops.fa3_attention(q, k, k, **kw)), (lambda **kw: ops.fa3_attention(q, k, k, sinks=torch.zeros(4), **kw)),
             (lambda **kw: ops.fa3_varlen_attention(qv, kv, kv, cu, cu, 3, 3, **kw)),
             (lambda **kw: ops.fa3_varlen_attention(qv, kv, kv, cu, cu, 3, 3, sinks=torch.zeros(4), **kw))]
    for call in calls:
        with pytest.raises(ValueError, match="q_norm_weight and k_norm_weight go together"):
            call(q_norm_weight=w)
        with pytest.raises(ValueError, match="q_norm_weight and k_norm_weight go together"):
            call(k_norm_weight=w)
        with pytest.raises(ValueError, match="needs q_norm_weight"):
            call(qk_norm_unit_offset=True)
        with pytest.raises(ValueError, match="norm weight"):
            call(q_norm_weight=w, k_norm_weight=torch.ones(32))
        with pytest.raises(ValueError, match="eps"):
            call(q_norm_weight=w, k_norm_weight=w, qk_norm_eps=-1.0)
        with pytest.raises(ValueError, match="go together"):
            call(q_norm_weight=w, k_norm_weight=w, rotary_cos=torch.zeros(8, 16))
    with pytest.raises(ValueError, match="bf16 / fp16 operands"):                        # fp32 operands are not normalised
        ops.fa3_attention(q.float(), k.float(), k.float(), q_norm_weight=w, k_norm_weight=w)
    new = ["q_norm_weight", "k_norm_weight", "qk_norm_eps", "qk_norm_unit_offset"]
    for fn in (ops.fa3_attention, ops.fa3_varlen_attention):
        sig = inspect.signature(fn).parameters
        assert all(sig[n].kind is inspect.Parameter.KEYWORD_ONLY for n in new) and [sig[n].default for n in new] == [None, None, 1e-6, False]


def test_modules_hold_the_norm_weights_in_the_state_dict_only_with_the_option_and_refuse_what_rotary_refuses():
    for cls in (FlashAttention3, PhotonicFlashAttention, PhotonicMultiHeadAttention, HybridFlashAttention):
        torch.manual_seed(5)
        plain = cls(256, 4)
        torch.manual_seed(5)
        off = cls(256, 4, qk_norm=False)
        torch.manual_seed(5)
        on = cls(256, 4, qk_norm=True, qk_norm_eps=1e-5)
        pre = "" if cls is FlashAttention3 else "gpu_attention."
        keys = [pre + n for n in ("qkv_proj.weight", "qkv_proj.bias", "out_proj.weight", "out_proj.bias")]
        assert list(plain.state_dict()) == keys == list(off.state_dict())
        assert list(on.state_dict()) == keys + [pre + "q_norm.weight", pre + "k_norm.weight"]
        for key in keys:                                                 # the option draws nothing from the generator
            assert torch.equal(plain.state_dict()[key], on.state_dict()[key]) and torch.equal(plain.state_dict()[key], off.state_dict()[key])
        core, core_off = (m if cls is FlashAttention3 else m.gpu_attention for m in (on, off))
        assert core.qk_norm and core.qk_norm_eps == 1e-5 and not core_off.qk_norm and not hasattr(core_off, "q_norm")
        for p in (core.q_norm.weight, core.k_norm.weight):
            assert isinstance(p, torch.nn.Parameter) and p.shape == (64,) and torch.equal(p, torch.ones(64))
        assert not plain.load_state_dict(on.state_dict(), strict=False).missing_keys
        assert sorted(on.load_state_dict(plain.state_dict(), strict=False).missing_keys) == sorted([pre + "k_norm.weight", pre + "q_norm.weight"])
    assert FlashAttention3(256, 4, dtype=torch.bfloat16, qk_norm=True).q_norm.weight.dtype == torch.bfloat16
    with pytest.raises(ValueError, match="qk_norm does not combine with attention dropout"):
        FlashAttention3(256, 4, dropout=0.1, qk_norm=True)
    with pytest.raises(ValueError, match="64 or 128"):
        FlashAttention3(64, 4, qk_norm=True)
    for kw, what in ((dict(qk_norm=True), "qk_norm"), (dict(qk_norm=True, rotary=True), "rotary")):
        m = FlashAttention3(256, 4, **kw)
        with pytest.raises(RuntimeError, match="MI355X only"):
            m(torch.zeros(1, 8, 256))
        m_cuda = type("Q", (), {"is_cuda": True, "requires_grad": False, "dtype": torch.float32})()
        with pytest.raises(NotImplementedError, match=f"need_weights together with {what}"):
            m._flash_attention_forward(m_cuda, m_cuda, m_cuda, None, True)
        with pytest.raises(ValueError, match='fp32_attention="bf16"'):
            m._flash_attention_forward(m_cuda, m_cuda, m_cuda, None, False)

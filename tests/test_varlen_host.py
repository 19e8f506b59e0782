"""CPU-side tests (no GPU) of the packed variable-length training path (``pfa_fa3_varlen_*``, ABI v9 additive):
every field rule through ``pfa_fa3_varlen_check`` / ``pfa_fa3_varlen_bwd_check`` and the order the rules are
reported in, the launch descriptions, and the plain-torch model (``ops.fa3_varlen_forward`` / ``fa3_varlen_backward`` /
``fa3_varlen_attention`` on CPU tensors: the executable specification) against ``dense_testlib.reference`` per sequence in fp64, its
exact cases and its clamping rule."""

from __future__ import annotations

import ctypes as C

import pytest
import torch

from capi_testlib import ALIGN, DTYPE, FLAGS, HEAD_DIM, NULL, SHAPE, SIZE, STRIDE, lib  # noqa: F401
from capi_testlib import varlen_args as _fwd, varlen_bwd_args as _bwd
from dense_testlib import BOUND_GRAD, BOUND_O, reference
from photonic_flash_attention_amd import _capi, ops

BF16, FP16, FP32 = 0, 1, 2
INF = float("inf")


def _fc(lib, a):
    return lib.pfa_fa3_varlen_check(C.byref(a))


def _bc(lib, a):
    return lib.pfa_fa3_varlen_bwd_check(C.byref(a))


def test_forward_field_rules_one_case_per_error_code(lib):
    assert _fc(lib, _fwd()) == 0
    assert _fc(lib, _fwd(dtype_in=FP16, dtype_out=FP32, D=64, lse=0, causal=0, o_stride_s=516, o_stride_h=132)) == 0     # fp32 out: strides of 4
    assert lib.pfa_fa3_varlen_check(None) == NULL
    bad = _fwd()
    bad.size -= 8
    assert _fc(lib, bad) == SIZE
    cases = [
        (dict(flags=1), FLAGS), (dict(flags=0x2C00), FLAGS), (dict(reserved0=1), FLAGS),
        (dict(q=0), NULL), (dict(k=0), NULL), (dict(v=0), NULL), (dict(o=0), NULL), (dict(cu_seqlens_q=0), NULL), (dict(cu_seqlens_k=0), NULL),
        (dict(B=0), SHAPE), (dict(H=0), SHAPE), (dict(Hkv=0), SHAPE), (dict(H=4, Hkv=3), SHAPE),
        (dict(total_q=0), SHAPE), (dict(total_k=0), SHAPE), (dict(max_seqlen_q=0), SHAPE), (dict(max_seqlen_k=0), SHAPE),
        (dict(max_seqlen_q=1001), SHAPE), (dict(max_seqlen_k=901), SHAPE),
        (dict(D=96), HEAD_DIM), (dict(D=256), HEAD_DIM),
        (dict(dtype_in=FP32, dtype_out=FP32), DTYPE), (dict(dtype_out=FP16), DTYPE), (dict(dtype_in=3), DTYPE),
        (dict(softmax_scale=0.0), SHAPE), (dict(softmax_scale=INF), SHAPE),
        (dict(q_stride_s=516), STRIDE), (dict(q_stride_h=132), STRIDE), (dict(k_stride_s=260), STRIDE), (dict(v_stride_h=4), STRIDE),
        (dict(o_stride_s=516), STRIDE),                                                # a 16-bit output leaves in 16-byte pieces
        (dict(dtype_out=FP32, o_stride_s=514), STRIDE), (dict(k_stride_s=-256), STRIDE),
        (dict(q=0x100008), ALIGN), (dict(k=0x200002), ALIGN), (dict(v=0x300004), ALIGN), (dict(o=0x400008), ALIGN),
        (dict(lse=0x500002), ALIGN), (dict(cu_seqlens_q=0x600001), ALIGN), (dict(cu_seqlens_k=0x700002), ALIGN),
        # one sequence's slab -- max_seqlen rows at the row stride -- past the 32-bit descriptor
        (dict(total_k=1 << 20, max_seqlen_k=1 << 20, k_stride_s=2048), SHAPE),
        (dict(total_q=1 << 20, max_seqlen_q=1 << 20, q_stride_s=2048), SHAPE),
        # more workgroups than a grid holds: ceil(2^22 / 256) * 2^10 * 2^8 = 2^32
        (dict(B=1 << 10, H=1 << 8, Hkv=1, total_q=1 << 22, max_seqlen_q=1 << 22, q_stride_s=128, q_stride_h=128), SHAPE),
    ]
    for over, want in cases:
        assert _fc(lib, _fwd(**over)) == want, over
    # the launch and the description refuse what the check refuses, before they touch a device
    assert lib.pfa_fa3_varlen_fwd(C.byref(_fwd(D=96)), None) == HEAD_DIM and lib.pfa_fa3_varlen_fwd(None, None) == NULL
    assert lib.pfa_fa3_varlen_describe(C.byref(_fwd(max_seqlen_q=0)), None, 0) == SHAPE


def test_backward_field_rules_one_case_per_error_code(lib):
    assert _bc(lib, _bwd()) == 0
    assert _bc(lib, _bwd(dtype=FP16, dtype_grad=FP32, D=64, causal=0, dq_stride_s=516, dk_stride_h=132, dv_stride_s=260)) == 0
    assert lib.pfa_fa3_varlen_bwd_check(None) == NULL
    bad = _bwd()
    bad.size = C.sizeof(_capi.PfaFa3VarlenArgs)
    assert _bc(lib, bad) == SIZE
    cases = [
        (dict(flags=4), FLAGS), (dict(reserved0=-1), FLAGS),
        (dict(dout=0), NULL), (dict(lse=0), NULL), (dict(dq=0), NULL), (dict(dk=0), NULL), (dict(dv=0), NULL), (dict(delta=0), NULL),
        (dict(q=0), NULL), (dict(cu_seqlens_q=0), NULL), (dict(cu_seqlens_k=0), NULL),
        (dict(B=-1), SHAPE), (dict(H=6, Hkv=4), SHAPE), (dict(total_q=0), SHAPE), (dict(max_seqlen_k=0), SHAPE),
        (dict(max_seqlen_q=1001), SHAPE), (dict(max_seqlen_k=901), SHAPE),
        (dict(D=32), HEAD_DIM),
        (dict(dtype=FP32, dtype_grad=FP32), DTYPE), (dict(dtype=BF16, dtype_grad=FP16), DTYPE),
        (dict(softmax_scale=-1.0), SHAPE),
        (dict(do_stride_s=516), STRIDE), (dict(o_stride_h=132), STRIDE), (dict(dq_stride_s=516), STRIDE), (dict(dv_stride_h=132), STRIDE),
        (dict(dtype_grad=FP32, dk_stride_s=258), STRIDE),
        (dict(dout=0x800008), ALIGN), (dict(dq=0x900004), ALIGN), (dict(dk=0xA00008), ALIGN), (dict(dv=0xB00002), ALIGN),
        (dict(delta=0xC00002), ALIGN), (dict(lse=0x500001), ALIGN),
        (dict(total_q=1 << 20, max_seqlen_q=1 << 20, do_stride_s=2048), SHAPE),
        (dict(B=1 << 12, H=1 << 7, Hkv=1 << 7, total_k=1 << 19, max_seqlen_k=1 << 19, k_stride_s=128, v_stride_s=128), SHAPE),   # dK/dV grid 2^31
    ]
    for over, want in cases:
        assert _bc(lib, _bwd(**over)) == want, over
    assert lib.pfa_fa3_varlen_bwd(C.byref(_bwd(D=32)), None) == HEAD_DIM and lib.pfa_fa3_varlen_bwd(None, None) == NULL
    assert lib.pfa_fa3_varlen_bwd_workspace_bytes(C.byref(_bwd())) == 4 * 1000 * 4
    assert lib.pfa_fa3_varlen_bwd_workspace_bytes(None) == 0


def test_rules_are_reported_in_the_documented_order(lib):
    """STRUCT_SIZE, FLAGS, NULL, SHAPE, HEAD_DIM, DTYPE, STRIDE, ALIGN, then slab and grid limits: of two violated rules the earlier wins."""
    for make, check, dt in ((_fwd, _fc, "dtype_in"), (_bwd, _bc, "dtype")):
        ladder = [("size", dict(), SIZE), ("flags", dict(flags=2), FLAGS), ("null", dict(cu_seqlens_k=0), NULL),
                  ("shape", dict(max_seqlen_q=2000), SHAPE), ("head_dim", dict(D=12), HEAD_DIM), ("dtype", {dt: 5}, DTYPE),
                  ("stride", dict(q_stride_h=2), STRIDE), ("align", dict(v=0x300008), ALIGN)]
        for i, (first, over_i, want) in enumerate(ladder):
            for later, over_j, _ in ladder[i + 1:]:
                a = make(**dict(over_j, **over_i))
                if first == "size":
                    a.size += 8
                assert check(lib, a) == want, (first, later)
        big = dict(total_k=1 << 20, max_seqlen_k=1 << 20, k_stride_s=2048)
        assert check(lib, make(**big)) == SHAPE and check(lib, make(k=0x200008, **big)) == ALIGN


def test_describe_names_and_workgroups(lib):
    """B 3, H 4, Hkv 2, max_seqlen_q 300, max_seqlen_k 257: 3 * 4 * 2 forward / dQ workgroups, 3 * 2 * 3 dK/dV workgroups."""
    assert _capi.describe_varlen(_fwd()) == ("fa3_fwd_varlen_bf16_d128_causal_o16", 3 * 4 * 2)
    assert _capi.describe_varlen(_fwd(dtype_in=FP16, dtype_out=FP32, D=64, causal=0)) == ("fa3_fwd_varlen_fp16_d64_full_splitp_o32", 24)
    assert _capi.describe_varlen(_fwd(max_seqlen_q=256))[1] == 12 and _capi.describe_varlen(_fwd(max_seqlen_q=257))[1] == 24
    assert _capi.describe_varlen_bwd(_bwd()) == ("fa3_bwd_dq_varlen_bf16_d128_causal_g16+fa3_bwd_dkdv_varlen_bf16_d128_causal_g16", 24, 3 * 2 * 3)
    name, nq, nk = _capi.describe_varlen_bwd(_bwd(dtype=FP16, dtype_grad=FP32, D=64, causal=0, max_seqlen_k=128, max_seqlen_q=1))
    assert (name, nq, nk) == ("fa3_bwd_dq_varlen_fp16_d64_full_g32+fa3_bwd_dkdv_varlen_fp16_d64_full_g32", 12, 6)
    with pytest.raises(_capi.PfaError):
        _capi.describe_varlen(_fwd(D=100))
    assert lib.pfa_fa3_varlen_bwd_describe(C.byref(_bwd()), None, 0, None) == 24          # buffer and count are optional


# --- the plain-torch model ----------------------------------------------------------------------------------------------------------

LQ, LK = [1, 31, 0, 64, 257], [1, 33, 5, 0, 129]
H, HKV, D = 4, 2, 64


def _cu(lens):
    out = [0]
    for n in lens:
        out.append(out[-1] + n)
    return torch.tensor(out, dtype=torch.int32)


def _packed(seed, total, heads, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(total, heads, D, generator=g).to(dtype)


@pytest.fixture(scope="module")
def problem():
    """fp32 packed operands (the model computes in fp32 whatever it is handed; fp32 inputs keep the rounding of 16-bit I/O out of the
    comparison), with the fp64 reference of every sequence computed once."""
    q, k, v, dout = _packed(1, sum(LQ), H), _packed(2, sum(LK), HKV), _packed(3, sum(LK), HKV), _packed(4, sum(LQ), H)
    return q, k, v, dout, _cu(LQ), _cu(LK)


def _model(q, k, v, cu_q, cu_k, causal, max_q=None, max_k=None):
    """The three ops on CPU tensors.  They take bf16 / fp16 operands: fp32 problems go through the model functions they run."""
    mq, mk = max_q or max(LQ), max_k or max(LK)
    scale = D ** -0.5
    out = torch.full(q.shape, 7.0)
    lse = torch.full((q.shape[1], q.shape[0]), 7.0)
    ops._varlen_forward_model(q, k, v, out, lse, cu_q.tolist(), cu_k.tolist(), mq, mk, causal, scale)
    return out, lse, mq, mk, scale


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
def test_model_matches_the_fp64_reference_per_sequence(problem, causal):
    q, k, v, dout, cu_q, cu_k = problem
    out, lse, mq, mk, scale = _model(q, k, v, cu_q, cu_k, causal)
    dq, dk, dv = torch.full(q.shape, 7.0), torch.full(k.shape, 7.0), torch.full(v.shape, 7.0)
    ops._varlen_backward_model(q, k, v, out, dout, lse, dq, dk, dv, cu_q.tolist(), cu_k.tolist(), mq, mk, causal, scale)
    for b, (nq, nk) in enumerate(zip(LQ, LK)):
        sq, sk = int(cu_q[b]), int(cu_k[b])
        o_b, lse_b, dq_b = out[sq:sq + nq], lse[:, sq:sq + nq], dq[sq:sq + nq]
        dk_b, dv_b = dk[sk:sk + nk], dv[sk:sk + nk]
        if nq == 0:                                   # keys no row sees: exact zeros
            assert bool((dk_b == 0).all()) and bool((dv_b == 0).all()), b
            continue
        if nk == 0:                                   # rows with no key: o = 0, lse = -inf, dq = 0, exactly
            assert bool((o_b == 0).all()) and bool((lse_b == -INF).all()) and bool((dq_b == 0).all()), b
            continue
        t = lambda x: x.transpose(0, 1)[None]         # [S, heads, D] -> [1, heads, S, D]
        ro, rl, rdq, rdk, rdv = reference(t(q[sq:sq + nq]), t(k[sk:sk + nk]), t(v[sk:sk + nk]), causal=causal, dout=t(dout[sq:sq + nq]))
        eo, el = float((t(o_b).double() - ro).abs().max()), float((lse_b[None].double() - rl).abs().max())
        print(f"seq {b} ({nq} x {nk}): o {eo:.2e} lse {el:.2e}")
        assert eo <= BOUND_O and el <= BOUND_O, (b, eo, el)
        for name, got, r in (("dq", dq_b, rdq), ("dk", dk_b, rdk), ("dv", dv_b, rdv)):
            err, bound = float((t(got).double() - r).abs().max()), BOUND_GRAD * max(1.0, float(r.abs().max()))
            print(f"seq {b} {name} {err:.2e} (bound {bound:.2e})")
            assert err <= bound, (b, name, err, bound)
        if causal and nk > nq:                        # under causal the keys j >= Sq_b are seen by no row
            assert bool((dk_b[nq:] == 0).all()) and bool((dv_b[nq:] == 0).all()), b
    for name, t_ in (("out", out), ("dq", dq), ("dk", dk), ("dv", dv)):      # cu[B] == total: every row is covered, nothing keeps the fill
        assert bool(torch.isfinite(t_).all()) and not bool((t_ == 7.0).any()), name


def test_public_ops_run_the_model_on_cpu_tensors_and_autograd_goes_through_it(problem):
    q, k, v, dout, cu_q, cu_k = (t.to(torch.bfloat16) if t.is_floating_point() else t for t in problem)
    kw = dict(cu_seqlens_q=cu_q, cu_seqlens_k=cu_k, max_seqlen_q=max(LQ), max_seqlen_k=max(LK), causal=True)
    out, lse = ops.fa3_varlen_forward(q, k, v, return_lse=True, **kw)
    assert out.shape == q.shape and out.dtype == torch.bfloat16 and lse.shape == (H, sum(LQ)) and lse.dtype == torch.float32
    want, want_lse, *_ = _model(q, k, v, cu_q, cu_k, True)
    assert torch.equal(out.float(), want.to(torch.bfloat16).float()) and torch.equal(lse, want_lse)
    o32, none = ops.fa3_varlen_forward(q, k, v, out_dtype=torch.float32, **kw)
    assert none is None and torch.equal(o32, want)
    grads = ops.fa3_varlen_backward(q, k, v, out, dout, lse, grad_dtype=torch.float32, **kw)
    qr, kr, vr = (t.clone().requires_grad_(True) for t in (q, k, v))
    res = ops.fa3_varlen_attention(qr, kr, vr, cu_q, cu_k, max(LQ), max(LK), 0.0, None, True)
    res.backward(dout)
    for g32, g in zip(grads, (qr.grad, kr.grad, vr.grad)):
        assert torch.equal(g32.to(torch.bfloat16), g)
    with pytest.raises(NotImplementedError):
        ops.fa3_varlen_attention(q, k, v, cu_q, cu_k, max(LQ), max(LK), 0.1)
    with pytest.raises(ValueError):
        ops.fa3_varlen_forward(q, k, v, **dict(kw, max_seqlen_q=sum(LQ) + 1))
    with pytest.raises(ValueError):
        ops.fa3_varlen_forward(q, k, v, **dict(kw, cu_seqlens_k=cu_k[:-1]))
    with pytest.raises(ValueError):
        ops.fa3_varlen_forward(q, k, v, **dict(kw, cu_seqlens_q=cu_q.long()))


@pytest.mark.parametrize("bad", ["decreasing", "past_total", "negative", "capped"])
def test_clamping_rule_touches_nothing_outside_and_leaves_uncovered_rows_unchanged(problem, bad):
    """s = clamp(cu[b], 0, total), e = clamp(cu[b + 1], s, total), S_b = min(e - s, max_seqlen): with bad device values the model reads
    and writes inside the tensors only, and rows no clamped sequence covers keep their bits."""
    q, k, v, dout, _, _ = problem
    tq, tk = q.shape[0], k.shape[0]
    mq, mk = 64, 40
    cu_q, cu_k = {"decreasing": ([0, 100, 40, 90, 200], [0, 50, 20, 20, 60]),
                  "past_total": ([0, 10, 300, tq + 50, tq + 90], [0, 30, 60, 90, tk + 1000]),
                  "negative": ([-5, 20, -3, 60, 100], [-100, -1, 10, 5, 70]),
                  "capped": ([0, 200, 210, 300, tq], [0, 100, 100, 160, tk])}[bad]
    seqs = ops._packed_seqs(cu_q, cu_k, tq, tk, mq, mk)
    cov_q, cov_k = torch.zeros(tq, dtype=torch.bool), torch.zeros(tk, dtype=torch.bool)
    for sq, nq, sk, nk in seqs:
        assert 0 <= sq <= sq + nq <= tq and 0 <= sk <= sk + nk <= tk and nq <= mq and nk <= mk
        cov_q[sq:sq + nq] = True
        cov_k[sk:sk + nk] = True
    assert not bool(cov_q.all()) and not bool(cov_k.all())                  # every case leaves rows uncovered
    fill = float.fromhex("0x1.23456p+3")
    out, lse = torch.full(q.shape, fill), torch.full((H, tq), fill)
    ops._varlen_forward_model(q, k, v, out, lse, cu_q, cu_k, mq, mk, True, D ** -0.5)
    dq, dk, dv = torch.full(q.shape, fill), torch.full(k.shape, fill), torch.full(v.shape, fill)
    ops._varlen_backward_model(q, k, v, out, dout, lse, dq, dk, dv, cu_q, cu_k, mq, mk, True, D ** -0.5)
    for name, t_, cov in (("out", out, cov_q), ("dq", dq, cov_q), ("dk", dk, cov_k), ("dv", dv, cov_k)):
        assert bool((t_[~cov] == fill).all()), f"{name}: an uncovered row was written"
        assert not bool((t_[cov] == fill).any()), f"{name}: a covered row was not written"
    assert bool((lse[:, ~cov_q] == fill).all()) and not bool((lse[:, cov_q] == fill).any())
    # the same through the public ops: torch.tensor cu on the CPU
    o2, l2 = ops.fa3_varlen_forward(q.bfloat16(), k.bfloat16(), v.bfloat16(), cu_seqlens_q=torch.tensor(cu_q, dtype=torch.int32),
                                    cu_seqlens_k=torch.tensor(cu_k, dtype=torch.int32), max_seqlen_q=mq, max_seqlen_k=mk, causal=True,
                                    return_lse=True, out=torch.full(q.shape, fill, dtype=torch.bfloat16))
    assert bool((o2[~cov_q].float() == torch.tensor(fill).bfloat16().float()).all())

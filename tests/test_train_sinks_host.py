"""CPU-side tests (no GPU) of attention sinks for training (``pfa_fa3_fwd_sink*``, ``pfa_fa3_varlen_fwd_sink*``, ``pfa_fa3_sink_grad*``,
ABI v9 additive, declared in ``include/pfa_hip_train_sinks.h`` and bound by ``_capi_sinks``; ``sinks=`` on the dense and packed ``ops`` calls; ``attention_sinks=`` on the modules): the status rules of the new
``_check`` exports in their documented order, a NULL block agreeing with the sibling, the describe names and the sink-grad workspace,
``ops``' refusals before anything is enqueued, the modules' state dicts -- and the plain-torch model of ``fa3_sink_grad`` (the
executable specification of the kernel) against fp64 autograd of an explicit softmax with one more key, with two mutants that must be
caught.  The header is held against its binding by tests/test_capi_conformance.py."""

from __future__ import annotations

import ctypes as C

import pytest
import torch

from capi_testlib import ALIGN, DTYPE, FLAGS, NULL, OK, SHAPE, SIZE, STRIDE, built_lib, fa3_args, name_of, sinks, varlen_args
from photonic_flash_attention_amd import _capi, _capi_sinks, _models, ops
from photonic_flash_attention_amd.core.flash_attention_3 import FlashAttention3
from photonic_flash_attention_amd.integration.pytorch.modules import PhotonicFlashAttention, PhotonicMultiHeadAttention

INF = float("inf")

# the sink block's own rules, each reported in front of the ones behind it
WRONG_BLOCK = [(dict(size=8, flags=1, sinks=0), SIZE), (dict(flags=1, sinks=0), FLAGS), (dict(sinks=0), NULL), (dict(sinks=0xA002), ALIGN)]
# argument blocks good and bad: the sibling's verdict must come through
BAD_DENSE = [dict(), dict(q=0), dict(B=0), dict(D=96), dict(dtype_out=1), dict(k_stride_s=257), dict(o=0x4008), dict(flags=1 << 20),
             dict(flags=42 << 8), dict(softmax_scale=0.0), dict(key_mask=0x9000, mask=0xA000), dict(kv_group=3), dict(size=8),
             dict(flags=_capi.PFA_FLAG_SPLIT_P), dict(dtype_out=2), dict(flags=44 << 8)]
BAD_PACKED = [dict(), dict(q=0), dict(B=0), dict(D=96), dict(dtype_out=1), dict(dtype_in=2), dict(k_stride_s=257), dict(o=0x400008), dict(flags=1),
              dict(reserved0=1), dict(cu_seqlens_q=0), dict(max_seqlen_q=2000), dict(H=3), dict(size=8), dict(dtype_out=2), dict(causal=0)]


def sink_grad_args(**over):
    """A valid dense ``pfa_fa3_sink_grad_args``: B 2, H 4, Sq 5000 (three chunks of 2048 rows)."""
    base = dict(lse=0x100000, delta=0x200000, sinks=0xA000, d_sinks=0xB000, workspace=0x300000, workspace_bytes=4 * 2 * 4 * 3, B=2, H=4, Sq=5000,
                lse_stride_b=20000, lse_stride_h=5000, delta_stride_b=20000, delta_stride_h=5000)
    base.update(over)
    return _capi_sinks.make_sink_grad_args(**base)


@pytest.fixture(scope="module")
def lib():
    built_lib()
    return _capi_sinks.load()


def test_a_null_block_is_the_sibling_call(lib):
    for over in BAD_DENSE + [dict(flags=43 << 8), dict(flags=45 << 8), dict(dtype_in=2, dtype_out=2)]:
        a = fa3_args(**over)
        assert lib.pfa_fa3_fwd_sink_check(C.byref(a), None) == lib.pfa_fa3_check(C.byref(a)), over
        assert name_of(lib.pfa_fa3_fwd_sink_describe, a, None) == name_of(lib.pfa_fa3_describe, a), over
    for over in BAD_PACKED:
        a = varlen_args(**over)
        assert lib.pfa_fa3_varlen_fwd_sink_check(C.byref(a), None) == lib.pfa_fa3_varlen_check(C.byref(a)), over
        assert name_of(lib.pfa_fa3_varlen_fwd_sink_describe, a, None) == name_of(lib.pfa_fa3_varlen_describe, a), over
    assert lib.pfa_fa3_fwd_sink_check(None, None) == NULL and lib.pfa_fa3_varlen_fwd_sink_check(None, None) == NULL


def test_block_rules_first_then_the_siblings_then_what_the_sink_refuses(lib):
    for make, chk, schk, sdesc, bad in ((fa3_args, lib.pfa_fa3_check, lib.pfa_fa3_fwd_sink_check, lib.pfa_fa3_fwd_sink_describe, BAD_DENSE),
                                        (varlen_args, lib.pfa_fa3_varlen_check, lib.pfa_fa3_varlen_fwd_sink_check,
                                         lib.pfa_fa3_varlen_fwd_sink_describe, BAD_PACKED)):
        for a in (make(), make(B=0), make(q=0), make(size=8)):
            for kw, want in WRONG_BLOCK:
                s = sinks(**kw)
                assert schk(C.byref(a), C.byref(s)) == want, kw
                assert name_of(sdesc, a, C.byref(s))[0] == want, kw
        good = sinks()
        n_ok = 0
        for over in bad:                      # behind a good block the sibling's errors come through, in the sibling's order
            a = make(**over)
            assert schk(C.byref(a), C.byref(good)) == chk(C.byref(a)), over
            n_ok += chk(C.byref(a)) == OK
        assert n_ok >= 3
        assert schk(None, C.byref(good)) == NULL
    good = sinks()
    # what the sink itself refuses, behind a block the plain call accepts: fp32 operands (with and without a drop_mask), a drop_mask
    # on 16-bit operands (the plain call's own rule), and the selectors of the kernels that carry no sink
    f32 = dict(dtype_in=2, dtype_out=2)
    assert lib.pfa_fa3_check(C.byref(fa3_args(**f32))) == OK and lib.pfa_fa3_fwd_sink_check(C.byref(fa3_args(**f32)), C.byref(good)) == DTYPE
    drop = dict(drop_mask=0x9000, drop_scale=2.0)
    assert lib.pfa_fa3_check(C.byref(fa3_args(**f32, **drop))) == OK
    assert lib.pfa_fa3_fwd_sink_check(C.byref(fa3_args(**f32, **drop)), C.byref(good)) == DTYPE
    assert lib.pfa_fa3_fwd_sink_check(C.byref(fa3_args(**drop)), C.byref(good)) == FLAGS
    big = dict(B=1, H=8, Sq=2048, Sk=2048, D=128, q_stride_b=2048 * 1024, k_stride_b=2048 * 1024, v_stride_b=2048 * 1024, o_stride_b=2048 * 1024,
               q_stride_s=1024, k_stride_s=1024, v_stride_s=1024, o_stride_s=1024, q_stride_h=128, k_stride_h=128, v_stride_h=128, o_stride_h=128)
    for shape in (dict(), big):
        for var, want in ((0, OK), (44, OK), (43, FLAGS), (45, FLAGS)):
            a = fa3_args(flags=var << 8, **shape)
            assert lib.pfa_fa3_check(C.byref(a)) == OK
            assert lib.pfa_fa3_fwd_sink_check(C.byref(a), C.byref(good)) == want, (var, shape)
    # ... and the block's rules still come in front of them
    assert lib.pfa_fa3_fwd_sink_check(C.byref(fa3_args(flags=43 << 8)), C.byref(sinks(sinks=0))) == NULL


def test_describe_names_are_the_8_wave_kernels_with_a_sink_fragment(lib):
    s = sinks()
    big = dict(B=1, H=8, Sq=2048, Sk=2048, D=128, q_stride_b=2048 * 1024, k_stride_b=2048 * 1024, v_stride_b=2048 * 1024, o_stride_b=2048 * 1024,
               q_stride_s=1024, k_stride_s=1024, v_stride_s=1024, o_stride_s=1024, q_stride_h=128, k_stride_h=128, v_stride_h=128, o_stride_h=128)
    for over, text in ((dict(), "fa3_fwd_bf16_d64_full_o16_sink_v8269"),
                       (dict(causal=1, dtype_in=1, dtype_out=2, flags=_capi.PFA_FLAG_SPLIT_P), "fa3_fwd_fp16_d64_causal_splitp_o32_sink_v8269"),
                       (dict(key_mask=0x9000, key_mask_stride_b=64), "fa3_fwd_bf16_d64_full_kmask_o16_sink_v8269"),
                       (dict(causal=1, **big), "fa3_fwd_bf16_d128_causal_o16_sink_v8269")):      # (the plain call takes the assembly kernel here)
        a = fa3_args(**over)
        got = name_of(lib.pfa_fa3_fwd_sink_describe, a, C.byref(s))
        forced = name_of(lib.pfa_fa3_describe, fa3_args(**{**over, "flags": over.get("flags", 0) | (44 << 8)}))
        assert got[1] == text and got[1].replace("_sink", "") == forced[1] and got[0] == forced[0] > 0, (got, forced)
    assert name_of(lib.pfa_fa3_describe, fa3_args(causal=1, **big))[1].startswith(("fa3_fwd_p4_", "fa3_fwd_w4_"))
    for over, text in ((dict(), "fa3_fwd_varlen_bf16_d128_causal_o16_sink"), (dict(causal=0, dtype_out=2), "fa3_fwd_varlen_bf16_d128_full_splitp_o32_sink")):
        a = varlen_args(**over)
        got, plain = name_of(lib.pfa_fa3_varlen_fwd_sink_describe, a, C.byref(s)), name_of(lib.pfa_fa3_varlen_describe, a)
        assert got[1] == text and got[1] == plain[1] + "_sink" and got[0] == plain[0] > 0


def test_sink_grad_rules_workspace_and_describe(lib):
    chk = lib.pfa_fa3_sink_grad_check
    assert chk(None) == NULL
    table = [(dict(), OK), (dict(size=8, flags=1), SIZE), (dict(flags=1, lse=0), FLAGS), (dict(reserved0=1, lse=0), FLAGS),
             (dict(lse=0, B=0), NULL), (dict(delta=0), NULL), (dict(sinks=0), NULL), (dict(d_sinks=0), NULL), (dict(workspace=0), NULL),
             (dict(B=0, lse_stride_h=1), SHAPE), (dict(H=0), SHAPE), (dict(Sq=0), SHAPE),
             (dict(lse_stride_h=4999, lse=0x100002), STRIDE), (dict(delta_stride_b=-8), STRIDE), (dict(delta_stride_b=100), STRIDE),
             (dict(B=1, delta_stride_b=0), OK), (dict(H=1, lse_stride_h=0, workspace_bytes=24), OK),
             (dict(lse=0x100002), ALIGN), (dict(delta=0x200001), ALIGN), (dict(sinks=0xA002), ALIGN), (dict(d_sinks=0xB002), ALIGN),
             (dict(workspace=0x300002), ALIGN),
             (dict(Sq=2 ** 31 - 2048, workspace_bytes=1 << 40, lse_stride_h=2 ** 31, delta_stride_h=2 ** 31, lse_stride_b=2 ** 33, delta_stride_b=2 ** 33),
              SHAPE),                                                              # the row index past 32 bits
             (dict(B=2 ** 20, H=2 ** 11, Sq=1, lse_stride_h=1, delta_stride_h=1, lse_stride_b=2 ** 11, delta_stride_b=2 ** 11,
                   workspace_bytes=1 << 40), SHAPE),                                # the grid past 32 bits
             (dict(workspace_bytes=95), NULL), (dict(workspace_bytes=96), OK),
             # packed: [H, total_q], Sq = max_seqlen_q; the strides are not looked at
             (dict(cu_seqlens_q=0x9000, total_q=9000, lse_stride_h=-1), OK), (dict(cu_seqlens_q=0x9000, total_q=0), SHAPE),
             (dict(cu_seqlens_q=0x9000, total_q=4999), SHAPE), (dict(cu_seqlens_q=0x9002, total_q=9000), ALIGN)]
    for over, want in table:
        assert chk(C.byref(sink_grad_args(**over))) == want, over
    ws = lib.pfa_fa3_sink_grad_workspace_bytes
    assert ws(None) == 0 and ws(C.byref(sink_grad_args(size=8))) == 0 and ws(C.byref(sink_grad_args(B=0))) == 0
    # H * B * ceil(Sq / 2048) fp32 partial sums, from the shapes alone (no pointer but cu_seqlens_q's presence is looked at)
    for B, H, Sq in ((2, 4, 5000), (1, 16, 16384), (3, 5, 1), (3, 5, 2048), (3, 5, 2049)):
        a = sink_grad_args(B=B, H=H, Sq=Sq, lse=0, delta=0, workspace=0, workspace_bytes=0)
        assert ws(C.byref(a)) == 4 * B * H * ((Sq + 2047) // 2048)
    assert ws(C.byref(sink_grad_args(cu_seqlens_q=0x9000, total_q=4999))) == 0
    assert name_of(lib.pfa_fa3_sink_grad_describe, sink_grad_args()) == (24, "sink_grad_dense_c2048+final", -1)
    assert name_of(lib.pfa_fa3_sink_grad_describe, sink_grad_args(cu_seqlens_q=0x9000, total_q=9000)) == (24, "sink_grad_packed_c2048+final", -1)
    assert name_of(lib.pfa_fa3_sink_grad_describe, sink_grad_args(workspace=0))[0] == NULL
    assert _capi_sinks.describe_sink_grad(sink_grad_args()) == ("sink_grad_dense_c2048+final", 24)


def test_ops_refuse_bad_sinks_on_cpu_tensors_before_anything_is_enqueued():
    q = torch.zeros(2, 8, 5, 64, dtype=torch.bfloat16)
    k = torch.zeros(2, 2, 7, 64, dtype=torch.bfloat16)
    qv, kv = torch.zeros(6, 8, 64, dtype=torch.bfloat16), torch.zeros(6, 2, 64, dtype=torch.bfloat16)
    cu = torch.tensor([0, 3, 6], dtype=torch.int32)
    pk = dict(cu_seqlens_q=cu, cu_seqlens_k=cu, max_seqlen_q=3, max_seqlen_k=3)
    lse = torch.zeros(2, 8, 5)
    calls = [lambda **kw: ops.fa3_forward(q, k, k, **kw), lambda **kw: ops.fa3_attention(q, k, k, **kw),
             lambda **kw: ops.fa3_backward(q, k, k, q, q, lse, **kw),
             lambda **kw: ops.fa3_varlen_forward(qv, kv, kv, **pk, **kw), lambda **kw: ops.fa3_varlen_attention(qv, kv, kv, cu, cu, 3, 3, **kw),
             lambda **kw: ops.fa3_varlen_backward(qv, kv, kv, qv, qv, torch.zeros(8, 6), **pk, **kw)]
    for call in calls:
        for bad, text in ((torch.zeros(8, dtype=torch.bfloat16), "sinks must be an fp32"), (torch.zeros(8, dtype=torch.float64), "sinks must be an fp32"),
                          ([0.0] * 8, "sinks must be an fp32"), (torch.zeros(4), r"sinks must be \[H\] = \[8\]"),
                          (torch.zeros(1, 8), r"sinks must be \[H\]"), (torch.zeros(16)[::2], "sinks must be contiguous"),
                          (torch.zeros(8, device="meta"), "sinks must live on the operands' device")):
            with pytest.raises(ValueError, match=text):
                call(sinks=bad)
    good = torch.zeros(8)
    with pytest.raises(ValueError, match="sinks need bf16 / fp16 operands"):
        ops.fa3_forward(q.float(), k.float(), k.float(), sinks=good)
    with pytest.raises(ValueError, match="sinks do not combine with attention dropout"):
        ops.fa3_forward(q, k, k, sinks=good, drop_mask=torch.ones(2, 8, 5, 7, dtype=torch.bool))
    with pytest.raises(ValueError, match="sinks do not combine with return_weights"):
        ops.fa3_forward(q, k, k, sinks=good, return_weights=True)
    with pytest.raises(ValueError, match="sinks do not combine with return_weights"):
        ops.fa3_attention(q, k, k, sinks=good, return_weights=True)
    with pytest.raises(ValueError, match="sinks need bf16 / fp16 operands and do not combine with attention dropout"):
        ops.fa3_backward(q.float(), k.float(), k.float(), q.float(), q.float(), lse, sinks=good)
    with pytest.raises(ValueError, match="sinks need device tensors"):
        ops.fa3_varlen_forward(qv, kv, kv, sinks=good, **pk)
    with pytest.raises(ValueError, match="needs device tensors"):          # a good block reaches the sink-less call's own refusal
        ops.fa3_forward(q, k, k, sinks=good)
    for bad in (dict(lse=lse.double()), dict(delta=torch.zeros(2, 8, 4)), dict(sinks=torch.zeros(4)), dict(sinks=torch.zeros(8).double()),
                dict(lse=lse.transpose(1, 2)), dict(cu_seqlens_q=cu), dict(sinks=torch.zeros(8, device="meta"))):
        with pytest.raises(ValueError):
            ops.fa3_sink_grad(**{**dict(lse=lse, delta=lse, sinks=good), **bad})
    with pytest.raises(ValueError, match="max_seqlen_q"):
        ops.fa3_sink_grad(torch.zeros(8, 6), torch.zeros(8, 6), good, cu_seqlens_q=cu, max_seqlen_q=7)


def test_modules_hold_the_sinks_only_when_asked():
    for cls in (FlashAttention3, PhotonicFlashAttention, PhotonicMultiHeadAttention):
        torch.manual_seed(5)
        plain = cls(64, 4)
        torch.manual_seed(5)
        off = cls(64, 4, attention_sinks=False)
        torch.manual_seed(5)
        on = cls(64, 4, attention_sinks=True)
        pre = "" if cls is FlashAttention3 else "gpu_attention."
        keys = [pre + n for n in ("qkv_proj.weight", "qkv_proj.bias", "out_proj.weight", "out_proj.bias")]
        assert list(plain.state_dict()) == keys == list(off.state_dict())
        assert sorted(on.state_dict()) == sorted(keys + [pre + "sinks"])
        core = on if cls is FlashAttention3 else on.gpu_attention
        assert isinstance(core.sinks, torch.nn.Parameter) and core.sinks.dtype == torch.float32 and core.sinks.shape == (4,)
        assert bool((core.sinks == 0).all()) and core.sinks.requires_grad
        assert (off if cls is FlashAttention3 else off.gpu_attention).sinks is None
        for k in keys:                                                   # the option draws nothing from the generator
            assert torch.equal(plain.state_dict()[k], on.state_dict()[k]) and torch.equal(plain.state_dict()[k], off.state_dict()[k])
        off.load_state_dict(plain.state_dict())                          # a checkpoint without sinks loads as before
        with pytest.raises(RuntimeError, match="sinks"):
            on.load_state_dict(plain.state_dict())
    with pytest.raises(ValueError, match="attention_sinks does not combine with attention dropout"):
        FlashAttention3(64, 4, dropout=0.1, attention_sinks=True)


# --- the plain-torch model of fa3_sink_grad against fp64 autograd of the softmax with one more key ---------------------------------------

def _problem(seed, B=2, H=3, Sq=5, Sk=6):
    """Tiny fp64 scores with a row that sees no key in every head, sinks with one -inf head -> (lse, delta, d_sinks) by autograd, all
    fp64: lse [B,H,Sq] (-inf where a row has neither key nor sink), delta = rowsum(dO o O)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, H, Sq, Sk, generator=g, dtype=torch.float64)
    vis = torch.rand(B, H, Sq, Sk, generator=g) > 0.3
    vis[0, :, 1] = False                                                 # no visible key: LSE = the sink, -inf under the -inf sink
    vis[1, :, 4] = False
    v = torch.randn(B, H, Sk, 4, generator=g, dtype=torch.float64)
    dout = torch.randn(B, H, Sq, 4, generator=g, dtype=torch.float64)
    sinks = torch.randn(H, generator=g, dtype=torch.float64)
    sinks[1] = -INF
    s = sinks.clone().requires_grad_(True)
    full = torch.cat([x.masked_fill(~vis, -INF), s.view(1, H, 1, 1).expand(B, H, Sq, 1)], dim=-1)
    dead = torch.isneginf(full).all(-1)
    safe = torch.where(dead[..., None], torch.zeros_like(full), full)    # (a softmax over nothing has no gradient to ask for)
    p = torch.where(dead[..., None], torch.zeros_like(full), torch.softmax(safe, dim=-1))
    o = p[..., :-1] @ v
    (ds,) = torch.autograd.grad(o, s, dout)
    lse = torch.where(dead, torch.full_like(dead, -INF, dtype=torch.float64), torch.logsumexp(safe, dim=-1)).detach()
    return lse, (dout * o.detach()).sum(-1), sinks, ds


def _run(model, lse, delta, sinks, rows=None):
    out = torch.empty(sinks.shape[0], dtype=torch.float32)
    model(lse.float().contiguous(), delta.float().contiguous(), sinks.float(), out, rows)
    return out


def _forgets_the_minus_sign(lse, delta, sinks, d_sinks, rows=None):
    _models._sink_grad_model(lse, delta, sinks, d_sinks, rows)
    d_sinks.neg_()


def _multiplies_skipped_rows_by_zero(lse, delta, sinks, d_sinks, rows=None):
    assert rows is None
    H = sinks.shape[0]
    l, d = lse.transpose(0, 1).reshape(H, -1), delta.transpose(0, 1).reshape(H, -1)
    w = torch.where(l > -INF, torch.exp(sinks[:, None] - torch.where(l > -INF, l, torch.zeros_like(l))), torch.zeros_like(l))
    d_sinks.copy_(-(w * d).sum(1))                                       # a weight of exactly 0 on the skipped rows, times their delta


def _check(got, want):
    assert bool(torch.isfinite(got).all()), got
    assert float((got.double() - want).abs().max()) <= 1e-5 * max(1.0, float(want.abs().max())), (got, want)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_cpu_model_of_the_sink_gradient_against_fp64_autograd(seed):
    lse, delta, sinks, want = _problem(seed)
    assert bool(torch.isneginf(lse[:, 1]).any()) and bool(torch.isfinite(lse[:, 0]).all()) and float(want[1]) == 0.0 and float(want.abs().min()) == 0.0
    assert float(want[[0, 2]].abs().min()) > 1e-3                        # the gradient is there to be got wrong
    poisoned = delta.clone()
    poisoned[torch.isneginf(lse)] = float("nan")                         # delta of a skipped row may hold anything
    _check(_run(_models._sink_grad_model, lse, poisoned, sinks), want)
    d = ops.fa3_sink_grad(lse.float().contiguous(), poisoned.float().contiguous(), sinks.float())          # ... through the public call
    assert d.dtype == torch.float32 and d.shape == (3,) and float(d[1]) == 0.0
    _check(d, want)
    # the packed layout [H, total_q]: the sequences' rows one after the other, a gap in front, between and behind them full of NaN
    B, H, Sq = lse.shape
    total = 2 + Sq + 3 + Sq + 4
    starts = [2, 2 + Sq + 3]
    pl, pd = torch.full((H, total), float("nan")), torch.full((H, total), float("nan"))
    for b, s0 in enumerate(starts):
        pl[:, s0:s0 + Sq], pd[:, s0:s0 + Sq] = lse[b].float(), poisoned[b].float()
    _check(_run(_models._sink_grad_model, pl, pd, sinks, [(s0, Sq) for s0 in starts]), want)
    # ... and through the public call, where cu_seqlens_q has no gaps: the NaN tail behind cu[B] and the rows past max_seqlen_q are not read
    cl, cd = torch.full((H, 2 * (Sq + 2) + 3), float("nan")), torch.full((H, 2 * (Sq + 2) + 3), float("nan"))
    for b in range(B):
        cl[:, b * (Sq + 2):b * (Sq + 2) + Sq], cd[:, b * (Sq + 2):b * (Sq + 2) + Sq] = lse[b].float(), poisoned[b].float()
    cu = torch.tensor([0, Sq + 2, 2 * (Sq + 2)], dtype=torch.int32)
    _check(ops.fa3_sink_grad(cl, cd, sinks.float(), cu_seqlens_q=cu, max_seqlen_q=Sq), want)


def test_mutants_of_the_model_are_caught():
    lse, delta, sinks, want = _problem(0)
    with pytest.raises(AssertionError):
        _check(_run(_forgets_the_minus_sign, lse, delta, sinks), want)
    _check(_run(_multiplies_skipped_rows_by_zero, lse, delta, sinks), want)      # on clean delta the two rules agree ...
    poisoned = delta.clone()
    poisoned[torch.isneginf(lse)] = float("nan")
    with pytest.raises(AssertionError):                                          # ... with NaN on the skipped rows they do not
        _check(_run(_multiplies_skipped_rows_by_zero, lse, poisoned, sinks), want)

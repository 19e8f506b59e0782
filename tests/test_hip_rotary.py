"""GPU tests of the rotary embedding for the training calls (``ops.apply_rotary`` / ``pfa_rotary``, the ``rotary_*=`` keywords of
``ops.fa3_attention`` and ``ops.fa3_varlen_attention``, ``FlashAttention3(rotary=True)``).

The kernel's arithmetic is fixed (operands widened to fp32, the two products and the add / subtract rounded separately, one rounding to
the dtype), so every comparison is bit for bit against the plain-torch model of the rule (``ops.apply_rotary`` on CPU tensors, itself
checked pair by pair against fp64 in tests/test_rotary_host.py) run on copies.  Every tensor is a view inside a buffer that holds NaN in
front of, between and behind its rows and heads; outputs start as a sentinel; every packed row no sequence owns holds NaN.  The
comparison covers the WHOLE buffers, inputs included: a stray write, a missing write and a read of a foreign element all show.

Shapes are the smallest that can still go wrong: B 3, H 4 / Hkv 2, S 67, D 64, R 32 (seven workgroups a sequence out of place with a
ragged last one, four in place), D 16 / R 16 (one unit), D 256 / R 256 at S 5, each as ``[B, H, S, D]`` and as a permuted
``[B, S, H, D]``; packed, the ragged fixture of the KV-cache tests (``q_lens = [1, 300, 0, 33, 257]``, 640 rows of which 49 are spare)
at ``max_seqlen`` 300 and 256, under tables of 128 positions so that rows at and past 128 rotate at 127."""

from __future__ import annotations

import functools
import itertools

import pytest
import torch

from kvcache_testlib import NAN, capture, device, i32
from photonic_flash_attention_amd import ops

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
CU, TOTAL = [0, 1, 301, 301, 334, 591], 640
DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
STYLES = pytest.mark.parametrize("interleaved", [False, True], ids=["half", "interleaved"])
PLACES = pytest.mark.parametrize("inplace", [False, True], ids=["fresh", "inplace"])
# (with K, conjugate): Q with K and Q alone, forward and conjugate
FORMS = list(itertools.product([True, False], [False, True]))


def bits(t):
    return t.contiguous().view(torch.int16)


@functools.lru_cache(maxsize=None)
def _tables(R, max_pos=128):
    """The standard tables, once per rot_dim, as a view of a wider array (the row stride is not the row length): on the CPU, never modified."""
    cos, sin = ops.rotary_tables(max_pos, R)
    wide = [torch.full((max_pos, R // 2 + 4), NAN) for _ in range(2)]
    wide[0][:, :R // 2], wide[1][:, :R // 2] = cos, sin
    return wide[0][:, :R // 2], wide[1][:, :R // 2]


def _padded(shape, dtype, seed, perm=None, fill=NAN, used=None):
    """A tensor of ``shape`` -- random data; rows at and past ``used`` of the first dim NaN -- as a view inside a buffer with one more index
    in front of every axis and eight more elements in front of every row, all ``fill``.  ``perm``: the order of the axes in memory.
    -> (buffer, view)."""
    phys = list(shape) if perm is None else [shape[i] for i in perm]
    base = torch.full([n + 1 for n in phys[:-1]] + [phys[-1] + 8], fill, dtype=dtype)
    view = base[tuple(slice(1, None) for _ in phys[:-1]) + (slice(8, None),)]
    if perm is not None:
        view = view.permute([perm.index(i) for i in range(len(perm))])
    assert tuple(view.shape) == tuple(shape)
    if seed is not None:
        view.copy_(torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dtype))
        if used is not None:
            view[used:] = NAN
    return base, view


def _on(base, view, dev):
    """A copy of the buffer on ``dev`` and the same view of it."""
    b = base.clone().to(dev)
    return b, b.as_strided(view.shape, view.stride(), view.storage_offset())


def _both(pairs, cos, sin, *, inplace, interleaved=False, conjugate=False, cu=None, max_seqlen=None, pos_offsets=None, position_ids=None):
    """One call on device copies of the (buffer, view) ``pairs`` and the model on CPU copies; the whole buffers of inputs and outputs
    are compared bit for bit.  Out of place the outputs are sentinel-filled buffers of the inputs' layout.  -> the device outputs."""
    res = []
    for dev in (torch.device("cpu"), device()):
        ins = [_on(b, v, dev) for b, v in pairs]
        outs = ins if inplace else [_on(torch.full_like(b, SENTINEL), v, dev) for b, v in pairs]
        kw = dict(cu_seqlens=None if cu is None else cu.to(dev), pos_offsets=None if pos_offsets is None else pos_offsets.to(dev),
                  position_ids=None if position_ids is None else position_ids.to(dev))
        xs = [v for _, v in ins]
        c, s = cos.to(dev), sin.to(dev)
        if c.stride() != cos.stride():                      # the tables keep their row stride on the device
            c, s = (torch.empty_strided(t.shape, t.stride(), dtype=t.dtype, device=dev).copy_(t) for t in (cos, sin))
        if inplace:
            got = ops.apply_rotary(*xs, rotary_cos=c, rotary_sin=s, rotary_interleaved=interleaved, max_seqlen=max_seqlen, conjugate=conjugate,
                                   inplace=True, **kw)
            assert (got if len(xs) == 1 else got[0]) is xs[0]
        else:
            geo = ops._rotary_geometry(xs[0], xs[1] if len(xs) > 1 else None, c, s, kw["cu_seqlens"], max_seqlen, kw["pos_offsets"], kw["position_ids"])
            ops._rotary_call(xs, geo, c, s, interleaved, kw["cu_seqlens"], kw["pos_offsets"], kw["position_ids"], conjugate, False,
                             outs=[v for _, v in outs])
        if dev.type != "cpu":
            torch.cuda.synchronize()
        res.append((ins, outs))
    (m_in, m_out), (d_in, d_out) = res
    for n, ((mb, _), (db, _)) in enumerate(zip(m_in + m_out, d_in + d_out)):
        assert torch.equal(bits(db.cpu()), bits(mb)), f"buffer {n} differs from the model's"
    for (mb, mv), (b, v) in zip(m_out, pairs):
        assert not bool(torch.isnan(mv[:CU[-1]] if cu is not None else mv).any()), "a foreign element was read"
        assert not torch.equal(bits(mv), bits(v)), "nothing was rotated"
    return [v for _, v in d_out]


# --- dense ------------------------------------------------------------------------------------------------------------------------------

DENSE = [(3, 4, 2, 67, 64, 32), (2, 3, 1, 9, 16, 16), (2, 2, 1, 5, 256, 256)]


@PLACES
@STYLES
@DTYPES
def test_dense_every_shape_layout_and_form_against_the_model(dtype, interleaved, inplace):
    for (B, H, Hkv, S, D, R), perm in itertools.product(DENSE, (None, (0, 2, 1, 3))):
        cos, sin = _tables(R)
        q, k = _padded((B, H, S, D), dtype, 11 + D, perm), _padded((B, Hkv, S, D), dtype, 12 + D, perm)
        for with_k, conj in FORMS:
            _both([q, k] if with_k else [q], cos, sin, inplace=inplace, interleaved=interleaved, conjugate=conj)


def test_the_public_call_allocates_the_layout_the_attention_prefers_and_counts_workgroups():
    B, H, Hkv, S, D, R = DENSE[0]
    cos, sin = (t.to(device()) for t in _tables(R))
    (_, q), (_, k) = _padded((B, H, S, D), torch.bfloat16, 1), _padded((B, Hkv, S, D), torch.bfloat16, 2)
    qo, ko = ops.apply_rotary(q.to(device()), k.to(device()), rotary_cos=cos, rotary_sin=sin)
    torch.cuda.synchronize()
    mq, mk = ops.apply_rotary(q, k, rotary_cos=cos.cpu(), rotary_sin=sin.cpu())
    assert torch.equal(qo.cpu(), mq) and torch.equal(ko.cpu(), mk)
    assert qo.stride() == (S * H * D, D, H * D, 1) and ko.stride() == (S * Hkv * D, D, Hkv * D, 1)
    # a misaligned operand is copied, not refused: q[..., 4:] starts 8 bytes off
    wide = torch.randn(B, H, S, D + 8, generator=torch.Generator().manual_seed(3)).bfloat16()
    odd = wide.to(device())[..., 4:4 + D]
    assert odd.data_ptr() % 16 == 8
    got = ops.apply_rotary(odd, rotary_cos=cos, rotary_sin=sin)
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), ops.apply_rotary(wide[..., 4:4 + D], rotary_cos=cos.cpu(), rotary_sin=sin.cpu()))


def test_dense_positions_offsets_and_strided_position_ids():
    B, H, Hkv, S, D, R = DENSE[0]
    cos, sin = _tables(R)
    q, k = _padded((B, H, S, D), torch.bfloat16, 21), _padded((B, Hkv, S, D), torch.bfloat16, 22, (0, 2, 1, 3))
    # a negative offset (rows 0 .. 29 clamp to 0), one that runs one past the table's end (row 66 at 128 -> 127), one far outside
    _both([q, k], cos, sin, inplace=False, pos_offsets=torch.tensor([-30, 62, 2 ** 31 - 40], dtype=torch.int32))
    # position_ids, not monotonic, out of range at both ends, as a transposed view: strides (1, B)
    g = torch.Generator().manual_seed(23)
    ids = torch.randint(-20, 150, (S, B), generator=g, dtype=torch.int32)
    ids[0, 0], ids[1, 0], ids[2, 0] = -2 ** 31, 2 ** 31 - 1, 128
    for inplace in (False, True):
        _both([q, k], cos, sin, inplace=inplace, interleaved=True, position_ids=ids.t())


# --- packed -----------------------------------------------------------------------------------------------------------------------------

@PLACES
@STYLES
@DTYPES
def test_packed_ragged_fixture_against_the_model(dtype, interleaved, inplace):
    cos, sin = _tables(32)
    q, k = _padded((TOTAL, 4, 64), dtype, 31, used=CU[-1]), _padded((TOTAL, 2, 64), dtype, 32, used=CU[-1])
    cu = torch.tensor(CU, dtype=torch.int32)
    for max_seqlen in (300, 256):                           # 256: rows 257 .. 300 of the 300-row sequence stay untouched
        for with_k, conj in FORMS:
            outs = _both([q, k] if with_k else [q], cos, sin, inplace=inplace, interleaved=interleaved, conjugate=conj, cu=cu,
                         max_seqlen=max_seqlen)
            if max_seqlen == 256:
                want = q[1][257:301] if inplace else torch.full_like(q[1][257:301], SENTINEL)
                assert torch.equal(outs[0][257:301].cpu(), want)


def test_packed_positions_offsets_and_position_ids():
    cos, sin = _tables(32)
    q, k = _padded((TOTAL, 4, 64), torch.bfloat16, 41, used=CU[-1]), _padded((TOTAL, 2, 64), torch.bfloat16, 42, used=CU[-1])
    cu = torch.tensor(CU, dtype=torch.int32)
    # negative (clamped to 0), exact, one past the table's end at its second row (127, then 128 -> 127), far outside
    off = torch.tensor([5, -3, 0, 127, -2 ** 31], dtype=torch.int32)
    for inplace in (False, True):
        _both([q, k], cos, sin, inplace=inplace, cu=cu, max_seqlen=300, pos_offsets=off)
    ids = torch.randint(-20, 150, (TOTAL,), generator=torch.Generator().manual_seed(43), dtype=torch.int32)
    ids[591:] = 2 ** 30                                     # never read
    _both([q, k], cos, sin, inplace=False, interleaved=True, cu=cu, max_seqlen=300, position_ids=ids)


# --- autograd ---------------------------------------------------------------------------------------------------------------------------

@STYLES
@pytest.mark.parametrize("packed", [False, True], ids=["dense", "packed"])
def test_autograd_gradients_are_the_conjugate_model_on_dout(packed, interleaved):
    dev = device()
    cos, sin = _tables(32)
    g = torch.Generator().manual_seed(51 + packed)
    shapes = ((591, 4, 64), (591, 2, 64)) if packed else ((3, 4, 67, 64), (3, 2, 67, 64))
    q, k, gq, gk = (torch.randn(s, generator=g).bfloat16() for s in shapes + shapes)
    kw = dict(rotary_interleaved=interleaved, pos_offsets=torch.tensor([3, 0, 70, -5, 9][:5 if packed else 3], dtype=torch.int32))
    if packed:
        kw.update(cu_seqlens=torch.tensor(CU, dtype=torch.int32), max_seqlen=300)
    dkw = {n: (t.to(dev) if isinstance(t, torch.Tensor) else t) for n, t in kw.items()}
    qd, kd = q.to(dev).requires_grad_(True), k.to(dev).requires_grad_(True)
    dq_in, dk_in = gq.to(dev), gk.to(dev)
    qo, ko = ops.apply_rotary(qd, kd, rotary_cos=cos.to(dev), rotary_sin=sin.to(dev), **dkw)
    torch.autograd.backward((qo, ko), (dq_in, dk_in))
    torch.cuda.synchronize()
    mq, mk = ops.apply_rotary(q, k, rotary_cos=cos, rotary_sin=sin, **kw)
    wq, wk = ops.apply_rotary(gq, gk, rotary_cos=cos, rotary_sin=sin, conjugate=True, **kw)
    assert torch.equal(qo.detach().cpu(), mq) and torch.equal(ko.detach().cpu(), mk)
    assert torch.equal(qd.grad.cpu(), wq) and torch.equal(kd.grad.cpu(), wk)
    assert torch.equal(dq_in.cpu(), gq) and torch.equal(dk_in.cpu(), gk)            # incoming gradients are not modified
    # only k asks for a gradient: one launch over dk alone, the same bits
    k2 = k.to(dev).requires_grad_(True)
    _, ko2 = ops.apply_rotary(q.to(dev), k2, rotary_cos=cos.to(dev), rotary_sin=sin.to(dev), **dkw)
    ko2.backward(dk_in)
    torch.cuda.synchronize()
    assert torch.equal(k2.grad.cpu(), wk)


# --- the fused calls --------------------------------------------------------------------------------------------------------------------

def _leaves(*ts):
    return [t.clone().requires_grad_(True) for t in ts]


@pytest.mark.parametrize("kind", ["plain", "gqa", "sinks", "cross"])
def test_dense_attention_with_rotary_is_the_existing_call_on_rotated_operands(kind):
    dev = device()
    B, H, Sq, D = 2, 4, 130, 64
    Hkv, Sk = (2 if kind in ("gqa", "sinks") else 4), (200 if kind == "cross" else Sq)
    g = torch.Generator().manual_seed(61)
    q = torch.randn(B, Sq, H, D, generator=g).bfloat16().permute(0, 2, 1, 3).to(dev)
    k, v = (torch.randn(B, Sk, Hkv, D, generator=g).bfloat16().permute(0, 2, 1, 3).to(dev) for _ in range(2))
    dout = torch.randn(B, Sq, H, D, generator=g).bfloat16().permute(0, 2, 1, 3).to(dev)
    sinks = torch.tensor([0.5, -1.0, 2.0, 0.0], device=dev) if kind == "sinks" else None
    cos, sin = (t.to(dev) for t in ops.rotary_tables(160, 32))          # the keys of the cross case at and past 160 clamp
    off = torch.tensor([0, 17], dtype=torch.int32, device=dev)
    rot = dict(rotary_cos=cos, rotary_sin=sin, pos_offsets=off)
    causal = kind != "cross"
    skw = {} if sinks is None else dict(sinks=sinks)
    ql, kl, vl = _leaves(q, k, v)
    out = ops.fa3_attention(ql, kl, vl, causal=causal, **skw, **rot)
    out.backward(dout)
    # the existing calls on apply_rotary's outputs
    if kind == "cross":
        qr, kr = ops.apply_rotary(q, **rot), ops.apply_rotary(k, **rot)
    else:
        qr, kr = ops.apply_rotary(q, k, **rot)
    want, lse = ops.fa3_forward(qr, kr, v, causal=causal, return_lse=True, **skw)
    grads = ops.fa3_backward(qr, kr, v, want, dout, lse, causal=causal, **skw)
    if kind == "cross":
        dq, dk = ops.apply_rotary(grads[0], conjugate=True, **rot), ops.apply_rotary(grads[1], conjugate=True, **rot)
    else:
        dq, dk = ops.apply_rotary(grads[0], grads[1], conjugate=True, **rot)
    torch.cuda.synchronize()
    assert torch.equal(out, want) and torch.equal(out, ops.fa3_attention(qr, kr, v, causal=causal, **skw))
    assert torch.equal(ql.grad, dq) and torch.equal(kl.grad, dk) and torch.equal(vl.grad, grads[2])
    assert not torch.equal(out, ops.fa3_attention(q, k, v, causal=causal, **skw))     # the rotation is there
    # against the CPU model of the rotation: the device rotation inside the fused call is the specification's
    mq, mk = ops.apply_rotary(q.cpu(), rotary_cos=cos.cpu(), rotary_sin=sin.cpu(), pos_offsets=off.cpu()), \
        ops.apply_rotary(k.cpu(), rotary_cos=cos.cpu(), rotary_sin=sin.cpu(), pos_offsets=off.cpu())
    assert torch.equal(qr.cpu(), mq) and torch.equal(kr.cpu(), mk)


@pytest.mark.parametrize("kind", ["plain", "gqa", "sinks", "cross"])
def test_packed_attention_with_rotary_is_the_existing_call_on_rotated_operands(kind):
    dev = device()
    H, D = 4, 64
    Hkv = 2 if kind in ("gqa", "sinks") else 4
    g = torch.Generator().manual_seed(71)
    cu_q = i32(CU)
    cu_k = i32([0, 40, 300, 300, 420, 500]) if kind == "cross" else cu_q
    tq, tk = 591, (500 if kind == "cross" else 591)
    mq_, mk_ = 300, (260 if kind == "cross" else 300)
    q = torch.randn(tq, H, D, generator=g).bfloat16().to(dev)
    k, v = (torch.randn(tk, Hkv, D, generator=g).bfloat16().to(dev) for _ in range(2))
    dout = torch.randn(tq, H, D, generator=g).bfloat16().to(dev)
    sinks = torch.tensor([0.5, -1.0, 2.0, 0.0], device=dev) if kind == "sinks" else None
    cos, sin = (t.to(dev) for t in ops.rotary_tables(256, 64))          # rows at and past 256 of the 300-row sequence clamp
    rot = dict(rotary_cos=cos, rotary_sin=sin, rotary_interleaved=True)
    skw = {} if sinks is None else dict(sinks=sinks)
    pk = dict(cu_seqlens_q=cu_q, cu_seqlens_k=cu_k, max_seqlen_q=mq_, max_seqlen_k=mk_)
    ql, kl, vl = _leaves(q, k, v)
    out = ops.fa3_varlen_attention(ql, kl, vl, cu_q, cu_k, mq_, mk_, causal=True, **skw, **rot)
    out.backward(dout)
    if kind == "cross":
        qr = ops.apply_rotary(q, cu_seqlens=cu_q, max_seqlen=mq_, **rot)
        kr = ops.apply_rotary(k, cu_seqlens=cu_k, max_seqlen=mk_, **rot)
    else:
        qr, kr = ops.apply_rotary(q, k, cu_seqlens=cu_q, max_seqlen=mq_, **rot)
    want, lse = ops.fa3_varlen_forward(qr, kr, v, causal=True, return_lse=True, **pk, **skw)
    grads = ops.fa3_varlen_backward(qr, kr, v, want, dout, lse, causal=True, **pk, **skw)
    if kind == "cross":
        dq = ops.apply_rotary(grads[0], cu_seqlens=cu_q, max_seqlen=mq_, conjugate=True, **rot)
        dk = ops.apply_rotary(grads[1], cu_seqlens=cu_k, max_seqlen=mk_, conjugate=True, **rot)
    else:
        dq, dk = ops.apply_rotary(grads[0], grads[1], cu_seqlens=cu_q, max_seqlen=mq_, conjugate=True, **rot)
    torch.cuda.synchronize()
    assert torch.equal(out, want) and torch.equal(out, ops.fa3_varlen_attention(qr, kr, v, cu_q, cu_k, mq_, mk_, causal=True, **skw))
    assert torch.equal(ql.grad, dq) and torch.equal(kl.grad, dk) and torch.equal(vl.grad, grads[2])
    mq = ops.apply_rotary(q.cpu(), rotary_cos=cos.cpu(), rotary_sin=sin.cpu(), rotary_interleaved=True, cu_seqlens=cu_q.cpu(), max_seqlen=mq_)
    assert torch.equal(qr.cpu(), mq)


# --- graph ------------------------------------------------------------------------------------------------------------------------------

def test_a_captured_packed_call_replays_while_everything_on_the_device_changes():
    dev = device()
    g = torch.Generator().manual_seed(81)
    q0, k0, q1, k1 = (torch.randn(TOTAL, h, 64, generator=g).bfloat16() for h in (4, 2, 4, 2))
    cu0, cu1 = torch.tensor(CU, dtype=torch.int32), torch.tensor([0, 200, 200, 230, 529, 640], dtype=torch.int32)
    ids0, ids1 = (torch.randint(-5, 140, (TOTAL,), generator=g, dtype=torch.int32) for _ in range(2))
    t0, t1 = ops.rotary_tables(128, 32), ops.rotary_tables(128, 32, base=500000.0)
    q, k, cu, ids, cos, sin = (t.clone().to(dev) for t in (q0, k0, cu0, ids0, *t0))
    graph, (qo, ko) = capture(lambda: ops.apply_rotary(q, k, rotary_cos=cos, rotary_sin=sin, cu_seqlens=cu, max_seqlen=300, position_ids=ids))
    for n, (hq, hk, hcu, hids, (hc, hs)) in enumerate(((q0, k0, cu0, ids0, t0), (q1, k1, cu1, ids1, t1), (q0, k1, cu0, ids1, t0))):
        for dst, src in ((q, hq), (k, hk), (cu, hcu), (ids, hids), (cos, hc), (sin, hs)):
            dst.copy_(src)
        qo.fill_(SENTINEL)
        ko.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        mq, mk = torch.full_like(hq, SENTINEL), torch.full_like(hk, SENTINEL)
        geo = ops._rotary_geometry(hq, hk, hc, hs, hcu, 300, None, hids)
        ops._rotary_call([hq, hk], geo, hc, hs, False, hcu, None, hids, False, False, outs=[mq, mk])
        assert torch.equal(qo.cpu(), mq) and torch.equal(ko.cpu(), mk), f"replay {n} is not the model's on the new data"
        assert int((mq == SENTINEL).all(-1).all(-1).sum()) == TOTAL - int(hcu[-1])      # the rows behind cu[B] were not written


# --- module -----------------------------------------------------------------------------------------------------------------------------

def test_module_with_rotary_against_the_module_without_it_fed_rotated_projections():
    from photonic_flash_attention_amd.core.flash_attention_3 import FlashAttention3
    dev = device()
    E, heads, S, B = 256, 4, 130, 2
    torch.manual_seed(91)
    on = FlashAttention3(E, heads, dtype=torch.bfloat16, rotary=True, rotary_max_position=96).to(dev)        # rows at and past 96 clamp
    torch.manual_seed(91)
    off = FlashAttention3(E, heads, dtype=torch.bfloat16).to(dev)
    assert list(on.state_dict()) == list(off.state_dict()) and all(torch.equal(a, b) for a, b in zip(on.state_dict().values(), off.state_dict().values()))
    assert on.rotary_cos.device.type == "cuda" and on.rotary_cos.dtype == torch.float32 and on.rotary_cos.shape == (96, 32)
    x = (torch.randn(B, S, E, generator=torch.Generator().manual_seed(92)) * 0.5).bfloat16().to(dev)
    gy = torch.randn(B, S, E, generator=torch.Generator().manual_seed(93)).bfloat16().to(dev)
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    y, w = on(xa, is_causal=True)
    assert w is None
    y.backward(gy)
    # the module without the option, its projections rotated by hand between qkv_proj and the attention seam
    cos, sin = (t.to(dev) for t in ops.rotary_tables(96, E // heads))
    q, k, v = (t.view(B, S, heads, E // heads).transpose(1, 2) for t in off.qkv_proj(xb).chunk(3, dim=-1))
    qr, kr = ops.apply_rotary(q, k, rotary_cos=cos, rotary_sin=sin)
    o, _ = off._flash_attention_forward(qr, kr, v, None, False, is_causal=True)
    want = off.out_proj(o.transpose(1, 2).contiguous().view(B, S, E))
    want.backward(gy)
    torch.cuda.synchronize()
    assert torch.equal(y, want) and torch.equal(xa.grad, xb.grad)
    for (name, a), (_, b) in zip(on.named_parameters(), off.named_parameters()):
        assert torch.equal(a.grad, b.grad), name
    y_off, _ = off(x, is_causal=True)
    assert not torch.equal(y_off, y)                                      # the rotation is there
    # inference (no grad) takes the same route; and .to(bfloat16), which narrows buffers with the weights, leaves the tables fp32 values
    with torch.no_grad():
        y2, _ = on(x, is_causal=True)
        on.to(torch.bfloat16)
        y3, _ = on(x, is_causal=True)
    torch.cuda.synchronize()
    assert torch.equal(y2, y) and torch.equal(y3, y) and on.rotary_cos.dtype == torch.float32 and torch.equal(on.rotary_cos, cos)
    with pytest.raises(NotImplementedError, match="need_weights together with rotary"):
        on(x, need_weights=True)

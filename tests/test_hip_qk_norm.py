"""GPU tests of QK-norm fused with the rotary embedding of the training calls (``ops.qk_norm`` / ``pfa_qk_norm`` / ``pfa_qk_norm_bwd``,
the ``q_norm_weight=`` keywords of ``ops.fa3_attention`` and ``ops.fa3_varlen_attention``, ``FlashAttention3(qk_norm=True)``), with the
method of tests/test_hip_rotary.py.

The kernels' arithmetic is fixed (every product and sum an fp32 rounding of its own, the sum over the head dim a fixed tree, the IEEE
square root and divide), so the forward's outputs and the backward's dx are compared bit for bit with the plain-torch model of the rule
(``ops.qk_norm`` on CPU tensors, itself checked element by element against fp64 in tests/test_qk_norm_host.py) run on copies.  Every
tensor is a view inside a buffer that holds NaN in front of, between and behind its rows and heads; outputs start as a sentinel; every
packed row no sequence owns holds NaN.  The comparison covers the WHOLE buffers, inputs included.  The weight gradient is held against
fp64 under the host test's bound (tests/qk_norm_testlib.py), must be bit-identical over two runs, and must stay finite.

Shapes are the smallest that can still go wrong: B 3, H 4 / Hkv 2, S 67, D 64, R 32 (24 units a row: rows straddle workgroups, the last
workgroup is ragged, and 67 rows are two full chunks of the backward's 32 and a ragged third); D 128 at R 128 and at R 0 with H 3 / Hkv
1 and S 5; each as ``[B, H, S, D]`` and as a permuted ``[B, S, H, D]``; packed, the ragged fixture ``q_lens = [1, 300, 0, 33, 257]`` (640
rows of which 49 are spare, one sequence empty, two longer than a chunk and no multiple of it) at ``max_seqlen`` 300 and 256 under tables
of 128 positions."""

from __future__ import annotations

import functools
import itertools

import pytest
import torch

import qk_norm_testlib as Q
from kvcache_testlib import NAN, capture, device, i32
from photonic_flash_attention_amd import ops

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
EPS = 1e-6
CU, TOTAL = [0, 1, 301, 301, 334, 591], 640
DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
STYLES = pytest.mark.parametrize("interleaved", [False, True], ids=["half", "interleaved"])
PLACES = pytest.mark.parametrize("inplace", [False, True], ids=["fresh", "inplace"])
# (fp32 weights, unit offset): crossed with every shape, layout, Q alone / Q with K, pairing, dtype and place
WEIGHTS = [(True, False), (False, True), (False, False), (True, True)]
# (B, H, Hkv, S, D, R)
DENSE = [(3, 4, 2, 67, 64, 32), (2, 3, 1, 5, 128, 128), (2, 3, 1, 5, 128, 0)]


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


@functools.lru_cache(maxsize=None)
def _tables(R, max_pos=128):
    """The standard tables as a view of a wider array (the row stride is not the row length), on the CPU; (None, None) at R = 0."""
    if R == 0:
        return None, None
    cos, sin = ops.rotary_tables(max_pos, R)
    wide = [torch.full((max_pos, R // 2 + 4), NAN) for _ in range(2)]
    wide[0][:, :R // 2], wide[1][:, :R // 2] = cos, sin
    return wide[0][:, :R // 2], wide[1][:, :R // 2]


def _padded(shape, dtype, seed, perm=None, fill=NAN, used=None):
    """tests/test_hip_rotary.py's: a random tensor of ``shape`` as a view inside a buffer of ``fill`` -> (buffer, view)."""
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


def _weights(D, dtype, w_fp32, n, seed=5):
    """n weights [D] around 1 (fp32 or the dtype), each a view behind 8 NaN elements -> [(buffer, view)]."""
    out = []
    for i in range(n):
        base, view = _padded((D,), torch.float32 if w_fp32 else dtype, None)
        view.copy_(1.0 + 0.5 * torch.randn(D, generator=torch.Generator().manual_seed(seed + i)))
        out.append((base, view))
    return out


def _on(base, view, dev):
    b = base.clone().to(dev)
    return b, b.as_strided(view.shape, view.stride(), view.storage_offset())


def _table_on(cos, sin, dev):
    if cos is None:
        return None, None
    return tuple(torch.empty_strided(t.shape, t.stride(), dtype=t.dtype, device=dev).copy_(t) for t in (cos, sin))     # the row stride stays


def _kw_on(dev, cu, pos_offsets, position_ids):
    return dict(cu_seqlens=None if cu is None else cu.to(dev), pos_offsets=None if pos_offsets is None else pos_offsets.to(dev),
                position_ids=None if position_ids is None else position_ids.to(dev))


def _same_buffers(model, dev, what):
    for n, ((mb, _), (db, _)) in enumerate(zip(model, dev)):
        assert torch.equal(bits(db.cpu()), bits(mb)), f"{what} buffer {n} differs from the model's"


def _fwd_both(pairs, ws, cos, sin, *, inplace, interleaved=False, unit_offset=False, cu=None, max_seqlen=None, pos_offsets=None,
              position_ids=None):
    """One forward call on device copies of the (buffer, view) ``pairs`` with the weights ``ws`` and the model on CPU copies; the whole
    buffers of inputs, weights and outputs are compared bit for bit.  -> the device outputs."""
    res = []
    for dev in (torch.device("cpu"), device()):
        ins, wts = [_on(b, v, dev) for b, v in pairs], [_on(b, v, dev) for b, v in ws]
        outs = ins if inplace else [_on(torch.full_like(b, SENTINEL), v, dev) for b, v in pairs]
        kw = _kw_on(dev, cu, pos_offsets, position_ids)
        xs, wv = [v for _, v in ins], [v for _, v in wts]
        c, s = _table_on(cos, sin, dev)
        k, kwt = (xs[1], wv[1]) if len(xs) > 1 else (None, None)
        if inplace:
            got = ops.qk_norm(xs[0], k, q_weight=wv[0], k_weight=kwt, eps=EPS, unit_offset=unit_offset, rotary_cos=c, rotary_sin=s,
                              rotary_interleaved=interleaved, max_seqlen=max_seqlen, inplace=True, **kw)
            assert (got if len(xs) == 1 else got[0]) is xs[0]
        else:
            geo = ops._qk_norm_geometry(xs[0], k, wv[0], kwt, EPS, c, s, kw["cu_seqlens"], max_seqlen, kw["pos_offsets"], kw["position_ids"])
            ops._qk_norm_call(xs, wv, geo, EPS, unit_offset, c, s, interleaved, kw["cu_seqlens"], kw["pos_offsets"], kw["position_ids"], False,
                              outs=[v for _, v in outs])
        if dev.type != "cpu":
            torch.cuda.synchronize()
        res.append((ins + wts, outs))
    (m_in, m_out), (d_in, d_out) = res
    _same_buffers(m_in + m_out, d_in + d_out, "forward")
    for (mb, mv), (b, v) in zip(m_out, pairs):
        assert not bool(torch.isnan(mv[:CU[-1]] if cu is not None else mv).any()), "a foreign element was read"
        assert not torch.equal(bits(mv), bits(v)), "nothing was computed"
    return [v for _, v in d_out]


def _bwd_both(xp, dyp, ws, cos, sin, *, interleaved=False, unit_offset=False, cu=None, max_seqlen=None, pos_offsets=None, position_ids=None):
    """One backward call on device copies and the model on CPU copies: x, dy, the weights and dx compared bit for bit over the whole
    buffers; dw against fp64 under the bound of tests/qk_norm_testlib.py, finite, and bit-identical over two runs."""
    res = []
    for dev in (torch.device("cpu"), device()):
        xi, dyi, wts = ([_on(b, v, dev) for b, v in ps] for ps in (xp, dyp, ws))
        dxs = [_on(torch.full_like(b, SENTINEL), v, dev) for b, v in xp]
        kw = _kw_on(dev, cu, pos_offsets, position_ids)
        xs, dys, wv = ([v for _, v in ps] for ps in (xi, dyi, wts))
        c, s = _table_on(cos, sin, dev)
        k, kwt = (xs[1], wv[1]) if len(xs) > 1 else (None, None)
        geo = ops._qk_norm_geometry(xs[0], k, wv[0], kwt, EPS, c, s, kw["cu_seqlens"], max_seqlen, kw["pos_offsets"], kw["position_ids"])
        args = (geo, EPS, unit_offset, c, s, interleaved, kw["cu_seqlens"], kw["pos_offsets"], kw["position_ids"])
        _, dws = ops._qk_norm_bwd_call(xs, dys, wv, *args, dxs=[v for _, v in dxs])
        if dev.type != "cpu":
            _, again = ops._qk_norm_bwd_call(xs, dys, wv, *args, dxs=[v for _, v in dxs])
            torch.cuda.synchronize()
            for a, b in zip(dws, again):
                assert torch.equal(bits(a), bits(b)), "dw differs between two runs"
        res.append((xi + dyi + wts + dxs, dws))
    (m_buf, m_dw), (d_buf, d_dw) = res
    _same_buffers(m_buf, d_buf, "backward")
    cul = None if cu is None else cu.tolist()
    for t, ((_, x), (_, dy), (_, w)) in enumerate(zip(xp, dyp, ws)):
        want, bound = Q.dw_reference(x, dy, w, EPS, unit_offset, cos, sin, interleaved, cul, max_seqlen, pos_offsets, position_ids)
        got = d_dw[t].cpu().double()
        assert bool(torch.isfinite(got).all()), "a spare row reached dw"
        ratio = float(((got - want).abs() / bound).max())
        print(f"dw{t}: worst ratio to the bound {ratio:.4f}; bit-equal to the model: {torch.equal(bits(d_dw[t].cpu()), bits(m_dw[t]))}")
        assert ratio <= 1.0 and float(want.abs().max()) > 0.0


# --- dense ------------------------------------------------------------------------------------------------------------------------------

@PLACES
@STYLES
@DTYPES
def test_dense_forward_every_shape_layout_and_form_against_the_model(dtype, interleaved, inplace):
    for (B, H, Hkv, S, D, R), perm in itertools.product(DENSE, (None, (0, 2, 1, 3))):
        cos, sin = _tables(R)
        q, k = _padded((B, H, S, D), dtype, 11 + D, perm), _padded((B, Hkv, S, D), dtype, 12 + D, perm)
        for with_k, (w_fp32, unit) in itertools.product((True, False), WEIGHTS):
            ws = _weights(D, dtype, w_fp32, 2 if with_k else 1)
            _fwd_both([q, k] if with_k else [q], ws, cos, sin, inplace=inplace, interleaved=interleaved, unit_offset=unit)


@STYLES
@DTYPES
def test_dense_backward_every_shape_and_layout_against_the_model(dtype, interleaved):
    for (B, H, Hkv, S, D, R), perm in itertools.product(DENSE, (None, (0, 2, 1, 3))):
        cos, sin = _tables(R)
        x = [_padded((B, h, S, D), dtype, 13 + D + h, perm) for h in (H, Hkv)]
        dy = [_padded((B, h, S, D), dtype, 17 + D + h, perm) for h in (H, Hkv)]
        for with_k, (w_fp32, unit) in itertools.product((True, False), WEIGHTS):
            ws = _weights(D, dtype, w_fp32, 2 if with_k else 1)
            cut = slice(None) if with_k else slice(0, 1)
            _bwd_both(x[cut], dy[cut], ws, cos, sin, interleaved=interleaved, unit_offset=unit)


def test_the_public_call_allocates_the_layout_the_attention_prefers_and_copies_a_misaligned_operand():
    B, H, Hkv, S, D, R = DENSE[0]
    cos, sin = (t.to(device()) for t in _tables(R))
    (_, q), (_, k) = _padded((B, H, S, D), torch.bfloat16, 1), _padded((B, Hkv, S, D), torch.bfloat16, 2)
    wq, wk = (v for _, v in _weights(D, torch.bfloat16, True, 2))
    kw = dict(rotary_cos=cos, rotary_sin=sin)
    qo, ko = ops.qk_norm(q.to(device()), k.to(device()), q_weight=wq.to(device()), k_weight=wk.to(device()), **kw)
    torch.cuda.synchronize()
    mq, mk = ops.qk_norm(q, k, q_weight=wq, k_weight=wk, rotary_cos=cos.cpu(), rotary_sin=sin.cpu())
    assert torch.equal(qo.cpu(), mq) and torch.equal(ko.cpu(), mk)
    assert qo.stride() == (S * H * D, D, H * D, 1) and ko.stride() == (S * Hkv * D, D, Hkv * D, 1)
    wide = torch.randn(B, H, S, D + 8, generator=torch.Generator().manual_seed(3)).bfloat16()
    odd = wide.to(device())[..., 4:4 + D]
    wodd = torch.randn(D + 1, generator=torch.Generator().manual_seed(4))
    assert odd.data_ptr() % 16 == 8 and wodd.to(device())[1:].data_ptr() % 16 == 4
    got = ops.qk_norm(odd, q_weight=wodd.to(device())[1:], **kw)
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), ops.qk_norm(wide[..., 4:4 + D], q_weight=wodd[1:], rotary_cos=cos.cpu(), rotary_sin=sin.cpu()))
    with pytest.raises(ValueError, match="inplace=True"):
        ops.qk_norm(odd, q_weight=wq.to(device()), inplace=True, **kw)


def test_dense_positions_offsets_and_strided_position_ids():
    B, H, Hkv, S, D, R = DENSE[0]
    cos, sin = _tables(R)
    q, k = _padded((B, H, S, D), torch.bfloat16, 21), _padded((B, Hkv, S, D), torch.bfloat16, 22, (0, 2, 1, 3))
    dq, dk = _padded((B, H, S, D), torch.bfloat16, 23), _padded((B, Hkv, S, D), torch.bfloat16, 24, (0, 2, 1, 3))
    ws = _weights(D, torch.bfloat16, True, 2)
    off = torch.tensor([-30, 62, 2 ** 31 - 40], dtype=torch.int32)
    _fwd_both([q, k], ws, cos, sin, inplace=False, pos_offsets=off)
    _bwd_both([q, k], [dq, dk], ws, cos, sin, pos_offsets=off)
    ids = torch.randint(-20, 150, (S, B), generator=torch.Generator().manual_seed(23), dtype=torch.int32)
    ids[0, 0], ids[1, 0], ids[2, 0] = -2 ** 31, 2 ** 31 - 1, 128
    for inplace in (False, True):
        _fwd_both([q, k], ws, cos, sin, inplace=inplace, interleaved=True, position_ids=ids.t())
    _bwd_both([q, k], [dq, dk], ws, cos, sin, interleaved=True, position_ids=ids.t())


# --- packed -----------------------------------------------------------------------------------------------------------------------------

@PLACES
@STYLES
@DTYPES
def test_packed_forward_ragged_fixture_against_the_model(dtype, interleaved, inplace):
    cos, sin = _tables(32)
    q, k = _padded((TOTAL, 4, 64), dtype, 31, used=CU[-1]), _padded((TOTAL, 2, 64), dtype, 32, used=CU[-1])
    cu = torch.tensor(CU, dtype=torch.int32)
    for max_seqlen, with_k, (w_fp32, unit) in itertools.product((300, 256), (True, False), WEIGHTS):      # 256: rows 257 .. 300 stay untouched
        ws = _weights(64, dtype, w_fp32, 2 if with_k else 1)
        outs = _fwd_both([q, k] if with_k else [q], ws, cos, sin, inplace=inplace, interleaved=interleaved, unit_offset=unit, cu=cu,
                         max_seqlen=max_seqlen)
        if max_seqlen == 256:
            want = q[1][257:301] if inplace else torch.full_like(q[1][257:301], SENTINEL)
            assert torch.equal(outs[0][257:301].cpu(), want)


@STYLES
@DTYPES
def test_packed_backward_ragged_fixture_against_the_model(dtype, interleaved):
    assert 300 > ops.QKNORM_BWD_ROWS and 300 % ops.QKNORM_BWD_ROWS and 257 % ops.QKNORM_BWD_ROWS and 0 in [b - a for a, b in zip(CU, CU[1:])]
    x = [_padded((TOTAL, h, 64), dtype, 33 + h, used=CU[-1]) for h in (4, 2)]
    dy = [_padded((TOTAL, h, 64), dtype, 35 + h, used=CU[-1]) for h in (4, 2)]
    cu = torch.tensor(CU, dtype=torch.int32)
    for (R, max_seqlen, with_k), (w_fp32, unit) in itertools.product(((32, 300, True), (32, 256, False), (0, 300, True)), WEIGHTS):
        cos, sin = _tables(R)
        ws = _weights(64, dtype, w_fp32, 2 if with_k else 1)
        cut = slice(None) if with_k else slice(0, 1)
        _bwd_both(x[cut], dy[cut], ws, cos, sin, interleaved=interleaved, unit_offset=unit, cu=cu, max_seqlen=max_seqlen)


def test_packed_positions_offsets_and_position_ids():
    cos, sin = _tables(32)
    q, k = _padded((TOTAL, 4, 64), torch.bfloat16, 41, used=CU[-1]), _padded((TOTAL, 2, 64), torch.bfloat16, 42, used=CU[-1])
    dq, dk = _padded((TOTAL, 4, 64), torch.bfloat16, 43, used=CU[-1]), _padded((TOTAL, 2, 64), torch.bfloat16, 44, used=CU[-1])
    ws = _weights(64, torch.bfloat16, False, 2)
    cu = torch.tensor(CU, dtype=torch.int32)
    off = torch.tensor([5, -3, 0, 127, -2 ** 31], dtype=torch.int32)
    for inplace in (False, True):
        _fwd_both([q, k], ws, cos, sin, inplace=inplace, cu=cu, max_seqlen=300, pos_offsets=off)
    _bwd_both([q, k], [dq, dk], ws, cos, sin, cu=cu, max_seqlen=300, pos_offsets=off)
    ids = torch.randint(-20, 150, (TOTAL,), generator=torch.Generator().manual_seed(43), dtype=torch.int32)
    ids[591:] = 2 ** 30                                     # never read
    _fwd_both([q, k], ws, cos, sin, inplace=False, interleaved=True, cu=cu, max_seqlen=300, position_ids=ids)
    _bwd_both([q, k], [dq, dk], ws, cos, sin, interleaved=True, cu=cu, max_seqlen=300, position_ids=ids)


# --- autograd ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w_fp32", [True, False], ids=["w32", "w16"])
@pytest.mark.parametrize("packed", [False, True], ids=["dense", "packed"])
def test_autograd_gives_the_models_four_gradients(packed, w_fp32):
    dev = device()
    cos, sin = ops.rotary_tables(128, 32)
    g = torch.Generator().manual_seed(51 + packed)
    shapes = ((591, 4, 64), (591, 2, 64)) if packed else ((3, 4, 67, 64), (3, 2, 67, 64))
    q, k, gq, gk = (torch.randn(s, generator=g).bfloat16() for s in shapes + shapes)
    wq, wk = ((1.0 + 0.5 * torch.randn(64, generator=g)).to(torch.float32 if w_fp32 else torch.bfloat16) for _ in range(2))
    kw = dict(pos_offsets=torch.tensor([3, 0, 70, -5, 9][:5 if packed else 3], dtype=torch.int32))
    if packed:
        kw.update(cu_seqlens=torch.tensor(CU, dtype=torch.int32), max_seqlen=300)

    def run(d):
        leaves = [t.clone().to(d).requires_grad_(True) for t in (q, k, wq, wk)]
        dkw = {n: (t.to(d) if isinstance(t, torch.Tensor) else t) for n, t in kw.items()}
        gin = (gq.to(d), gk.to(d))
        outs = ops.qk_norm(leaves[0], leaves[1], q_weight=leaves[2], k_weight=leaves[3], eps=EPS, rotary_cos=cos.to(d), rotary_sin=sin.to(d), **dkw)
        torch.autograd.backward(outs, gin)
        if d.type != "cpu":
            torch.cuda.synchronize()
        assert torch.equal(gin[0].cpu(), gq) and torch.equal(gin[1].cpu(), gk)             # incoming gradients are not modified
        return [o.detach().cpu() for o in outs], [t.grad.cpu() for t in leaves]

    (mo, mg), (do, dg) = run(torch.device("cpu")), run(dev)
    assert torch.equal(do[0], mo[0]) and torch.equal(do[1], mo[1])
    assert torch.equal(dg[0], mg[0]) and torch.equal(dg[1], mg[1])                          # dq, dk: bit for bit
    cul = CU if packed else None
    for t, (x, dy, w) in enumerate(((q, gq, wq), (k, gk, wk))):
        want, bound = Q.dw_reference(x, dy, w, EPS, False, cos, sin, False, cul, 300 if packed else None, kw["pos_offsets"], None)
        # the fp32 sum is inside the bound; a 16-bit weight's gradient is that sum rounded once more to the weight's dtype
        bound = bound + (0.0 if w_fp32 else 2.0 ** -8 * want.abs())
        assert dg[2 + t].dtype == w.dtype and mg[2 + t].dtype == w.dtype
        for got in (dg[2 + t], mg[2 + t]):
            assert float(((got.double() - want).abs() / bound).max()) <= 1.0 and bool(torch.isfinite(got).all()) and float(got.abs().max()) > 0
    # only k and its weight ask for a gradient
    k2, wk2 = k.to(dev).requires_grad_(True), wk.to(dev).requires_grad_(True)
    dkw = {n: (t.to(dev) if isinstance(t, torch.Tensor) else t) for n, t in kw.items()}
    _, ko2 = ops.qk_norm(q.to(dev), k2, q_weight=wq.to(dev), k_weight=wk2, eps=EPS, rotary_cos=cos.to(dev), rotary_sin=sin.to(dev), **dkw)
    ko2.backward(gk.to(dev))
    torch.cuda.synchronize()
    assert torch.equal(k2.grad.cpu(), dg[1]) and torch.equal(wk2.grad.cpu(), dg[3])


# --- the fused calls --------------------------------------------------------------------------------------------------------------------

def _leaves(*ts):
    return [t.clone().requires_grad_(True) for t in ts]


@pytest.mark.parametrize("kind", ["plain", "sinks", "cross", "norm_only"])
def test_dense_attention_with_qk_norm_is_the_existing_call_on_qk_norms_outputs(kind):
    dev = device()
    B, H, Hkv, Sq, D = 2, 4, 2, 130, 64
    Sk = 200 if kind == "cross" else Sq
    g = torch.Generator().manual_seed(61)
    q = torch.randn(B, Sq, H, D, generator=g).bfloat16().permute(0, 2, 1, 3).to(dev)
    k, v = (torch.randn(B, Sk, Hkv, D, generator=g).bfloat16().permute(0, 2, 1, 3).to(dev) for _ in range(2))
    dout = torch.randn(B, Sq, H, D, generator=g).bfloat16().permute(0, 2, 1, 3).to(dev)
    wq, wk = ((1.0 + 0.5 * torch.randn(D, generator=g)).to(dev) for _ in range(2))
    sinks = torch.tensor([0.5, -1.0, 2.0, 0.0], device=dev) if kind == "sinks" else None
    rot = {}
    if kind != "norm_only":
        cos, sin = (t.to(dev) for t in ops.rotary_tables(160, 32))
        rot = dict(rotary_cos=cos, rotary_sin=sin, pos_offsets=torch.tensor([0, 17], dtype=torch.int32, device=dev))
    causal = kind != "cross"
    skw = {} if sinks is None else dict(sinks=sinks)
    ql, kl, vl, wql, wkl = _leaves(q, k, v, wq, wk)
    out = ops.fa3_attention(ql, kl, vl, causal=causal, q_norm_weight=wql, k_norm_weight=wkl, qk_norm_eps=EPS, **skw, **rot)
    out.backward(dout)
    # the existing calls on qk_norm's outputs, and pfa_qk_norm_bwd on their gradients
    if kind == "cross":
        qn, kn = ops.qk_norm(q, q_weight=wq, eps=EPS, **rot), ops.qk_norm(k, q_weight=wk, eps=EPS, **rot)
    else:
        qn, kn = ops.qk_norm(q, k, q_weight=wq, k_weight=wk, eps=EPS, **rot)
    want, lse = ops.fa3_forward(qn, kn, v, causal=causal, return_lse=True, **skw)
    grads = ops.fa3_backward(qn, kn, v, want, dout, lse, causal=causal, **skw)
    lq, lk, lwq, lwk = _leaves(q, k, wq, wk)
    if kind == "cross":
        torch.autograd.backward((ops.qk_norm(lq, q_weight=lwq, eps=EPS, **rot), ops.qk_norm(lk, q_weight=lwk, eps=EPS, **rot)), (grads[0], grads[1]))
    else:
        torch.autograd.backward(ops.qk_norm(lq, lk, q_weight=lwq, k_weight=lwk, eps=EPS, **rot), (grads[0], grads[1]))
    torch.cuda.synchronize()
    assert torch.equal(out, want) and torch.equal(out, ops.fa3_attention(qn, kn, v, causal=causal, **skw))
    assert torch.equal(ql.grad, lq.grad) and torch.equal(kl.grad, lk.grad) and torch.equal(vl.grad, grads[2])
    assert torch.equal(wql.grad, lwq.grad) and torch.equal(wkl.grad, lwk.grad) and float(wql.grad.abs().max()) > 0
    assert not torch.equal(out, ops.fa3_attention(q, k, v, causal=causal, **skw, **rot))     # the norm is there
    # the device norm inside the fused call is the specification's
    cpu_rot = {n: t.cpu() for n, t in rot.items()}
    assert torch.equal(qn.cpu(), ops.qk_norm(q.cpu(), q_weight=wq.cpu(), eps=EPS, **cpu_rot))


@pytest.mark.parametrize("kind", ["plain", "sinks", "cross"])
def test_packed_attention_with_qk_norm_is_the_existing_call_on_qk_norms_outputs(kind):
    dev = device()
    H, Hkv, D = 4, 2, 64
    g = torch.Generator().manual_seed(71)
    cu_q = i32(CU)
    cu_k = i32([0, 40, 300, 300, 420, 500]) if kind == "cross" else cu_q
    tq, tk = 591, (500 if kind == "cross" else 591)
    mq_, mk_ = 300, (260 if kind == "cross" else 300)
    q = torch.randn(tq, H, D, generator=g).bfloat16().to(dev)
    k, v = (torch.randn(tk, Hkv, D, generator=g).bfloat16().to(dev) for _ in range(2))
    dout = torch.randn(tq, H, D, generator=g).bfloat16().to(dev)
    wq, wk = ((1.0 + 0.5 * torch.randn(D, generator=g)).bfloat16().to(dev) for _ in range(2))
    sinks = torch.tensor([0.5, -1.0, 2.0, 0.0], device=dev) if kind == "sinks" else None
    cos, sin = (t.to(dev) for t in ops.rotary_tables(256, 64))
    rot = dict(rotary_cos=cos, rotary_sin=sin, rotary_interleaved=True)
    skw = {} if sinks is None else dict(sinks=sinks)
    pk = dict(cu_seqlens_q=cu_q, cu_seqlens_k=cu_k, max_seqlen_q=mq_, max_seqlen_k=mk_)
    ql, kl, vl, wql, wkl = _leaves(q, k, v, wq, wk)
    out = ops.fa3_varlen_attention(ql, kl, vl, cu_q, cu_k, mq_, mk_, causal=True, q_norm_weight=wql, k_norm_weight=wkl, qk_norm_eps=EPS,
                                   **skw, **rot)
    out.backward(dout)
    lq, lk, lwq, lwk = _leaves(q, k, wq, wk)
    if kind == "cross":
        qn = ops.qk_norm(lq, q_weight=lwq, eps=EPS, cu_seqlens=cu_q, max_seqlen=mq_, **rot)
        kn = ops.qk_norm(lk, q_weight=lwk, eps=EPS, cu_seqlens=cu_k, max_seqlen=mk_, **rot)
    else:
        qn, kn = ops.qk_norm(lq, lk, q_weight=lwq, k_weight=lwk, eps=EPS, cu_seqlens=cu_q, max_seqlen=mq_, **rot)
    want, lse = ops.fa3_varlen_forward(qn.detach(), kn.detach(), v, causal=True, return_lse=True, **pk, **skw)
    grads = ops.fa3_varlen_backward(qn.detach(), kn.detach(), v, want, dout, lse, causal=True, **pk, **skw)
    torch.autograd.backward((qn, kn), (grads[0], grads[1]))
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    assert torch.equal(ql.grad, lq.grad) and torch.equal(kl.grad, lk.grad) and torch.equal(vl.grad, grads[2])
    assert torch.equal(wql.grad, lwq.grad) and torch.equal(wkl.grad, lwk.grad) and wql.grad.dtype == torch.bfloat16
    mq = ops.qk_norm(q.cpu(), q_weight=wq.cpu(), eps=EPS, rotary_cos=cos.cpu(), rotary_sin=sin.cpu(), rotary_interleaved=True,
                     cu_seqlens=cu_q.cpu(), max_seqlen=mq_)
    assert torch.equal(qn.detach().cpu()[:591], mq[:591])


# --- graph ------------------------------------------------------------------------------------------------------------------------------

def test_a_captured_forward_and_backward_replay_while_everything_on_the_device_changes():
    dev = device()
    g = torch.Generator().manual_seed(81)
    host = [[torch.randn(TOTAL, h, 64, generator=g).bfloat16() for h in (4, 2, 4, 2)] for _ in range(2)]       # q, k, dq, dk
    cus = [torch.tensor(CU, dtype=torch.int32), torch.tensor([0, 200, 200, 230, 529, 640], dtype=torch.int32)]
    idss = [torch.randint(-5, 140, (TOTAL,), generator=g, dtype=torch.int32) for _ in range(2)]
    tabs = [ops.rotary_tables(128, 32), ops.rotary_tables(128, 32, base=500000.0)]
    wss = [[1.0 + 0.5 * torch.randn(64, generator=g) for _ in range(2)] for _ in range(2)]
    q, k, dq, dk = (t.clone().to(dev) for t in host[0])
    cu, ids, cos, sin, wq, wk = (t.clone().to(dev) for t in (cus[0], idss[0], *tabs[0], *wss[0]))
    outs = [torch.empty_like(t) for t in (q, k, q, k)]                                                          # q_out, k_out, dx_q, dx_k
    geo = ops._qk_norm_geometry(q, k, wq, wk, EPS, cos, sin, cu, 300, None, ids)

    def step():
        ops._qk_norm_call([q, k], [wq, wk], geo, EPS, False, cos, sin, False, cu, None, ids, False, outs=outs[:2])
        return ops._qk_norm_bwd_call([q, k], [dq, dk], [wq, wk], geo, EPS, False, cos, sin, False, cu, None, ids, dxs=outs[2:])[1]

    graph, dws = capture(step)
    for n, (a, b) in enumerate(((0, 0), (1, 1), (0, 1))):      # data and weights of set a; lengths, positions and tables of set b
        for dst, src in zip((q, k, dq, dk, wq, wk, cu, ids, cos, sin), (*host[a], *wss[a], cus[b], idss[b], *tabs[b])):
            dst.copy_(src)
        for o in outs:
            o.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        hq, hk, hdq, hdk = host[a]
        want = [torch.full_like(t, SENTINEL) for t in (hq, hk, hq, hk)]
        hgeo = ops._qk_norm_geometry(hq, hk, *wss[a], EPS, *tabs[b], cus[b], 300, None, idss[b])
        ops._qk_norm_call([hq, hk], wss[a], hgeo, EPS, False, *tabs[b], False, cus[b], None, idss[b], False, outs=want[:2])
        _, mdw = ops._qk_norm_bwd_call([hq, hk], [hdq, hdk], wss[a], hgeo, EPS, False, *tabs[b], False, cus[b], None, idss[b], dxs=want[2:])
        for o, w in zip(outs, want):
            assert torch.equal(o.cpu(), w), f"replay {n} is not the model's on the new data"
        assert int((want[0] == SENTINEL).all(-1).all(-1).sum()) == TOTAL - int(cus[b][-1])      # the rows behind cu[B] were not written
        for t, (x, dy, w) in enumerate(((hq, hdq, wss[a][0]), (hk, hdk, wss[a][1]))):
            wantw, bound = Q.dw_reference(x, dy, w, EPS, False, *tabs[b], False, cus[b].tolist(), 300, None, idss[b])
            assert float(((dws[t].cpu().double() - wantw).abs() / bound).max()) <= 1.0, f"replay {n}: dw{t}"


# --- module -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rotary", [True, False], ids=["rotary", "norm_only"])
def test_module_step_gives_the_models_gradients_in_the_norm_weights(rotary):
    from photonic_flash_attention_amd.core.flash_attention_3 import FlashAttention3
    dev = device()
    E, heads, S, B = 256, 4, 130, 2
    torch.manual_seed(91)
    on = FlashAttention3(E, heads, dtype=torch.bfloat16, rotary=rotary, rotary_max_position=96, qk_norm=True, qk_norm_eps=EPS).to(dev)
    torch.manual_seed(91)
    off = FlashAttention3(E, heads, dtype=torch.bfloat16).to(dev)
    assert list(on.state_dict()) == list(off.state_dict()) + ["q_norm.weight", "k_norm.weight"]
    with torch.no_grad():
        for p, seed in ((on.q_norm.weight, 94), (on.k_norm.weight, 95)):
            p.copy_(1.0 + 0.5 * torch.randn(E // heads, generator=torch.Generator().manual_seed(seed)))
    x = (torch.randn(B, S, E, generator=torch.Generator().manual_seed(92)) * 0.5).bfloat16().to(dev)
    gy = torch.randn(B, S, E, generator=torch.Generator().manual_seed(93)).bfloat16().to(dev)
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    y, w = on(xa, is_causal=True)
    assert w is None
    loss = (y.float() * gy.float()).sum()
    loss.backward()
    # the module without the option, its projections normalised by hand between qkv_proj and the attention seam
    rot = dict(zip(("rotary_cos", "rotary_sin"), (t.to(dev) for t in ops.rotary_tables(96, E // heads)))) if rotary else {}
    q, k, v = (t.view(B, S, heads, E // heads).transpose(1, 2) for t in off.qkv_proj(xb).chunk(3, dim=-1))
    wq, wk = _leaves(on.q_norm.weight.detach(), on.k_norm.weight.detach())
    qn, kn = ops.qk_norm(q, k, q_weight=wq, k_weight=wk, eps=EPS, **rot)
    for t in (q, k, qn, kn):
        t.retain_grad()
    o, _ = off._flash_attention_forward(qn, kn, v, None, False, is_causal=True)
    want = off.out_proj(o.transpose(1, 2).contiguous().view(B, S, E))
    (want.float() * gy.float()).sum().backward()
    torch.cuda.synchronize()
    assert torch.equal(y, want) and torch.equal(xa.grad, xb.grad) and bool(torch.isfinite(loss))
    for name, p in off.named_parameters():
        assert torch.equal(dict(on.named_parameters())[name].grad, p.grad), name
    for got, ref in ((on.q_norm.weight.grad, wq.grad), (on.k_norm.weight.grad, wk.grad)):
        assert torch.equal(got, ref) and bool(torch.isfinite(got).all()) and float(got.abs().max()) > 0
    # ... which are the model's: qk_norm's backward on the CPU, fed the gradients the attention handed back
    cq, ck, cwq, cwk = _leaves(q.detach().cpu(), k.detach().cpu(), wq.detach().cpu(), wk.detach().cpu())
    cpu_rot = {n: t.cpu() for n, t in rot.items()}
    torch.autograd.backward(ops.qk_norm(cq, ck, q_weight=cwq, k_weight=cwk, eps=EPS, **cpu_rot), (qn.grad.cpu(), kn.grad.cpu()))
    assert torch.equal(q.grad.cpu(), cq.grad) and torch.equal(k.grad.cpu(), ck.grad)
    for x_, dy_, w_, dev_dw, cpu_dw in ((q, qn.grad, wq, wq.grad, cwq.grad), (k, kn.grad, wk, wk.grad, cwk.grad)):
        want64, bound = Q.dw_reference(x_.detach().cpu(), dy_.cpu(), w_.detach().cpu(), EPS, False, cpu_rot.get("rotary_cos"),
                                       cpu_rot.get("rotary_sin"), False)
        bound = bound + 2.0 ** -8 * want64.abs()            # the fp32 sum rounded once more, to the bf16 of the weight
        for got in (dev_dw.cpu(), cpu_dw):
            assert float(((got.double() - want64).abs() / bound).max()) <= 1.0
    y_off, _ = off(x, is_causal=True)
    assert not torch.equal(y_off, y)                                      # the norm is there
    with pytest.raises(NotImplementedError, match="need_weights together with"):
        on(x, need_weights=True)

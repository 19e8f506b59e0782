"""GPU tests of attention sinks for training: ``sinks=`` of ``ops.fa3_forward`` / ``fa3_backward`` / ``fa3_attention``, of the packed
``ops.fa3_varlen_*`` calls, ``ops.fa3_sink_grad`` and ``FlashAttention3(attention_sinks=True)`` (``pfa_fa3_fwd_sink``,
``pfa_fa3_varlen_fwd_sink``, ``pfa_fa3_sink_grad``).

The rule: ``sinks[h]`` (fp32, one per QUERY head, in the units of the scaled scores) is one more key with that score and a zero value row,
inside the LSE; a row with no visible key has O = 0 and LSE = sinks[h]; a sink of -inf leaves the sink-less 8-wave call's bits.

The forward reference is ``dense_testlib.reference`` (fp64, CPU, the dense top-left causal rule) folded as ``kvcache_testlib.with_sink``
folds it: ``O l / (l + e^(sink - m))``, LSE by logaddexp.  Sinks are drawn from N(0, 1) per head; head 1 is -inf and head 2 is +20, where
the sink dominates every row.  The bounds are ``kvcache_testlib.check_out`` / ``check_lse``, derived for this 8-wave schedule: each case
first shows that the sink-less selector-44 call meets them on the same inputs and then holds the sink call to the same bounds (were the
sink-less call to miss one, the sink call would be held to twice that call's measured error: one more exp2 and one more multiply in the
epilogue; on the cases here it does not miss).  O and the LSE are written into NaN-guarded buffers through the C ABI.

The backward kernels are unchanged: with the sink inside the LSE and a zero value row behind it, ``P = exp(x - LSE)`` and
``delta = rowsum(dO o O)`` are already those of the softmax with the sink.  ``test_chained_backward_*`` pins that with
``dense_testlib.check_grads16`` / ``backward_bound`` evaluated on the sink-holding ``out`` and ``lse`` the device produced, and holds
``d_sinks`` to fp64 autograd of the explicit softmax with one more key by the whole-tensor criterion ``TOL16[dtype] * max(1, max|ref|)``.

``fa3_sink_grad`` alone is held to the fp64 formula on the very arrays the device holds.  Its kernel sums in fp32 in an order fixed by the
shapes: thread t of workgroup (chunk, batch, head) takes rows t, t + 256, ... of its chunk of SINK_GRAD_CHUNK = 2048 rows, lanes and waves
are folded pairwise, and one workgroup per head adds the B * ceil(Sq / 2048) partial sums.  With u = 2^-24, n the rows of a head and
t_i = exp(sink - lse_i) delta_i: any fp32 summation order of n terms is within (n - 1) u sum|t_i| of the exact sum; a term carries the
subtraction's rounding (|sink - lse_i| u relative, through the exponential), the exponential's own (2 u) and the product's (u).  The
bound used is ``(n + 4 + max|sink - lse|) u sum|t_i|``.  The row counts cross the chunk edge (2047, 2048, 2049, 4100 rows)."""

from __future__ import annotations

import ctypes as C

import pytest
import torch

import probe_testlib as pt
from dense_testlib import (DEV, GUARD, NAN32, TOL16, backward_bound, backward_given, check_grads16, guarded, reference, seen, softmax_parts,
                           visible)
from kvcache_testlib import check_lse, check_out, with_sink
from photonic_flash_attention_amd import _capi, _capi_sinks, ops

pytestmark = pytest.mark.gpu

INF = float("inf")
U = 2.0 ** -24
CHUNK = 2048                                      # SINK_GRAD_CHUNK of csrc/sink_grad_kernel.h: rows per stage-1 workgroup
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
B, H, HKV = 2, 4, 2


def _sinks(seed, n=H):
    """N(0, 1) per head; head 1 is -inf, head 2 is +20 (the sink dominates)."""
    s = torch.randn(n, generator=torch.Generator().manual_seed(700 + seed))
    s[1], s[2] = -INF, 20.0
    return s


def _qkv(Sq, Sk, D, dtype, seed, b=B, h=H, hkv=HKV):
    """[B,H,S,D] views of [B,S,H,D] arrays on the CPU, rounded to ``dtype``"""
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(b, s, n, D, generator=g).to(dtype).permute(0, 2, 1, 3) for s, n in ((Sq, h), (Sk, hkv), (Sk, hkv)))


def _ref(q, k, v, sinks, *, causal, seqlens=None, keep=None):
    """fp64 on the CPU -> ((o, lse, pnorm) without the sink, the same three with it)"""
    Bq, Hq, Sq, D = q.shape
    o, lse = reference(q, k, v, causal=causal, seqlens=seqlens, keep=keep)
    vis = visible(Bq, Hq, Sq, k.shape[2], causal=causal, seqlens=seqlens, keep=keep)
    _, w, _ = softmax_parts(q.double(), k.double(), vis, D ** -0.5)
    plain = (o, lse, w.norm(dim=-1, keepdim=True))
    return plain, with_sink(plain, sinks)


LG = 64                                           # guard entries on either side of the LSE


def _fwd(q, k, v, *, sinks=None, out_dtype=None, variant=0, **kw):
    """``pfa_fa3_fwd_sink`` (``pfa_fa3_fwd`` without sinks) on device copies of the operands, O and the LSE written into NaN-guarded
    buffers (``dense_testlib.guarded``'s for O, LG entries around the LSE) -> (o [B,H,Sq,D], lse) on the CPU.  Nothing outside the rows
    may be written."""
    Bq, Hq, Sq, D = q.shape
    odt = q.dtype if out_dtype is None else out_dtype
    qd, kd, vd = (t.to(DEV) for t in (q, k, v))
    obuf, oi, pat = guarded(Bq, Sq, Hq, D, odt)
    out = obuf[:, GUARD:GUARD + Sq, :, :D].permute(0, 2, 1, 3)
    n = Bq * Hq * Sq
    li = torch.full((LG + n + LG,), NAN32, dtype=torch.int32, device=DEV)
    lse = li[LG:LG + n].view(torch.float32).view(Bq, Hq, Sq)
    kw = {name: (t.to(DEV) if isinstance(t, torch.Tensor) else t) for name, t in kw.items()}
    args, keep = ops.build_args(qd, kd, vd, out, lse=lse, split_p=odt == torch.float32, variant=variant, **kw)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if sinks is None:
        st = _capi.load().pfa_fa3_fwd(C.byref(args), stream)
    else:
        sd = sinks.to(DEV)
        st = _capi_sinks.load().pfa_fa3_fwd_sink(C.byref(args), C.byref(_capi.make_sinks(sinks=sd.data_ptr())), stream)
    _capi.check_status(st)
    torch.cuda.synchronize()
    outside = torch.ones_like(oi, dtype=torch.bool)
    outside[:, GUARD:GUARD + Sq, :, :D] = False
    assert bool((oi[outside] == pat).all()), "O was written outside its rows"
    assert bool((li[:LG] == NAN32).all()) and bool((li[LG + n:] == NAN32).all()), "the LSE was written outside its rows"
    return out.cpu(), lse.cpu()


def _held_to_the_bounds(o, lse, ref, dtype, vmax, what, plain=None):
    """``check_out`` / ``check_lse``; ``plain``: (err of O, err of the LSE) of a sink-less call that missed them -- then twice those."""
    if plain is None:
        check_out(o, ref[0], ref[2], vmax, dtype, what)
        check_lse(o, lse, ref[1], what)
        return
    fin = torch.isfinite(ref[1])
    eo, el = float((o.double() - ref[0]).abs().max()), float((lse.double() - ref[1])[fin].abs().max())
    print(f"{what}: held to twice the sink-less call's measured error: o {eo:.3e} <= 2 x {plain[0]:.3e}, lse {el:.3e} <= 2 x {plain[1]:.3e}")
    assert bool(torch.isfinite(o).all()) and torch.equal(torch.isfinite(lse), fin)
    assert eo <= 2 * plain[0] and el <= 2 * plain[1], (what, eo, el, plain)


def _forward_case(q, k, v, sinks, dtype, out32, causal, what, **kw):
    """The sink-less selector-44 call against the bounds, then the sink call against the same; -> the sink call's (o, lse)."""
    ref_kw = dict(seqlens=kw.get("seqlens_k"), keep=kw["mask"] if "mask" in kw else (kw["key_mask"][:, None, None, :] if "key_mask" in kw else None))
    plain_ref, sink_ref = _ref(q, k, v, sinks, causal=causal, **ref_kw)
    odt = torch.float32 if out32 else None
    vmax = float(v.abs().max())
    o0, lse0 = _fwd(q, k, v, out_dtype=odt, variant=44, causal=causal, **kw)
    missed = None
    try:
        _held_to_the_bounds(o0, lse0, plain_ref, dtype, vmax, what + ", no sink (selector 44)")
    except AssertionError:
        fin = torch.isfinite(plain_ref[1])
        missed = (float((o0.double() - plain_ref[0]).abs().max()), float((lse0.double() - plain_ref[1])[fin].abs().max()))
        print(f"{what}: the sink-less call misses its bound: measured o {missed[0]:.3e}, lse {missed[1]:.3e}")
    o, lse = _fwd(q, k, v, sinks=sinks, out_dtype=odt, causal=causal, **kw)
    _held_to_the_bounds(o, lse, sink_ref, dtype, vmax, what + ", sinks", plain=missed)
    assert torch.equal(o[:, 1], o0[:, 1]) and torch.equal(lse[:, 1], lse0[:, 1]), f"{what}: the head with a sink of -inf has other bits"
    assert float(lse[:, 2].min()) >= 20.0 - 1e-4 and float(o[:, 2].abs().max()) < float(o0[:, 2].abs().max()), f"{what}: the +20 sink does not dominate"
    return o, lse


SHAPES = [(1, 1), (63, 63), (65, 65), (257, 257), (257, 130)]


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dt", list(DTYPES))
def test_forward_with_sinks_against_fp64(dt, D):
    dtype = DTYPES[dt]
    for n, (Sq, Sk) in enumerate(SHAPES):
        q, k, v = _qkv(Sq, Sk, D, dtype, 100 * D + n)
        for causal in (False, True):
            for out32 in (False, True):
                what = f"{dt} D{D} Sq{Sq} Sk{Sk} {'causal' if causal else 'full'} {'o32' if out32 else 'o16'}"
                _forward_case(q, k, v, _sinks(n), dtype, out32, causal, what)


@pytest.mark.parametrize("kind", ["seqlens_k", "key_mask", "band"])
def test_forward_with_sinks_and_masks_against_fp64(kind):
    dtype, D, Sq, Sk = torch.bfloat16, 64, 257, 257
    q, k, v = _qkv(Sq, Sk, D, dtype, 31)
    if kind == "seqlens_k":
        kw, causal = dict(seqlens_k=[77, 257]), False
    elif kind == "key_mask":
        km = torch.rand(B, Sk, generator=torch.Generator().manual_seed(3)) < 0.7
        km[:, 0] = True
        kw, causal = dict(key_mask=km), True
    else:                                          # a banded element mask, window 32: row i sees keys (i - 32, i]
        i, j = torch.arange(Sq)[:, None], torch.arange(Sk)[None, :]
        kw, causal = dict(mask=((j <= i) & (j > i - 32))[None, None].expand(B, 1, Sq, Sk).contiguous()), False
    for out32 in (False, True):
        _forward_case(q, k, v, _sinks(9), dtype, out32, causal, f"{kind} {'o32' if out32 else 'o16'}", **kw)


def test_the_ops_call_returns_the_guarded_calls_bits():
    q, k, v = _qkv(257, 130, 64, torch.bfloat16, 5)
    s = _sinks(5)
    for causal in (False, True):
        for odt in (None, torch.float32):
            o, lse = _fwd(q, k, v, sinks=s, out_dtype=odt, causal=causal)
            o2, lse2 = ops.fa3_forward(q.to(DEV), k.to(DEV), v.to(DEV), causal=causal, out_dtype=odt, return_lse=True, sinks=s.to(DEV))
            assert torch.equal(o2.cpu(), o) and torch.equal(lse2.cpu(), lse)


# --- exact properties --------------------------------------------------------------------------------------------------------------------

def _cu(lens):
    return torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32, device=DEV)


LENS = [1, 64, 65, 0, 257]                        # ... plus one empty sequence


def _packed(D, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    total = sum(LENS)
    q = torch.randn(total, H, D, generator=g).to(dtype).to(DEV)
    k, v = (torch.randn(total, HKV, D, generator=g).to(dtype).to(DEV) for _ in range(2))
    cu = _cu(LENS)
    return q, k, v, dict(cu_seqlens_q=cu, cu_seqlens_k=cu, max_seqlen_q=max(LENS), max_seqlen_k=max(LENS))


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dt", list(DTYPES))
def test_sinks_of_minus_infinity_give_the_bits_of_the_sink_less_8_wave_call(dt, D):
    dtype = DTYPES[dt]
    off = torch.full((H,), -INF)
    q, k, v = _qkv(257, 257, D, dtype, 41)
    km = torch.rand(B, 257, generator=torch.Generator().manual_seed(4)) < 0.7
    for kw in (dict(causal=False), dict(causal=True), dict(causal=False, seqlens_k=[0, 200]), dict(causal=True, key_mask=km),
               dict(causal=False, mask=torch.tril(torch.ones(257, 257, dtype=torch.bool))[None, None].expand(B, 1, 257, 257).contiguous())):
        for odt in (None, torch.float32):
            o0, lse0 = _fwd(q, k, v, out_dtype=odt, variant=44, **kw)
            o, lse = _fwd(q, k, v, sinks=off, out_dtype=odt, **kw)
            assert torch.equal(o, o0) and torch.equal(lse, lse0), (dt, D, sorted(kw), odt)
            if "seqlens_k" in kw:
                assert bool((lse[0] == -INF).all()) and bool((o[0] == 0).all())      # a row without keys keeps LSE = -inf
    qp, kp, vp, pk = _packed(D, dtype, 43)
    for causal in (False, True):
        for odt in (None, torch.float32):
            o0, lse0 = ops.fa3_varlen_forward(qp, kp, vp, causal=causal, out_dtype=odt, return_lse=True, **pk)
            o, lse = ops.fa3_varlen_forward(qp, kp, vp, causal=causal, out_dtype=odt, return_lse=True, sinks=off.to(DEV), **pk)
            torch.cuda.synchronize()
            assert torch.equal(o, o0) and torch.equal(lse, lse0), (dt, D, causal, odt)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dt", list(DTYPES))
def test_packed_sink_call_equals_the_dense_sink_calls_per_sequence(dt, D):
    dtype = DTYPES[dt]
    qp, kp, vp, pk = _packed(D, dtype, 47)
    s = _sinks(2).to(DEV)
    for causal in (False, True):
        for odt in (None, torch.float32):
            o, lse = ops.fa3_varlen_forward(qp, kp, vp, causal=causal, out_dtype=odt, return_lse=True, sinks=s, **pk)
            at = 0
            for n in LENS:
                if n:
                    qb, kb, vb = (t[at:at + n].transpose(0, 1)[None] for t in (qp, kp, vp))
                    ob, lb = ops.fa3_forward(qb, kb, vb, causal=causal, out_dtype=odt, return_lse=True, sinks=s)
                    assert torch.equal(o[at:at + n], ob[0].transpose(0, 1)) and torch.equal(lse[:, at:at + n], lb[0]), (dt, D, causal, odt, n)
                at += n
            assert bool(torch.isfinite(o.float()).all())


def test_a_batch_without_keys_has_zero_rows_and_the_sink_as_lse():
    s = _sinks(3)
    for dtype, D in ((torch.bfloat16, 64), (torch.float16, 128)):
        q, k, v = _qkv(65, 65, D, dtype, 53)
        for odt in (None, torch.float32):
            o, lse = _fwd(q, k, v, sinks=s, out_dtype=odt, causal=False, seqlens_k=[0, 65])
            assert bool((o[0] == 0).all()), "a row with no visible key is not exactly zero"
            want = s.view(H, 1).expand(H, 65)
            fin = torch.isfinite(want)
            assert bool((lse[0][~fin] == -INF).all()) and float((lse[0] - want)[fin].abs().max()) <= 2e-3      # (tests/test_hip_attn_sinks.py's 2e-3)
            assert bool(torch.isfinite(lse[1]).all())


def test_count_probe_one_sink_per_row_not_per_wave_or_tile():
    # q = 0, V of 0s and 1s, a sink of 0.0 (weight exactly 1): row i of the causal problem has O = ones_visible / (i + 1 + 1).  300 rows
    # and keys: the row size crosses a wave (32), a 256-row block and a 64-key tile.  A sink added once per wave or per tile is a count off.
    Sq = Sk = 300
    for dtype, D in ((torch.bfloat16, 64), (torch.float16, 128)):
        pr = pt.count(1, 2, 1, Sq, Sk, D, dtype)
        v = pt.probe_v(1, 1, Sk, D, dtype)
        sinks = torch.zeros(2)
        for causal in (True, False):
            vis = pt.dense_visible(1, 2, Sq, Sk, causal=causal)
            exp = pt.expected(vis, v, sinks=sinks)
            assert torch.equal(exp["L"], vis.sum(-1).double() + 1)
            o, lse = _fwd(pr["q"], pr["k"], v, sinks=sinks, out_dtype=torch.float32, causal=causal)
            pt.check_probe(o, lse, exp, torch.float32, f"count probe {dtype} D{D} causal={causal}", count_mode=True)


# --- the sink gradient alone -------------------------------------------------------------------------------------------------------------

def _sink_grad_formula(lse, delta, sinks, rows=None):
    """fp64 on the CPU from the arrays the device holds -> (d_sinks [H], the bound of the module docstring [H])."""
    Hn = sinks.shape[0]
    if rows is None:
        l, d = lse.cpu().double().transpose(0, 1).reshape(Hn, -1), delta.cpu().double().transpose(0, 1).reshape(Hn, -1)
    else:
        idx = torch.cat([torch.arange(s0, s0 + n) for s0, n in rows])
        l, d = lse.cpu().double()[:, idx], delta.cpu().double()[:, idx]
    s = sinks.cpu().double()[:, None]
    live = (l > -INF) & (s > -INF)
    x = torch.where(live, s - l, torch.zeros_like(l))
    t = torch.where(live, torch.exp(x) * torch.where(live, d, torch.zeros_like(d)), torch.zeros_like(l))
    n = l.shape[1]
    return -t.sum(1), (n + 4 + x.abs().amax(1)) * U * t.abs().sum(1)


def _check_sink_grad(got, lse, delta, sinks, rows, what):
    want, bound = _sink_grad_formula(lse, delta, sinks, rows)
    got = got.cpu().double()
    assert bool(torch.isfinite(got).all()), f"{what}: {got}"
    err = (got - want).abs()
    print(f"{what}: max err / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}, max |d_sinks| {float(want.abs().max()):.3e}")
    assert bool((err <= bound).all()), (what, got, want, bound)
    assert float(got[1]) == 0.0, f"{what}: a sink of -inf has a gradient"


@pytest.mark.parametrize("Sq", [1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 4])
def test_sink_grad_dense_against_the_fp64_formula_on_the_device_arrays(Sq):
    g = torch.Generator().manual_seed(Sq)
    lse = (torch.randn(3, H, Sq, generator=g) + 3.0)
    delta = torch.randn(3, H, Sq, generator=g)
    dead = torch.rand(3, H, Sq, generator=g) < 0.1
    lse[dead], delta[dead] = -INF, float("nan")                      # skipped rows: delta may hold anything
    sinks = _sinks(Sq % 7)
    sinks[2] = 5.0                                                   # (a sink above every LSE drawn here)
    ld, dd, sd = lse.to(DEV), delta.to(DEV), sinks.to(DEV)
    got = ops.fa3_sink_grad(ld, dd, sd)
    again = ops.fa3_sink_grad(ld, dd, sd)
    torch.cuda.synchronize()
    assert torch.equal(got, again), "two runs differ: the summation order is not fixed"
    _check_sink_grad(got, ld, dd, sd, None, f"dense, {Sq} rows a sequence")
    a = _capi_sinks.make_sink_grad_args(lse=ld.data_ptr(), delta=dd.data_ptr(), sinks=sd.data_ptr(), d_sinks=got.data_ptr(), workspace=ld.data_ptr(),
                                  workspace_bytes=1 << 30, B=3, H=H, Sq=Sq, lse_stride_b=H * Sq, lse_stride_h=Sq, delta_stride_b=H * Sq,
                                  delta_stride_h=Sq, device_id=torch.cuda.current_device())
    assert _capi_sinks.describe_sink_grad(a) == ("sink_grad_dense_c2048+final", 3 * H * ((Sq + CHUNK - 1) // CHUNK))


def test_sink_grad_packed_reads_no_row_behind_the_last_sequence():
    lens = [1, CHUNK, CHUNK + 1, 0, 300]
    pad = 77                                                         # packed rows behind cu[B]: NaN in both arrays
    total = sum(lens) + pad
    g = torch.Generator().manual_seed(11)
    lse = torch.randn(H, total, generator=g) + 3.0
    delta = torch.randn(H, total, generator=g)
    dead = torch.rand(H, total, generator=g) < 0.1
    lse[dead], delta[dead] = -INF, float("nan")
    lse[:, -pad:], delta[:, -pad:] = float("nan"), float("nan")
    sinks = _sinks(4)
    sinks[2] = 5.0
    ld, dd, sd, cu = lse.to(DEV), delta.to(DEV), sinks.to(DEV), _cu(lens)
    got = ops.fa3_sink_grad(ld, dd, sd, cu_seqlens_q=cu, max_seqlen_q=max(lens))
    again = ops.fa3_sink_grad(ld, dd, sd, cu_seqlens_q=cu, max_seqlen_q=max(lens))
    torch.cuda.synchronize()
    assert torch.equal(got, again)
    starts = [0] + list(torch.tensor(lens).cumsum(0))[:-1]
    _check_sink_grad(got, ld, dd, sd, [(int(s0), n) for s0, n in zip(starts, lens) if n], "packed")
    # a smaller max_seqlen_q: only the first rows of a longer sequence take part, the others are not read
    got = ops.fa3_sink_grad(ld, dd, sd, cu_seqlens_q=cu, max_seqlen_q=300)
    torch.cuda.synchronize()
    _check_sink_grad(got, ld, dd, sd, [(int(s0), min(n, 300)) for s0, n in zip(starts, lens) if n], "packed, max_seqlen_q 300")


# --- forward and backward chained ----------------------------------------------------------------------------------------------------------

def _sink_grad_autograd(q, k, v, dout, sinks, vis):
    """fp64 autograd of the explicit softmax over the visible keys and one more key of score sinks[h] with a zero value row -> d_sinks [H]"""
    Bq, Hq, Sq, D = q.shape
    g = Hq // k.shape[1]
    qd, kd, vd, gd = (t.detach().cpu().double() for t in (q, k, v, dout))
    s = sinks.detach().cpu().double().clone().requires_grad_(True)
    x = ((qd @ kd.repeat_interleave(g, dim=1).transpose(-1, -2)) * D ** -0.5).masked_fill(~vis, -INF)
    full = torch.cat([x, s.view(1, Hq, 1, 1).expand(Bq, Hq, Sq, 1)], dim=-1)
    dead = torch.isneginf(full).all(-1, keepdim=True)
    p = torch.where(dead, torch.zeros_like(full), torch.softmax(torch.where(dead, torch.zeros_like(full), full), dim=-1))
    o = p[..., :-1] @ vd.repeat_interleave(g, dim=1)
    (ds,) = torch.autograd.grad(o, s, gd)
    return ds


def _chain_dense(q, k, v, dout, sinks, dtype, causal, what, seqlens=None):
    """Forward with sinks, then ``fa3_backward`` with fp32 gradients on the device's own out and lse: dq, dk, dv within ``backward_bound`` of
    ``backward_given`` on those operands, d_sinks against fp64 autograd; then autograd through ``fa3_attention`` returns those numbers."""
    Bq, Hq, Sq, D = q.shape
    Hkv, Sk = k.shape[1], k.shape[2]
    qd, kd, vd, gd, sd = (t.to(DEV) for t in (q, k, v, dout, sinks))
    kw = dict(causal=causal, seqlens_k=seqlens)
    out, lse = ops.fa3_forward(qd, kd, vd, return_lse=True, sinks=sd, **kw)
    dq, dk, dv, ds = ops.fa3_backward(qd, kd, vd, out, gd, lse, grad_dtype=torch.float32, sinks=sd, **kw)
    torch.cuda.synchronize()
    vis = visible(Bq, Hq, Sq, Sk, causal=causal, seqlens=seqlens)
    scale = D ** -0.5
    *given, parts = backward_given(q, k, v, out.cpu(), dout, lse.cpu(), vis=vis, scale=scale)
    bounds = backward_bound(q, k, v, out.cpu(), dout, lse.cpu(), parts, scale=scale, dtype=dtype)
    row_seen, key_seen = seen(vis, Hkv)
    check_grads16((dq, dk, dv), given, bounds, row_seen, key_seen, what)          # (rows without keys: dq exactly 0, finite everywhere)
    want = _sink_grad_autograd(q, k, v, dout, sinks, vis)
    err, tol = float((ds.cpu().double() - want).abs().max()), TOL16[dtype] * max(1.0, float(want.abs().max()))
    print(f"{what}: d_sinks max-abs {err:.3e} (bound {tol:.3e}, max |ref| {float(want.abs().max()):.3e})")
    assert bool(torch.isfinite(ds).all()) and err <= tol and float(ds[1]) == 0.0, (what, ds, want)
    # rows without keys contribute nothing: O = 0 there, so delta = 0 -- the sum over the other batches alone is the same number
    if seqlens is not None and 0 in seqlens:
        live = [b for b, n in enumerate(seqlens) if n]
        ds_live = ops.fa3_backward(qd[live], kd[live], vd[live], out[live], gd[live], lse[live].contiguous(), sinks=sd, causal=causal,
                                   seqlens_k=[seqlens[b] for b in live])[3]
        assert torch.equal(ds_live, ds), f"{what}: the rows without keys changed d_sinks"
    # autograd: the same kernels, 16-bit gradients
    qa, ka, va = (t.clone().requires_grad_(True) for t in (qd, kd, vd))
    sa = sd.clone().requires_grad_(True)
    ops.fa3_attention(qa, ka, va, sinks=sa, **kw).backward(gd)
    g16 = ops.fa3_backward(qd, kd, vd, out, gd, lse, sinks=sd, **kw)
    torch.cuda.synchronize()
    for name, got, ref in zip(("dq", "dk", "dv", "d_sinks"), (qa.grad, ka.grad, va.grad, sa.grad), g16):
        assert torch.equal(got, ref), f"{what}: autograd's {name} is not fa3_backward's"
    assert torch.equal(sa.grad, ds)
    return qa.grad, ka.grad, va.grad


@pytest.mark.parametrize("dt", list(DTYPES))
def test_chained_backward_dense(dt):
    dtype = DTYPES[dt]
    for n, (Sq, Sk, D, causal, seqlens) in enumerate([(257, 257, 64, True, None), (130, 257, 128, False, None), (65, 65, 64, False, [0, 65]),
                                                      (257, 257, 128, True, [100, 0])]):
        q, k, v = _qkv(Sq, Sk, D, dtype, 900 + n)
        dout = torch.randn(B, Sq, H, D, generator=torch.Generator().manual_seed(950 + n)).to(dtype).permute(0, 2, 1, 3)
        _chain_dense(q, k, v, dout, _sinks(n), dtype, causal, f"{dt} Sq{Sq} Sk{Sk} D{D} causal={causal} seqlens={seqlens}", seqlens)


@pytest.mark.parametrize("causal", [False, True])
def test_chained_backward_packed(causal):
    dtype, D = torch.bfloat16, 64
    qp, kp, vp, pk = _packed(D, dtype, 61)
    gp = torch.randn(qp.shape, generator=torch.Generator().manual_seed(62)).to(dtype).to(DEV)
    sinks = _sinks(6)
    sd = sinks.to(DEV)
    out, lse = ops.fa3_varlen_forward(qp, kp, vp, causal=causal, return_lse=True, sinks=sd, **pk)
    dq, dk, dv, ds = ops.fa3_varlen_backward(qp, kp, vp, out, gp, lse, causal=causal, grad_dtype=torch.float32, sinks=sd, **pk)
    torch.cuda.synchronize()
    want, at = torch.zeros(H, dtype=torch.float64), 0
    for n in LENS:
        if n:
            qb, kb, vb, gb, ob = (t[at:at + n].cpu().transpose(0, 1)[None] for t in (qp, kp, vp, gp, out))
            lb = lse[:, at:at + n].cpu()[None]
            vis = visible(1, H, n, n, causal=causal)
            *given, parts = backward_given(qb, kb, vb, ob, gb, lb, vis=vis, scale=D ** -0.5)
            bounds = backward_bound(qb, kb, vb, ob, gb, lb, parts, scale=D ** -0.5, dtype=dtype)
            grads = tuple(t[at:at + n].transpose(0, 1)[None] for t in (dq, dk, dv))
            check_grads16(grads, given, bounds, *seen(vis, HKV), f"packed causal={causal}, sequence of {n}")
            want += _sink_grad_autograd(qb, kb, vb, gb, sinks, vis)
        at += n
    err, tol = float((ds.cpu().double() - want).abs().max()), TOL16[dtype] * max(1.0, float(want.abs().max()))
    print(f"packed causal={causal}: d_sinks max-abs {err:.3e} (bound {tol:.3e})")
    assert bool(torch.isfinite(ds).all()) and err <= tol and float(ds[1]) == 0.0
    qa, ka, va = (t.clone().requires_grad_(True) for t in (qp, kp, vp))
    sa = sd.clone().requires_grad_(True)
    ops.fa3_varlen_attention(qa, ka, va, pk["cu_seqlens_q"], pk["cu_seqlens_k"], pk["max_seqlen_q"], pk["max_seqlen_k"], causal=causal,
                             sinks=sa).backward(gp)
    g16 = ops.fa3_varlen_backward(qp, kp, vp, out, gp, lse, causal=causal, sinks=sd, **pk)
    torch.cuda.synchronize()
    for name, got, ref in zip(("dq", "dk", "dv", "d_sinks"), (qa.grad, ka.grad, va.grad, sa.grad), g16):
        assert torch.equal(got, ref), f"packed: autograd's {name} is not fa3_varlen_backward's"
    assert torch.equal(sa.grad, ds)


def test_sinks_without_requires_grad_skip_the_sink_grad_launches(monkeypatch):
    calls = []
    real = ops.fa3_sink_grad
    monkeypatch.setattr(ops, "fa3_sink_grad", lambda *a, **kw: (calls.append(1), real(*a, **kw))[1])
    q, k, v = (t.to(DEV) for t in _qkv(130, 130, 64, torch.bfloat16, 71))
    dout = torch.randn(B, 130, H, 64, generator=torch.Generator().manual_seed(72)).bfloat16().permute(0, 2, 1, 3).to(DEV)
    qp, kp, vp, pk = _packed(64, torch.bfloat16, 73)
    gp = torch.randn(qp.shape, generator=torch.Generator().manual_seed(74)).bfloat16().to(DEV)
    pos = (pk["cu_seqlens_q"], pk["cu_seqlens_k"], pk["max_seqlen_q"], pk["max_seqlen_k"])
    for run, ops_q, ops_g in ((lambda a, b, c, s: ops.fa3_attention(a, b, c, causal=True, sinks=s), (q, k, v), dout),
                              (lambda a, b, c, s: ops.fa3_varlen_attention(a, b, c, *pos, causal=True, sinks=s), (qp, kp, vp), gp)):
        grads = {}
        for needs in (True, False):
            del calls[:]
            leaves = [t.clone().requires_grad_(True) for t in ops_q]
            s = _sinks(7).to(DEV).requires_grad_(needs)
            run(*leaves, s).backward(ops_g)
            torch.cuda.synchronize()
            assert len(calls) == (1 if needs else 0), "the sink-grad launches do not follow sinks.requires_grad"
            assert (s.grad is not None) == needs
            grads[needs] = [t.grad for t in leaves]
        for a, b in zip(grads[True], grads[False]):
            assert torch.equal(a, b)


# --- graph ---------------------------------------------------------------------------------------------------------------------------------

def test_a_captured_forward_and_backward_replay_while_the_sinks_change():
    from kvcache_testlib import capture
    q, k, v = (t.to(DEV) for t in _qkv(257, 257, 64, torch.bfloat16, 81, b=1, h=4, hkv=2))
    dout = torch.randn(1, 257, 4, 64, generator=torch.Generator().manual_seed(82)).bfloat16().permute(0, 2, 1, 3).to(DEV)
    sinks = torch.tensor([0.5, -INF, 20.0, -1.0], device=DEV)

    def step():
        out, lse = ops.fa3_forward(q, k, v, causal=True, return_lse=True, sinks=sinks)
        return (out, lse) + tuple(ops.fa3_backward(q, k, v, out, dout, lse, causal=True, sinks=sinks))

    graph, res = capture(step)
    sinks.copy_(torch.tensor([-INF, 2.0, -3.0, 1.0], device=DEV))
    graph.replay()
    torch.cuda.synchronize()
    eager = step()
    torch.cuda.synchronize()
    for name, a, b in zip(("out", "lse", "dq", "dk", "dv", "d_sinks"), res, eager):
        assert torch.equal(a, b), f"the replayed {name} is not the eager call's on the new sinks"
    assert float(res[5][0]) == 0.0 and float(res[5][1]) != 0.0


# --- modules -------------------------------------------------------------------------------------------------------------------------------

def test_module_with_attention_sinks_against_its_math_in_fp64():
    from photonic_flash_attention_amd.core.flash_attention_3 import FlashAttention3
    torch.manual_seed(91)
    E, heads, S = 256, 4, 130
    m = FlashAttention3(E, heads, dtype=torch.bfloat16, attention_sinks=True).to(DEV)
    assert m.sinks.dtype == torch.float32 and m.sinks.device.type == "cuda"
    with torch.no_grad():
        m.sinks.copy_(torch.tensor([0.7, -0.4, 1.5, 0.0]))
    x = (torch.randn(2, S, E, generator=torch.Generator().manual_seed(92)) * 0.5).bfloat16().to(DEV).requires_grad_(True)
    gy = torch.randn(2, S, E, generator=torch.Generator().manual_seed(93)).bfloat16().to(DEV)
    y, w = m(x, is_causal=True)
    assert w is None
    y.backward(gy)
    torch.cuda.synchronize()
    # the same module math in fp64 on the CPU
    W, bq, Wo, bo = (t.detach().cpu().double() for t in (m.qkv_proj.weight, m.qkv_proj.bias, m.out_proj.weight, m.out_proj.bias))
    xs = x.detach().cpu().double().requires_grad_(True)
    s64 = m.sinks.detach().cpu().double().requires_grad_(True)
    qkv = xs @ W.T + bq
    q, k, v = (t.view(2, S, heads, E // heads).transpose(1, 2) for t in qkv.chunk(3, dim=-1))
    sc = (q @ k.transpose(-1, -2)) * (E // heads) ** -0.5
    sc = sc.masked_fill(~torch.tril(torch.ones(S, S, dtype=torch.bool)), -INF)
    p = torch.softmax(torch.cat([sc, s64.view(1, heads, 1, 1).expand(2, heads, S, 1)], dim=-1), dim=-1)
    yr = (p[..., :-1] @ v).transpose(1, 2).reshape(2, S, E) @ Wo.T + bo
    gx, gs = torch.autograd.grad(yr, (xs, s64), gy.cpu().double())
    tol = TOL16[torch.bfloat16]
    for name, got, ref in (("y", y, yr.detach()), ("x.grad", x.grad, gx), ("sinks.grad", m.sinks.grad, gs)):
        err, bound = float((got.detach().cpu().double() - ref).abs().max()), 2 * tol * max(1.0, float(ref.abs().max()))
        print(f"module {name}: max-abs {err:.3e} (bound {bound:.3e}, max |ref| {float(ref.abs().max()):.3e})")
        assert err <= bound, (name, err, bound)          # (2 x: the projections round to bf16 on either side of the attention)
    assert float(gs.abs().max()) > 1e-3 and m.sinks.grad.dtype == torch.float32


def test_the_default_module_returns_the_bits_it_returned_before_the_option():
    from photonic_flash_attention_amd.core.flash_attention_3 import FlashAttention3
    torch.manual_seed(95)
    E, heads, S = 256, 4, 130
    m = FlashAttention3(E, heads, dtype=torch.bfloat16).to(DEV)
    assert m.sinks is None and "sinks" not in m.state_dict()
    x = torch.randn(2, S, E, generator=torch.Generator().manual_seed(96)).bfloat16().to(DEV).requires_grad_(True)
    y, _ = m(x, is_causal=True)
    # what the module computed before the option existed: the projections around ops.fa3_attention without sinks
    q, k, v = (t.view(2, S, heads, E // heads).transpose(1, 2) for t in m.qkv_proj(x).chunk(3, dim=-1))
    o = ops.fa3_attention(q, k, v, causal=True, key_mask=None, mask=None, softmax_scale=(E // heads) ** -0.5, out_dtype=q.dtype)
    want = m.out_proj(o.transpose(1, 2).contiguous().view(2, S, E))
    torch.cuda.synchronize()
    assert torch.equal(y, want)
    with torch.no_grad():
        y2, _ = m(x.detach(), is_causal=True)
        o2, _ = ops.fa3_forward(q.detach(), k.detach(), v.detach(), causal=True, softmax_scale=(E // heads) ** -0.5)
        assert torch.equal(y2, m.out_proj(o2.transpose(1, 2).contiguous().view(2, S, E)))

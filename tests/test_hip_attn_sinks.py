"""GPU tests of attention sinks over the KV cache: ``sinks=`` of ``ops.fa3_decode``, ``ops.fa3_prefill_cache`` and
``ops.fa3_prefill_varlen`` (``pfa_fa3_*_sink`` with a ``pfa_fa3_sinks`` block).

The rule: ``sinks[h]`` (fp32, one per query head, in the units of the scaled scores) is one extra key with that score and a zero value
row -- ``den_i = sum_j exp(x_ij) + exp(sinks[h])``, ``LSE_i = log(den_i)``; a row with no visible key has O = 0 and LSE = sinks[h].

The reference: ``kvcache_testlib.with_sink`` turns ``reference``'s fp64 ``(o, lse, pnorm)`` into the sink result with
``w = sigmoid(lse - sink_h)``: ``o' = o w``, ``pnorm' = pnorm w``, ``lse' = logaddexp(lse, sink_h)``, and on rows with ``lse = -inf``
``o' = 0``, ``lse' = sink_h``.  tests/test_attn_sinks_host.py checks it on the CPU against the formulation that appends a key.  The
bounds are ``check_out`` and ``check_lse`` of tests/kvcache_testlib.py, unchanged, with ``pnorm'``.

Sinks that matter: ``choose_sinks`` puts head h's sink at the median of its finite reference LSEs plus an offset spread over
[-1.5, 1.5] across the heads; head 0 gets -inf and the last head 20 below its median (the two ends of the spread).  Every numeric test
first asserts on the reference alone (``assert_sinks_matter``) that at least a quarter of all rows have a sink share ``1 - w`` in
[0.2, 0.8] and that on those rows the reference with the sink counted twice (``sink_h + ln 2``) and the reference without a sink each
differ from the true one by more than 10 x ``check_out``'s bound in at least one element: a sink dropped, applied in every split or in
both passes of a shared prefix cannot pass.  Inputs are drawn on the CPU, so tests/test_attn_sinks_host.py runs the same assertion over
``CASES`` without a GPU.

Every kernel call gets caches with NaN behind the lengths (and, under a window, below the 64-key boundary the kernels promise not to
read); the reference reads clean copies."""

from __future__ import annotations

import functools
import math

import pytest
import torch

from capi_testlib import decode_args
from kvcache_testlib import (EPS, INF, capture, check_lse, check_out, device, guard, i32, ragged_equals_uniform, reference, run_and_check,
                             scatter, with_sink)
from photonic_flash_attention_amd import ops

pytestmark = pytest.mark.gpu

LN2 = math.log(2.0)
DT_D = [(torch.bfloat16, 64), (torch.float16, 128), (torch.float16, 64), (torch.bfloat16, 128)]
DT_IDS = ["bf16-d64", "fp16-d128", "fp16-d64", "bf16-d128"]


# --- the reference with sinks, and sinks that matter (CPU or GPU tensors; no kernel) -------------------------------------------------

def choose_sinks(rlse):
    """``rlse [B,H,Sq]`` (the sink-less reference LSE) -> fp32 ``sinks [H]`` on the CPU: per head the median of the finite LSEs plus an
    offset spread over [-1.5, 1.5] across the heads; head 0 is -inf, the last head 20 below its median."""
    H = rlse.shape[1]
    offs = torch.linspace(-1.5, 1.5, H, dtype=torch.float64)
    med = torch.stack([torch.quantile(x[torch.isfinite(x)], 0.5) for x in (rlse[:, h].reshape(-1).cpu() for h in range(H))])
    s = med + offs
    s[0] = -INF
    s[H - 1] = med[H - 1] - 20.0
    return s.float()


def assert_sinks_matter(ref, sinks, dtype, vmax, out32=False):
    """The two conditions of the module docstring, on the sink-less reference ``ref`` and ``sinks`` alone."""
    o, lse, pn = ref
    true = with_sink(ref, sinks)
    s = sinks.to(lse.device).double().view(1, -1, 1).expand_as(lse)
    share = torch.where(torch.isneginf(s), torch.zeros_like(lse), torch.sigmoid(s - lse))          # 1 - w; 1 on rows without keys
    rows = (share >= 0.2) & (share <= 0.8)
    frac = float(rows.double().mean())
    assert frac >= 0.25, f"only {frac:.3f} of the rows have a sink share in [0.2, 0.8]"
    bound = torch.full_like(true[0], 1e-3) if out32 else EPS[dtype] * true[0].abs() + 3 * EPS[dtype] * vmax * true[2] + 2e-6
    twice = with_sink(ref, sinks.double() + LN2)
    for name, other in (("the sink counted twice", twice[0]), ("no sink", o)):
        far = ((other - true[0]).abs() > 10 * bound) & rows[..., None]
        assert bool(far.any()), f"{name} is within 10 x the bound of the true reference on every row that matters"
    return frac


# --- the problems: drawn on the CPU, shared, never modified --------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def problem(B, H, Hkv, Sq, Smax, D, dtype, seed=0):
    """CPU tensors: q as a [B,H,Sq,D] view of a [B,Sq,H,D] buffer, contiguous k, v [B,Hkv,Smax,D]."""
    g = torch.Generator().manual_seed(7000 + 131 * seed + 17 * Sq + D + (0 if dtype is torch.bfloat16 else 1))
    q = torch.randn(B, Sq, H, D, generator=g).to(dtype).permute(0, 2, 1, 3)
    k = torch.randn(B, Hkv, Smax, D, generator=g).to(dtype)
    v = torch.randn(B, Hkv, Smax, D, generator=g).to(dtype)
    return q, k, v


@functools.lru_cache(maxsize=None)
def case(B, H, Hkv, Sq, Smax, D, dtype, lens, causal=True, window=None, mask_seed=None, seed=0):
    """One uniform problem with its lengths, optional key mask, the sink-less fp64 reference and the chosen sinks, all on the CPU."""
    q, k, v = problem(B, H, Hkv, Sq, Smax, D, dtype, seed)
    km = None
    if mask_seed is not None:
        km = torch.rand(B, Smax, generator=torch.Generator().manual_seed(mask_seed)) > 0.3
    ref = reference(q, k, v, seqlens=torch.tensor(lens), key_mask=km, causal=causal, window=window)
    return dict(q=q, k=k, v=v, lens=lens, km=km, ref=ref, sinks=choose_sinks(ref[1]), causal=causal, window=window, dtype=dtype,
                vmax=float(v.abs().max()))


DECODE_LENS = {(1, 448): (0, 300, 448), (5, 448): (0, 3, 440), (1, 1024): (0, 700, 1000), (5, 1024): (0, 3, 1000)}
PREFILL_LENS = {1: (320, 0), 70: (320, 60), 257: (320, 250)}
RAGGED_Q = (1, 70, 0, 257)
RAGGED_LENS = (300, 60, 50, 250)
RAGGED_WIN_LENS = (1000, 517, 50, 700)


def decode_case(dtype, D, Sq, Smax, mask_seed=None):
    return case(3, 8, 2, Sq, Smax, D, dtype, DECODE_LENS[(Sq, Smax)], mask_seed=mask_seed)


def prefill_case(dtype, D, Sq, causal=True):
    return case(2, 8, 2, Sq, 320, D, dtype, PREFILL_LENS[Sq], causal=causal)


@functools.lru_cache(maxsize=None)
def ragged_case(dtype, D, window=None, H=8, Smax=320, lens=RAGGED_LENS):
    """The ragged step of ``RAGGED_Q`` rows: per-sequence uniform cases over one cache, one sinks vector from all their LSEs."""
    B = len(RAGGED_Q)
    _, k, v = problem(B, H, 2, 1, Smax, D, dtype, seed=3)
    g = torch.Generator().manual_seed(7100 + D + H)
    q = torch.randn(sum(RAGGED_Q), H, D, generator=g).to(dtype)
    refs, at = [], 0
    for b, n in enumerate(RAGGED_Q):
        qb = q[at:at + n].permute(1, 0, 2)[None]
        refs.append(reference(qb, k[b:b + 1], v[b:b + 1], seqlens=torch.tensor(lens[b:b + 1]), window=window) if n else None)
        at += n
    packed = tuple(torch.cat([r[i] for r in refs if r is not None], dim=2) for i in range(3))          # [1,H,total,...]
    return dict(q=q, k=k, v=v, lens=lens, ref=packed, sinks=choose_sinks(packed[1]), window=window, dtype=dtype, vmax=float(v.abs().max()))


def window_case(kind, dtype=torch.bfloat16):
    if kind == "decode":
        return case(2, 16, 2, 1, 1024, 64, dtype, (1000, 517), window=128)
    if kind == "decode-split":          # a window wide enough for the plan to split its span
        return case(2, 16, 2, 1, 1024, 64, dtype, (1000, 517), window=640)
    return case(2, 16, 2, 200, 1024, 64, dtype, (1000, 517), window=128)


def split_case(dtype, D):
    return case(1, 8, 2, 256, 2048, D, dtype, (2000,))


@functools.lru_cache(maxsize=None)
def prefix_case(dtype, D, Sq, P=128, private=(64, 130, 200, 77), Smax=384):
    """A shared-prefix step: every sequence's first P keys are sequence 0's, lengths P + private, every row behind the prefix."""
    B = len(private)
    q, k, v = problem(B, 8, 2, Sq, Smax, D, dtype, seed=5)
    k, v = k.clone(), v.clone()
    k[:, :, :P], v[:, :, :P] = k[:1, :, :P], v[:1, :, :P]
    lens = tuple(P + max(n, Sq) for n in private)
    ref = reference(q, k, v, seqlens=torch.tensor(lens))
    return dict(q=q, k=k, v=v, lens=lens, km=None, ref=ref, sinks=choose_sinks(ref[1]), causal=True, window=None, dtype=dtype,
                vmax=float(v.abs().max()), P=P)


def all_cases():
    """(name, case, out32) of every numeric test below: what tests/test_attn_sinks_host.py runs ``assert_sinks_matter`` over on the CPU."""
    for (dtype, D), tag in zip(DT_D, DT_IDS):
        for (Sq, Smax) in DECODE_LENS:
            yield f"decode {tag} Sq {Sq} Smax {Smax}", decode_case(dtype, D, Sq, Smax), False
        yield f"decode key mask {tag}", decode_case(dtype, D, 5, 1024, mask_seed=11), False
        yield f"decode fp32 {tag}", decode_case(dtype, D, 5, 1024), True
        for Sq in PREFILL_LENS:
            for causal in (True, False):
                yield f"prefill {tag} Sq {Sq} causal {causal}", prefill_case(dtype, D, Sq, causal), False
            yield f"prefill fp32 {tag} Sq {Sq}", prefill_case(dtype, D, Sq), True
        yield f"ragged {tag}", ragged_case(dtype, D), False
        yield f"split {tag}", split_case(dtype, D), False
        for Sq in (1, 70):
            yield f"prefix {tag} Sq {Sq}", prefix_case(dtype, D, Sq), False
    for kind in ("decode", "decode-split", "prefill"):
        yield f"window {kind}", window_case(kind), False
    yield "window ragged", ragged_case(torch.bfloat16, 64, window=128, H=16, Smax=1024, lens=RAGGED_WIN_LENS), False


CASES = all_cases


# --- on the device -----------------------------------------------------------------------------------------------------------------

def _matter(c, out32=False):
    return assert_sinks_matter(c["ref"], c["sinks"], c["dtype"], c["vmax"], out32)


def _nsplit_decode(q, k, Smax, window=None, sinks=True):
    from photonic_flash_attention_amd import _capi
    B, H, Sq, D = q.shape
    dt = 0 if q.dtype == torch.bfloat16 else 1
    a = decode_args(dict(B=B, H=H, Hkv=k.shape[1], D=D, dtype_in=dt, dtype_out=dt), Sq=Sq, Smax=Smax)
    ext = None if window is None else _capi.make_cache_ext(window=window)
    name, _, ns = _capi.describe_decode_sink(a, ext, _capi.make_sinks(sinks=0x9000) if sinks else None)
    assert ("_sink" in name) == sinks
    return ns


def _varlen(q, kn, vn, **kw):
    """``ops.fa3_prefill_varlen`` of ``RAGGED_Q`` rows -> (o [1,H,total,D], lse [1,H,total]) in the layout of the packed reference."""
    cu = i32([0] + list(torch.tensor(RAGGED_Q).cumsum(0)))
    o, lse = ops.fa3_prefill_varlen(q, kn, vn, cu_seqlens_q=cu, max_seqlen_q=max(RAGGED_Q), **kw)
    return o.permute(1, 0, 2)[None], lse[None]


def _run(fn, c, what, sinks="case", paged=None, o_plain=None, **kw):
    """``fn`` on the case's caches, guarded (``run_and_check``), against the case's reference with ``sinks`` ("case": the case's own; None:
    the sink-less call) -> (o, lse).  paged: the seed of a scatter over pages of 64 keys.  Then the mode's own assertions: rows without
    keys exactly zero with LSE = sink; head 0 (sink -inf) with the bits of the sink-less call ``o_plain``."""
    dev = device()
    s = c["sinks"].to(dev) if isinstance(sinks, str) else sinks

    def on_pages(q, kn, vn, **kw2):
        kp, vp, table = scatter(kn, vn, 64, seed=paged)
        return fn(q, kp, vp, block_table=table, **kw2)

    km = c.get("km")
    o, lse = run_and_check(fn if paged is None else on_pages, c["q"].to(dev), c["k"].to(dev), c["v"].to(dev), c["lens"],
                           causal=c.get("causal", True), window=c["window"], key_mask=None if km is None else km.to(dev), ref=c["ref"],
                           with_ref=None if s is None else (lambda ref: with_sink(ref, s)), what=what, sinks=s, **kw)
    if s is not None:
        rlse = with_sink(c["ref"], s)[1].to(dev)
        dead = torch.isneginf(c["ref"][1]).to(dev)
        assert bool((o[dead[..., None].expand_as(o)] == 0).all()), f"{what}: a row with no visible key is not exactly zero"
        assert bool((lse.double() - rlse)[dead & torch.isfinite(rlse)].abs().le(2e-3).all()), f"{what}: LSE of a row without keys is not its sink"
    if o_plain is not None:
        assert torch.equal(o[:, 0], o_plain[:, 0]), f"{what}: the head with a sink of -inf does not have the sink-less call's bits"
    return o, lse


def _ragged_equals_uniform(c, o, lse):
    """The ragged result against per-sequence uniform calls with the same sinks: bit for bit."""
    dev = device()
    kn, vn = guard(c["k"].to(dev), c["v"].to(dev), c["lens"], RAGGED_Q, c["window"])
    cu = [0] + torch.tensor(RAGGED_Q).cumsum(0).tolist()
    ragged_equals_uniform(ops.fa3_prefill_cache, o[0].permute(1, 0, 2), lse[0], c["q"].to(dev), kn, vn, cu, c["lens"], window=c["window"],
                          sinks=c["sinks"].to(dev))


# --- 1. decode -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,D", DT_D, ids=DT_IDS)
def test_decode_with_sinks_against_fp64(dtype, D):
    for (Sq, Smax) in DECODE_LENS:
        c = decode_case(dtype, D, Sq, Smax)
        _matter(c)
        ns = _nsplit_decode(c["q"], c["k"], Smax)
        assert ns == _nsplit_decode(c["q"], c["k"], Smax, sinks=False) and (ns > 1) == (Smax == 1024)
        o_plain, _ = _run(ops.fa3_decode, c, "decode, no sinks", sinks=None)
        o, lse = _run(ops.fa3_decode, c, f"decode Sq {Sq} Smax {Smax}", o_plain=o_plain)
        op, lsep = _run(ops.fa3_decode, c, f"decode paged Sq {Sq} Smax {Smax}", paged=3, o_plain=o_plain)
        assert torch.equal(o, op) and torch.equal(lse, lsep)


@pytest.mark.parametrize("dtype,D", DT_D, ids=DT_IDS)
def test_decode_with_sinks_key_mask_and_fp32_output(dtype, D):
    c = decode_case(dtype, D, 5, 1024, mask_seed=11)
    _matter(c)
    _run(ops.fa3_decode, c, "decode key mask")
    c = decode_case(dtype, D, 5, 1024)
    _matter(c, out32=True)
    o, lse = _run(ops.fa3_decode, c, "decode fp32", out_dtype=torch.float32)
    assert o.dtype == torch.float32


# --- 2. sinks all -inf: the sink-less call -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,D", DT_D[:2], ids=DT_IDS[:2])
def test_sinks_of_minus_infinity_give_the_sink_less_bits(dtype, D):
    off = torch.full((8,), -INF, device=device())
    for what, fn, c, kw in (("decode one split", ops.fa3_decode, decode_case(dtype, D, 5, 448), {}),
                            ("decode four splits", ops.fa3_decode, decode_case(dtype, D, 5, 1024), {}),
                            ("prefill", ops.fa3_prefill_cache, prefill_case(dtype, D, 257), {}),
                            ("prefill key_splits 3", ops.fa3_prefill_cache, prefill_case(dtype, D, 257), dict(key_splits=3)),
                            ("ragged", _varlen, ragged_case(dtype, D), dict(sqs=RAGGED_Q))):
        o0, lse0 = _run(fn, c, what, sinks=None, **kw)
        o, lse = _run(fn, c, what, sinks=off, **kw)
        assert torch.equal(o, o0), what
        check_lse(o, lse, lse0.double(), what)


# --- 3. prefill ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,D", DT_D, ids=DT_IDS)
def test_prefill_with_sinks_against_fp64(dtype, D):
    for Sq in PREFILL_LENS:
        for causal in (True, False):
            c = prefill_case(dtype, D, Sq, causal)
            _matter(c)
            o_plain, _ = _run(ops.fa3_prefill_cache, c, "prefill, no sinks", sinks=None)
            o, lse = _run(ops.fa3_prefill_cache, c, f"prefill Sq {Sq} causal {causal}", o_plain=o_plain)
            op, lsep = _run(ops.fa3_prefill_cache, c, "prefill paged", paged=4)
            assert torch.equal(o, op) and torch.equal(lse, lsep)
        c = prefill_case(dtype, D, Sq)
        _matter(c, out32=True)
        o, lse = _run(ops.fa3_prefill_cache, c, f"prefill fp32 Sq {Sq}", out_dtype=torch.float32, paged=4 if Sq == 70 else None)
        assert o.dtype == torch.float32


# --- 4. ragged -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,D", DT_D, ids=DT_IDS)
def test_ragged_prefill_with_sinks(dtype, D):
    c = ragged_case(dtype, D)
    _matter(c)
    o, lse = _run(_varlen, c, "ragged", sqs=RAGGED_Q)
    _ragged_equals_uniform(c, o, lse)
    op, lsep = _run(_varlen, c, "ragged paged", sqs=RAGGED_Q, paged=5)
    assert torch.equal(o, op) and torch.equal(lse, lsep)


# --- 5. window plus sinks ------------------------------------------------------------------------------------------------------------

def test_window_and_sinks_decode():
    for kind, W in (("decode", 128), ("decode-split", 640)):
        c = window_case(kind)
        _matter(c)
        ns = _nsplit_decode(c["q"], c["k"], 1024, window=W)
        # the plan is the sink-less call's: the span of a 128-key window is below two splits' worth of keys, that of 640 keys is not
        assert ns == _nsplit_decode(c["q"], c["k"], 1024, window=W, sinks=False) and (ns > 1) == (W == 640)
        o_plain, _ = _run(ops.fa3_decode, c, "decode, no sinks", sinks=None)
        o, lse = _run(ops.fa3_decode, c, f"decode W {W}", o_plain=o_plain)
        op, lsep = _run(ops.fa3_decode, c, f"decode paged W {W}", paged=3)
        assert torch.equal(o, op) and torch.equal(lse, lsep)


def test_window_and_sinks_prefill_and_ragged():
    c = window_case("prefill")
    _matter(c)
    o_plain, _ = _run(ops.fa3_prefill_cache, c, "prefill, no sinks", sinks=None)
    o, lse = _run(ops.fa3_prefill_cache, c, "prefill W 128", o_plain=o_plain)
    op, lsep = _run(ops.fa3_prefill_cache, c, "prefill paged W 128", paged=4)
    assert torch.equal(o, op) and torch.equal(lse, lsep)
    c = ragged_case(torch.bfloat16, 64, window=128, H=16, Smax=1024, lens=RAGGED_WIN_LENS)
    _matter(c)
    o, lse = _run(_varlen, c, "ragged W 128", sqs=RAGGED_Q)
    _ragged_equals_uniform(c, o, lse)


# --- 6. split over keys ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,D", DT_D, ids=DT_IDS)
def test_key_splits_with_sinks(dtype, D):
    c = split_case(dtype, D)
    _matter(c)
    o_plain, _ = _run(ops.fa3_prefill_cache, c, "unsplit, no sinks", sinks=None)
    o1, lse1 = _run(ops.fa3_prefill_cache, c, "unsplit", o_plain=o_plain)
    for ks in (1, 2, 3, 8, "auto"):
        o, lse = _run(ops.fa3_prefill_cache, c, f"key_splits {ks}", key_splits=ks)
        if ks == 1:
            assert torch.equal(o, o1) and torch.equal(lse, lse1)
    _run(ops.fa3_prefill_cache, c, "key_splits 3 paged", key_splits=3, paged=4)


# --- 7. shared prefix --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,D", DT_D, ids=DT_IDS)
def test_shared_prefix_with_sinks(dtype, D):
    for Sq, fn, kws in ((1, ops.fa3_decode, ({},)), (70, ops.fa3_prefill_cache, ({}, dict(prefix_key_splits=2)))):
        c = prefix_case(dtype, D, Sq)
        _matter(c)
        for kw in kws:
            _run(fn, c, f"shared_prefix Sq {Sq} {kw}", shared_prefix=c["P"], **kw)


# --- 8. graph replay -----------------------------------------------------------------------------------------------------------------

def test_captured_step_replays_while_sinks_lengths_and_rows_change():
    dev = device()
    B, H, Hkv, Sq, Smax, D, dtype = 3, 8, 2, 2, 1024, 64, torch.bfloat16
    q0, k, v = (t.to(dev) for t in problem(B, H, Hkv, Sq, Smax, D, dtype, seed=8))
    q1, kn1, vn1 = (t.to(dev) for t in problem(B, H, Hkv, Sq, Smax, D, dtype, seed=9))
    q, kc, vc = q0.clone(), k.clone(), v.clone()
    k_new, v_new = kc[:, :, :Sq].clone(), vc[:, :, :Sq].clone()
    lens = i32([300, 2, 900])
    sinks = torch.tensor([-INF, 4.0, 5.0, 6.0, 5.5, 6.5, 7.0, -14.0], device=dev)

    def step():
        return ops.fa3_decode(q, kc, vc, cache_seqlens=lens, k_new=k_new, v_new=v_new, sinks=sinks, return_lse=True)

    graph, (o, lse) = capture(step)
    q.copy_(q1)
    k_new.copy_(kn1[:, :, 5:5 + Sq])
    v_new.copy_(vn1[:, :, 5:5 + Sq])
    lens.copy_(i32([1000, 640, 2]))
    sinks.copy_(torch.tensor([6.0, -INF, 5.0, 7.5, 3.0, 6.5, 6.0, 5.0], device=dev))
    ke, ve = kc.clone(), vc.clone()
    oe, lsee = ops.fa3_decode(q, ke, ve, cache_seqlens=lens, k_new=k_new, v_new=v_new, sinks=sinks, return_lse=True)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(o, oe) and torch.equal(lse, lsee) and torch.equal(kc, ke) and torch.equal(vc, ve)
    ref = with_sink(reference(q, ke, ve, seqlens=lens), sinks)
    check_out(o, ref[0], ref[2], float(ve.abs().max()), dtype, "replay")
    check_lse(o, lse, ref[1], "replay")


# --- 9. refusals on device tensors: nothing is enqueued --------------------------------------------------------------------------------

def test_refusals_enqueue_nothing():
    dev = device()
    q, k, v = (t.to(dev) for t in problem(2, 8, 2, 2, 128, 64, torch.bfloat16, seed=10))
    lens = i32([100, 50])
    sinks = torch.zeros(8, device=dev)
    k_new, v_new = torch.ones_like(k[:, :, :2]), torch.ones_like(v[:, :, :2])
    k8, v8 = k.to(torch.float8_e4m3fn), v.to(torch.float8_e4m3fn)
    ones = torch.ones(2, device=dev)
    for what, match, fn, kc, vc, kw in (
            ("tree_mask", "sinks is not supported with tree_mask", ops.fa3_decode, k, v,
             dict(sinks=sinks, tree_mask=torch.ones(2, 2, dtype=torch.int64, device=dev))),
            ("fp8 decode", "sinks is not supported with an FP8", ops.fa3_decode, k8, v8, dict(sinks=sinks, k_descale=ones, v_descale=ones)),
            ("fp8 prefill", "sinks is not supported with an FP8", ops.fa3_prefill_cache, k8, v8, dict(sinks=sinks, k_descale=ones, v_descale=ones)),
            ("bf16 sinks decode", "sinks must be an fp32", ops.fa3_decode, k, v, dict(sinks=sinks.bfloat16())),
            ("bf16 sinks prefill", "sinks must be an fp32", ops.fa3_prefill_cache, k, v, dict(sinks=sinks.bfloat16()))):
        kc, vc = kc.clone(), vc.clone()
        k0, v0 = kc.clone(), vc.clone()
        out = torch.full((2, 2, 8, 64), 7.0, dtype=torch.bfloat16, device=dev).permute(0, 2, 1, 3)
        with pytest.raises(ValueError, match=match):
            fn(q, kc, vc, cache_seqlens=lens, k_new=k_new, v_new=v_new, out=out, **kw)
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()), what
        assert torch.equal(kc.view(torch.uint8), k0.view(torch.uint8)) and torch.equal(vc.view(torch.uint8), v0.view(torch.uint8)), what
    cu = i32([0, 2, 4])
    with pytest.raises(ValueError, match="sinks must be an fp32"):
        ops.fa3_prefill_varlen(q.permute(0, 2, 1, 3).reshape(4, 8, 64), k, v, cu_seqlens_q=cu, max_seqlen_q=2, cache_seqlens=lens,
                               sinks=sinks.bfloat16())

"""GPU tests of the packed variable-length training path (``ops.fa3_varlen_forward`` / ``fa3_varlen_backward`` /
``fa3_varlen_attention``, ``pfa_fa3_varlen_fwd`` / ``pfa_fa3_varlen_bwd``).

Packed inputs are N(0,1), bf16 and fp16, D 64 and 128, H 4 / Hkv 2 and H = Hkv = 2, causal and full.  Self-attention lengths
``[1, 31, 33, 64, 255, 256, 257, 300, 0, 128]`` sit on every side of the 32-row wave, the 64-key tile, the 128-key block and the 256-row
block and include an empty sequence; the cross-attention case pairs q lengths ``[5, 0, 257, 64]`` with k lengths ``[129, 7, 0, 300]``
(rows with no keys, keys with no rows, causal with more keys than rows).

1. bit equality with the dense kernels per sequence (the main test); 2. the project's existing 16-bit bounds against the fp64
reference of tests/dense_testlib.py; 3. containment in NaN-patterned buffers; 4. independence of the sequences; 5. autograd;
6. graph capture with changing ``cu_seqlens`` contents; 7. the Hugging Face routing.

The bounds are the existing ones, no new numbers: fp32-store forward max-abs <= 1e-3 and LSE <= 2e-3 (tests/test_hip_parity.py);
fp32 gradients <= 1.5e-2 * max|ref| for bf16 and 4e-3 * max|ref| for fp16 (tests/test_hip_backward.py), max|ref| taken over the
gradient tensor of the whole (packed) batch, as that file takes it over its whole batch."""

from __future__ import annotations

import types

import pytest
import torch

from dense_testlib import DEV, GUARD, NAN16, NAN32, reference
from photonic_flash_attention_amd import _capi, ops
from photonic_flash_attention_amd.integration.pytorch import hf

pytestmark = pytest.mark.gpu

INF = float("inf")
SELF = ([1, 31, 33, 64, 255, 256, 257, 300, 0, 128],) * 2
CROSS = ([5, 0, 257, 64], [129, 7, 0, 300])
LAYOUTS = {"self": SELF, "cross": CROSS}
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
CASES = [pytest.param(dt, D, heads, causal, id=f"{dt}-d{D}-h{heads[0]}kv{heads[1]}-{'causal' if causal else 'full'}")
         for dt in DTYPES for D in (64, 128) for heads in ((4, 2), (2, 2)) for causal in (False, True)]


def _cu(lens):
    out = [0]
    for n in lens:
        out.append(out[-1] + n)
    return out


def _randn(shape, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g).to(dtype).to(DEV)


class Problem:
    """Packed N(0,1) operands of one layout on the device, their cu_seqlens, and the keyword arguments of the three ops."""

    def __init__(self, dt, D, heads, layout, seed=11):
        self.dtype, self.D, (self.H, self.Hkv) = DTYPES[dt], D, heads
        self.lq, self.lk = LAYOUTS[layout]
        self.cq, self.ck = _cu(self.lq), _cu(self.lk)
        tq, tk = self.cq[-1], self.ck[-1]
        self.q, self.dout = _randn((tq, self.H, D), seed, self.dtype), _randn((tq, self.H, D), seed + 3, self.dtype)
        self.k, self.v = _randn((tk, self.Hkv, D), seed + 1, self.dtype), _randn((tk, self.Hkv, D), seed + 2, self.dtype)
        self.cu_q = torch.tensor(self.cq, dtype=torch.int32, device=DEV)
        self.cu_k = self.cu_q if layout == "self" else torch.tensor(self.ck, dtype=torch.int32, device=DEV)
        self.kw = dict(cu_seqlens_q=self.cu_q, cu_seqlens_k=self.cu_k, max_seqlen_q=max(self.lq), max_seqlen_k=max(self.lk))

    def seqs(self):
        return [(self.cq[b], self.lq[b], self.ck[b], self.lk[b]) for b in range(len(self.lq))]

    def run(self, causal, q=None, k=None, v=None, dout=None):
        """-> dict: the 16-bit and the fp32 / split-P forward with their LSEs, the 16-bit and the fp32 gradients (behind the 16-bit O)."""
        q, k, v, dout = (x if x is not None else d for x, d in ((q, self.q), (k, self.k), (v, self.v), (dout, self.dout)))
        r = {}
        r["o16"], r["lse16"] = ops.fa3_varlen_forward(q, k, v, causal=causal, return_lse=True, **self.kw)
        r["o32"], r["lse32"] = ops.fa3_varlen_forward(q, k, v, causal=causal, return_lse=True, out_dtype=torch.float32, **self.kw)
        r["g16"] = ops.fa3_varlen_backward(q, k, v, r["o16"], dout, r["lse16"], causal=causal, **self.kw)
        r["g32"] = ops.fa3_varlen_backward(q, k, v, r["o16"], dout, r["lse16"], causal=causal, grad_dtype=torch.float32, **self.kw)
        torch.cuda.synchronize()
        return r


_CACHE = {}


def _solved(dt, D, heads, causal, layout):
    """A problem with its varlen results, computed once per parameter set and shared by the tests that only read them."""
    key = (dt, D, heads, causal, layout)
    if key not in _CACHE:
        p = Problem(dt, D, heads, layout)
        _CACHE[key] = (p, p.run(causal))
    return _CACHE[key]


def _bhsd(t, s, n):
    """rows s .. s + n of a packed [total, heads, D] tensor as the dense calls' [1, heads, n, D] view"""
    return t[s:s + n].transpose(0, 1)[None]


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


# --- 1. bit equality with the dense kernels -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["self", "cross"])
@pytest.mark.parametrize("dt,D,heads,causal", CASES)
def test_bits_are_those_of_the_dense_kernels_per_sequence(dt, D, heads, causal, layout):
    p, r = _solved(dt, D, heads, causal, layout)
    compared = 0
    for sq, nq, sk, nk in p.seqs():
        o16, o32 = r["o16"][sq:sq + nq], r["o32"][sq:sq + nq]
        l16, l32 = r["lse16"][:, sq:sq + nq], r["lse32"][:, sq:sq + nq]
        if nq == 0 or nk == 0:                 # the dense call rejects S = 0: the exact values directly
            for o, l in ((o16, l16), (o32, l32)):
                assert bool((o == 0).all()) and bool((l == -INF).all()), (sq, nq, nk)
            for dq, dk, dv in (r["g16"], r["g32"]):
                assert bool((dq[sq:sq + nq] == 0).all()) and bool((dk[sk:sk + nk] == 0).all()) and bool((dv[sk:sk + nk] == 0).all()), (sq, nq, nk)
            continue
        qb, kb, vb, gb = _bhsd(p.q, sq, nq), _bhsd(p.k, sk, nk), _bhsd(p.v, sk, nk), _bhsd(p.dout, sq, nq)
        d16, dl16 = ops.fa3_forward(qb, kb, vb, causal=causal, _variant=44, return_lse=True)
        d32, dl32 = ops.fa3_forward(qb, kb, vb, causal=causal, _variant=44, return_lse=True, out_dtype=torch.float32)
        assert torch.equal(_bits(o16), _bits(d16[0].transpose(0, 1))) and torch.equal(l16, dl16[0]), ("o16", sq, nq, nk)
        assert torch.equal(_bits(o32), _bits(d32[0].transpose(0, 1))) and torch.equal(l32, dl32[0]), ("o32", sq, nq, nk)
        for name, gdt in (("g16", None), ("g32", torch.float32)):
            dense = ops.fa3_backward(qb, kb, vb, d16, gb, dl16, causal=causal, grad_dtype=gdt)
            for what, got, want, s, n in zip(("dq", "dk", "dv"), r[name], dense, (sq, sk, sk), (nq, nk, nk)):
                assert torch.equal(_bits(got[s:s + n]), _bits(want[0].transpose(0, 1))), (name, what, sq, nq, nk)
        if causal and nk > nq:                 # keys no row sees: exact zeros
            assert bool((r["g32"][1][sk + nq:sk + nk] == 0).all()) and bool((r["g32"][2][sk + nq:sk + nk] == 0).all())
        compared += 1
    assert compared == sum(1 for a, b in zip(p.lq, p.lk) if a and b)


# --- 2. against fp64 ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["self", "cross"])
@pytest.mark.parametrize("dt,D,heads,causal", CASES)
def test_fp32_store_forward_and_gradients_against_fp64(dt, D, heads, causal, layout):
    p, r = _solved(dt, D, heads, causal, layout)
    q, k, v, dout = (t.cpu() for t in (p.q, p.k, p.v, p.dout))
    ref = [torch.zeros(t.shape, dtype=torch.float64) for t in (q, k, v)]
    eo = el = 0.0
    for sq, nq, sk, nk in p.seqs():
        if nq == 0 or nk == 0:
            continue                           # (their exact values: the bit-equality test)
        ro, rl, rdq, rdk, rdv = reference(_bhsd(q, sq, nq), _bhsd(k, sk, nk), _bhsd(v, sk, nk), causal=causal, dout=_bhsd(dout, sq, nq))
        eo = max(eo, float((_bhsd(r["o32"].cpu(), sq, nq).double() - ro).abs().max()))
        el = max(el, float((r["lse32"].cpu()[None, :, sq:sq + nq].double() - rl).abs().max()))
        for dst, src, s, n in ((ref[0], rdq, sq, nq), (ref[1], rdk, sk, nk), (ref[2], rdv, sk, nk)):
            dst[s:s + n] = src[0].transpose(0, 1)
    print(f"o32 max-abs {eo:.3e} (bound 1e-3), lse {el:.3e} (bound 2e-3)")
    assert eo <= 1e-3 and el <= 2e-3, (eo, el)
    tol = 1.5e-2 if dt == "bf16" else 4e-3
    for name, got, rg in zip(("dq", "dk", "dv"), r["g32"], ref):
        got = got.cpu()
        assert bool(torch.isfinite(got).all()), name
        err, scale = float((got.double() - rg).abs().max()), float(rg.abs().max())
        print(f"{name}: max-abs {err:.3e} (bound {tol * scale:.3e}, max |ref| {scale:.3e})")
        assert err <= tol * scale, (name, err, scale)


# --- 3. containment -----------------------------------------------------------------------------------------------------------------

# A sequence 7 rows longer than max_seqlen leaves its last 7 rows uncovered: the gap between it and the next sequence that a
# well-formed (non-decreasing) cu can hold.  9 rows behind cu[B] belong to nobody.
C_LENS, C_MAX, C_TAIL = [257, 64, 307, 0, 31], 300, 9


def _guarded_rows(total, heads, D, dtype):
    """[32 + total + 32, heads, D + 8] filled with a NaN pattern -> (the [total, heads, D] window at row 32, the integer view, pattern)"""
    idt, pat = (torch.int32, NAN32) if dtype == torch.float32 else (torch.int16, NAN16)
    ibuf = torch.full((GUARD + total + GUARD, heads, D + 8), pat, dtype=idt, device=DEV)
    return ibuf.view(dtype)[GUARD:GUARD + total, :, :D], ibuf, pat


def _check_rows(ibuf, pat, covered, D, what):
    i = ibuf.cpu()
    inside = torch.zeros(i.shape, dtype=torch.bool)
    inside[GUARD:GUARD + covered.numel(), :, :D] = covered[:, None, None]
    hit, left = (i != pat) & ~inside, (i == pat) & inside
    assert not bool(hit.any()), f"{what}: {int(hit.sum())} elements outside the covered rows overwritten, the first at {tuple(int(x) for x in torch.nonzero(hit)[0])}"
    assert not bool(left.any()), f"{what}: {int(left.sum())} covered elements never written, the first at {tuple(int(x) for x in torch.nonzero(left)[0])}"


@pytest.mark.parametrize("store32", [False, True], ids=["store16", "store32"])
@pytest.mark.parametrize("dt,D,heads,causal", CASES)
def test_nothing_outside_the_covered_rows_is_written(dt, D, heads, causal, store32):
    dtype, (H, Hkv) = DTYPES[dt], heads
    cu = _cu(C_LENS)
    total = cu[-1] + C_TAIL
    covered = torch.zeros(total, dtype=torch.bool)
    for b, n in enumerate(C_LENS):
        covered[cu[b]:cu[b] + min(n, C_MAX)] = True
    q, dout = _randn((total, H, D), 21, dtype), _randn((total, H, D), 24, dtype)
    k, v = _randn((total, Hkv, D), 22, dtype), _randn((total, Hkv, D), 23, dtype)
    cu_t = torch.tensor(cu, dtype=torch.int32, device=DEV)
    geo = ops._varlen_operands("test", q, k, v, cu_t, cu_t, C_MAX, C_MAX)
    sdt = torch.float32 if store32 else dtype
    o, o_i, o_pat = _guarded_rows(total, H, D, sdt)
    lse_i = torch.full((GUARD + H * total + GUARD,), NAN32, dtype=torch.int32, device=DEV)
    lse = lse_i.view(torch.float32)[GUARD:GUARD + H * total].view(H, total)
    ops._varlen_fwd_launch(q, k, v, o, lse, cu_t, cu_t, geo, causal, None)
    torch.cuda.synchronize()
    _check_rows(o_i, o_pat, covered, D, "o")
    li = lse_i.cpu()
    in_lse = torch.zeros(li.shape, dtype=torch.bool)
    in_lse[GUARD:GUARD + H * total] = covered.repeat(H)
    assert not bool(((li != NAN32) & ~in_lse).any()) and not bool(((li == NAN32) & in_lse).any()), "lse"
    # the backward behind a clean 16-bit forward of the same problem (uncovered rows of o / lse hold what torch.empty left: never read)
    o16, lse16 = ops.fa3_varlen_forward(q, k, v, cu_seqlens_q=cu_t, cu_seqlens_k=cu_t, max_seqlen_q=C_MAX, max_seqlen_k=C_MAX, causal=causal,
                                        return_lse=True)
    o16[~covered.to(DEV)] = float("nan")
    lse16[:, ~covered.to(DEV)] = float("nan")
    (dq, dq_i, pat), (dk, dk_i, _), (dv, dv_i, _) = (_guarded_rows(total, h, D, sdt) for h in (H, Hkv, Hkv))
    ops._varlen_bwd_launch(q, k, v, o16, dout, lse16, dq, dk, dv, cu_t, cu_t, geo, causal, None)
    torch.cuda.synchronize()
    for name, ibuf in (("dq", dq_i), ("dk", dk_i), ("dv", dv_i)):
        _check_rows(ibuf, pat, covered, D, name)
    assert bool(torch.isfinite(dq[covered.to(DEV)].float()).all()) and bool(torch.isfinite(dk[covered.to(DEV)].float()).all())


# --- 4. independence ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt,D,heads,causal", CASES)
def test_a_poisoned_sequence_changes_no_other_sequence(dt, D, heads, causal):
    p, r = _solved(dt, D, heads, causal, "self")
    victim = 5                                                       # the 256-row sequence, in the middle of the packed tensors
    s, n = p.cq[victim], p.lq[victim]
    q, k, v, dout = (t.clone() for t in (p.q, p.k, p.v, p.dout))
    for t in (q, k, v, dout):
        t[s:s + n] = float("nan")
    r2 = p.run(causal, q, k, v, dout)
    others = torch.ones(p.cq[-1], dtype=torch.bool, device=DEV)
    others[s:s + n] = False
    for name in ("o16", "o32"):
        assert torch.equal(_bits(r[name][others]), _bits(r2[name][others])), name
        assert bool(torch.isnan(r2[name][s:s + n].float()).all()), name          # (the victim itself did run)
    for name in ("lse16", "lse32"):
        assert torch.equal(_bits(r[name][:, others]), _bits(r2[name][:, others])), name
    for name in ("g16", "g32"):
        for what, a, b in zip(("dq", "dk", "dv"), r[name], r2[name]):
            assert torch.equal(_bits(a[others]), _bits(b[others])), (name, what)


# --- 5. autograd --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt,D,heads,causal", CASES)
def test_autograd_equals_the_two_ops_by_hand(dt, D, heads, causal):
    p, r = _solved(dt, D, heads, causal, "self")
    q, k, v = (t.clone().requires_grad_(True) for t in (p.q, p.k, p.v))
    out = ops.fa3_varlen_attention(q, k, v, p.cu_q, p.cu_k, max(p.lq), max(p.lk), 0.0, None, causal)
    assert torch.equal(_bits(out.detach()), _bits(r["o16"]))
    out.float().square().sum().backward()
    dout = (2.0 * r["o16"].float()).to(p.dtype)
    hand = ops.fa3_varlen_backward(p.q, p.k, p.v, r["o16"], dout, r["lse16"], causal=causal, **p.kw)
    for what, g, h in zip(("dq", "dk", "dv"), (q.grad, k.grad, v.grad), hand):
        assert torch.equal(_bits(g), _bits(h)), what
    # a dout that is a non-contiguous view (offset by 8 bytes, rows D + 8 apart) is copied, as fa3_backward copies it
    wide = torch.zeros((p.cq[-1], p.H, D + 8), dtype=p.dtype, device=DEV)
    view = wide[:, :, 4:4 + D]
    view.copy_(p.dout)
    assert not view.is_contiguous() and view.data_ptr() % 16 != 0
    for what, a, b in zip(("dq", "dk", "dv"), ops.fa3_varlen_backward(p.q, p.k, p.v, r["o16"], view, r["lse16"], causal=causal, **p.kw), r["g16"]):
        assert torch.equal(_bits(a), _bits(b)), what
    q2, k2, v2 = (t.clone().requires_grad_(True) for t in (p.q, p.k, p.v))
    ops.fa3_varlen_attention(q2, k2, v2, p.cu_q, p.cu_k, max(p.lq), max(p.lk), 0.0, None, causal).backward(view)
    for what, g, b in zip(("dq", "dk", "dv"), (q2.grad, k2.grad, v2.grad), r["g16"]):
        assert torch.equal(_bits(g), _bits(b)), what


# --- 6. graph capture ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt,D,heads,causal", CASES)
def test_a_captured_graph_replays_while_cu_seqlens_change(dt, D, heads, causal):
    dtype, (H, Hkv) = DTYPES[dt], heads
    total, max_len = 700, 300
    q, dout = _randn((total, H, D), 31, dtype), _randn((total, H, D), 34, dtype)
    k, v = _randn((total, Hkv, D), 32, dtype), _randn((total, Hkv, D), 33, dtype)
    cu = torch.zeros(5, dtype=torch.int32, device=DEV)
    kw = dict(cu_seqlens_q=cu, cu_seqlens_k=cu, max_seqlen_q=max_len, max_seqlen_k=max_len, causal=causal)

    def step():
        o, lse = ops.fa3_varlen_forward(q, k, v, return_lse=True, **kw)
        return (o, lse) + tuple(ops.fa3_varlen_backward(q, k, v, o, dout, lse, **kw))

    contents = ([0, 300, 300, 443, 700], [0, 1, 258, 400, 700])
    cu.copy_(torch.tensor(contents[0], dtype=torch.int32))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                       # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for c in contents[::-1] + contents:
        cu.copy_(torch.tensor(c, dtype=torch.int32))
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in captured]
        eager = step()
        torch.cuda.synchronize()
        covered = torch.zeros(total, dtype=torch.bool, device=DEV)
        for b in range(4):
            covered[c[b]:c[b] + min(c[b + 1] - c[b], max_len)] = True
        assert bool(covered.all())
        for name, a, b in zip(("o", "lse", "dq", "dk", "dv"), got, eager):
            assert torch.equal(_bits(a), _bits(b)), (name, c)


# --- 7. Hugging Face routing --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt,D,heads,causal", CASES)
def test_hf_attention_routes_packed_batches_to_the_varlen_path(dt, D, heads, causal):
    p, r = _solved(dt, D, heads, causal, "self")
    module = types.SimpleNamespace(is_causal=True, training=True)
    query, key, value = (t.transpose(0, 1)[None] for t in (p.q, p.k, p.v))          # [1, H(kv), total, D]
    packed = dict(cu_seq_lens_q=p.cu_q, cu_seq_lens_k=p.cu_k, max_length_q=max(p.lq), max_length_k=max(p.lk))
    out, weights = hf.pfa_attention_forward(module, query, key, value, None, is_causal=causal, **packed)
    assert weights is None and out.shape == (1, p.cq[-1], p.H, D)
    assert torch.equal(_bits(out[0]), _bits(r["o16"]))
    # differentiable, through the packed backward
    qr = query.clone().requires_grad_(True)
    o2, _ = hf.pfa_attention_forward(module, qr, key, value, None, is_causal=causal, **packed)
    o2.backward(p.dout[None])
    assert torch.equal(_bits(qr.grad[0].transpose(0, 1).contiguous()), _bits(r["g16"][0]))
    # without the kwargs: today's path -- one dense sequence of `total` rows, whatever kernel the library picks for it
    dense, _ = hf.pfa_attention_forward(module, query, key, value, None, is_causal=causal)
    want = ops.fa3_attention(query, key, value, causal=causal)
    assert torch.equal(_bits(dense), _bits(want.transpose(1, 2)))
    name = _capi.describe(ops.build_args(query, key, value, want, causal=causal)[0])[0]
    assert name.startswith("fa3_fwd_") and "varlen" not in name
    assert not torch.equal(_bits(dense[0]), _bits(out[0]))                       # the documents attended to one another there
    # a mask, a batch of 2 or a max_length that is no host int keep today's path as well
    for kwargs in (dict(packed, max_length_q=torch.tensor(max(p.lq))), dict(packed, cu_seq_lens_k=None)):
        o3, _ = hf.pfa_attention_forward(module, query, key, value, None, is_causal=causal, **kwargs)
        assert torch.equal(_bits(o3), _bits(dense))

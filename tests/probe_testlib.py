"""Exact visibility probes: inputs on which attention's answer is a COUNT of the keys a row sees.  Plain functions and constants; pytest
collects nothing from here, and tests/test_probe_testlib.py tests it on the CPU with a stand-in kernel and its mutants.  The
counterpart of tests/kvcache_testlib.py and tests/dense_testlib.py, whose random-data bounds measure arithmetic and see one wrong
key among n only as a change of about ``|v| / n`` in O and ``1 / n`` in the LSE.

Two probes, for ``q [B,H,Sq,D]`` over ``k/v [B,Hkv,S,D]``:

  ``count``   q = 0: every score is exactly 0, every weight exactly 1.0 (in bf16, fp16 and fp32 alike), so with V of 0 and 1 every
              value a kernel forms is an integer below 2^24 -- in any summation order, any split, any merge.  ``L`` is the number n
              of visible keys, ``O[d] * n`` the number of visible keys with a 1 in column d, ``LSE = ln n``.
  ``stair``   q = e_0, ``K[..., 0]`` = small integers ("steps"), ``softmax_scale = ln 2``: ``float32(ln 2) * float32(log2 e)`` is
              exactly 1.0f, so every score is an integer in log2 units, every weight a power of two, and the running maximum jumps
              exactly where the test puts a step.  ``stair`` asserts ``2^(max step - min step) * keys < 2^24``: every fp32 sum is
              again exact in any order, and so is every partial ``(m, l, O)`` of a wave or a split.

In both, the columns of K that q zeroes hold N(0,1) draws (finite, so 0 * k = 0), and ``kvcache_testlib.guard``'s NaN goes wherever a
kernel promises not to read: that rule is unchanged.

``probe_v`` is the V operand.  Columns 0..15 hold bit t of the logical key index j, columns 16..31 its complement, column 32 the
constant 1 (so ``O[32]`` must be 1: the normalisation), columns 33..40 the bits of ``b * Hkv + hkv`` (a page or a head taken from
another sequence shows), column 41 a 1 exactly on the keys that no row of their sequence and K/V head sees (the expected count there is
0); the rest is 0.  A count vector that is off by one key is off by that key's bit pattern: ``check_probe`` then names the key and
whether it is missing or extra.

``cache_visible`` / ``dense_visible`` return bool ``[B,H,Sq,S]`` from integer rules spelled as index ranges, independently of
``kvcache_testlib.reference`` / ``tree_visible`` and ``dense_testlib.visible``, against which tests/test_probe_testlib.py pins them.
``expected`` works in float64, which is exact for these integers.

The tolerances of ``check_probe`` (u = 2^-24, the unit roundoff of fp32), derived and not measured:

  fp32 O      ``|o - ref| <= 16 u |ref|``.  Every sum is exact, so the only roundings are the final ones; the longest path (a split
              prefill with a sink through ``pfa_attn_merge``) has about ten: an exp2, a product and a division for the sink, then
              two exps, two products, an add, a division and a log in the merge.  One key changes O by at least
              ``1 / (max weight * n)`` relative: 16 x the tolerance at n = 65536 with max weight 1.
  16-bit O    ``|o - ref| <= half_ulp16(ref) (1 + 2^-10) + 16 u |ref|``: the fp32 value is known to 16 u, so a store that rounds to
              nearest lands within half a unit in the last place of the 16-bit format AT ref; a store that truncates misses by up to
              a whole one.  The half ulp is computed from ref's binade (8 significant bits for bf16, 11 for fp16, fp16 subnormals
              2^-24 apart), not as ``kvcache_testlib.EPS * |ref|``: ``EPS[bf16]`` is 2^-9, HALF the unit roundoff of bf16 (2^-8), and
              a correctly rounded store of 257/512 (-> 0.5) is 2^-8 |ref| away; for fp16 ``EPS`` is the unit roundoff and the half
              ulp is never above ``EPS |ref|``.  tests/test_probe_testlib.py pins both facts.
  merged O    ``|o - ref| <= (16 + 8 A) u |ref|`` (plus the half ulp) with ``A = max(1, |ref_lse|, ln 2 max|step|)`` for a result that went
              through ``pfa_attn_merge`` (``merged=True``: a prefill split over keys, a shared-prefix step).  The parts reach the merge
              as NATURAL-LOG LSEs in fp32, and a rounding of a value of size |lse| is an ABSOLUTE error of up to u |lse|: a part's
              ``lse = (M + log2 l) ln 2`` carries the log2's, the sum's and the product's, and the merge's ``exp(lse - m)`` one more in
              the subtraction or the exponent's scaling -- 4 u A at the most, where no part's |lse| exceeds A because a part's keys
              are a subset of the row's.  ``exp`` turns an absolute error of its argument into the same RELATIVE error of the weight,
              and ``O = sum w_n O_n / sum w_n`` moves by at most twice the largest of them: 8 u A.  The 16 u above count each of these
              roundings as one u; at |lse| = ln 2^15 that is short by a factor of 10, and the fp32 stand-in of
              tests/test_probe_testlib.py (``_attn_merge_model``, the specification itself) shows it.  At the largest merged problem
              of the suite (4096 keys, A = 8.3) the tolerance is 83 u = 4.9e-6 against 1 / n = 2.4e-4 for one key.
  LSE         ``|lse - ref| <= 8 u max(1, |ref|)``: at most 5.4e-6 at ln 65536, where ``ln n - ln(n - 1)`` is at least 1.5e-5.

and, as equalities: every output finite; on rows that see no key O exactly 0 and the LSE exactly -inf (with a sink: the sink); in
``count`` mode with an fp32 output ``round(o * L) == C`` per column and, for any output, ``round(exp(lse)) == L``.

A sink (``sinks [H]``, natural-log units) of 0.0 adds ``2^-M`` to ``L``, one of -inf nothing; a row with no key and a sink has O = 0
and LSE = sink."""

from __future__ import annotations

import math

import torch

from kvcache_testlib import INF

U = 2.0 ** -24
LN2 = math.log(2.0)
LOG2E = 1.4426950408889634
BITS = 16                                   # columns 0 .. 15: the key's bits; 16 .. 31: their complement
COL_ONE, COL_SEQ, SEQ_BITS, COL_UNSEEN = 32, 33, 8, 41
O_ULPS, LSE_ULPS, MERGE_ULPS = 16, 8, 8      # the tolerances, in units of u (MERGE_ULPS: per unit of |lse|, merged results only)


# --- the operands ----------------------------------------------------------------------------------------------------------------------

def probe_v(B, Hkv, S, D, dtype=torch.float32, unseen=None):
    """V ``[B,Hkv,S,D]`` of 0 and 1 (module docstring).  unseen: bool ``[B,Hkv,S]`` (``unseen_keys``) for column 41, or None (zeros).
    For an e4m3 cache make it fp32 and take ``kvcache_testlib.quant(v, ones)``: the codes of 0.0 and 1.0."""
    assert D in (64, 128) and S <= 1 << BITS and B * Hkv <= 1 << SEQ_BITS
    j = torch.arange(S)
    bits = ((j[:, None] >> torch.arange(BITS)[None, :]) & 1).to(torch.float32)                      # [S, 16]
    v = torch.zeros(B, Hkv, S, D, dtype=torch.float32)
    v[..., :BITS] = bits
    v[..., BITS:2 * BITS] = 1.0 - bits
    v[..., COL_ONE] = 1.0
    seq = torch.arange(B * Hkv).reshape(B, Hkv)
    v[..., COL_SEQ:COL_SEQ + SEQ_BITS] = ((seq[..., None] >> torch.arange(SEQ_BITS)) & 1).to(torch.float32)[:, :, None, :]
    if unseen is not None:
        v[..., COL_UNSEEN] = unseen.to(torch.float32)
    return v.to(dtype)


def unseen_keys(vis, Hkv):
    """``vis [B,H,Sq,S]`` -> bool ``[B,Hkv,S]``: the keys no row of any query head of their K/V head sees."""
    B, H, _, S = vis.shape
    return ~vis.any(dim=2).reshape(B, Hkv, H // Hkv, S).any(dim=2)


def _q(B, H, Sq, D, dtype, col0):
    q = torch.zeros(B, Sq, H, D, dtype=dtype)
    q[..., 0] = col0
    return q.permute(0, 2, 1, 3)                                   # the [B,H,Sq,D] view of a [B,Sq,H,D] buffer the calls return


def count(B, H, Hkv, Sq, S, D, dtype, seed=0):
    """-> dict(q, k, steps=None, scale=None): q = 0, K all N(0,1) draws.  Any softmax scale gives the same result."""
    g = torch.Generator().manual_seed(9100 + seed)
    return dict(q=_q(B, H, Sq, D, dtype, 0.0), k=torch.randn(B, Hkv, S, D, generator=g).to(dtype), steps=None, scale=None)


def stair(B, H, Hkv, Sq, S, D, dtype, steps, seed=0):
    """-> dict(q, k, steps [B,Hkv,S] int64, scale = ln 2): q = e_0, ``K[..., 0] = steps``.  steps: one ``{key: height}`` for every
    sequence or a list of one per sequence; the other keys stand at height 0.  Heights are integers (exact in every format from
    e4m3 up for |h| <= 16)."""
    g = torch.Generator().manual_seed(9200 + seed)
    st = torch.zeros(B, Hkv, S, dtype=torch.int64)
    for b, marks in enumerate([steps] * B if isinstance(steps, dict) else steps):
        for j, h in marks.items():
            assert 0 <= j < S and int(h) == h and abs(h) <= 16
            st[b, :, j] = int(h)
    span = int(st.max() - st.min())
    assert 2 ** span * S < 2 ** 24, f"steps span 2^{span} over {S} keys: an fp32 sum of these weights is no longer exact in any order"
    k = torch.randn(B, Hkv, S, D, generator=g).to(dtype)
    k[..., 0] = st.to(dtype)
    return dict(q=_q(B, H, Sq, D, dtype, 1.0), k=k, steps=st, scale=LN2)


# --- who sees whom: integer rules as index ranges ----------------------------------------------------------------------------------------

def cache_visible(B, H, Sq, S, lens=None, *, causal=True, window=None, key_mask=None, tree=None):
    """The rule of the calls over a KV cache -> bool ``[B,H,Sq,S]``.  lens: a list (None: S each), clamped to 0 .. S.  Bottom-right
    causal per sequence: row i sees keys ``[max(0, d - W), d)`` with ``d = min(len, len - Sq + i + 1)``.  tree: int64 words ``[B,Sq]``
    (a list or a tensor) that replace the triangle over the step's own keys ``len - Sq ..``: bit t of row i's word shows key
    ``len - Sq + t``.  key_mask: ``[B,S]``, AND."""
    vis = torch.zeros(B, H, Sq, S, dtype=torch.bool)
    words = None if tree is None else torch.as_tensor(tree).tolist()
    for b in range(B):
        n = S if lens is None else min(max(int(lens[b]), 0), S)
        off = n - Sq
        for i in range(Sq):
            if words is not None:
                vis[b, :, i, :max(0, min(off, n))] = True
                w = words[b][i] & ((1 << 64) - 1)
                for t in range(min(Sq, 64)):
                    if (w >> t) & 1 and 0 <= off + t < n:
                        vis[b, :, i, off + t] = True
                continue
            hi = min(n, off + i + 1) if causal else n
            lo = 0 if window is None else max(0, off + i + 1 - window)
            if hi > lo:
                vis[b, :, i, lo:hi] = True
    if key_mask is not None:
        vis &= torch.as_tensor(key_mask).cpu().bool()[:, None, None, :]
    return vis


def dense_visible(B, H, Sq, Sk, *, causal=False, seqlens=None, key_mask=None, mask=None):
    """The rule of the dense calls -> bool ``[B,H,Sq,Sk]``: top-left causal (row i sees keys ``[0, i]``), ``seqlens`` clamped to
    0 .. Sk, a ``[B,Sk]`` key mask, and a 3-D ``[B,Sq|1,Sk]`` or 4-D ``[B|1,H|1,Sq|1,Sk]`` element mask (0 = hidden), all AND."""
    vis = torch.zeros(B, H, Sq, Sk, dtype=torch.bool)
    for b in range(B):
        n = Sk if seqlens is None else min(max(int(seqlens[b]), 0), Sk)
        if not causal:
            vis[b, :, :, :n] = True
            continue
        for i in range(Sq):
            vis[b, :, i, :min(n, i + 1)] = True
    if key_mask is not None:
        vis &= torch.as_tensor(key_mask).cpu().bool()[:, None, None, :]
    if mask is not None:
        m = torch.as_tensor(mask).cpu() != 0
        vis &= m[:, None] if m.dim() == 3 else m
    return vis


# --- the expected result, in float64 ---------------------------------------------------------------------------------------------------

def expected(vis, v, steps=None, sinks=None, v_scale=None):
    """``vis [B,H,Sq,S]``, ``v [B,Hkv,S,D]`` (0 and 1, any float dtype), ``steps [B,Hkv,S]`` or None (all 0), ``sinks [H]`` or None,
    ``v_scale [B,Hkv]``, ``[Hkv]`` or None (an FP8 cache's v_descale: a power of two) -> dict of float64 tensors:
    ``C [B,H,Sq,D]`` the weighted counts, ``L``, ``M [B,H,Sq]`` (M in log2 units, 0 on dead rows; L with the sink), ``n`` the visible
    keys, ``dead`` (no visible key), ``ref_o = v_scale C / L`` and ``ref_lse = (M + log2 L) ln 2``, ``o_mul`` (v_scale per
    head) and ``lse_mag`` -- the A of a merged result's tolerance, ``max(1, |ref_lse|, ln 2 max|step|)``: no part's natural-log LSE is
    larger (module docstring, "merged O")."""
    B, H, Sq, S = vis.shape
    Hkv = v.shape[1]
    g = H // Hkv
    st = torch.zeros(B, Hkv, S, dtype=torch.float64) if steps is None else steps.to(torch.float64)
    sc = st.repeat_interleave(g, dim=1)[:, :, None, :].expand(B, H, Sq, S).masked_fill(~vis, -INF)
    n = vis.sum(-1).to(torch.float64)
    dead = n == 0
    M = torch.where(dead, torch.zeros_like(n), sc.amax(-1))
    w = torch.where(vis, torch.exp2(sc - M[..., None]), torch.zeros((), dtype=torch.float64))
    L = w.sum(-1)
    C = w @ v.to(torch.float64).repeat_interleave(g, dim=1)
    lse = torch.where(dead, torch.full_like(L, -INF), (M + torch.log2(L.clamp_min(2.0 ** -1000))) * LN2)
    if sinks is not None:
        s = sinks.to(torch.float64).view(1, H, 1).expand(B, H, Sq)
        L = torch.where(dead, torch.exp(s), L + torch.exp(s) * torch.exp2(-M))       # a sink of 0.0: exactly 2^-M; of -inf: 0
        lse = torch.where(dead, s, torch.where(torch.isneginf(s), lse, (M + torch.log2(L.clamp_min(2.0 ** -1000))) * LN2))
    mul = torch.ones(B, Hkv, dtype=torch.float64) if v_scale is None else v_scale.to(torch.float64).expand(B, Hkv)
    mul = mul.repeat_interleave(g, dim=1)[:, :, None, None]
    ref_o = torch.where((L > 0)[..., None], mul * C / L.clamp_min(2.0 ** -1000)[..., None], torch.zeros_like(C))
    mag = torch.where(dead, torch.ones_like(lse), lse.abs()).clamp_min(max(1.0, LN2 * float(st.abs().max())))
    return dict(C=C, L=L, M=M, n=n, dead=dead, ref_o=ref_o, ref_lse=lse, o_mul=mul, lse_mag=mag)


# --- the check -------------------------------------------------------------------------------------------------------------------------

def half_ulp16(ref, dtype):
    """Half a unit in the last place of ``dtype`` (bf16 or fp16) at the float64 values ``ref``; 0 at 0."""
    p = 8 if dtype == torch.bfloat16 else 11
    _, e = torch.frexp(ref.abs())                                   # |ref| = m 2^e, m in [0.5, 1): the ulp is 2^(e - p)
    e = e.to(torch.int64) - p
    if dtype == torch.float16:
        e = e.clamp_min(-24)
    return torch.where(ref == 0, torch.zeros_like(ref), torch.ldexp(torch.full_like(ref, 0.5), e))


def _one_key(diff):
    """A count difference over the columns -> (key, "extra" | "missing") if it is exactly one key's bit pattern, else None."""
    for sign, word in ((1.0, "extra"), (-1.0, "missing")):
        d = diff * sign
        bits, comp = d[:BITS], d[BITS:2 * BITS]
        if d[COL_ONE] == 1 and bool(((bits == 0) | (bits == 1)).all()) and bool((bits + comp == 1).all()):
            return int((bits.long() << torch.arange(BITS)).sum()), word
    return None


def check_probe(o, lse, exp, out_dtype, what="", count_mode=False, merged=False):
    """``o [B,H,Sq,D]`` and ``lse [B,H,Sq]`` of a call against ``expected(...)`` (module docstring) -> (largest err / tolerance of O,
    of the LSE).  A failure names ``(b, h, row)`` with the keys expected and found, and in ``count_mode`` the one key at fault if the
    count vector is off by exactly one key's pattern.  merged: the result went through ``pfa_attn_merge``."""
    tag = f"{what}: " if what else ""
    assert o.dtype == out_dtype and lse.dtype == torch.float32, f"{tag}the output is {o.dtype}, the LSE {lse.dtype}"
    o64, l64 = o.detach().cpu().double(), lse.detach().cpu().double()
    ref_o, ref_lse, dead, L = exp["ref_o"], exp["ref_lse"], exp["dead"], exp["L"]
    assert o64.shape == ref_o.shape and l64.shape == ref_lse.shape, f"{tag}shapes {tuple(o64.shape)}, {tuple(l64.shape)}"
    assert bool(torch.isfinite(o64).all()), f"{tag}non-finite output -- a key or a page the call must never read was read"
    assert not bool(torch.isnan(l64).any()), f"{tag}NaN in the LSE"

    def where(idx):
        b, h, i = (int(x) for x in idx)
        found = math.exp(float(l64[b, h, i])) * 2.0 ** -float(exp["M"][b, h, i]) if math.isfinite(float(l64[b, h, i])) else 0.0
        return f"{tag}(b, h, row) = ({b}, {h}, {i}): {float(L[b, h, i]):g} keys expected, {found:.6g} found"

    def first(bad):
        return tuple(torch.nonzero(bad)[0].tolist())

    bad = dead & ((o64 != 0).any(-1) | (l64 != ref_lse))
    assert not bool(bad.any()), f"{where(first(bad))} -- a row with no visible key is not O = 0, LSE = {float(ref_lse[first(bad)])}"
    bad = ~dead & ~torch.isfinite(l64)
    assert not bool(bad.any()), f"{where(first(bad))} -- a row that sees keys has a non-finite LSE"
    live = ~dead

    if count_mode:
        found_L = torch.where(live, torch.exp(l64).round(), L)
        found_C = (o64 / exp["o_mul"] * found_L[..., None]).round() if out_dtype == torch.float32 else None
        bad = found_L != L if found_C is None else (found_L != L) | (found_C != exp["C"]).any(-1)
        if bool(bad.any()):
            at = first(bad)
            key = None if found_C is None else _one_key(found_C[at] - exp["C"][at])
            blame = "" if key is None else f"; key {key[0]} is {key[1]}"
            cols = "" if found_C is None else f"; columns off: {torch.nonzero(found_C[at] != exp['C'][at]).flatten().tolist()[:12]}"
            raise AssertionError(f"{where(at)} -- the counts differ{blame}{cols}")

    tol = (O_ULPS + (MERGE_ULPS * exp["lse_mag"][..., None] if merged else 0.0)) * U * ref_o.abs()
    if out_dtype != torch.float32:
        tol = tol + half_ulp16(ref_o, out_dtype) * (1 + 2.0 ** -10)
    err = (o64 - ref_o).abs()
    ratio = torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, INF), torch.zeros_like(err)))
    ro = float(ratio.max())
    ltol = LSE_ULPS * U * ref_lse.abs().clamp_min(1.0)
    lerr = torch.where(live, (l64 - ref_lse).abs(), torch.zeros_like(l64))
    rl = float((lerr / ltol).max())
    print(f"{tag}O err / tolerance {ro:.3f}, LSE err / tolerance {rl:.3f}")
    if ro > 1:
        at = tuple(int(x) for x in torch.unravel_index(ratio.argmax(), ratio.shape))
        raise AssertionError(f"{where(at[:3])} -- O over the tolerance: column {at[3]} is {float(o64[at])!r}, expected {float(ref_o[at])!r}, "
                             f"err / tolerance {ro:.3g}")
    if rl > 1:
        at = tuple(int(x) for x in torch.unravel_index((lerr / ltol).argmax(), lerr.shape))
        raise AssertionError(f"{where(at)} -- LSE over the tolerance: {float(l64[at])!r}, expected {float(ref_lse[at])!r}, "
                             f"err / tolerance {rl:.3g}")
    return ro, rl

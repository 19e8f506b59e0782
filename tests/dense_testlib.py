"""What the tests of the dense calls (``ops.fa3_forward`` / ``ops.fa3_backward`` on the exact-fp32 kernels, and the attention-weights pass
``pfa_fa3_weights``: the section before the last; the 16-bit backward's per-element bound: the last) share: one fp64 reference, the error bounds, the checks, and the guarded buffers of the containment tests.  Plain functions and constants; pytest collects nothing
from here, and tests/test_dense_testlib.py tests it on the CPU.  The counterpart of tests/kvcache_testlib.py.

The reference is fp64 attention of ``q [B,H,Sq,D]`` over ``k/v [B,Hkv,Sk,D]`` (grouped heads by ``repeat_interleave``, so autograd sums
each group) with the DENSE causal rule of this project -- row i sees key j iff ``j <= i``, aligned top-left; the caches' rule is
bottom-right -- ``seqlens`` clamped to ``0 .. Sk``, and a bool ``keep`` broadcastable to ``[B,H,Sq,Sk]``.  The dropout keep-mask ``drop``
multiplies the NORMALISED weights, scaled by ``drop_scale``: the row sum and the LSE stay un-dropped.  A row that sees no key has
``o = 0``, ``lse = -inf`` and zero gradients.  Gradients come from autograd through the fp64 expression.

The bounds are the fp32 kernels' own (tests/test_hip_modules.py::test_exact_fp32_kernel_against_the_oracle,
tests/test_hip_backward.py::test_fp32_backward_matches_autograd_of_oracle and ::test_dense_branch_dropout_statistics_and_gradients):

    o and finite lse            max-abs 2e-5
    gradients, no dropout       2e-5 * max(1, max|ref|)
    gradients, with dropout     3e-5 * max(1, max|ref|)

and, as equalities: every output finite; ``lse`` -inf on exactly the reference's rows; ``o`` and ``dq`` exactly 0.0 on those rows; ``dk``
and ``dv`` exactly 0.0 for keys that no row of the group sees.

Random operands measure the arithmetic; which keys a row of the dense forward sees (the causal diagonal, ``seqlens_k``, key and element
masks, block and tile edges, on every kernel family) is checked by the exact probes of tests/probe_testlib.py
(tests/test_hip_dense_probes.py), on inputs whose answer is a count of keys.  There an exactly known fp32 value also pins the 16-bit
store to half a unit in the last place: the truncating store that ``backward_bound`` cannot tell from a rounding one."""

from __future__ import annotations

import ctypes as C
import functools

import torch

INF = float("inf")
BOUND_O = 2e-5                 # o and finite lse, max-abs
BOUND_GRAD = 2e-5              # x max(1, max|ref|)
BOUND_GRAD_DROP = 3e-5         # x max(1, max|ref|), with a dropout keep-mask
DEV = "cuda:0"


# --- the fp64 reference --------------------------------------------------------------------------------------------------------------

def visible(B, H, Sq, Sk, *, causal=False, seqlens=None, keep=None):
    """bool [B,H,Sq,Sk]: row i of (b, h) sees key j.  Dropout is no part of it: a dropped key is seen."""
    vis = torch.ones(B, H, Sq, Sk, dtype=torch.bool)
    if causal:
        vis = vis & torch.tril(torch.ones(Sq, Sk, dtype=torch.bool))
    if seqlens is not None:
        L = torch.as_tensor(seqlens).long().cpu().clamp(0, Sk)
        vis = vis & (torch.arange(Sk)[None, :] < L[:, None])[:, None, None, :]
    if keep is not None:
        vis = vis & keep.cpu().bool()
    return vis


def softmax_parts(qd, kd, vis, scale):
    """What ``reference`` and ``weights_reference`` share.  fp64 ``qd [B,H,Sq,D]``, ``kd [B,Hkv,Sk,D]`` and ``vis [B,H,Sq,Sk]`` -> (the
    scaled scores before masking; the normalised weights, zero rows where no key is seen; the detached LSE [B,H,Sq], -inf there)."""
    g = qd.shape[1] // kd.shape[1]
    raw = (qd @ kd.repeat_interleave(g, dim=1).transpose(-1, -2)) * scale
    s = raw.masked_fill(~vis, -INF)
    m = s.detach().amax(-1, keepdim=True)
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    p = torch.exp(s - m)
    l = p.sum(-1, keepdim=True)
    safe = torch.where(l > 0, l, torch.ones_like(l))
    w = p / safe                                                  # the normalised weights: zero rows where no key is seen
    lse = torch.where(l > 0, m + torch.log(safe), torch.full_like(l, -INF))[..., 0].detach()
    return raw, w, lse


def reference(q, k, v, *, causal=False, seqlens=None, keep=None, drop=None, drop_scale=1.0, scale=None, dout=None):
    """fp64 on the CPU -> (o [B,H,Sq,D], lse [B,H,Sq]), and (dq [B,H,Sq,D], dk, dv [B,Hkv,Sk,D]) behind them when ``dout`` is given."""
    B, H, Sq, D = q.shape
    Hkv, Sk = k.shape[1], k.shape[2]
    g = H // Hkv
    assert H == g * Hkv and k.shape == (B, Hkv, Sk, D) and v.shape == (B, Hkv, Sk, D)
    qd, kd, vd = (t.detach().cpu().double().clone().requires_grad_(dout is not None) for t in (q, k, v))
    vis = visible(B, H, Sq, Sk, causal=causal, seqlens=seqlens, keep=keep)
    _, w, lse = softmax_parts(qd, kd, vis, D ** -0.5 if scale is None else scale)
    if drop is not None:
        w = w * (drop.cpu().to(torch.float64) * float(drop_scale))
    o = w @ vd.repeat_interleave(g, dim=1)
    if dout is None:
        return o, lse
    dq, dk, dv = torch.autograd.grad(o, (qd, kd, vd), dout.detach().cpu().double())
    return o.detach(), lse, dq, dk, dv


def seen(vis, Hkv):
    """``visible(...)`` -> (rows that see a key [B,H,Sq], keys that a row of their group sees [B,Hkv,Sk])"""
    B, H, Sq, Sk = vis.shape
    return vis.any(dim=3), vis.any(dim=2).reshape(B, Hkv, H // Hkv, Sk).any(dim=2)


# --- the checks ----------------------------------------------------------------------------------------------------------------------

def check_forward(o, lse, ref_o, ref_lse, what=""):
    """``o`` and ``lse`` of a forward call against the reference's -> (max-abs of o, max-abs of the finite lse)."""
    tag = f"{what}: " if what else ""
    o, lse = o.detach().cpu(), lse.detach().cpu()
    assert o.dtype == torch.float32 and lse.dtype == torch.float32, (o.dtype, lse.dtype)
    assert tuple(o.shape) == tuple(ref_o.shape) and tuple(lse.shape) == tuple(ref_lse.shape), (tuple(o.shape), tuple(lse.shape))
    assert bool(torch.isfinite(o).all()), f"{tag}non-finite output"
    assert not bool(torch.isnan(lse).any()), f"{tag}NaN in the LSE"
    fin = torch.isfinite(ref_lse)
    assert torch.equal(torch.isfinite(lse), fin), f"{tag}the rows with a finite LSE are not the reference's"
    assert bool((lse[~fin] == -INF).all()), f"{tag}a row with no visible key has an LSE other than -inf"
    assert bool((o[~fin] == 0).all()), f"{tag}a row with no visible key is not exactly zero"
    eo = float((o.double() - ref_o).abs().max())
    el = float((lse.double() - ref_lse)[fin].abs().max()) if bool(fin.any()) else 0.0
    print(f"{tag}o max-abs {eo:.3e}, lse max-abs {el:.3e} (bound {BOUND_O:.0e})")
    assert eo <= BOUND_O, f"{tag}o max-abs {eo:.3e} > {BOUND_O:.0e}"
    assert el <= BOUND_O, f"{tag}lse max-abs {el:.3e} > {BOUND_O:.0e}"
    return eo, el


def check_grads(grads, ref, row_seen, key_seen, what="", dropout=False):
    """(dq, dk, dv) against the reference's, with the rows / keys that are seen (``seen``) -> the largest error relative to its bound's
    scale ``max(1, max|ref|)``."""
    tag = f"{what}: " if what else ""
    rel = BOUND_GRAD_DROP if dropout else BOUND_GRAD
    worst = 0.0
    for name, got, r, live in zip(("dq", "dk", "dv"), grads, ref, (row_seen, key_seen, key_seen)):
        got = got.detach().cpu()
        assert got.dtype == torch.float32 and tuple(got.shape) == tuple(r.shape), (name, got.dtype, tuple(got.shape), tuple(r.shape))
        assert bool(torch.isfinite(got).all()), f"{tag}{name} not finite"
        unseen = got[~live]
        assert unseen.numel() == 0 or bool((unseen == 0).all()), f"{tag}{name} of rows / keys nothing sees is not exactly zero"
        err, scale = float((got.double() - r).abs().max()), max(1.0, float(r.abs().max()))
        print(f"{tag}{name} max-abs {err:.3e} (bound {rel * scale:.3e}, max |ref| {float(r.abs().max()):.3e})")
        assert err <= rel * scale, f"{tag}{name} max-abs {err:.3e} > {rel * scale:.3e}"
        worst = max(worst, err / scale)
    return worst


# --- containment: gradients written into guarded buffers through the C ABI ----------------------------------------------------------

NAN16, NAN32 = 0x7FC1, 0x7FC00001                  # NaN in bf16 and in fp16; NaN in fp32
GUARD = 32                                         # rows of one wave: a whole stray wave still lands inside the test's buffer


def guarded(B, S, H, D, gdt, pad=8):
    """[B, 32 + S + 32, H, D + pad] filled with a NaN pattern -> (buffer, its integer view, the pattern)"""
    idt, pat = (torch.int32, NAN32) if gdt == torch.float32 else (torch.int16, NAN16)
    ibuf = torch.full((B, GUARD + S + GUARD, H, D + pad), pat, dtype=idt, device=DEV)
    return ibuf.view(gdt), ibuf, pat


def bwd_into(q, k, v, out, dout, lse, causal, gdt, bufs):
    """pfa_fa3_bwd writing dq, dk, dv at element [0, 32, 0, 0] of the three guarded buffers, with the buffers' strides.  16-bit
    operands: gradient rows leave in 16-byte pieces (aligned base, strides in multiples of 8); fp32 operands: 4-byte stores, any stride."""
    from photonic_flash_attention_amd import _capi, ops
    B, H, Sq, D = q.shape
    Hkv, Sk = k.shape[1], k.shape[2]
    f32 = q.dtype == torch.float32
    delta = torch.empty((B, H, Sq), dtype=torch.float32, device=q.device)
    a = _capi.PfaFa3BwdArgs()
    a.size = C.sizeof(_capi.PfaFa3BwdArgs)
    for name, t in (("q", q), ("k", k), ("v", v), ("o", out), ("do", dout)):
        setattr(a, "dout" if name == "do" else name, t.data_ptr())
        for ax, s in zip("bhs", t.stride()[:3]):
            setattr(a, f"{name}_stride_{ax}", s)
        assert t.stride(3) == 1
    for name, buf in zip(("dq", "dk", "dv"), bufs):
        inner = buf[:, GUARD:]                    # [B, S + 32, H, D + pad] view: same strides, base at row 32
        assert inner.data_ptr() % 4 == 0 if f32 else (inner.data_ptr() % 16 == 0 and buf.stride(1) % 8 == 0)
        setattr(a, name, inner.data_ptr())
        setattr(a, f"{name}_stride_b", buf.stride(0))
        setattr(a, f"{name}_stride_s", buf.stride(1))
        setattr(a, f"{name}_stride_h", buf.stride(2))
    a.lse, a.delta = lse.data_ptr(), delta.data_ptr()
    a.B, a.H, a.Sq, a.Sk, a.D, a.kv_group = B, H, Sq, Sk, D, H // Hkv
    a.dtype, a.dtype_grad, a.causal = ops._DT[q.dtype], ops._DT[gdt], 1 if causal else 0
    a.softmax_scale = float(D ** -0.5)
    a.device_id = torch.cuda.current_device()
    _capi.check_status(_capi.load().pfa_fa3_bwd(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()


# --- the attention-weights pass (pfa_fa3_weights): reference, a-priori bound, check, guarded call ----------------------------------

LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
U32 = 2.0 ** -24                                   # unit roundoff of fp32
ROUND16 = {torch.bfloat16: (2.0 ** -8, 0.0),       # 16-bit W: (unit roundoff of round-to-nearest, half the subnormal spacing where
           torch.float16: (2.0 ** -11, 2.0 ** -25)}   # subnormals occur: fp16's are 2^-24 apart; bf16 has fp32's exponent range)


def weights_reference(q, k, *, causal=False, seqlens=None, keep=None, scale=None, lse32=None):
    """fp64 on the CPU -> (W [B,H,Sq,Sk], the fp32 LSE [B,H,Sq] it was formed with).  ``W = exp(scale * <q_i, k_j> - lse_i)`` where
    ``visible(...)`` holds and exactly 0 elsewhere; grouped heads by ``repeat_interleave``.  ``lse32=None``: the fp64 LSE rounded to
    fp32, returned so that the kernel under test is handed the same values.  ``lse32`` given (a forward kernel's own output): used as
    it is, which keeps the forward's error out of a check of the weights pass.  Rows whose LSE is -inf are all zero."""
    B, H, Sq, D = q.shape
    Hkv, Sk = k.shape[1], k.shape[2]
    assert H % Hkv == 0 and k.shape == (B, Hkv, Sk, D)
    qd, kd = q.detach().cpu().double(), k.detach().cpu().double()
    vis = visible(B, H, Sq, Sk, causal=causal, seqlens=seqlens, keep=keep)
    raw, _, lse = softmax_parts(qd, kd, vis, D ** -0.5 if scale is None else scale)
    lse32 = lse.float() if lse32 is None else lse32.detach().cpu().float()
    assert tuple(lse32.shape) == (B, H, Sq)
    live = vis & torch.isfinite(lse32)[..., None]
    e = raw - torch.where(torch.isfinite(lse32), lse32.double(), torch.zeros((), dtype=torch.float64))[..., None]
    return torch.where(live, torch.exp(e), torch.zeros((), dtype=torch.float64)), lse32


def weights_bound(q, k, ref, lse32, *, scale=None, wdt=torch.float32):
    """The per-element a-priori error bound of a W that the kernel's arithmetic computes for ``ref`` -- fp32 MFMA accumulation of the D
    exact 16-bit products (two roundings a step), ``fma(s, c, -lse * log2e)`` with its three fp32 roundings, ``v_exp_f32``, and for a
    16-bit W the store's round-to-nearest.  With u = 2^-24, c = scale * log2(e), A_ij = sum_d |q_id k_jd|, L_i = |lse_i * log2(e)|:

        bound32 = W * (ln2 * (2 D u c A + 4 u (|c s| + L)) + 2 u)          bound16 = bound32 * (1 + h) + W * h + t

    Derived from the arithmetic, never from what a kernel returned.  Zero where ``ref`` is zero: those elements must be exact."""
    B, H, Sq, D = q.shape
    g = H // k.shape[1]
    c = (D ** -0.5 if scale is None else scale) * LOG2E
    qd, kd = q.detach().cpu().double(), k.detach().cpu().double().repeat_interleave(g, dim=1)
    s = qd @ kd.transpose(-1, -2)
    A = qd.abs() @ kd.abs().transpose(-1, -2)
    L = torch.where(torch.isfinite(lse32), lse32.double() * LOG2E, torch.zeros((), dtype=torch.float64)).abs()[..., None]
    b32 = ref * (LN2 * (2 * D * U32 * c * A + 4 * U32 * ((c * s).abs() + L)) + 2 * U32)
    if wdt == torch.float32:
        return b32
    h, t = ROUND16[wdt]
    return torch.where(ref > 0, b32 * (1 + h) + ref * h + t, torch.zeros((), dtype=torch.float64))


def check_weights(w, ref, bound, vis, what="", wdt=None):
    """A weights tensor against ``weights_reference`` within ``weights_bound``: dtype and shape, every element finite, exactly 0.0
    wherever ``vis`` is False, ``|w - ref| <= bound`` at EVERY element -> the largest ``err / bound`` (printed)."""
    tag = f"{what}: " if what else ""
    w = w.detach().cpu()
    assert w.dtype in (torch.float32, torch.bfloat16, torch.float16) and (wdt is None or w.dtype == wdt), (w.dtype, wdt)
    assert tuple(w.shape) == tuple(ref.shape) == tuple(vis.shape) == tuple(bound.shape), (tuple(w.shape), tuple(ref.shape))
    wd = w.double()
    assert bool(torch.isfinite(wd).all()), f"{tag}non-finite weight"
    hidden = wd[~vis]
    assert hidden.numel() == 0 or bool((hidden == 0).all()), f"{tag}a weight nothing sees is not exactly zero"
    err = (wd - ref).abs()
    ratio = torch.where(err > 0, err / bound, torch.zeros((), dtype=torch.float64))          # (x / 0 = inf: over a zero bound)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print(f"{tag}weights ({str(w.dtype).replace('torch.', '')}) max err / bound {worst:.3f}, max-abs {float(err.max()):.3e}")
    over = err > bound
    if bool(over.any()):
        i = tuple(int(x) for x in torch.nonzero(over)[0])
        raise AssertionError(f"{tag}{int(over.sum())} weights over their bound, the first at {i}: {float(wd[i]):.9e} for "
                             f"{float(ref[i]):.9e}, bound {float(bound[i]):.3e}; worst err / bound {worst:.3f}")
    return worst


def guarded_weights(wdt, B, H, Sq, Sk, *, pad, col_off, device=DEV):
    """[B, H + 1, 32 + Sq + 32, col_off + Sk + pad] filled with a NaN pattern -> (its [B,H,Sq,Sk] window at [0, 0, 32, col_off] as
    ``wdt``, the whole buffer's integer view)"""
    idt, pat = (torch.int32, NAN32) if wdt == torch.float32 else (torch.int16, NAN16)
    ibuf = torch.full((B, H + 1, GUARD + Sq + GUARD, col_off + Sk + pad), pat, dtype=idt, device=device)
    return ibuf.view(wdt)[:, :H, GUARD:GUARD + Sq, col_off:col_off + Sk], ibuf


def weights_into(args, wdt, B, H, Sq, Sk, *, pad, col_off):
    """pfa_fa3_weights for the forward arguments ``args`` (``ops.build_args``; ``args.lse`` set) writing W into the window of a
    ``guarded_weights`` buffer, with the buffer's strides -> (the window, the buffer's integer view).  ``check_guards`` on the latter."""
    from photonic_flash_attention_amd import _capi, ops
    inner, ibuf = guarded_weights(wdt, B, H, Sq, Sk, pad=pad, col_off=col_off)
    st = _capi.load().pfa_fa3_weights(C.byref(args), C.c_void_p(inner.data_ptr()), ops._DT[wdt], inner.stride(0), inner.stride(1),
                                      inner.stride(2), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    _capi.check_status(st)
    torch.cuda.synchronize()
    return inner, ibuf


def check_guards(ibuf, H, Sq, Sk, col_off, what=""):
    """The integer view of ``weights_into``'s buffer: every element outside the [B,H,Sq,Sk] window still holds the NaN pattern bit for
    bit (nothing was written out of bounds), and no element inside does (every one was written)."""
    tag = f"{what}: " if what else ""
    i = ibuf.detach().cpu()
    pat = NAN32 if i.dtype == torch.int32 else NAN16
    inside = torch.zeros(i.shape, dtype=torch.bool)
    inside[:, :H, GUARD:GUARD + Sq, col_off:col_off + Sk] = True
    hit = (i != pat) & ~inside
    assert not bool(hit.any()), f"{tag}{int(hit.sum())} guard elements overwritten, the first at {tuple(int(x) for x in torch.nonzero(hit)[0])}"
    left = (i == pat) & inside
    assert not bool(left.any()), f"{tag}{int(left.sum())} elements of W never written, the first at {tuple(int(x) for x in torch.nonzero(left)[0])}"


# --- the 16-bit backward (fa3_bwd_dq_kernel / fa3_bwd_dkdv_kernel): what they compute from their operands, its a-priori bound, the check --

C_P = 3.0                                          # the 5-sigma tail of a sum of independent roundings: tests/test_hip_parity.py's docstring
TOL16 = {torch.bfloat16: 1.5e-2, torch.float16: 4e-3}      # the whole-tensor criterion of tests/test_hip_backward.py, kept beside the bound
MUTANTS = ("delta0_last_rows", "p_scaled_last_block", "dq_dk_scaled", "last_key_dropped", "diagonal_dropped")

# B, H, Hkv, Sq, Sk, D, causal, extra.  The dQ block is 256 rows (8 waves x 32), the key tile 64 keys, the dK/dV block 128 keys (4 waves x
# 32) streaming 64-row query tiles in two 32-row halves.
BWD16_CASES = [
    (2, 2, 2, 1, 1, 64, False, None),                  # 1  one key: reference dq and dk exactly 0, their bound is the fp32 term alone
    (1, 2, 2, 33, 129, 128, False, None),              # 2  a wave with one row; a key block with one key
    (1, 2, 2, 300, 300, 128, True, None),              # 3  second Q block of 44 rows, third key block of 44 keys
    (2, 4, 2, 200, 333, 64, False, ("lens", [333, 77])),   # 4  groups of 2, Sk % 4 != 0
    (1, 3, 1, 520, 260, 128, True, None),              # 5  group of 3 on one K/V head; Sq > Sk; third Q block of 8 rows
    (1, 2, 2, 257, 513, 64, True, ("peaked", 3.0)),    # 6  q x 3: peaked softmax, dP - delta cancels; keys >= Sq seen by nobody
    (1, 2, 2, 130, 200, 128, False, ("scale", 0.3)),   # 7  softmax_scale = 0.3
    (2, 2, 2, 130, 260, 128, True, ("key",)),          # 8  key_mask, Sk % 4 == 0: the key-only path of the unmasked kernels
    (2, 4, 2, 130, 333, 64, False, ("key",)),          # 9  key_mask, Sk % 4 != 0: the element-mask kernels, groups of 2
    (1, 2, 2, 192, 200, 128, False, ("elem",)),        # 10 [B,1,Sq,Sk] mask; rows 5 and 100..132 fully masked
    (1, 4, 2, 320, 320, 64, True, ("elem_h",)),        # 11 [B,H,Sq,Sk] mask differing per head, groups of 2: column ranges over the group
    (2, 2, 2, 100, 100, 96, True, None),               # 12 head dim padded to 128 ...
    (1, 2, 1, 70, 90, 40, False, None),                #    ... and to 64
]


def bwd16_problem(idx, dtype):
    """BWD16_CASES[idx] in ``dtype`` -> a dict: the operands ``q, k, v, dout`` ([B,H,S,D] views of [B,S,H,D] arrays, on the CPU, rounded to
    ``dtype``), the kernels' keywords ``kw`` (CPU tensors), ``causal``, ``scale``, ``vis``.  Masks are drawn as in
    tests/test_hip_backward_store.py: keep probability 0.7 .. 0.8, key 0 kept where the row is meant to live."""
    B, H, Hkv, Sq, Sk, D, causal, extra = BWD16_CASES[idx]
    from photonic_flash_attention_amd import synth
    shapes = ((B, Sq, H, D), (B, Sk, Hkv, D), (B, Sk, Hkv, D), (B, Sq, H, D))
    q, k, v, dout = (torch.from_numpy(synth.normal_f32(s, 8100 + 10 * idx + i)) for i, s in enumerate(shapes))
    kind = extra[0] if extra is not None else None
    if kind == "peaked":
        q = q * extra[1]
    q, k, v, dout = (t.to(dtype).permute(0, 2, 1, 3) for t in (q, k, v, dout))
    g = torch.Generator().manual_seed(9000 + idx)
    kw, lens, keep = {}, None, None
    if kind == "lens":
        lens = extra[1]
        kw["seqlens_k"] = lens
    elif kind == "scale":
        kw["softmax_scale"] = extra[1]
    elif kind == "key":
        key_mask = torch.rand(B, Sk, generator=g) < 0.8
        key_mask[:, 0] = True
        kw["key_mask"] = key_mask
        keep = key_mask[:, None, None, :]
    elif kind in ("elem", "elem_h"):
        mask = torch.rand(B, H if kind == "elem_h" else 1, Sq, Sk, generator=g) < (0.75 if kind == "elem_h" else 0.7)
        mask[..., 0] = True                        # every remaining row sees at least key 0
        if kind == "elem":
            mask[:, :, 5] = False
            mask[:, :, 100:133] = False
        kw["mask"] = mask
        keep = mask
    scale = float(kw.get("softmax_scale", D ** -0.5))
    return dict(q=q, k=k, v=v, dout=dout, kw=kw, causal=causal, scale=scale,
                vis=visible(B, H, Sq, Sk, causal=causal, seqlens=lens, keep=keep))


@functools.lru_cache(maxsize=None)
def bwd16_isolated(idx, dtype):
    """``bwd16_problem(idx, dtype)`` with what every test of it shares, built once and never modified: the true fp64 ``reference`` (o, lse and
    the gradients ``true``), the forward operands made on the CPU -- ``o16`` = o rounded to ``dtype``, ``lse32`` = lse rounded to fp32, so
    that a backward call on them depends on no forward kernel --, ``backward_given`` on those (``given``, ``parts``), its ``bounds``, and
    ``row_seen`` / ``key_seen``."""
    p = dict(bwd16_problem(idx, dtype))
    kw = p["kw"]
    keep = kw["mask"] if "mask" in kw else (kw["key_mask"][:, None, None, :] if "key_mask" in kw else None)
    o, lse, *true = reference(p["q"], p["k"], p["v"], causal=p["causal"], seqlens=kw.get("seqlens_k"), keep=keep, scale=p["scale"], dout=p["dout"])
    p["true"], p["o16"], p["lse32"] = tuple(true), o.to(dtype), lse.float()
    *given, parts = backward_given(p["q"], p["k"], p["v"], p["o16"], p["dout"], p["lse32"], vis=p["vis"], scale=p["scale"])
    p["given"], p["parts"] = tuple(given), parts
    p["bounds"] = backward_bound(p["q"], p["k"], p["v"], p["o16"], p["dout"], p["lse32"], parts, scale=p["scale"], dtype=dtype)
    p["row_seen"], p["key_seen"] = seen(p["vis"], p["k"].shape[1])
    return p


def _group_sum(t, Hkv):
    """[B,H,Sk,D] per query head -> [B,Hkv,Sk,D] summed over each group"""
    B, H, Sk, D = t.shape
    return t.reshape(B, Hkv, H // Hkv, Sk, D).sum(2)


def backward_given(q, k, v, o, dout, lse32, *, vis, scale):
    """fp64 on the CPU -> (dq [B,H,Sq,D], dk, dv [B,Hkv,Sk,D], parts): the value of what the two kernels compute from the operands they are
    HANDED -- ``o`` (a 16-bit tensor, widened) and the fp32 ``lse32`` as given --, not autograd through a forward:

        P = exp(scale * s - lse32) where ``vis`` holds and the LSE is finite, 0 elsewhere         s = q k^T
        delta = rowsum(dout * o)        dP = dout v^T        dS = P o (dP - delta)
        dq = scale * dS k        dk = scale * dS^T q, summed over each group        dv = P^T dout, summed over each group

    With the exact fp64 ``o`` and ``lse`` this is the gradient (tests/test_dense_testlib.py pins it against ``reference``).  ``parts``:
    P, dS, dPd = dP - delta, the raw scores s, and the absolute-value sums ``backward_bound`` needs (A = sum_d |q k|, Av = sum_d |dout v|,
    Ao = sum_d |dout o|)."""
    Hkv = k.shape[1]
    g = q.shape[1] // Hkv
    qd, od, gd = (t.detach().cpu().double() for t in (q, o, dout))
    ke, ve = (t.detach().cpu().double().repeat_interleave(g, dim=1) for t in (k, v))
    lse = lse32.detach().cpu().double()
    fin = torch.isfinite(lse)
    zero = torch.zeros((), dtype=torch.float64)
    s = qd @ ke.transpose(-1, -2)
    P = torch.where(vis & fin[..., None], torch.exp(scale * s - torch.where(fin, lse, zero)[..., None]), zero)
    delta = (gd * od).sum(-1)
    dPd = gd @ ve.transpose(-1, -2) - delta[..., None]
    dS = P * dPd
    dq = scale * (dS @ ke)
    dk = _group_sum(scale * (dS.transpose(-1, -2) @ qd), Hkv)
    dv = _group_sum(P.transpose(-1, -2) @ gd, Hkv)
    parts = dict(P=P, dS=dS, dPd=dPd, s=s, A=qd.abs() @ ke.abs().transpose(-1, -2), Av=gd.abs() @ ve.abs().transpose(-1, -2),
                 Ao=(gd.abs() * od.abs()).sum(-1))
    return dq, dk, dv, parts


def backward_bound(q, k, v, o, dout, lse32, parts, *, scale, dtype):
    """The per-element a-priori error bounds (bdq [B,H,Sq,D], bdk, bdv [B,Hkv,Sk,D]) of the fp32-store gradients that the arithmetic of
    csrc/fa3_bwd_kernels.h computes for ``backward_given``'s values.  Derived from that arithmetic, never from what a kernel returned.

    The dominant term is statistical, as the forward's (tests/test_hip_parity.py): the kernels round dS (both kernels) and P (the dK/dV
    kernel) to 16 bits to feed the last MFMA products; each element carries one independent rounding of relative size at most u, or of
    absolute size at most t where fp16 goes subnormal ((u, t) = ROUND16[dtype]); the C_P = 3 multiple of the root of the summed squares is
    the 5-sigma tail:

        dq[i,d]   scale * C_P * sqrt( sum_j              ((u dS_ij)^2 + t^2 [P_ij > 0]) k_jd^2 )
        dk[j,d]   scale * C_P * sqrt( sum_{h in group} sum_i ((u dS_ij)^2 + t^2 [P_ij > 0]) q_id^2 )
        dv[j,d]           C_P * sqrt( sum_{h in group} sum_i ((u P_ij)^2  + t^2 [P_ij > 0]) dout_id^2 )

    What stays in fp32 is bounded in the worst case (L1), w = 2^-24, c = scale * log2(e), M = |lse| / scale:

        P, dQ kernel     exp2(fma(S, c, -lse * log2e)): ``weights_bound``'s bound32,  eq = ln2 (2 D w c A + 4 w (|c s| + |lse| log2e)) + 2 w
        P, dK/dV kernel  exp2((S - lse / scale) * c): the accumulator starts at fl(-lse / scale) (4 w M: the division) and every partial sum of
                         the D products is at most M + A in size; then the product by c (c itself rounded) and v_exp_f32:
                         ek = ln2 c (2 D w (M + A) + 4 w M + 2 w (|s| + M)) + 2 w
        dP - delta       delta is D fp32 additions of exact products and the lane pair's sum, (D + 1) w Ao; the accumulator starts at
                         -delta and takes the D products of dout and v (16-bit products are exact in fp32: one rounding each, every
                         partial sum at most Av + Ao in size):      eD = w (D (Av + Ao) + (D + 1) Ao)
        dS = P (dP - delta)    e(dS) = |dS| (e + w) + P eD,  with e = eq in the dQ kernel and ek in the dK/dV kernel
        the last products      their fp32 errors pass through the 16-bit rounding enlarged by at most 1 + u; the accumulation chain has one
                               MFMA per 16 keys (dQ) or per 16 rows of every head of the group (dK, dV), two roundings a step, over
                               sum |dS k|, sum |dS q|, sum |P dout|
        the multiply by scale  2 w |dq|, 2 w |dk|   (the product and the fp32 ``scale`` itself)

    Every term carries a factor P_ij: the bound is exactly 0 for rows that see no key and for keys that no row of the group sees, and the
    kernels' results there must be exactly 0.0.  Known blind spot: a conversion that truncates instead of rounding to nearest doubles the
    rounding error's size and biases it; that sits at about 1.0 of a 5-sigma bound and is not reliably caught."""
    B, H, Sq, D = q.shape
    Hkv, Sk = k.shape[1], k.shape[2]
    g = H // Hkv
    u, t = ROUND16[dtype]
    w, c = U32, scale * LOG2E
    qd, gd = q.detach().cpu().double().abs(), dout.detach().cpu().double().abs()
    ke = k.detach().cpu().double().abs().repeat_interleave(g, dim=1)
    P, dS, s, A = parts["P"], parts["dS"].abs(), parts["s"], parts["A"]
    lse = lse32.detach().cpu().double()
    La = torch.where(torch.isfinite(lse), lse, torch.zeros((), dtype=torch.float64)).abs()[..., None]
    M = La / scale
    eq = LN2 * (2 * D * w * c * A + 4 * w * ((c * s).abs() + La * LOG2E)) + 2 * w
    ek = LN2 * c * (2 * D * w * (M + A) + 4 * w * M + 2 * w * (s.abs() + M)) + 2 * w
    Ao = parts["Ao"][..., None]
    eD = w * (D * (parts["Av"] + Ao) + (D + 1) * Ao)
    live = (P > 0).double()
    e_dS_q = (dS * (eq + w) + P * eD) * (1 + u)
    e_dS_k = (dS * (ek + w) + P * eD) * (1 + u)
    e_P_k = P * ek * (1 + u)
    stat_dS = (u * dS) ** 2 + t * t * live
    stat_P = (u * P) ** 2 + t * t * live
    ck, cq = 2 * w * ((Sk + 15) // 16), 2 * w * g * ((Sq + 15) // 16)          # accumulation chains: MFMAs x two roundings
    T = lambda x: x.transpose(-1, -2)
    bdq = scale * (C_P * torch.sqrt(stat_dS @ ke ** 2) + e_dS_q @ ke + ck * (dS @ ke))
    bdq = bdq * (1 + 2 * w) + 2 * w * scale * (dS @ ke)
    bdk = scale * (C_P * torch.sqrt(_group_sum(T(stat_dS) @ qd ** 2, Hkv)) + _group_sum(T(e_dS_k) @ qd + cq * (T(dS) @ qd), Hkv))
    bdk = bdk * (1 + 2 * w) + 2 * w * scale * _group_sum(T(dS) @ qd, Hkv)
    bdv = C_P * torch.sqrt(_group_sum(T(stat_P) @ gd ** 2, Hkv)) + _group_sum(T(e_P_k) @ gd + cq * (T(P) @ gd), Hkv)
    return bdq, bdk, bdv


def check_grads16(grads, ref, bounds, row_seen, key_seen, what=""):
    """(dq, dk, dv) of an fp32-store call of the 16-bit backward against ``backward_given``'s within ``backward_bound``'s: dtype fp32 and shape,
    every element finite, exactly 0.0 for rows that see no key and keys no row of the group sees, ``|got - ref| <= bound`` at EVERY element
    -> the largest ``err / bound`` of dq, dk, dv (printed).  A failure names the number of offenders and the first."""
    tag = f"{what}: " if what else ""
    worst, bad = [], []
    for name, got, r, bound, live in zip(("dq", "dk", "dv"), grads, ref, bounds, (row_seen, key_seen, key_seen)):
        got = got.detach().cpu()
        assert got.dtype == torch.float32 and tuple(got.shape) == tuple(r.shape) == tuple(bound.shape), (name, got.dtype, tuple(got.shape), tuple(r.shape))
        gd = got.double()
        assert bool(torch.isfinite(gd).all()), f"{tag}{name} not finite"
        unseen = gd[~live]
        assert unseen.numel() == 0 or bool((unseen == 0).all()), f"{tag}{name} of rows / keys nothing sees is not exactly zero"
        err = (gd - r).abs()
        ratio = torch.where(err > 0, err / bound, torch.zeros((), dtype=torch.float64))              # (x / 0 = inf: over a zero bound)
        worst.append(float(ratio.max()) if ratio.numel() else 0.0)
        print(f"{tag}{name} max err / bound {worst[-1]:.3f}, max-abs {float(err.max()):.3e}, max bound {float(bound.max()):.3e}, "
              f"max |ref| {float(r.abs().max()):.3e}")
        over = err > bound
        if bool(over.any()):
            i = tuple(int(x) for x in torch.nonzero(over)[0])
            bad.append(f"{name}: {int(over.sum())} elements over their bound, the first at {i}: {float(gd[i]):.9e} for {float(r[i]):.9e}, "
                       f"bound {float(bound[i]):.3e}; worst err / bound {worst[-1]:.3f}")
    assert not bad, tag + "; ".join(bad)
    return tuple(worst)


def backward_model(q, k, v, o, dout, lse32, *, vis, scale, dtype, mutant=None):
    """A CPU emulation of the two kernels' rounding points -> fp32 (dq, dk, dv); for tests/test_dense_testlib.py only.  fp32 matmuls for S and
    dP, ``exp2`` of the fp32 exponent each kernel forms (``S * c - lse * log2e`` in the dQ kernel, ``(S - lse / scale) * c`` in the dK/dV
    kernel), P and dS rounded to nearest even in ``dtype``, fp32 products for the outputs.  ``mutant``: one of MUTANTS, a wrong kernel that
    ``check_grads16`` has to reject -- delta forced to 0 for the last 32 rows; P x 1.03 in the last 256-row block; dq and dk x 1.01; the
    last key's column dropped from dS; the diagonal element dropped for the last 32 rows (causal problems)."""
    assert mutant is None or mutant in MUTANTS, mutant
    B, H, Sq, D = q.shape
    Hkv, Sk = k.shape[1], k.shape[2]
    g = H // Hkv
    f32 = lambda x: torch.tensor(x, dtype=torch.float32)
    qf, of, gf = (t.detach().cpu().float() for t in (q, o, dout))
    ke, ve = (t.detach().cpu().float().repeat_interleave(g, dim=1) for t in (k, v))
    lse = lse32.detach().cpu().float()
    fin = torch.isfinite(lse)
    lz = torch.where(fin, lse, f32(0.0))[..., None]
    c = f32(scale * LOG2E)
    s = qf @ ke.transpose(-1, -2)
    live = vis & fin[..., None]
    if mutant == "diagonal_dropped":
        live = live.clone()
        for i in range(max(0, Sq - 32), min(Sq, Sk)):
            live[:, :, i, i] = False
    Pq = torch.where(live, torch.exp2(s * c - lz * f32(LOG2E)), f32(0.0))
    Pk = torch.where(live, torch.exp2((s + (-lz / f32(scale))) * c), f32(0.0))
    if mutant == "p_scaled_last_block":
        r0 = 256 * ((Sq - 1) // 256)
        Pq, Pk = Pq.clone(), Pk.clone()
        Pq[:, :, r0:] *= 1.03
        Pk[:, :, r0:] *= 1.03
    delta = (gf * of).sum(-1)
    if mutant == "delta0_last_rows":
        delta[:, :, max(0, Sq - 32):] = 0.0
    dPd = gf @ ve.transpose(-1, -2) - delta[..., None]
    dSq, dSk = Pq * dPd, Pk * dPd
    if mutant == "last_key_dropped":
        dSq[..., Sk - 1] = 0.0
        dSk[..., Sk - 1] = 0.0
    dSq, dSk, Pk = (x.to(dtype).float() for x in (dSq, dSk, Pk))
    dq = (dSq @ ke) * f32(scale)
    dk = _group_sum(dSk.transpose(-1, -2) @ qf, Hkv) * f32(scale)
    dv = _group_sum(Pk.transpose(-1, -2) @ gf, Hkv)
    if mutant == "dq_dk_scaled":
        dq, dk = dq * 1.01, dk * 1.01
    return dq, dk, dv

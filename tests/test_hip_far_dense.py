"""GPU tests of the dense and the packed training calls on tensors spread past 4 and 8 GiB -- ``ops.fa3_forward`` on every kernel family
(selectors 44, 43, 45 and the default), the fp32-store output, the exact fp32 kernels forward and backward, key and element masks, the
weights pass, ``pfa_fa3_bwd`` with 16-bit and fp32 gradients, and the packed ``pfa_fa3_varlen_fwd`` / ``_bwd``.  Every case runs one
tiny problem twice, on ordinary tensors and on far views of one 12.5 GiB arena, and ``far_testlib.two_runs`` asserts (a) - (e) as
tests/test_hip_far_cache.py spells them out.  Where ``ops`` allocates an output itself or copies an operand (gradients, the weights,
masks) the case fills the argument block directly, so that those tensors lie far too.

H 4, Hkv 2.  300 x 300 causal: the ragged (``kl``) flavour of the persistent kernel, the 8-wave and the 4-wave HIP kernel; 256 x 256 full:
the aligned persistent flavour.  The u32max stride (2^31 - 8 elements) is the largest the persistent kernel admits and the narrow one
(2^30 - 8) overflows only as a product: both run the persistent kernel.  The wide stride (2^31 + 2^20) leaves it: the far run must name
a HIP kernel, and the near run is forced onto the same with a selector.  The dense backward has no describe export (one kernel pair
per dtype, head dim and mask mode): its cases compare the strings ``describe`` below forms from the block.

(d) uses the existing bounds only: the per-element bound of tests/kvcache_testlib.py for a 16-bit O (square problems: top-left and
bottom-right causal coincide) and its 2e-3 on the LSE; 1e-3 / 2e-3 for the fp32-store forward (tests/test_hip_parity.py,
tests/test_hip_varlen.py); 2e-5 for the fp32 kernels (tests/dense_testlib.py); 1.5e-2 / 4e-3 x max|ref| for fp32 gradients
(tests/test_hip_backward.py) plus half a unit in the last place for 16-bit ones (tests/test_hip_backward_store.py); the a-priori bound
of ``dense_testlib.weights_bound`` for W.

fp32 tensors are placed to 4 GiB only (wide, two indices) and claim the two byte models alone: the int32-elements alias of an fp32 tensor
8 GiB out would fall in front of the arena (tests/far_testlib.py)."""

from __future__ import annotations

import ctypes as C

import pytest
import torch

import dense_testlib as DT
import far_testlib as F
from far_testlib import FarCase, Spec, saw_view
from kvcache_testlib import check_lse, check_out, reference as cache_reference
from photonic_flash_attention_amd import _capi, ops

BF, FP, F32 = torch.bfloat16, torch.float16, torch.float32
H, HKV = 4, 2
ROW_STRIDE, ROW_LENS = 2 ** 22 + 8, [255, 255, 255, 255, 4, 40]
TOL = {BF: 1.5e-2, FP: 4e-3}
HALF_ULP = {BF: 2.0 ** -9, FP: 2.0 ** -12}


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bshd(B, S, heads, D, dtype, g):
    """[B,heads,S,D] view of a [B,S,heads,D] array"""
    return torch.randn(B, S, heads, D, generator=g).to(dtype).permute(0, 2, 1, 3)


def _empty(B, S, heads, D, dtype, device=None):
    return torch.empty(B, S, heads, D, dtype=dtype, device=device).permute(0, 2, 1, 3)


def _stream(t):
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _is_far(t):
    return any(s >= 2 ** 21 for s in t.stride())


def _check_16bit_or_o32(o, lse, q, k, v, causal, dtype, what):
    ref = cache_reference(q, k, v, causal=causal)
    if o.dtype == F32:
        eo, el = float((o.double() - ref[0]).abs().max()), float((lse.double() - ref[1]).abs().max())
        print(f"{what}: o32 max-abs {eo:.3e} (bound 1e-3), lse {el:.3e} (bound 2e-3)")
        assert bool(torch.isfinite(o).all()) and eo <= 1e-3 and el <= 2e-3, (eo, el)
    else:
        check_out(o, ref[0], ref[2], float(v.abs().max()), dtype, what)
        check_lse(o, lse, ref[1], what)


# --- ops.fa3_forward on the 16-bit kernels ---------------------------------------------------------------------------------------------

def forward(selector, kind, *, axis=0, B=3, S=300, causal=True, D=128, dtype=BF, seed, o32=False, kv_kind=None):
    """q, k, v and o far along the batch (``axis`` 0) or the head axis (1).  ``kind`` wide leaves the persistent kernel: selectors 0 and
    45 then fall to the 8-wave HIP kernel, which the near run is forced onto.  ``kv_kind``: the stride of k and v where it differs
    (two K/V heads: the narrow stride reaches 2 GiB only, so they take a larger one)."""
    g = _gen(seed)
    q, k, v = _bshd(B, S, H, D, dtype, g), _bshd(B, S, HKV, D, dtype, g), _bshd(B, S, HKV, D, dtype, g)
    odt = F32 if o32 else dtype
    case = FarCase()
    for name, t, role in (("q", q, "in"), ("k", k, "in"), ("v", v, "in"), ("o", _empty(B, S, H, D, odt), "out")):
        case.put(name, t, kv_kind if kv_kind and name in "kv" else kind, axis, role)
    leaves_p4 = kind == "wide" and selector in (0, 45)
    if selector in (0, 45) and not leaves_p4:
        family = "fa3_fwd_p4_"
    elif selector == 43 and D == 128 and not o32:
        family = "fa3_fwd_w4_"
    else:
        family = "fa3_fwd_bf16_" if dtype == BF else "fa3_fwd_fp16_"

    def call(t):
        sel = 44 if leaves_p4 and not _is_far(t["q"]) else selector
        o, lse = ops.fa3_forward(t["q"], t["k"], t["v"], causal=causal, out=t["o"], out_dtype=odt, return_lse=True, _variant=sel or None)
        assert o is t["o"]
        return {"lse": lse}

    def seen(blocks, t):
        a = blocks.of("PfaFa3Args")
        for name in "qkvo":
            saw_view(a, name, t[name])

    def check(near, ex):
        _check_16bit_or_o32(near["o"], ex["lse"], near["q"], near["k"], near["v"], causal, dtype, f"selector {selector}")

    return Spec(case, call, seen, lambda blocks: _capi.describe(blocks.of("PfaFa3Args")), check, family)


# --- masks: the block filled by ops, the mask pointed far -----------------------------------------------------------------------------------

def masked(dims, *, D, dtype, seed, S=300):
    """A [B,Sk] key mask (dims 2), a [B,Sq,Sk] and a [B,H,Sq,Sk] element mask with a wide batch stride (bytes: B 2).  q, k, v stay
    ordinary tensors; o is an fp32 store.  ``ops`` would copy such a mask, so the case points the block's mask fields at the view."""
    B = 2
    g = _gen(seed)
    q, k, v = _bshd(B, S, H, D, dtype, g), _bshd(B, S, HKV, D, dtype, g), _bshd(B, S, HKV, D, dtype, g)
    shape = {2: (B, S), 3: (B, S, S), 4: (B, H, S, S)}[dims]
    m = (torch.rand(shape, generator=g) > 0.4).to(torch.uint8)
    m[..., 0] = 1
    if dims > 2:
        m[0, ..., 7, :] = 0                                          # a fully masked row
    case = FarCase()
    case.put("mask", m, "wide")
    for name, t in (("q", q), ("k", k), ("v", v)):
        case.plain(name, t)
    keep = {2: m[:, None, None, :], 3: m[:, None], 4: m}[dims].bool()

    def call(t):
        dev = t["q"].device
        o = _empty(B, S, H, D, F32, dev)
        lse = torch.empty(B, H, S, dtype=F32, device=dev)
        a, _ = ops.build_args(t["q"], t["k"], t["v"], o, lse=lse, split_p=True, variant=44)     # (44: a near key mask would take the persistent kernel)
        mk = t["mask"]
        if dims == 2:
            a.key_mask, a.key_mask_stride_b = mk.data_ptr(), mk.stride(0)
        else:
            a.mask, a.mask_stride_k = mk.data_ptr(), 1
            a.mask_stride_b, a.mask_stride_q = mk.stride(0), mk.stride(-2)
            a.mask_stride_h = mk.stride(1) if dims == 4 else 0
        _capi.check_status(_capi.load().pfa_fa3_fwd(C.byref(a), _stream(o)))
        return {"o": o, "lse": lse}

    def seen(blocks, t):
        a, mk = blocks.of("PfaFa3Args"), t["mask"]
        assert (a.key_mask if dims == 2 else a.mask) == mk.data_ptr() and (a.key_mask_stride_b if dims == 2 else a.mask_stride_b) == mk.stride(0)

    def check(near, ex):
        ro, rl = DT.reference(near["q"], near["k"], near["v"], keep=keep)
        o, lse = ex["o"].cpu(), ex["lse"].cpu()
        fin = torch.isfinite(rl)
        assert bool(torch.isfinite(o).all()) and torch.equal(torch.isfinite(lse), fin) and bool((o[~fin] == 0).all())
        eo, el = float((o.double() - ro).abs().max()), float((lse.double() - rl)[fin].abs().max())
        print(f"{dims}-D mask: o32 max-abs {eo:.3e} (bound 1e-3), lse {el:.3e} (bound 2e-3)")
        assert eo <= 1e-3 and el <= 2e-3, (eo, el)

    return Spec(case, call, seen, lambda blocks: _capi.describe(blocks.of("PfaFa3Args")), check, "fa3_fwd_")


# --- the weights pass ---------------------------------------------------------------------------------------------------------------------------

def weights(wdt, *, D, dtype, seed, S=300, causal=True):
    """``pfa_fa3_weights`` writing W [B,H,Sq,Sk] far along the batch, behind a forward on ordinary tensors.  16-bit W: three indices, wide;
    fp32 W: two."""
    B = 2 if wdt == F32 else 3
    g = _gen(seed)
    q, k, v = _bshd(B, S, H, D, dtype, g), _bshd(B, S, HKV, D, dtype, g), _bshd(B, S, HKV, D, dtype, g)
    case = FarCase()
    case.put("w", torch.empty(B, H, S, S, dtype=wdt), "wide", role="out")
    for name, t in (("q", q), ("k", k), ("v", v)):
        case.plain(name, t)

    def call(t):
        dev = t["q"].device
        o, lse = _empty(B, S, H, D, dtype, dev), torch.empty(B, H, S, dtype=F32, device=dev)
        a, _ = ops.build_args(t["q"], t["k"], t["v"], o, causal=causal, lse=lse)
        _capi.check_status(_capi.load().pfa_fa3_fwd(C.byref(a), _stream(o)))
        w = t["w"]
        call.passed = (w.data_ptr(), w.stride(0), w.stride(1), w.stride(2))
        _capi.check_status(_capi.load().pfa_fa3_weights(C.byref(a), C.c_void_p(w.data_ptr()), ops._DT[wdt], w.stride(0), w.stride(1),
                                                        w.stride(2), _stream(o)))
        return {"lse": lse}

    def seen(blocks, t):
        assert call.passed == (t["w"].data_ptr(),) + t["w"].stride()[:3] and _is_far(t["w"])

    def check(near, ex):
        ref, lse32 = DT.weights_reference(near["q"], near["k"], causal=causal, lse32=ex["lse"])
        bound = DT.weights_bound(near["q"], near["k"], ref, lse32, wdt=wdt)
        DT.check_weights(near["w"], ref, bound, DT.visible(B, H, S, S, causal=causal), f"W {wdt}", wdt)

    return Spec(case, call, seen, lambda blocks: _capi.describe(blocks.of("PfaFa3Args")), check)


# --- pfa_fa3_bwd, and the exact fp32 kernels -----------------------------------------------------------------------------------------------------

def _bwd_block(t, causal, gdt):
    """A ``pfa_fa3_bwd_args`` over the tensors ``t`` (q, k, v, o, dout, lse in; dq, dk, dv out), every stride the tensor's own."""
    q, k = t["q"], t["k"]
    B, Hq, Sq, D = q.shape
    kw = dict(lse=t["lse"].data_ptr(), B=B, H=Hq, Sq=Sq, Sk=k.shape[2], D=D, kv_group=Hq // k.shape[1], dtype=ops._DT[q.dtype],
              dtype_grad=ops._DT[gdt], causal=1 if causal else 0, softmax_scale=float(D ** -0.5), device_id=torch.cuda.current_device())
    for name in ("q", "k", "v", "o", "dout", "dq", "dk", "dv"):
        kw[name] = t[name].data_ptr()
        for ax, s in zip("bhs", t[name].stride()[:3]):
            kw[f"{'do' if name == 'dout' else name}_stride_{ax}"] = s
    return _capi._make(_capi.PfaFa3BwdArgs, kw)


def backward(kind, *, B, D, dtype, gdt, seed, S=300, causal=True, heads=(H, HKV)):
    """``pfa_fa3_bwd`` with all eight tensors far along the batch.  o and the LSE are the fp64 reference's, rounded: the case depends on
    no forward kernel.  dtype fp32: the exact fp32 kernels (one K/V head per query head)."""
    hq, hkv = heads
    g = _gen(seed)
    q, k, v, dout = _bshd(B, S, hq, D, dtype, g), _bshd(B, S, hkv, D, dtype, g), _bshd(B, S, hkv, D, dtype, g), _bshd(B, S, hq, D, dtype, g)
    ro, rl, *rg = DT.reference(q, k, v, causal=causal, dout=dout)
    o = torch.empty(B, S, hq, D, dtype=dtype).permute(0, 2, 1, 3)
    o.copy_(ro)
    case = FarCase()
    for name, t in (("q", q), ("k", k), ("v", v), ("o", o), ("dout", dout)):
        case.put(name, t, kind)
    case.plain("lse", rl.float())                    # (contiguous [B,H,Sq] by the ABI: it has no strides to place it with)
    for name, heads_n in (("dq", hq), ("dk", hkv), ("dv", hkv)):
        case.put(name, _empty(B, S, heads_n, D, gdt), kind, role="out")

    def call(t):
        delta = torch.empty(B, hq, S, dtype=F32, device=t["q"].device)
        a = _bwd_block(t, causal, gdt)
        a.delta = delta.data_ptr()
        _capi.check_status(_capi.load().pfa_fa3_bwd(C.byref(a), _stream(delta)))
        return {}

    def seen(blocks, t):
        a = blocks.of("PfaFa3BwdArgs")
        for name in ("q", "k", "v", "o", "dout", "dq", "dk", "dv"):
            saw_view(a, name, t[name])
            assert _is_far(t[name])

    def describe(blocks):
        a = blocks.of("PfaFa3BwdArgs")
        return (f"fa3_bwd dtype {a.dtype} grad {a.dtype_grad} D {a.D} causal {a.causal} group {a.kv_group}", 0)

    def check(near, ex):
        for name, ref in zip(("dq", "dk", "dv"), rg):
            got = near[name].cpu().double()
            assert bool(torch.isfinite(got).all()), name
            err, scale = float((got - ref).abs().max()), float(ref.abs().max())
            if dtype == F32:
                bound = DT.BOUND_GRAD * max(1.0, scale)
            else:
                bound = (TOL[dtype] + (HALF_ULP[dtype] if gdt != F32 else 0.0)) * scale + (1e-6 if gdt != F32 else 0.0)
            print(f"{name}: max-abs {err:.3e} (bound {bound:.3e}, max |ref| {scale:.3e})")
            assert err <= bound, (name, err, bound)

    return Spec(case, call, seen, describe, check)


def forward_f32(*, seed, Sq=130, Sk=257, D=64):
    """The exact fp32 forward: every operand fp32, wide along the batch, two indices."""
    B = 2
    g = _gen(seed)
    q = _bshd(B, Sq, H, D, F32, g)
    k, v = _bshd(B, Sk, HKV, D, F32, g), _bshd(B, Sk, HKV, D, F32, g)
    case = FarCase()
    for name, t, role in (("q", q, "in"), ("k", k, "in"), ("v", v, "in"), ("o", _empty(B, Sq, H, D, F32), "out")):
        case.put(name, t, "wide", role=role)

    def call(t):
        o, lse = ops.fa3_forward(t["q"], t["k"], t["v"], causal=True, out=t["o"], return_lse=True)
        assert o is t["o"]
        return {"lse": lse}

    def seen(blocks, t):
        for name in "qkvo":
            saw_view(blocks.of("PfaFa3Args"), name, t[name])

    def check(near, ex):
        ro, rl = DT.reference(near["q"], near["k"], near["v"], causal=True)
        DT.check_forward(near["o"], ex["lse"], ro, rl, "fp32 forward")

    return Spec(case, call, seen, lambda blocks: _capi.describe(blocks.of("PfaFa3Args")), check, "fa3_fwd_f32_")


# --- the packed forward and backward ----------------------------------------------------------------------------------------------------------

def varlen(direction, *, D, dtype, seed, causal=True):
    """``ops._varlen_fwd_launch`` / ``_varlen_bwd_launch`` on packed rows 2^22 + 8 elements apart: sequences of ``ROW_LENS`` rows start
    at rows 0, 255, 510, 765, 1020 and 1024, 2, 4, 6 and 8 GiB out, and every slab stays inside the library's own ``slab_fits32``."""
    lens = ROW_LENS
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    total, B = cu[-1], len(lens)
    g = _gen(seed)
    t0 = {"q": torch.randn(total, H, D, generator=g).to(dtype), "k": torch.randn(total, HKV, D, generator=g).to(dtype),
          "v": torch.randn(total, HKV, D, generator=g).to(dtype)}
    bwd = direction == "bwd"
    refs = []
    o, lse = torch.zeros(total, H, D, dtype=dtype), torch.zeros(H, total)
    if bwd:
        t0["dout"] = torch.randn(total, H, D, generator=g).to(dtype)
        for b in range(B):
            r = slice(cu[b], cu[b + 1])
            ro, rl, *rg = DT.reference(*(t0[n][r].transpose(0, 1)[None] for n in "qkv"), causal=causal, dout=t0["dout"][r].transpose(0, 1)[None])
            o[r], lse[:, r] = ro[0].transpose(0, 1).to(dtype), rl[0].float()
            refs.append(rg)
        t0["o"] = o
    case = FarCase()
    outs = ("dq", "dk", "dv") if bwd else ("o",)
    for name in tuple(t0) + outs:
        heads_n = HKV if name in ("k", "v", "dk", "dv") else H
        like = t0["k"] if heads_n == HKV else t0["q"]
        case.put_at(name, t0.get(name, like), case.layout.rows(name, total, (heads_n, D), (D, 1), 2, ROW_STRIDE, range(total)),
                    "out" if name in outs else "in")
    cu_t = torch.tensor(cu, dtype=torch.int32)

    def call(t):
        dev = t["q"].device
        cud = cu_t.to(dev)
        geo = ops._varlen_operands("pfa_fa3_varlen", t["q"], t["k"], t["v"], cud, cud, max(lens), max(lens))
        if bwd:
            ops._varlen_bwd_launch(t["q"], t["k"], t["v"], t["o"], t["dout"], lse.to(dev), t["dq"], t["dk"], t["dv"], cud, cud, geo, causal, None)
            return {}
        out_lse = torch.empty(H, total, dtype=F32, device=dev)
        ops._varlen_fwd_launch(t["q"], t["k"], t["v"], t["o"], out_lse, cud, cud, geo, causal, None)
        return {"lse": out_lse}

    block = "PfaFa3VarlenBwdArgs" if bwd else "PfaFa3VarlenArgs"

    def seen(blocks, t):
        for name in tuple(t0) + outs:
            saw_view(blocks.of(block), name, t[name], "sh")
            assert t[name].stride(0) == ROW_STRIDE

    def describe(blocks):
        return _capi.describe_varlen_bwd(blocks.of(block)) if bwd else _capi.describe_varlen(blocks.of(block))

    def check(near, ex):
        for b in range(B):
            r = slice(cu[b], cu[b + 1])
            seq = lambda x: x[r].transpose(0, 1)[None]
            if not bwd:
                _check_16bit_or_o32(seq(near["o"]), ex["lse"][None, :, r], seq(near["q"]), seq(near["k"]), seq(near["v"]), causal, dtype,
                                    f"sequence {b}")
        if bwd:
            for n, name in enumerate(("dq", "dk", "dv")):
                ref = torch.cat([refs[b][n][0].transpose(0, 1) for b in range(B)])
                got = near[name].cpu().double()
                err, scale = float((got - ref).abs().max()), float(ref.abs().max())
                bound = (TOL[dtype] + HALF_ULP[dtype]) * scale + 1e-6
                print(f"{name}: max-abs {err:.3e} (bound {bound:.3e}, max |ref| {scale:.3e})")
                assert bool(torch.isfinite(got).all()) and err <= bound, (name, err, bound)

    return Spec(case, call, seen, describe, check, "varlen")


# --- the cases ------------------------------------------------------------------------------------------------------------------------------

CASES = {
    # fa3_forward, selectors 44, 43, 45 and the default: u32max and narrow (the persistent kernel runs), wide (it does not)
    "fwd-44-u32max-batch": lambda: forward(44, "u32max", seed=1),
    "fwd-43-u32max-batch": lambda: forward(43, "u32max", seed=2),
    "fwd-45-u32max-batch": lambda: forward(45, "u32max", seed=3),
    "fwd-default-u32max-batch": lambda: forward(0, "u32max", seed=4, D=64, dtype=FP),
    "fwd-45-aligned-u32max-batch": lambda: forward(45, "u32max", seed=5, S=256, causal=False, D=64, dtype=FP),
    "fwd-default-aligned-narrow-batch": lambda: forward(0, "narrow", seed=6, S=256, causal=False, B=5),
    "fwd-45-narrow-batch": lambda: forward(45, "narrow", seed=7, B=5, D=64, dtype=FP),
    "fwd-44-narrow-batch": lambda: forward(44, "narrow", seed=8, B=5, D=64, dtype=FP),
    "fwd-43-narrow-head": lambda: forward(43, "narrow", seed=9, axis=1, kv_kind="wide"),
    "fwd-45-narrow-head": lambda: forward(45, "narrow", seed=10, axis=1, kv_kind="u32max"),
    "fwd-44-narrow-head": lambda: forward(44, "narrow", seed=11, axis=1, D=64, dtype=FP, kv_kind="wide"),
    "fwd-default-wide-batch": lambda: forward(0, "wide", seed=12),
    "fwd-45-wide-batch": lambda: forward(45, "wide", seed=13, S=256, causal=False, D=64, dtype=FP),
    "fwd-43-wide-batch": lambda: forward(43, "wide", seed=14),
    "fwd-44-wide-batch": lambda: forward(44, "wide", seed=15, D=64, dtype=FP),
    # fp32-store outputs, the exact fp32 kernels
    "fwd-o32-wide-batch": lambda: forward(44, "wide", seed=16, B=2, o32=True),
    "fwd-f32-wide-batch": lambda: forward_f32(seed=17),
    "bwd-f32-wide-batch": lambda: backward("wide", B=2, D=64, dtype=F32, gdt=F32, seed=18, S=130, heads=(2, 2)),
    # key mask [B,Sk], 3-D and 4-D element masks
    "key-mask-wide-batch": lambda: masked(2, D=128, dtype=BF, seed=19),
    "mask3-wide-batch": lambda: masked(3, D=64, dtype=FP, seed=20),
    "mask4-wide-batch": lambda: masked(4, D=128, dtype=BF, seed=21),
    # the weights pass
    "weights-16bit-wide-batch": lambda: weights(BF, D=128, dtype=BF, seed=22),
    "weights-f32-wide-batch": lambda: weights(F32, D=64, dtype=FP, seed=23),
    # fa3_backward, 16-bit and fp32 store
    "bwd-16bit-wide-batch": lambda: backward("wide", B=3, D=64, dtype=FP, gdt=FP, seed=24),
    "bwd-16bit-narrow-batch": lambda: backward("narrow", B=5, D=128, dtype=BF, gdt=BF, seed=25),
    "bwd-o32-wide-batch": lambda: backward("wide", B=2, D=128, dtype=BF, gdt=F32, seed=26),
    # fa3_varlen_forward / _backward on packed rows
    "varlen-fwd-packed-rows": lambda: varlen("fwd", D=128, dtype=BF, seed=27),
    "varlen-bwd-packed-rows": lambda: varlen("bwd", D=64, dtype=FP, seed=28),
}


@pytest.mark.gpu
def test_the_persistent_kernel_is_named_exactly_up_to_the_u32_limit():
    """``p4_eligible`` on the device (without one ``pfa_fa3_describe`` never names the persistent kernel: tests/test_far_strides_host.py
    asserts the rest): every q / k / v / o batch or head stride at 2^31 - 8 elements names it, one unit more names a HIP kernel."""
    q = torch.empty(2, 300, H, 128, dtype=BF, device="cuda:0").permute(0, 2, 1, 3)
    k = torch.empty(2, 300, HKV, 128, dtype=BF, device="cuda:0").permute(0, 2, 1, 3)
    for name in "qkvo":
        for axis in "bh":
            for stride, named in ((2 ** 31 - 8, True), (2 ** 31, False)):
                a, _ = ops.build_args(q, k, k, torch.empty_like(q), causal=True)
                setattr(a, f"{name}_stride_{axis}", stride)
                got = _capi.describe(a)[0]
                assert got.startswith("fa3_fwd_p4_") == named and _capi.load().pfa_fa3_check(C.byref(a)) == 0, (name, axis, stride, got)


@pytest.fixture(scope="module")
def arena():
    """The module's one arena.  Less than the arena plus 2 GiB free: the module skips, and says how much there was."""
    free = torch.cuda.mem_get_info()[0]
    if free < F.ARENA_BYTES + 2 * 2 ** 30:
        pytest.skip(f"{free / 2 ** 30:.1f} GiB of device memory free: the far-address tests need {F.ARENA_BYTES / 2 ** 30 + 2:.1f} GiB")
    torch.cuda.reset_peak_memory_stats()
    a = F.make_arena(torch.device("cuda:0"))
    yield a
    print(f"\ntests/test_hip_far_dense.py: peak device memory {torch.cuda.max_memory_allocated() / 2 ** 30:.3f} GiB")
    del a
    torch.cuda.empty_cache()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_far(name, arena):
    F.two_runs(arena, CASES[name]())

"""GPU tests of the backward's 16-bit gradient store -- the epilogue training runs (``grad_dtype=None``: ``OT = T`` in
fa3_bwd_kernels.h, ``store_tile_rows_via_lds`` + ``store_rows_from_lds``), which tests/test_hip_backward.py never compares
with numbers (it asks for fp32 gradients) -- of what the store writes and leaves alone, and of the ``dout`` layouts autograd
hands ``ops.fa3_backward``.

Reference: plain fp64 attention on the CPU under autograd (`_ref_grads`), on the 16-bit operands widened after rounding.

Tolerance of a 16-bit gradient:  |got - ref|_max <= (tol + u) |ref|_max + 1e-6,  tol = the bound of the fp32-store path
(tests/test_hip_backward.py: 1.5e-2 bf16, 4e-3 fp16), u = the relative half-ulp of the one extra rounding (2^-9 bf16,
2^-12 fp16); cosine >= 0.9995 as there.  Everything else here is an exact equality."""

from __future__ import annotations

import functools

import pytest
import torch

from dense_testlib import GUARD, bwd_into as _bwd_into, guarded as _guarded      # (shared with tests/test_hip_fp32_kernels.py)
from photonic_flash_attention_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

TORCH_DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
TOL = {"bf16": 1.5e-2, "fp16": 4e-3}             # tests/test_hip_backward.py
HALF_ULP = {"bf16": 2.0 ** -9, "fp16": 2.0 ** -12}


# ---- reference -------------------------------------------------------------------------------------------------------
def _ref_grads(q, k, v, dout, keep, scale):
    """fp64 dq, dk, dv as [B,H|Hkv,S,D].  q, dout: [B,Sq,H,D], k, v: [B,Sk,Hkv,D] (query head h reads K/V head h // g:
    repeat_interleave, so autograd sums the group); keep: bool, broadcastable to [B,H,Sq,Sk], or None.  Rows with no key kept
    give zero output and zero gradient (the kernels' documented convention)."""
    g = q.shape[2] // k.shape[2]
    qf, kf, vf = (t.double().permute(0, 2, 1, 3).clone().requires_grad_(True) for t in (q, k, v))
    s = (qf @ kf.repeat_interleave(g, dim=1).transpose(-1, -2)) * scale
    if keep is not None:
        s = s.masked_fill(~keep, float("-inf"))
    p = torch.nan_to_num(torch.softmax(s, dim=-1), nan=0.0)
    (p @ vf.repeat_interleave(g, dim=1)).backward(dout.double().permute(0, 2, 1, 3))
    return qf.grad, kf.grad, vf.grad


def _operands(B, H, Hkv, Sq, Sk, D, dtype, seed):
    """(q, k, v, dout) in the [B,S,H,D] layout, on the CPU, rounded to ``dtype``"""
    shapes = ((B, Sq, H, D), (B, Sk, Hkv, D), (B, Sk, Hkv, D), (B, Sq, H, D))
    return tuple(torch.from_numpy(synth.normal_f32(s, seed + i)).to(TORCH_DT[dtype]) for i, s in enumerate(shapes))


def _keep_mask(B, H, Sq, Sk, causal, lens=None, key_mask=None, mask=None):
    """what the kernels are told, as one bool [B,1|H,Sq,Sk] (None: everything visible); causal = key index <= row index"""
    keep = torch.ones(B, 1, Sq, Sk, dtype=torch.bool)
    if causal:
        keep = keep & torch.tril(torch.ones(Sq, Sk, dtype=torch.bool))
    if lens is not None:
        keep = keep & (torch.arange(Sk)[None, :] < torch.tensor(lens)[:, None])[:, None, None, :]
    if key_mask is not None:
        keep = keep & key_mask[:, None, None, :]
    if mask is not None:
        keep = keep & mask
    return keep


def _check_against_ref(name, got, ref, dtype, what):
    """assertion (b); got: a device or CPU tensor shaped like ref"""
    got = got.detach().cpu().double()
    assert bool(torch.isfinite(got).all()), f"{name} {what}: not finite"
    err, scale = float((got - ref).abs().max()), float(ref.abs().max())
    cos = float(torch.nn.functional.cosine_similarity(got.flatten(), ref.flatten(), dim=0)) if scale > 0 else 1.0
    bound = (TOL[dtype] + HALF_ULP[dtype]) * scale + 1e-6
    print(f"{what} {dtype} {name}: max-abs {err:.3e} (bound {bound:.3e}, max |ref| {scale:.3e}), cosine {cos:.6f}")
    assert err <= bound, f"{name} {what} {dtype}: err {err:.3e} > {bound:.3e}"
    assert cos >= 0.9995, f"{name} {what} {dtype}: cosine {cos}"


# ---- 1. 16-bit gradients at the store's edges ------------------------------------------------------------------------
# dQ block: 8 waves x 32 rows = 256 rows; dK/dV block: 4 waves x 32 keys = 128 keys; tile: 64.
# (One key: the softmax is 1 and dS = P (dP - delta) = 0, so the reference's dq and dk are exactly zero and their bound is the
#  absolute 1e-6 alone; the kernels leave the fp32 rounding of dP - delta there, 7.0e-7 bf16 / 1.8e-7 fp16 on an MI355X.)
STORE_CASES = [
    # B, H, Hkv, Sq, Sk, D, causal, extra
    (2, 2, 2, 1, 1, 64, False, None),                  # rows_valid = 1 in wave 0, <= 0 in every other wave
    (2, 3, 3, 33, 129, 128, False, None),              # a wave with one valid row; a second key block that holds one key
    (2, 2, 2, 257, 257, 64, True, None),               # a second Q block with one row
    (2, 1, 1, 97, 513, 64, True, ("lens", [513, 40])),   # keys past Sq no query sees: stored as zeros; kv_len inside a wave
    (2, 4, 2, 200, 333, 128, False, ("lens", [333, 77])),   # grouped-query heads with seqlens_k
    (1, 6, 2, 300, 300, 64, True, None),               # groups of three
    (2, 2, 2, 130, 260, 128, True, ("key",)),          # Sk % 4 == 0: the key mask runs on the unmasked kernels
    (2, 4, 2, 130, 333, 64, False, ("key",)),          # Sk % 4 != 0: the element-mask kernels, 16-bit store, grouped heads
    (1, 2, 2, 192, 200, 128, False, ("elem",)),        # [B,1,Sq,Sk] mask, rows 5 and 100..132 fully masked
    (2, 2, 2, 100, 100, 96, True, None),               # head dim zero-padded to 128 in ops
]


@functools.lru_cache(maxsize=None)
def _store_problem(idx, dtype):
    """operands, kernel keywords, visibility and the fp64 reference of STORE_CASES[idx]: built once, never modified"""
    B, H, Hkv, Sq, Sk, D, causal, extra = STORE_CASES[idx]
    q, k, v, dout = _operands(B, H, Hkv, Sq, Sk, D, dtype, 3100 + 10 * idx)
    g = torch.Generator().manual_seed(7000 + idx)
    kw, lens, key_mask, mask = {}, None, None, None
    if extra is not None and extra[0] == "lens":
        lens = extra[1]
        kw["seqlens_k"] = lens
    elif extra is not None and extra[0] == "key":
        key_mask = torch.rand(B, Sk, generator=g) < 0.8
        key_mask[:, 0] = True
        kw["key_mask"] = key_mask
    elif extra is not None:
        mask = torch.rand(B, 1, Sq, Sk, generator=g) < 0.7
        mask[..., 0] = True                    # every remaining row sees at least key 0
        mask[:, :, 5] = False
        mask[:, :, 100:133] = False
        kw["mask"] = mask
    keep = _keep_mask(B, H, Sq, Sk, causal, lens, key_mask, mask)
    ref = _ref_grads(q, k, v, dout, keep, D ** -0.5)
    row_seen = keep.any(dim=3).expand(B, H, Sq)                                      # [B,H,Sq]: the row sees a key
    key_seen = keep.any(dim=2).expand(B, H, Sk).reshape(B, Hkv, H // Hkv, Sk).any(dim=2)   # [B,Hkv,Sk]: a row of the group sees the key
    return (q, k, v, dout), kw, ref, row_seen, key_seen


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("idx", range(len(STORE_CASES)), ids=[f"case{i}" for i in range(len(STORE_CASES))])
def test_16bit_gradient_store_at_block_edges(idx, dtype):
    from photonic_flash_attention_amd import ops
    B, H, Hkv, Sq, Sk, D, causal, _ = STORE_CASES[idx]
    (q, k, v, dout), kw, ref, row_seen, key_seen = _store_problem(idx, dtype)
    qd, kd, vd, gd = (t.to(DEV).permute(0, 2, 1, 3) for t in (q, k, v, dout))
    kwd = {n: (m.to(DEV) if isinstance(m, torch.Tensor) else m) for n, m in kw.items()}
    out, lse = ops.fa3_forward(qd, kd, vd, causal=causal, return_lse=True, **kwd)
    g16 = ops.fa3_backward(qd, kd, vd, out, gd, lse, causal=causal, **kwd)                                # the training path
    g32 = ops.fa3_backward(qd, kd, vd, out, gd, lse, causal=causal, grad_dtype=torch.float32, **kwd)
    torch.cuda.synchronize()
    what = f"case{idx} {STORE_CASES[idx]}"
    shapes = ((B, H, Sq, D), (B, Hkv, Sk, D), (B, Hkv, Sk, D))
    for name, got, wide, r, shape, seen in zip(("dq", "dk", "dv"), g16, g32, ref, shapes, (row_seen, key_seen, key_seen)):
        # (a) type and shape
        assert got.dtype == TORCH_DT[dtype] and tuple(got.shape) == shape, (name, got.dtype, tuple(got.shape))
        assert wide.dtype == torch.float32 and tuple(wide.shape) == shape, (name, wide.dtype, tuple(wide.shape))
        # (b) the reference
        _check_against_ref(name, got, r, dtype, what)
        # rows no key is visible to, keys no row sees: the gradient is stored, and is exactly zero
        dead = got.cpu()[~seen]
        assert dead.numel() == 0 or float(dead.float().abs().max()) == 0.0, f"{name} {what}: unseen rows not stored as zeros"
        # (c) the store alone: same arithmetic up to the epilogue, one rounding to nearest even of acc * mul in either
        same = torch.equal(wide.to(got.dtype), got)
        if not same:
            d = (wide.to(got.dtype).float() - got.float()).abs()
            print(f"{what} {dtype} {name}: {int((d != 0).sum())} of {d.numel()} elements differ from the rounded fp32 store, "
                  f"max {float(d.max()):.3e}, first at {tuple(int(x) for x in (d != 0).nonzero()[0])}")
        assert same, f"{name} {what} {dtype}: the 16-bit store is not the rounded fp32 store"


# ---- 2. containment and full writes, through the C ABI ---------------------------------------------------------------
CONTAIN_CASES = [
    # B, H, Hkv, Sq, Sk, D, causal
    (2, 2, 2, 33, 129, 128, True),
    (2, 4, 2, 257, 100, 64, False),
]


@pytest.mark.parametrize("wide", [False, True], ids=["grad16", "grad32"])
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("case", CONTAIN_CASES)
def test_backward_writes_every_gradient_element_and_nothing_else(case, dtype, wide):
    from photonic_flash_attention_amd import ops
    B, H, Hkv, Sq, Sk, D, causal = case
    q, k, v, dout = _operands(B, H, Hkv, Sq, Sk, D, dtype, 5200 + Sq)
    gdt = torch.float32 if wide else TORCH_DT[dtype]
    ref = _ref_grads(q, k, v, dout, _keep_mask(B, H, Sq, Sk, causal), D ** -0.5)
    qd, kd, vd, gd = (t.to(DEV).permute(0, 2, 1, 3) for t in (q, k, v, dout))
    out, lse = ops.fa3_forward(qd, kd, vd, causal=causal, return_lse=True)
    plain = ops.fa3_backward(qd, kd, vd, out, gd, lse, causal=causal, grad_dtype=gdt)
    bufs, ibufs, pats = zip(*(_guarded(B, S, Hx, D, gdt) for S, Hx in ((Sq, H), (Sk, Hkv), (Sk, Hkv))))
    _bwd_into(qd, kd, vd, out, gd, lse, causal, gdt, bufs)
    what = f"{case} grad {gdt}"
    for name, buf, ibuf, pat, S, r, p in zip(("dq", "dk", "dv"), bufs, ibufs, pats, (Sq, Sk, Sk), ref, plain):
        inside = torch.zeros(ibuf.shape, dtype=torch.bool, device=DEV)
        inside[:, GUARD:GUARD + S, :, :D] = True
        stray = (ibuf != pat) & ~inside
        assert not bool(stray.any()), f"{name} {what}: written outside the tensor, first at [b, row, h, d] = " \
                                      f"{tuple(int(x) for x in stray.nonzero()[0])} (rows {GUARD}..{GUARD + S - 1} are the tensor)"
        got = buf[:, GUARD:GUARD + S, :, :D].permute(0, 2, 1, 3)       # [B,H,S,D]
        holes = torch.isnan(got)
        assert not bool(holes.any()), f"{name} {what}: {int(holes.sum())} elements never written, first at [b, h, row, d] = " \
                                      f"{tuple(int(x) for x in holes.nonzero()[0])}"
        _check_against_ref(name, got, r, dtype, what)
        assert torch.equal(got, p), f"{name} {what}: differs from ops.fa3_backward on the same operands"


# ---- 3. dout layouts through autograd --------------------------------------------------------------------------------
# kind -> what _FA3Function.backward is handed; pad: elements worth 8 bytes
DOUT_KINDS = ["sum", "weighted", "expanded", "misaligned_base", "odd_row_stride"]


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("kind", DOUT_KINDS)
def test_autograd_dout_layouts(kind, dtype, monkeypatch):
    """Every layout of ``dout`` autograd produces gives the gradients of the same values laid out contiguously, bit for bit.
    bf16 operands (16-byte pieces = 8 elements) as in training; fp32 operands for the fp32 kernels' rule (4 elements)."""
    from photonic_flash_attention_amd import ops
    B, H, S, D = 2, 2, 96, 64
    dt = TORCH_DT[dtype]
    unit = 16 // dt.itemsize                   # elements of a 16-byte piece
    pad_w = unit // 2                          # 8 bytes
    q, k, v, w = (t.to(DEV).permute(0, 2, 1, 3) for t in _operands(B, H, H, S, S, D, dtype, 6100))
    w = w[:1, :1, :1].contiguous()             # [1,1,1,D]
    q, k, v = (t.detach().requires_grad_(True) for t in (q, k, v))
    pad = torch.zeros((B, H, S, pad_w), dtype=dt, device=DEV)

    seen = []
    real = ops.fa3_backward

    def spy(q_, k_, v_, out_, dout_, lse_, **kw):
        seen.append((out_, dout_, lse_, kw))
        return real(q_, k_, v_, out_, dout_, lse_, **kw)

    monkeypatch.setattr(ops, "fa3_backward", spy)
    out = ops.fa3_attention(q, k, v, causal=True)
    if kind == "sum":
        out.sum().backward()
    elif kind == "weighted":
        (out * w).sum().backward()
    elif kind == "expanded":
        out.backward(w.expand_as(out))
    elif kind == "misaligned_base":
        torch.cat([pad, out, pad], dim=-1)[..., pad_w:pad_w + D].square().sum().backward()
    else:
        torch.cat([out, pad], dim=-1)[..., :D].square().sum().backward()
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert len(seen) == 1
    o_saved, dout, lse, kw = seen[0]
    assert tuple(dout.shape) == (B, H, S, D) and dout.dtype == dt
    print(f"{kind} {dtype}: dout strides {dout.stride()}, base % 16 = {dout.data_ptr() % 16}")
    # the hard layouts really occurred
    if kind == "sum":
        assert dout.stride() == (0, 0, 0, 0)
    elif kind == "expanded":
        assert dout.stride() == (0, 0, 0, 1)
    elif kind == "misaligned_base":
        assert dout.stride(3) == 1 and dout.data_ptr() % 16 == 8 and all(s % unit == 0 for s in dout.stride()[:3])
    elif kind == "odd_row_stride":
        assert dout.stride(3) == 1 and dout.data_ptr() % 16 == 0 and dout.stride(2) % unit != 0
    want = real(q.detach(), k.detach(), v.detach(), o_saved, dout.contiguous(), lse, **kw)
    torch.cuda.synchronize()
    for name, leaf, g in zip(("dq", "dk", "dv"), (q, k, v), want):
        assert leaf.grad is not None and leaf.grad.dtype == dt and bool(torch.isfinite(leaf.grad).all()), name
        assert float(g.float().abs().max()) > 0, name
        assert torch.equal(leaf.grad, g), f"{name}: dout laid out as {dout.stride()} (base % 16 = {dout.data_ptr() % 16}) " \
                                          f"gives other gradients than the same values laid out contiguously"

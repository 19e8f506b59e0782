"""The attention-weights pass (csrc/fa3_weights_kernel.h behind ``pfa_fa3_weights``: the ``need_weights=True`` output of every converted
``nn.MultiheadAttention``) against the fp64 reference of tests/dense_testlib.py, element by element inside the a-priori bound
``weights_bound``, on every path the kernel has: the two schedules (D = 64: a wave per fourth key block, D = 128: a strip per wave and
the trailing zero tiles), the 64-key fast path and the per-lane tail (vector and scalar stores), the ``whole_block`` shortcut, the
zero tiles, the mask as words and as bytes, dead rows, and both workgroup orders.

Every call goes through the C ABI (``ops.build_args`` then ``pfa_fa3_weights``) with the reference's own fp32 LSE, so no forward runs and
the forward's error is no part of the check; only group (h) runs the two passes together.  W is written into a buffer of NaN patterns
with guard rows, columns and a guard head around it: every guard element must survive bit for bit and every element of W must have been
written.  Distinct heads and batches come from the generator, so a permuted head, strip or key block cannot pass.  q is scaled by 2.5
in most cases: a row then holds weights from about 1 down to 1e-9, and fp16 subnormals occur.

Three things in the kernel that no test of its output can tell apart, by construction: WHICH workgroup takes a (batch, head, Q block) --
any bijection of the XCD remap gives the same W (a remap that is none leaves heads unwritten, which the guards' "never written" check
reports); ``strip_kv_end``'s ``+ 32`` against ``+ 31`` -- it is only compared with multiples of 64; and the clamp of ``seqlens_k`` to
``0 .. Sk`` -- no key at or past Sk is ever stored, and a negative length hides every key as 0 does."""

from __future__ import annotations

import ctypes as C
import functools

import pytest
import torch

from dense_testlib import DEV, check_guards, check_weights, visible, weights_bound, weights_into, weights_reference
from photonic_flash_attention_amd import _capi, ops, synth

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "fp16": torch.float16}


@functools.lru_cache(maxsize=None)
def _operands(dt, D, B, H, Hkv, Sq, Sk, qscale, seed):
    """q [B,H,Sq,D], k [B,Hkv,Sk,D] (views of the generator's [B,S,H,D] arrays) on the CPU, and on the device"""
    q, k, _ = synth.qkv(B, H, Sq, Sk, D, seed, dt)
    q, k = q.permute(0, 2, 1, 3), k.permute(0, 2, 1, 3)[:, :Hkv]
    if qscale != 1.0:
        q = (q.float() * qscale).to(q.dtype)
    return q, k, q.to(DEV), k.to(DEV)


@functools.lru_cache(maxsize=None)
def _mask(kind, B, H, Sq, Sk, seed=3):
    """A bool mask in one of the reference's forms: keys 0..69 visible, 128..191 hidden, the rest random at 0.6; where the form has
    rows, rows 5 and 100..132 see nothing.  (Made once per form and shape, and never changed.)"""
    shape = {"key": (B, Sk), "b1qk": (B, 1, Sq, Sk), "bhqk": (B, H, Sq, Sk), "11qk": (1, 1, Sq, Sk), "b11k": (B, 1, 1, Sk),
             "1hqk": (1, H, Sq, Sk), "3d": (B, Sq, Sk)}[kind]
    m = torch.rand(shape, generator=torch.Generator().manual_seed(seed)) < 0.6
    m[..., :70] = True
    m[..., 128:192] = False
    if kind not in ("key", "b11k"):
        m[..., 5, :] = False
        m[..., 100:133, :] = False
    return m


_KEEP4 = {}


def _keep4(m):
    """a 2-D [B,Sk] / 3-D [B,Sq,Sk] mask in the reference's 4-D form (one view per mask, kept: its identity names the problem)"""
    if m is None or m.dim() == 4:
        return m
    if id(m) not in _KEEP4:
        _KEEP4[id(m)] = (m[:, None, None, :] if m.dim() == 2 else m[:, None], m)
    return _KEEP4[id(m)][0]


def _vec_pad(Sk, col_off, wdt):
    """the fewest guard columns (at least one) that leave W's row stride a multiple of 16 bytes: the fast path stays on"""
    per16 = 16 // torch.empty((), dtype=wdt).element_size()
    return next(p for p in range(1, per16 + 1) if (col_off + Sk + p) % per16 == 0)


_REFS = {}


def _reference(key, q, k, causal, lens, keep, dead=None):
    """(W fp64, its fp32 LSE, the same on the device, the visibility): computed once per problem and shared between the runs on it.
    The entry holds on to q, k, keep and dead, whose identities are part of the key.  ``dead`` [B,H,Sq]: rows whose LSE is set to -inf
    although they see keys -- the weights of such a row are zero."""
    key = key + (id(q), id(k), id(keep), id(dead), causal, None if lens is None else tuple(lens))
    if key not in _REFS:
        B, H, Sq, _ = q.shape
        ref, lse32 = weights_reference(q, k, causal=causal, seqlens=lens, keep=keep)
        vis = visible(B, H, Sq, k.shape[2], causal=causal, seqlens=lens, keep=keep)
        if dead is not None:
            ref, lse32 = weights_reference(q, k, causal=causal, seqlens=lens, keep=keep, lse32=lse32.masked_fill(dead, float("-inf")))
            vis = vis & ~dead[..., None]
        _REFS[key] = (ref, lse32, lse32.to(DEV), vis, (q, k, keep, dead))
    return _REFS[key][:4]


def _run(what, dt, D, B, H, Sq, Sk, wdt, *, Hkv=None, causal=False, lens=None, mask=None, key_mask=None, raw_mask=None, qscale=2.5,
         pad=None, col_off=0, workspace=True, seed=8100, operands=None, dead=None):
    """One guarded call of pfa_fa3_weights checked against the reference -> (W on the device, err / bound).  ``mask`` / ``key_mask``
    go through ``ops.build_args``; ``raw_mask`` is a (u8 device view [.,.,.,Sk], bool keep) pair handed over with the view's own byte
    strides.  ``workspace=False``: the mask is read as bytes."""
    dtt = DT[dt]
    wdt = dtt if wdt == "16" else wdt
    Hkv = H if Hkv is None else Hkv
    q, k, qd, kd = operands or _operands(dt, D, B, H, Hkv, Sq, Sk, qscale, seed)
    keep = raw_mask[1] if raw_mask is not None else _keep4(key_mask if key_mask is not None else mask)
    ref, lse32, lse_dev, vis = _reference((dt, D), q, k, causal, lens, keep, dead)
    kw = {}
    if mask is not None:
        kw["mask"] = mask.to(DEV)
    if key_mask is not None:
        kw["key_mask"] = key_mask.to(DEV)
    a, hold = ops.build_args(qd, kd, kd, torch.empty_like(qd), causal=causal, seqlens_k=lens, lse=lse_dev, **kw)
    if raw_mask is not None:
        m4 = raw_mask[0]
        assert m4.dtype == torch.uint8 and m4.dim() == 4 and m4.shape[3] == Sk
        a.mask = m4.data_ptr()
        a.mask_stride_b, a.mask_stride_h, a.mask_stride_q, a.mask_stride_k = (0 if m4.shape[i] == 1 else m4.stride(i) for i in range(4))
        nbytes = int(_capi.load().pfa_fa3_workspace_bytes(C.byref(a)))
        assert nbytes > 0
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
        hold += [m4, ws]
    if keep is not None:
        assert a.workspace_bytes > 0
        if not workspace:
            a.workspace, a.workspace_bytes = None, 0
    pad = _vec_pad(Sk, col_off, wdt) if pad is None else pad
    w, ibuf = weights_into(a, wdt, B, H, Sq, Sk, pad=pad, col_off=col_off)
    check_guards(ibuf, H, Sq, Sk, col_off, what)
    return w, check_weights(w, ref, weights_bound(q, k, ref, lse32, wdt=wdt), vis, what, wdt=wdt)


# ---- (a) the path matrix: operand type x head dim x W type x causal x mask, at a fast path with a tail and on the per-lane path alone ----
@pytest.mark.parametrize("mask", ["none", "key", "b1qk"])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("wdt", [torch.float32, "16"], ids=["w32", "w16"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_path_matrix(dt, D, wdt, causal, mask):
    B, H, Sq = 2, 3, 200
    for Sk in (328, 333):                 # 328: keys 0..319 leave as 64-key segments, 8 through the tail
        kw = {} if mask == "none" else {"key_mask": _mask("key", B, H, Sq, Sk)} if mask == "key" else {"mask": _mask("b1qk", B, H, Sq, Sk)}
        for pad in ((None,) if Sk == 328 else (3, 2)):                # 333 + 3: a fast path again, and a tail that ends in scalar stores;
            _run(f"(a) {dt} D{D} Sk{Sk}+{pad} causal={causal} mask={mask}", dt, D, B, H, Sq, Sk, wdt, causal=causal, seed=8100 + D, pad=pad,
                 **kw)                                                # 333 + 2: an odd row stride, every key through the tail


# ---- (b) the workgroup order: the XCD remap of (B H) % 8 == 0 against the linear order ---------------------------------------------
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("shape", [(2, 4, 4, 160), (1, 8, 8, 300), (1, 16, 4, 129), (2, 3, 3, 160)], ids=lambda s: "B%dH%dkv%dSq%d" % s)
def test_workgroup_order(shape, D, causal):
    B, H, Hkv, Sq = shape                 # two or three Q blocks per head; B H = 8, 8, 16 (remapped) and 6 (linear)
    for wdt in (torch.float32, "16"):
        _run(f"(b) B{B} H{H}/{Hkv} Sq{Sq} D{D} causal={causal}", "bf16" if D == 64 else "fp16", D, B, H, Sq, 136, wdt, Hkv=Hkv, causal=causal,
             qscale=1.0 if B == 2 else 2.5, seed=8200)


# ---- (c) causal geometry without a mask ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wdt", [torch.float32, "16"], ids=["w32", "w16"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Sq, Sk", [(200, 72), (72, 328), (192, 192)])
def test_causal_geometry(Sq, Sk, D, wdt):
    """(200, 72): rows past the last key; (72, 328): keys past the last row, the zero tiles of both schedules (D = 128: its trailing
    loop); (192, 192): the diagonal crosses the 64-key blocks at strips 1 and 2 of each Q block, where ``whole_block`` must say no."""
    for dt in ("bf16", "fp16"):
        _run(f"(c) Sq{Sq} Sk{Sk} D{D} {dt}", dt, D, 2, 3, Sq, Sk, wdt, causal=True, seed=8300)


# ---- (d) seqlens_k: 0, 1, the block edges, past Sk and negative ---------------------------------------------------------------------
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("lens", [[0, 1, 63, 64], [65, 200, 205, -3]], ids=["0-1-63-64", "65-200-205-neg"])
def test_seqlens(lens, D, causal):
    B, H, Sq, Sk = 4, 2, 130, 200
    for wdt in (torch.float32, "16"):
        w, _ = _run(f"(d) lens={lens} D{D} causal={causal}", "fp16" if D == 64 else "bf16", D, B, H, Sq, Sk, wdt, causal=causal, lens=lens,
                    seed=8400)
        for b, n in enumerate(lens):
            if n <= 0:                    # a batch with no key: lse = -inf on every row, W exactly zero
                assert bool((w[b] == 0).all())


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("D", [64, 128])
def test_rows_the_lse_declares_dead(D, causal):
    """lse = -inf IS the statement that a row has no weights (the forward writes it for a row that sees no key): such a row is zero
    even where the masks of this call would show it keys -- on the fast path's unmasked blocks (exp2(x - inf)) and under the
    per-element tests alike.  A single row, a whole strip, rows across a Q-block edge and a whole head."""
    B, H, Sq, Sk = 2, 2, 200, 200
    dead = torch.zeros(B, H, Sq, dtype=torch.bool)
    dead[0, 0, 3] = dead[0, 1, 199] = True
    dead[0, 0, 64:96] = dead[1, 0, 120:140] = True
    dead[1, 1] = True
    for wdt in (torch.float32, "16"):
        w, _ = _run(f"(d) dead rows D{D} causal={causal}", "bf16" if D == 64 else "fp16", D, B, H, Sq, Sk, wdt, causal=causal, dead=dead, seed=8450)
        assert bool((w[dead.to(DEV)] == 0).all()) and bool((w[1, 0, 0] > 0).any())


# ---- (e) ragged rows: Sq not a multiple of 32 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("Sk", [128, 72])
@pytest.mark.parametrize("Sq", [1, 31, 33, 127, 129])
def test_ragged_rows(Sq, Sk):
    """rows_valid of the segment stores and of the zero tiles: Sk 128 leaves as two 64-key segments, Sk 72 as one and an 8-key tail"""
    for D, causal in ((64, False), (64, True), (128, False), (128, True)):
        for wdt in (torch.float32, "16"):
            _run(f"(e) Sq{Sq} Sk{Sk} D{D} causal={causal}", "bf16" if causal else "fp16", D, 1, 2, Sq, Sk, wdt, causal=causal, qscale=1.0,
                 seed=8500)


# ---- (f) masks, as words and as bytes ---------------------------------------------------------------------------------------------------
def _words_and_bytes(what, dt, D, B, H, Sq, Sk, **kw):
    """the same call with the workspace (the mask condensed to words) and without (a byte per score): both inside the bound, same bits"""
    for wdt in (torch.float32, "16"):
        ww, _ = _run(f"{what} words", dt, D, B, H, Sq, Sk, wdt, workspace=True, **kw)
        wb, _ = _run(f"{what} bytes", dt, D, B, H, Sq, Sk, wdt, workspace=False, **kw)
        assert torch.equal(ww, wb), f"{what}: the words path and the bytes path differ"


@pytest.mark.parametrize("mode", ["alone", "causal", "seqlens"])
@pytest.mark.parametrize("kind", ["key", "bhqk", "11qk", "b11k", "1hqk", "3d"])
def test_masks_as_words_and_as_bytes(kind, mode):
    B, H, Sq, Sk = 2, 3, 200, 330         # (with the buffer's pad: keys 0..319 on the fast path, 10 through the tail)
    D, dt = (64, "bf16") if kind in ("key", "11qk", "3d") else (128, "fp16")
    m = _mask(kind, B, H, Sq, Sk)
    kw = {"key_mask": m} if kind == "key" else {"mask": m}
    _words_and_bytes(f"(f) {kind} {mode} D{D}", dt, D, B, H, Sq, Sk, causal=mode == "causal", lens=[150, 330] if mode == "seqlens" else None,
                     seed=8600, **kw)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("form", ["expanded", "strided"])
def test_masks_handed_over_with_their_own_strides(form, D):
    """The C ABI takes four byte strides: an expanded [B,1,1,Sk] mask (strides 0 over heads and rows) and every second byte of a wider
    mask (key stride 2, which no tensor-level caller produces: ``ops`` copies such a mask)."""
    B, H, Sq, Sk = 2, 3, 200, 330
    if form == "expanded":
        base = _mask("b11k", B, H, Sq, Sk).to(torch.uint8).to(DEV)
        view = base.expand(B, H, Sq, Sk)
        assert view.stride() == (Sk, 0, 0, 1)
    else:
        wide = torch.zeros(B, 1, Sq, 2 * Sk, dtype=torch.uint8)
        wide[..., 0::2] = _mask("b1qk", B, H, Sq, Sk).to(torch.uint8)
        wide[..., 1::2] = 1 - wide[..., 0::2]                         # the bytes in between say the opposite
        base = wide.to(DEV)
        view = base[..., 0::2]
        assert view.stride(3) == 2
    _words_and_bytes(f"(f) {form} D{D}", "bf16" if D == 128 else "fp16", D, B, H, Sq, Sk, raw_mask=(view, view.cpu().bool()), causal=form == "strided",
                     seed=8650)


# ---- (g) layouts ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [64, 128])
def test_operands_in_a_fused_qkv_buffer(D):
    B, S, H = 2, 136, 4
    for dt in ("bf16", "fp16"):
        fused = torch.stack(synth.qkv(B, H, S, S, D, 8700, dt), dim=2)                    # [B, S, 3, H, D]
        fused[:, :, 0] = (fused[:, :, 0].float() * 2.5).to(fused.dtype)
        fd = fused.to(DEV)
        ops_ = tuple(t[:, :, i].permute(0, 2, 1, 3) for t in (fused, fd) for i in (0, 1))
        assert ops_[2].stride() == (S * 3 * H * D, D, 3 * H * D, 1)
        for wdt in (torch.float32, "16"):
            _run(f"(g) fused {dt} D{D}", dt, D, B, H, S, S, wdt, causal=True, operands=ops_)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("H, Hkv", [(4, 2), (6, 2), (4, 1)], ids=["group2", "group3", "one-kv-head"])
def test_grouped_query_heads(H, Hkv, D):
    for wdt in (torch.float32, "16"):
        _run(f"(g) H{H}/{Hkv} D{D}", "fp16" if D == 64 else "bf16", D, 2, H, 100, 136, wdt, Hkv=Hkv, causal=Hkv == 2, seed=8710)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("wdt", [torch.float32, "16"], ids=["w32", "w16"])
@pytest.mark.parametrize("layout", ["odd-row-stride", "base-off-by-one", "base-off-by-16-bytes"])
def test_weights_strides_and_base(layout, wdt, D):
    """Sk = 128 is all fast path for an aligned W.  A row stride that is no multiple of 16 bytes (pad 1 / 3) or a base one element off
    (which also takes the tail's scalar stores) sends every key down the per-lane path; a base 16 bytes in keeps the fast path."""
    n16 = 4 if wdt == torch.float32 else 8
    pad, off = {"odd-row-stride": (1 if wdt == torch.float32 else 3, 0), "base-off-by-one": (n16 - 1, 1), "base-off-by-16-bytes": (n16, n16)}[layout]
    for causal in (False, True):
        _run(f"(g) {layout} D{D} causal={causal}", "bf16" if D == 64 else "fp16", D, 2, 2, 100, 128, wdt, causal=causal, pad=pad, col_off=off,
             seed=8720)


# ---- (h) end to end: the forward's LSE into the weights pass ---------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_forward_then_weights(dt, D):
    B, H, S, lens = 2, 2, 200, [200, 77]
    q, k, v = (t.permute(0, 2, 1, 3) for t in synth.qkv(B, H, S, S, D, 8800, dt))
    q = (q.float() * 2.5).to(q.dtype)
    qd, kd, vd = (t.to(DEV) for t in (q, k, v))
    vis = visible(B, H, S, S, causal=True, seqlens=lens)
    for wdt in (torch.float32, DT[dt]):
        _, lse, w = ops.fa3_forward(qd, kd, vd, causal=True, seqlens_k=lens, return_lse=True, return_weights=True, weights_dtype=wdt)
        torch.cuda.synchronize()
        ref, lse32 = weights_reference(q, k, causal=True, seqlens=lens, lse32=lse)          # the kernel's own LSE: the weights pass alone
        check_weights(w, ref, weights_bound(q, k, ref, lse32, wdt=wdt), vis, f"(h) {dt} D{D}", wdt=wdt)
        if wdt == torch.float32:
            sums = w.double().sum(-1).cpu()
            assert float((sums - 1).abs().max()) <= 1e-3                                    # every row sees key 0: all are live
    out, w = ops.fa3_attention(qd.requires_grad_(True), kd, vd, causal=True, seqlens_k=lens, return_weights=True)
    assert out.requires_grad and not w.requires_grad and w.grad_fn is None and tuple(w.shape) == (B, H, S, S)

"""Host side of the hot path: tensor -> C-ABI argument marshalling for ``pfa_fa3_fwd``.

``fa3_forward`` has the call shape of the reference seam
``FlashAttention3._flash_attention_forward(q, k, v, attention_mask, need_weights)``
(core/flash_attention_3.py:120-150): operands are ``[B, H, S, D]`` tensors (usually strided
views of the fused QKV projection, :97-99), the result is ``[B, H, Sq, D]``.  The kernel
reads the views in place and writes a ``[B, Sq, H, D]`` buffer, returned as the transposed
view, so the reference's ``.transpose(1, 2).contiguous()`` at :107 costs nothing.

No fallback lives here: unsupported arguments raise ``ValueError`` (pre-launch
``pfa_status``) or ``PfaError``.
"""

from __future__ import annotations

import ctypes as C
import math
import operator
import threading
from typing import NamedTuple, Optional, Tuple

import torch

from . import _capi, _capi_qk_norm, _capi_rotary, _capi_sinks, _models
from ._models import (FP8, FP8_MAX, _attn_merge_model, _kv_append_model, _kv_append_q8_model, _packed_seqs, _page_copy_model,      # noqa: F401
                      _qk_norm_bwd_model, _qk_norm_model, _rope_append_model, _rope_rotate, _rotary_model, _sink_grad_model, _varlen_backward_model, _varlen_forward_model, dequantize_kv, quantize_kv)

_DT = {torch.bfloat16: _capi.PFA_DTYPE_BF16, torch.float16: _capi.PFA_DTYPE_FP16, torch.float32: _capi.PFA_DTYPE_FP32}

SUPPORTED_HEAD_DIMS = (64, 128)      # kernel instantiations; other head dims <= 128 run zero-padded to the next one


def _padded_head_dim(D: int) -> int:
    """Kernel head dim for a problem of head dim ``D`` (``D`` itself when a kernel exists for it)."""
    if D in SUPPORTED_HEAD_DIMS:
        return D
    if 1 <= D < SUPPORTED_HEAD_DIMS[-1]:
        return next(d for d in SUPPORTED_HEAD_DIMS if d > D)
    raise ValueError(f"head_dim {D} has no kernel (<= {SUPPORTED_HEAD_DIMS[-1]} supported)")


def _pad_d(t: torch.Tensor, Dp: int) -> torch.Tensor:
    """``[B,H,S,D]`` -> zero-padded ``[B,H,S,Dp]`` view of a fresh ``[B,S,H,Dp]`` buffer (zero q/k columns add nothing to the
    scores, zero v columns give zero output columns)."""
    B, H, S, D = t.shape
    buf = torch.zeros((B, S, H, Dp), dtype=t.dtype, device=t.device)
    buf[..., :D] = t.permute(0, 2, 1, 3)
    return buf.permute(0, 2, 1, 3)


def is_available(device: Optional[torch.device] = None) -> bool:
    """True when the native library is present and ``device`` is a gfx950 GPU."""
    if not torch.cuda.is_available():
        return False
    try:
        lib = _capi.load()
    except OSError:
        return False
    idx = torch.cuda.current_device() if device is None or device.index is None else device.index
    return lib.pfa_device_supported(int(idx)) == 1


_SEQLENS_CACHE: "dict[tuple, torch.Tensor]" = {}
_SEQLENS_LOCK = threading.Lock()      # the wrappers above this module are entered from several threads (hybrid_router's pool)


def _seqlens_tensor(seqlens_k, device) -> torch.Tensor:
    """``seqlens_k`` as a contiguous int32 device tensor.  Python lists are uploaded once per distinct value (a pageable
    host-to-device copy costs ~15 us per call, more than the C2 kernel); tensors are used as they are."""
    if isinstance(seqlens_k, torch.Tensor):
        return seqlens_k.to(device=device, dtype=torch.int32).contiguous()
    key = (tuple(int(x) for x in seqlens_k), str(device))
    with _SEQLENS_LOCK:
        t = _SEQLENS_CACHE.get(key)
        if t is None:
            if len(_SEQLENS_CACHE) >= 64:
                _SEQLENS_CACHE.clear()
            t = _SEQLENS_CACHE[key] = torch.tensor(key[0], dtype=torch.int32, device=device)
    return t


def _drop_mask_ptr(drop_mask, B, H, Sq, Sk, like) -> int:
    """keep-mask of the dense branch's attention dropout: contiguous u8 / bool [B,H,Sq,Sk] on the operands' device, fp32 kernels only"""
    if like.dtype != torch.float32:
        raise ValueError("attention dropout runs on the fp32 kernels: hand over fp32 operands")
    if drop_mask.shape != (B, H, Sq, Sk) or drop_mask.dtype not in (torch.uint8, torch.bool) or not drop_mask.is_contiguous() \
            or drop_mask.device != like.device:
        raise ValueError("drop_mask must be a contiguous u8 / bool [B, H, Sq, Sk] tensor on the operands' device")
    return drop_mask.data_ptr()


def _bhsd_strides(t: torch.Tensor):
    sb, sh, ss, sd = t.stride()
    if sd != 1 and t.shape[3] != 1:
        raise ValueError("last (head_dim) stride must be 1")
    return sb, sh, ss


def _as_mask4(mask: torch.Tensor, B: int, H: int, Sq: int, Sk: int, device) -> torch.Tensor:
    """Normalise a reference-style mask (0 = masked) to a u8 tensor broadcastable as [B,H,Sq,Sk].
    2-D [B,Sk] -> [B,1,1,Sk] (flash_attention_3.py:166-167); 3-D [B,Sq|1,Sk] -> [B,1,Sq|1,Sk]; 4-D as is."""
    if mask.dim() == 2:
        mask = mask[:, None, None, :]
    elif mask.dim() == 3:
        mask = mask[:, None, :, :]
    elif mask.dim() != 4:
        raise ValueError(f"attention mask must be 2-D, 3-D or 4-D, got {mask.dim()}-D")
    for got, want, name in zip(mask.shape, (B, H, Sq, Sk), "BHQK"):
        if got not in (1, want):
            raise ValueError(f"mask dim {name} is {got}, expected 1 or {want}")
    if mask.shape[3] != Sk:
        mask = mask.expand(-1, -1, -1, Sk)
    dev = device if isinstance(device, torch.device) else torch.device(device)
    if mask.dtype == torch.bool and mask.device == dev:
        m = mask.view(torch.uint8)            # bools are 0 / 1 bytes already: no conversion pass over the mask
    elif mask.dtype == torch.uint8 and mask.device == dev:
        m = mask                              # the kernels test for non-zero
    else:
        m = (mask != 0).to(device=device, dtype=torch.uint8)
    if m.stride(3) not in (0, 1) or (m.shape[3] > 1 and m.stride(3) == 0):
        m = m.contiguous()
    return m


def _set_element_mask(a, mask, B: int, H: int, Sq: int, Sk: int, device, keep: list) -> None:
    """The element-mask fields of ``pfa_fa3_args`` / ``pfa_fa3_bwd_args``: the ``_as_mask4`` form of ``mask`` (appended to ``keep``)
    with its byte strides, 0 for a broadcast dim."""
    m4 = _as_mask4(mask, B, H, Sq, Sk, device)
    a.mask = m4.data_ptr()
    st = [0 if m4.shape[i] == 1 else m4.stride(i) for i in range(4)]
    a.mask_stride_b, a.mask_stride_h, a.mask_stride_q, a.mask_stride_k = st[0], st[1], st[2], (st[3] or 1)
    keep.append(m4)


_STRIDE_FIELDS = {name: tuple(f"{'do' if name == 'dout' else name}_stride_{axis}" for axis in "bhs")
                  for name in ("q", "k", "v", "o", "dout", "dq", "dk", "dv")}


def _set_strides(a, fields) -> None:
    """``fields``: (pointer field, tensor) pairs of ``[B,H,S,D]``-shaped tensors -> the pointers and the ``*_stride_b/h/s`` triplets
    (``dout``'s strides are the ``do_stride_*`` fields)."""
    for name, t in fields:
        setattr(a, name, t.data_ptr())
        fb, fh, fs = _STRIDE_FIELDS[name]
        sb, sh, ss = _bhsd_strides(t)
        setattr(a, fb, sb); setattr(a, fh, sh); setattr(a, fs, ss)


# pointer field -> the prefix of its ``*_stride_*`` fields, over all blocks; and per (pointer field, axis letters in a block's order) the
# (stride field, tensor dim) pairs: "bhs" / "bsh" name the dims of a [B,H,S,D]-shaped tensor, "sh" those of packed [total,heads,D] rows
_STRIDE_PREFIX = {**{n: n for n in ("q", "k", "v", "o", "dq", "dk", "dv")}, "dout": "do", "k_cache": "k", "v_cache": "v", "k_pool": "k",
                  "v_pool": "v", "k_new": "kn", "v_new": "vn", "q_out": "qo"}
_VIEW_FIELDS = {(name, axes): tuple((f"{pre}_stride_{x}", ("bhs" if "b" in axes else "sh").index(x)) for x in axes)
                for axes in ("bhs", "bsh", "sh") for name, pre in _STRIDE_PREFIX.items()}


def _set_view(a, name: str, t: torch.Tensor, axes: str = "bhs") -> None:
    """``_set_strides`` for every other block: ``t``'s pointer into field ``name`` and, for each letter of ``axes`` (the block's own
    order of them), the stride of the axis it names into that ``*_stride_<letter>`` field.  The head dim must be contiguous."""
    st = t.stride()
    if st[-1] != 1 and t.shape[-1] != 1:
        raise ValueError("last (head_dim) stride must be 1")
    setattr(a, name, t.data_ptr())
    for field, dim in _VIEW_FIELDS[name, axes]:
        setattr(a, field, st[dim])


def _set_block_table(a, block_table, page_size: int, num_pages: int) -> None:
    """The four paging fields of a block over a KV cache; nothing without a table."""
    if block_table is not None:
        a.block_table, a.block_table_stride_b = block_table.data_ptr(), block_table.stride(0)
        a.page_size, a.num_pages = page_size, num_pages


def _attach_workspace(a, nbytes, device, keep: list, field: str = "workspace") -> None:
    """``nbytes`` (what the library asked for) of fresh device scratch into ``field`` / ``{field}_bytes``, kept in ``keep``; nothing for 0."""
    nbytes = int(nbytes)
    if nbytes:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        setattr(a, field, ws.data_ptr())
        setattr(a, field + "_bytes", nbytes)
        keep.append(ws)


def _hold(keep, stream) -> None:
    """Tensors made for a call must outlive the kernels enqueued on ``stream``."""
    for t in keep:
        t.record_stream(stream)


def _host_int(value):
    """``value`` as a host integer, or None for a bool and for anything without ``__index__``."""
    if isinstance(value, bool):
        return None
    try:
        return operator.index(value)
    except TypeError:
        return None


def _lse_ptr(lse: torch.Tensor, B: int, H: int, Sq: int) -> int:
    if lse.shape != (B, H, Sq) or lse.dtype != torch.float32 or not lse.is_contiguous():
        raise ValueError("lse must be contiguous fp32 [B, H, Sq]")
    return lse.data_ptr()


def _scale(softmax_scale: Optional[float], D: int) -> float:
    """The softmax scale handed to the library: the caller's, or ``1 / sqrt(D)``."""
    return float(D ** -0.5 if softmax_scale is None else softmax_scale)


_ARANGE1 = {}


def _mask_bound(km: torch.Tensor) -> torch.Tensor:
    """int32 [B]: 1 + the index of the last non-zero byte of every row of a [B, Sk] uint8 mask (0 for an empty row)."""
    if km.is_cuda and torch.cuda.is_current_stream_capturing():     # nothing allocated inside a graph capture is kept across calls
        idx = torch.arange(1, km.shape[1] + 1, dtype=torch.int32, device=km.device)
        return (idx * (km != 0)).amax(dim=1).to(torch.int32)
    key = (km.shape[1], str(km.device))
    with _SEQLENS_LOCK:
        idx = _ARANGE1.get(key)
        if idx is None:
            if len(_ARANGE1) > 64:
                _ARANGE1.clear()
            idx = _ARANGE1[key] = torch.arange(1, km.shape[1] + 1, dtype=torch.int32, device=km.device)
    return (idx * (km != 0)).amax(dim=1).to(torch.int32)


def build_args(q, k, v, out, *, causal=False, seqlens_k=None, key_mask=None, softmax_scale=None,
               lse=None, split_p=False, variant=0, mask=None, drop_mask=None, drop_scale=1.0):
    """Fill a ``pfa_fa3_args`` from ``[B,H,S,D]``-shaped (arbitrarily strided) tensors."""
    B, H, Sq, D = q.shape
    Sk, Hkv = k.shape[2], k.shape[1]
    # grouped-query attention: k, v may carry H / g heads (query head h reads K/V head h // g); nothing is expanded
    if Hkv < 1 or H % Hkv or k.shape != (B, Hkv, Sk, D) or v.shape != (B, Hkv, Sk, D):
        raise ValueError(f"shape mismatch: q {tuple(q.shape)} k {tuple(k.shape)} v {tuple(v.shape)}")
    if out.shape != (B, H, Sq, D):
        raise ValueError("output shape mismatch")
    if q.dtype not in (torch.bfloat16, torch.float16, torch.float32) or k.dtype != q.dtype or v.dtype != q.dtype:
        raise ValueError("q, k, v must share dtype bf16, fp16 or fp32 (fp32: the exact, slow kernel)")
    if out.dtype not in (q.dtype, torch.float32):
        raise ValueError("output dtype must be the input dtype or fp32")
    if q.dtype == torch.float32 and (split_p or variant):
        raise ValueError("fp32 operands run the exact fp32 kernel: no split P, no kernel selector")
    if not (q.is_cuda and k.is_cuda and v.is_cuda and out.is_cuda):
        raise ValueError("pfa_fa3_fwd needs device tensors (there is no CPU path)")
    a = _capi.make_args(
        flags=(_capi.PFA_FLAG_SPLIT_P if split_p else 0) | ((int(variant) & 0xFF) << 8),
        B=B, H=H, Sq=Sq, Sk=Sk, D=D,
        dtype_in=_DT[q.dtype], dtype_out=_DT[out.dtype], causal=1 if causal else 0,
        softmax_scale=_scale(softmax_scale, D),
        device_id=_device_index(q.device),
        kv_group=H // Hkv,
    )
    _set_strides(a, (("q", q), ("k", k), ("v", v), ("o", out)))
    keep = []
    if seqlens_k is not None:
        sl = _seqlens_tensor(seqlens_k, q.device)
        if sl.numel() != B:
            raise ValueError("seqlens_k must have B entries")
        a.seqlens_k = sl.data_ptr()
        keep.append(sl)
    if key_mask is not None:
        km = key_mask
        if km.shape != (B, Sk):
            raise ValueError("key_mask must be [B, Sk]")
        if km.dtype == torch.bool and km.device == q.device:
            km = km.contiguous().view(torch.uint8)          # bools are 0 / 1 bytes already: no conversion kernel
        else:
            km = (km != 0).to(device=q.device, dtype=torch.uint8).contiguous()
        a.key_mask = km.data_ptr()
        a.key_mask_stride_b = km.stride(0)
        keep.append(km)
        # A padding mask's tail is dead weight the kernel cannot see coming (it reads the bytes two tiles ahead): hand it, as seqlens_k,
        # the position behind each row's LAST visible key -- two small device ops, no sync, nothing changes in the result (those keys are
        # masked anyway) -- and the persistent kernel cuts every item's tile count to it.  Only where that kernel takes the problem and
        # the launch is long enough to carry the two extra ops (>= ~0.15 ms of attention).
        if (seqlens_k is None and (not causal or Sq == Sk) and q.dtype != torch.float32 and D in (64, 128) and Sq >= 128 and Sk >= 193
                and 4.0 * B * H * Sq * Sk * D >= 1.5e11):       # (under the causal mask too since round 3: the padded decoder batch)
            sl = _mask_bound(km)
            a.seqlens_k = sl.data_ptr()
            keep.append(sl)
    if mask is not None:
        if key_mask is not None:
            raise ValueError("pass either key_mask or mask")
        _set_element_mask(a, mask, B, H, Sq, Sk, q.device, keep)
    if key_mask is not None or mask is not None:
        # scratch for the mask condensed to one 64-bit word per row and 64-key tile (pfa_fa3_workspace_bytes; optional for the
        # C ABI, always given here): a padding mask then costs about what seqlens_k costs, an element mask 1/3 of the byte path
        _attach_workspace(a, _capi.load().pfa_fa3_workspace_bytes(C.byref(a)), q.device, keep)
    if lse is not None:
        a.lse = _lse_ptr(lse, B, H, Sq)
    if drop_mask is not None:
        a.drop_mask, a.drop_scale = _drop_mask_ptr(drop_mask, B, H, Sq, Sk, q), float(drop_scale)
        keep.append(drop_mask)
    return a, keep


def fa3_forward(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, *, causal: bool = False,
                seqlens_k=None, key_mask: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None,
                softmax_scale: Optional[float] = None, out_dtype: Optional[torch.dtype] = None,
                return_lse: bool = False, return_weights: bool = False, weights_dtype: Optional[torch.dtype] = None,
                split_p: Optional[bool] = None, drop_mask: Optional[torch.Tensor] = None, drop_scale: float = 1.0,
                out: Optional[torch.Tensor] = None, sinks: Optional[torch.Tensor] = None,
                _variant: Optional[int] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """softmax(scale * q k^T + mask) v on the MI355X kernel.

    q: ``[B,H,Sq,D]``, k/v: ``[B,H,Sk,D]`` (any batch/head/seq strides that are multiples of 8
    elements; head_dim contiguous).  Returns ``(out [B,H,Sq,D] view of a [B,Sq,H,D] buffer, lse or None)``;
    with ``return_weights=True`` a third element, the softmax matrix ``[B,H,Sq,Sk]`` (second kernel pass,
    the reference's ``need_weights``).  ``mask``: any 2-/3-/4-D reference-style mask (0 = masked);
    ``key_mask``: the cheaper ``[B,Sk]`` special case.

    ``out_dtype=torch.float32`` selects the parity variant: fp32 store and, unless
    ``split_p=False`` is forced, P carried as bf16 hi+lo so the result is within 1e-3 of the
    fp32 reference ("numerics").

    ``sinks``: fp32 ``[H]`` on q's device, one learned attention sink per query head in the units of the scaled scores -- one more key of
    that score and a zero value row in every row's softmax, inside the returned LSE (``pfa_fa3_fwd_sink``).  A row with no
    visible key gets O = 0 and LSE = the sink; a ``-inf`` sink gives its head the bits of the sink-less 8-wave call.  Runs the 8-wave
    kernel only; 16-bit operands; refused with dropout and ``return_weights``.
    """
    B, H, Sq, D = q.shape
    snk = _sinks_arg(sinks, q)
    if snk is not None:
        if q.dtype == torch.float32:
            raise ValueError("sinks need bf16 / fp16 operands: the exact fp32 kernels carry no sink")
        if drop_mask is not None:
            raise ValueError("sinks do not combine with attention dropout (drop_mask)")
        if return_weights:
            raise ValueError("sinks do not combine with return_weights: the weights pass carries no sink")
    Dp = _padded_head_dim(D)
    if Dp != D:
        # no kernel instantiation for this head dim: run the next larger one on zero-padded operands (same scores, the
        # extra output columns are zero and dropped).  The scale stays the TRUE head dim's.
        res = fa3_forward(_pad_d(q, Dp), _pad_d(k, Dp), _pad_d(v, Dp), causal=causal, seqlens_k=seqlens_k,
                          key_mask=key_mask, mask=mask,
                          softmax_scale=_scale(softmax_scale, D), out_dtype=out_dtype,
                          return_lse=return_lse, return_weights=return_weights, weights_dtype=weights_dtype,
                          split_p=split_p, drop_mask=drop_mask, drop_scale=drop_scale, sinks=sinks, _variant=_variant)
        o = res[0][..., :D]
        if out is not None:
            out.copy_(o)
            o = out
        return (o,) + tuple(res[1:])
    if _variant is None:   # tools / tests only: kernel selector (include/pfa_hip.h PFA_FLAG_VARIANT_MASK); never read from the environment
        _variant = 0
    odt = q.dtype if out_dtype is None else out_dtype
    if q.dtype == torch.float32:
        # exact fp32 kernel (csrc/fa3_fwd_f32_kernel.h): every product and sum in fp32, ~two orders of magnitude slower than the
        # MFMA path; the softmax matrix, if wanted, comes from a 16-bit pass of its own (the weights kernel is MFMA only)
        if return_weights:
            raise ValueError("return_weights with fp32 operands: call again with 16-bit operands for the weights")
        if split_p or _variant:
            raise ValueError("fp32 operands run the exact fp32 kernel: no split P, no kernel selector")
        split_p = False
    elif split_p is None:
        split_p = odt == torch.float32
    if out is None:
        out = torch.empty((B, Sq, H, D), dtype=odt, device=q.device).permute(0, 2, 1, 3)
    lse = torch.empty((B, H, Sq), dtype=torch.float32, device=q.device) if (return_lse or return_weights) else None
    args, keep = build_args(q, k, v, out, causal=causal, seqlens_k=seqlens_k, key_mask=key_mask, mask=mask,
                            softmax_scale=softmax_scale, lse=lse, split_p=split_p, variant=_variant,
                            drop_mask=drop_mask, drop_scale=drop_scale)
    held = torch.cuda.current_stream(q.device)
    stream = held.cuda_stream
    if snk is None:
        st = _capi.load().pfa_fa3_fwd(C.byref(args), C.c_void_p(stream))
        _raise_status("pfa_fa3_fwd", st)
    else:
        st = _capi_sinks.load().pfa_fa3_fwd_sink(C.byref(args), C.byref(snk), C.c_void_p(stream))
        _raise_status("pfa_fa3_fwd_sink", st)
    weights = None
    if return_weights:
        Sk = k.shape[2]
        wdt = q.dtype if weights_dtype is None else weights_dtype
        weights = torch.empty((B, H, Sq, Sk), dtype=wdt, device=q.device)     # the kernel writes every element, masked ones as zeros
        stw = _capi.load().pfa_fa3_weights(C.byref(args), C.c_void_p(weights.data_ptr()), _DT[wdt],
                                           weights.stride(0), weights.stride(1), weights.stride(2), C.c_void_p(stream))
        _raise_status("pfa_fa3_weights", stw)
    if keep:
        _hold(keep, held)
    if return_weights:
        return out, (lse if return_lse else None), weights
    return out, lse


def fa3_forward_bshd(q, k, v, **kw):
    """Same, for operands laid out ``[B,S,H,D]``; returns ``[B,Sq,H,D]`` (+ lse)."""
    res = fa3_forward(q.permute(0, 2, 1, 3), k.permute(0, 2, 1, 3), v.permute(0, 2, 1, 3), **kw)
    return (res[0].permute(0, 2, 1, 3),) + tuple(res[1:])


def _dout_meets_abi(dout: torch.Tensor, D: int) -> bool:
    """``pfa_fa3_bwd``'s rules for ``dout`` (check_bwd in csrc/pfa_bwd_capi.hip): head dim contiguous, read in 16-byte pieces --
    base 16-byte aligned, every stride a multiple of 8 elements (fp32: 4) -- and, on the fp32 kernels, rows at least ``D`` apart.
    Autograd hands over whatever view the loss produced (a slice of a wider tensor, a broadcast): what fails a rule is copied."""
    unit = 16 // dout.element_size()
    sb, sh, ss, sd = dout.stride()
    return (sd == 1 and dout.data_ptr() % 16 == 0 and sb % unit == 0 and sh % unit == 0 and ss % unit == 0
            and (dout.dtype != torch.float32 or ss >= D))


def fa3_backward(q, k, v, out, dout, lse, *, causal: bool = False, seqlens_k=None, key_mask=None, mask=None,
                 softmax_scale: Optional[float] = None, grad_dtype: Optional[torch.dtype] = None,
                 drop_mask: Optional[torch.Tensor] = None, drop_scale: float = 1.0, sinks: Optional[torch.Tensor] = None):
    """dQ, dK, dV of ``fa3_forward`` (``pfa_fa3_bwd``).  All operands ``[B,H,S,D]``-shaped (any strides, head dim
    contiguous), ``lse`` the forward's ``[B,H,Sq]`` fp32 LSE.  Returns gradients as ``[B,H,S,D]`` views of
    ``[B,S,H,D]`` buffers, in ``grad_dtype`` (input dtype by default, or fp32).  ``key_mask`` / ``mask``: the masks
    the forward was called with (same conventions as ``fa3_forward``).  Grouped-query heads: ``k`` / ``v`` may hold ``H / g`` heads as in
    the forward; ``dk`` / ``dv`` then have ``H / g`` heads too (summed over each group inside the dK/dV kernel, ABI v7).

    ``sinks``: the forward's sinks; ``out`` and ``lse`` are then that forward's.  The backward kernels run unchanged (the LSE holds the
    sink, its value row is zero), ``fa3_sink_grad`` follows on the same stream and the same ``delta``, and the result is
    ``(dq, dk, dv, d_sinks)`` with ``d_sinks`` fp32 ``[H]``."""
    B, H, Sq, D = q.shape
    Sk = k.shape[2]
    Hkv = k.shape[1]
    if _sinks_arg(sinks, q) is not None and (q.dtype == torch.float32 or drop_mask is not None):
        raise ValueError("sinks need bf16 / fp16 operands and do not combine with attention dropout")
    if v.shape[1] != Hkv or Hkv <= 0 or H % Hkv:
        raise ValueError(f"k / v carry {k.shape[1]} / {v.shape[1]} heads: both must hold H / g heads for an integer g (H = {H})")
    if Hkv != H and q.dtype == torch.float32:
        # the exact-fp32 kernels take one K/V head per query head: expand, and sum dK / dV over each group here
        g = H // Hkv
        dq, dk, dv = fa3_backward(q, k.repeat_interleave(g, dim=1), v.repeat_interleave(g, dim=1), out, dout, lse, causal=causal,
                                  seqlens_k=seqlens_k, key_mask=key_mask, mask=mask, softmax_scale=softmax_scale, grad_dtype=grad_dtype,
                                  drop_mask=drop_mask, drop_scale=drop_scale)
        return dq, dk.reshape(B, Hkv, g, Sk, D).sum(2), dv.reshape(B, Hkv, g, Sk, D).sum(2)
    Dp = _padded_head_dim(D)
    if Dp != D:   # as in fa3_forward: zero-padded head dim; the gradients' extra columns are exactly zero and dropped
        grads = fa3_backward(_pad_d(q, Dp), _pad_d(k, Dp), _pad_d(v, Dp), _pad_d(out, Dp), _pad_d(dout, Dp), lse,
                             causal=causal, seqlens_k=seqlens_k, key_mask=key_mask, mask=mask,
                             softmax_scale=_scale(softmax_scale, D),
                             grad_dtype=grad_dtype, drop_mask=drop_mask, drop_scale=drop_scale, sinks=sinks)
        return tuple(g[..., :D] for g in grads[:3]) + tuple(grads[3:])
    gdt = q.dtype if grad_dtype is None else grad_dtype
    if not _dout_meets_abi(dout, D):
        dout = dout.contiguous()
    dq = torch.empty((B, Sq, H, D), dtype=gdt, device=q.device).permute(0, 2, 1, 3)
    dk = torch.empty((B, Sk, Hkv, D), dtype=gdt, device=q.device).permute(0, 2, 1, 3)      # grouped-query heads: dK / dV summed over
    dv = torch.empty((B, Sk, Hkv, D), dtype=gdt, device=q.device).permute(0, 2, 1, 3)      # each group inside the kernel (ABI v7)
    delta = torch.empty((B, H, Sq), dtype=torch.float32, device=q.device)
    a = _capi.PfaFa3BwdArgs()
    a.size = C.sizeof(_capi.PfaFa3BwdArgs)
    _set_strides(a, (("q", q), ("k", k), ("v", v), ("o", out), ("dout", dout), ("dq", dq), ("dk", dk), ("dv", dv)))
    a.lse, a.delta = _lse_ptr(lse, B, H, Sq), delta.data_ptr()
    keep = [delta]
    if seqlens_k is not None:
        sl = _seqlens_tensor(seqlens_k, q.device)
        a.seqlens_k = sl.data_ptr()
        keep.append(sl)
    if key_mask is not None:
        if mask is not None:
            raise ValueError("pass either key_mask or mask")
        if key_mask.shape != (B, Sk):
            raise ValueError("key_mask must be [B, Sk]")
        mask = key_mask
    if mask is not None:
        _set_element_mask(a, mask, B, H, Sq, Sk, q.device, keep)
    if drop_mask is not None:
        a.drop_mask, a.drop_scale = _drop_mask_ptr(drop_mask, B, H, Sq, Sk, q), float(drop_scale)
        keep.append(drop_mask)
    a.B, a.H, a.Sq, a.Sk, a.D = B, H, Sq, Sk, D
    a.kv_group = H // Hkv
    a.dtype, a.dtype_grad, a.causal = _DT[q.dtype], _DT[gdt], 1 if causal else 0
    a.softmax_scale = _scale(softmax_scale, D)
    a.device_id = _device_index(q.device)
    stream = torch.cuda.current_stream(q.device)
    if a.mask:   # element masks: scratch for the condensed words / tile ranges (0 bytes for key-only masks; optional for the library)
        _attach_workspace(a, _capi.load().pfa_fa3_bwd_mask_workspace_bytes(C.byref(a)), q.device, keep, "mask_workspace")
    st = _capi.load().pfa_fa3_bwd(C.byref(a), C.c_void_p(stream.cuda_stream))
    _raise_status("pfa_fa3_bwd", st)
    _hold(keep, stream)
    if sinks is not None:
        return dq, dk, dv, fa3_sink_grad(lse, delta, sinks)
    return dq, dk, dv


def fa3_sink_grad(lse: torch.Tensor, delta: torch.Tensor, sinks: torch.Tensor, *, cu_seqlens_q: Optional[torch.Tensor] = None,
                  max_seqlen_q: Optional[int] = None) -> torch.Tensor:
    """The gradient of the attention sinks (``pfa_fa3_sink_grad``): ``d_sinks[h] = - sum_rows exp(sinks[h] - lse) * delta``, fp32 ``[H]``.

    ``lse``: the LSE of a forward with ``sinks``; ``delta``: ``rowsum(dO o O)`` as the backward leaves it.  Dense: both contiguous fp32
    ``[B, H, Sq]``.  Packed (``cu_seqlens_q`` int32 ``[B + 1]`` on the device, ``max_seqlen_q`` a host int): both contiguous ``[H, total_q]``;
    rows no sequence covers are not read.  Rows with ``lse = -inf`` are skipped, a ``-inf`` sink gets gradient 0.  Two launches on q's
    current stream, no atomics, bitwise reproducible; grids from host shapes only (capturable, valid while the sink values change).
    On CPU tensors the same rule runs in plain torch (the executable specification)."""
    packed = cu_seqlens_q is not None
    if lse.dim() != (2 if packed else 3) or delta.shape != lse.shape or lse.dtype != torch.float32 or delta.dtype != torch.float32 \
            or not lse.is_contiguous() or not delta.is_contiguous() or delta.device != lse.device:
        raise ValueError("lse and delta must be contiguous fp32 tensors of one shape, [B, H, Sq] or packed [H, total_q], on one device")
    H = lse.shape[0] if packed else lse.shape[1]
    if not isinstance(sinks, torch.Tensor) or sinks.dtype != torch.float32 or sinks.shape != (H,) or not sinks.is_contiguous() \
            or sinks.device != lse.device:
        raise ValueError(f"sinks must be a contiguous fp32 [H] = [{H}] tensor on the device of lse")
    if packed:
        if cu_seqlens_q.dtype != torch.int32 or cu_seqlens_q.dim() != 1 or cu_seqlens_q.numel() < 2 or not cu_seqlens_q.is_contiguous() \
                or cu_seqlens_q.device != lse.device:
            raise ValueError("cu_seqlens_q must be a contiguous int32 [B + 1] tensor on the device of lse")
        B, total_q, Sq = cu_seqlens_q.numel() - 1, lse.shape[1], operator.index(max_seqlen_q)
        if not 1 <= Sq <= total_q:
            raise ValueError(f"max_seqlen_q {Sq}: must lie in 1 .. {total_q}")
    else:
        (B, _, Sq), total_q = lse.shape, 0
    d_sinks = torch.empty((H,), dtype=torch.float32, device=lse.device)
    if lse.device.type == "cpu":
        rows = [sq[:2] for sq in _packed_seqs(cu_seqlens_q.tolist(), cu_seqlens_q.tolist(), total_q, total_q, Sq, Sq)] if packed else None
        _sink_grad_model(lse, delta, sinks.detach(), d_sinks, rows)
        return d_sinks
    a = _capi_sinks.make_sink_grad_args(lse=lse.data_ptr(), delta=delta.data_ptr(), sinks=sinks.data_ptr(), d_sinks=d_sinks.data_ptr(),
                                  B=B, H=H, Sq=Sq, total_q=total_q, device_id=_device_index(lse.device))
    if packed:
        a.cu_seqlens_q = cu_seqlens_q.data_ptr()
    else:
        a.lse_stride_b = a.delta_stride_b = H * Sq
        a.lse_stride_h = a.delta_stride_h = Sq
    keep = []
    _attach_workspace(a, _capi_sinks.load().pfa_fa3_sink_grad_workspace_bytes(C.byref(a)), lse.device, keep)
    stream = torch.cuda.current_stream(lse.device)
    st = _capi_sinks.load().pfa_fa3_sink_grad(C.byref(a), C.c_void_p(stream.cuda_stream))
    _raise_status("pfa_fa3_sink_grad", st, null_too=True)
    _hold(keep, stream)
    return d_sinks


class _FA3Function(torch.autograd.Function):
    """Differentiable ``fa3_forward`` (causal / seqlens_k / key / element masks): saves q, k, v, o and the LSE.
    ``out_dtype`` fp32 (fp32 modules) runs the parity forward (fp32 store) and keeps a 16-bit copy of O for the
    backward's delta = rowsum(dO o O)."""

    @staticmethod
    def forward(ctx, q, k, v, causal, seqlens_k, softmax_scale, key_mask, mask, out_dtype, want_weights, weights_dtype):
        res = fa3_forward(q, k, v, causal=causal, seqlens_k=seqlens_k, key_mask=key_mask, mask=mask,
                          softmax_scale=softmax_scale, return_lse=True, out_dtype=out_dtype,
                          return_weights=want_weights, weights_dtype=weights_dtype)
        out, lse = res[0], res[1]
        o16 = out if out.dtype == q.dtype else out.to(q.dtype)     # (fp32 operands: the fp32 kernels in both directions, nothing is narrowed)
        ctx.save_for_backward(q, k, v, o16, lse)
        ctx.causal, ctx.seqlens_k, ctx.softmax_scale = causal, seqlens_k, softmax_scale
        ctx.key_mask, ctx.mask = key_mask, mask          # masks carry no gradient
        if want_weights:
            # the softmax matrix from the second pass on the saved LSE: returned for inspection (nn.MultiheadAttention's
            # default need_weights=True), detached -- the gradient flows through the output only
            ctx.mark_non_differentiable(res[2])
            return out, res[2]
        return out

    @staticmethod
    def backward(ctx, dout, *_dweights):
        q, k, v, out, lse = ctx.saved_tensors
        dq, dk, dv = fa3_backward(q, k, v, out, dout.to(q.dtype), lse, causal=ctx.causal, seqlens_k=ctx.seqlens_k,
                                  key_mask=ctx.key_mask, mask=ctx.mask, softmax_scale=ctx.softmax_scale)
        return dq, dk, dv, None, None, None, None, None, None, None, None


class _FA3SinkFunction(torch.autograd.Function):
    """``_FA3Function`` with attention sinks (no weights): saves the sinks beside q, k, v, o and the LSE.  A sibling, so that the
    sink-less Function keeps its saved tensors and its launches.  ``sinks.requires_grad`` False: the backward skips the sink-grad launches."""

    @staticmethod
    def forward(ctx, q, k, v, sinks, causal, seqlens_k, softmax_scale, key_mask, mask, out_dtype):
        out, lse = fa3_forward(q, k, v, causal=causal, seqlens_k=seqlens_k, key_mask=key_mask, mask=mask, softmax_scale=softmax_scale,
                               return_lse=True, out_dtype=out_dtype, sinks=sinks)
        o16 = out if out.dtype == q.dtype else out.to(q.dtype)
        ctx.save_for_backward(q, k, v, o16, lse, sinks)
        ctx.causal, ctx.seqlens_k, ctx.softmax_scale = causal, seqlens_k, softmax_scale
        ctx.key_mask, ctx.mask = key_mask, mask
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, out, lse, sinks = ctx.saved_tensors
        grads = fa3_backward(q, k, v, out, dout.to(q.dtype), lse, causal=ctx.causal, seqlens_k=ctx.seqlens_k, key_mask=ctx.key_mask,
                             mask=ctx.mask, softmax_scale=ctx.softmax_scale, sinks=sinks if ctx.needs_input_grad[3] else None)
        return grads[0], grads[1], grads[2], (grads[3] if len(grads) > 3 else None), None, None, None, None, None, None


class _FA3DropoutFunction(torch.autograd.Function):
    """Attention with dropout on the softmax weights (the reference's dense branch, flash_attention_3.py:174-175), forward and
    backward on the fp32 kernels.  The keep-mask is drawn on the device with torch's generator (``torch.manual_seed`` governs it,
    as it governs ``nn.Dropout`` in the reference) and replayed by the backward."""

    @staticmethod
    def forward(ctx, q, k, v, p_drop, causal, softmax_scale, key_mask, mask):
        B, H, Sq, _ = q.shape
        Sk = k.shape[2]
        keep = torch.rand((B, H, Sq, Sk), device=q.device) >= p_drop
        scale = 1.0 / (1.0 - p_drop)
        q32, k32, v32 = q.float(), k.float(), v.float()
        out, lse = fa3_forward(q32, k32, v32, causal=causal, key_mask=key_mask, mask=mask, softmax_scale=softmax_scale,
                               return_lse=True, drop_mask=keep, drop_scale=scale)
        ctx.save_for_backward(q32, k32, v32, out, lse, keep)
        ctx.meta = (causal, softmax_scale, key_mask, mask, scale, q.dtype)
        return out.to(q.dtype)

    @staticmethod
    def backward(ctx, dout):
        q, k, v, out, lse, keep = ctx.saved_tensors
        causal, softmax_scale, key_mask, mask, scale, dt = ctx.meta
        dq, dk, dv = fa3_backward(q, k, v, out, dout.float(), lse, causal=causal, key_mask=key_mask, mask=mask,
                                  softmax_scale=softmax_scale, drop_mask=keep, drop_scale=scale)
        return dq.to(dt), dk.to(dt), dv.to(dt), None, None, None, None, None


def fa3_attention_dropout(q, k, v, p_drop: float, *, causal: bool = False, key_mask=None, mask=None,
                          softmax_scale: Optional[float] = None):
    """``dropout(softmax(scale q k^T + mask), p_drop) v`` on ``[B,H,S,D]`` operands of any float dtype, differentiable; fp32 kernels
    (meant for the short sequences of the reference's dense branch)."""
    if not 0.0 <= p_drop < 1.0:
        raise ValueError("dropout probability must be in [0, 1)")
    return _FA3DropoutFunction.apply(q, k, v, float(p_drop), causal, softmax_scale, key_mask, mask)


def fa3_attention(q, k, v, *, causal: bool = False, seqlens_k=None, key_mask=None, mask=None,
                  softmax_scale: Optional[float] = None, out_dtype: Optional[torch.dtype] = None,
                  return_weights: bool = False, weights_dtype: Optional[torch.dtype] = None, sinks: Optional[torch.Tensor] = None,
                  q_norm_weight: Optional[torch.Tensor] = None, k_norm_weight: Optional[torch.Tensor] = None, qk_norm_eps: float = 1e-6,
                  qk_norm_unit_offset: bool = False,
                  rotary_cos: Optional[torch.Tensor] = None, rotary_sin: Optional[torch.Tensor] = None, rotary_interleaved: bool = False,
                  pos_offsets: Optional[torch.Tensor] = None, position_ids: Optional[torch.Tensor] = None):
    """Autograd-aware attention on ``[B,H,S,D]`` bf16/fp16 operands: forward + backward on the HIP kernels.
    ``return_weights=True`` -> ``(out, weights)``; the weights are detached (no gradient flows through them).
    ``sinks``: fp32 ``[H]`` attention sinks (``fa3_forward``), differentiable: ``sinks.grad`` is ``fa3_sink_grad``'s result.
    ``rotary_cos`` / ``rotary_sin`` (with ``rotary_interleaved``, ``pos_offsets``, ``position_ids``): q and k are rotated first by
    ``apply_rotary`` -- one launch, two where ``Sq != Sk`` -- and the call is the one without them on the rotated operands, in both
    directions: the backward's dq and dk go through the conjugate launch.
    ``q_norm_weight`` / ``k_norm_weight`` (with ``qk_norm_eps``, ``qk_norm_unit_offset``): ``qk_norm`` takes the place of the
    ``apply_rotary`` step -- the norm of every head of q and k, and the rotation when tables are given, in the same launch (two where
    ``Sq != Sk``) -- and the call is the one without them on its outputs; the weights' gradients come from ``pfa_qk_norm_bwd``."""
    rot = _train_rotary_kw(rotary_cos, rotary_sin, rotary_interleaved, pos_offsets, position_ids)
    qkn = _train_qk_norm_kw(q_norm_weight, k_norm_weight, qk_norm_eps, qk_norm_unit_offset)
    if qkn is not None:
        qkn.update(rot or {})
        if q.dim() == 4 and k.dim() == 4 and q.shape[2] != k.shape[2]:
            q, k = qk_norm(q, q_weight=q_norm_weight, **qkn), qk_norm(k, q_weight=k_norm_weight, **qkn)
        else:
            q, k = qk_norm(q, k, q_weight=q_norm_weight, k_weight=k_norm_weight, **qkn)
    elif rot is not None:
        if q.dim() == 4 and k.dim() == 4 and q.shape[2] != k.shape[2]:
            q, k = apply_rotary(q, **rot), apply_rotary(k, **rot)
        else:
            q, k = apply_rotary(q, k, **rot)
    if sinks is not None:
        if return_weights:
            raise ValueError("sinks do not combine with return_weights: the weights pass carries no sink")
        return _FA3SinkFunction.apply(q, k, v, sinks, causal, seqlens_k, softmax_scale, key_mask, mask, out_dtype)
    return _FA3Function.apply(q, k, v, causal, seqlens_k, softmax_scale, key_mask, mask, out_dtype, bool(return_weights), weights_dtype)


def _device_index(device: torch.device) -> int:
    return device.index if device.index is not None else torch.cuda.current_device()


def _raise_status(entry: str, st: int, null_too: bool = False) -> None:
    """A non-zero status of the C entry point ``entry``: what the caller's arguments caused as ``ValueError`` (``null_too``: the
    calls over a KV cache count a missing pointer among them), anything else as ``PfaError``."""
    if st in (-3, -4, -5, -6, -7, -10) or (null_too and st == -1):
        raise ValueError(f"{entry}: {_capi.status_string(st)}")
    _capi.check_status(st)




def _kv_quant_arg(entry: str, k_cache, v_cache, k_descale, v_descale, B: int, Hkv: int, device):
    """The ``pfa_fa3_kv_quant`` block of a call over the caches, or None for 16-bit caches.  FP8 caches need both descales (fp32,
    contiguous, ``[Hkv]`` or ``[B, Hkv]``, on ``device``); 16-bit caches refuse them.  The block points into the caller's tensors, so a
    captured call sees their contents change."""
    if k_cache.dtype != FP8 and v_cache.dtype != FP8:
        if k_descale is not None or v_descale is not None:
            raise ValueError("k_descale / v_descale go with torch.float8_e4m3fn caches only")
        return None
    if k_cache.dtype != FP8 or v_cache.dtype != FP8:
        raise ValueError("k_cache and v_cache must both be torch.float8_e4m3fn")
    if k_descale is None or v_descale is None:
        raise ValueError(f"{entry}: torch.float8_e4m3fn caches need k_descale and v_descale (fp32 [Hkv] or [B, Hkv])")
    for name, d in (("k_descale", k_descale), ("v_descale", v_descale)):
        if not isinstance(d, torch.Tensor) or d.dtype != torch.float32 or d.shape not in ((Hkv,), (B, Hkv)) or not d.is_contiguous():
            raise ValueError(f"{name} must be a contiguous fp32 tensor [Hkv] = [{Hkv}] or [B, Hkv] = [{B}, {Hkv}]")
        if d.device != device:
            raise ValueError(f"{name} must live on the operands' device")
    if k_descale.shape != v_descale.shape:
        raise ValueError("k_descale and v_descale must have one shape")
    return _capi.make_kv_quant(k_descale=k_descale.data_ptr(), v_descale=v_descale.data_ptr(),
                               descale_stride_b=Hkv if k_descale.dim() == 2 else 0)


def _cache_geometry(name: str, rows, B, Hkv, D, k_cache, v_cache, block_table, H=None):
    """What every call over a KV cache, reading or writing, checks about its 4-D caches (or pools and block table) against B
    sequences of Hkv key heads and head dim D.  ``rows`` (printed as ``name``) is the tensor they are matched with: q, or k_new.
    The readers pass H: Hkv must divide it.  -> ``(Smax, page_size, num_pages)``, the paging pair 0 without a table."""
    Smax = k_cache.shape[2]
    page_size = num_pages = 0
    bad_heads = H is not None and (Hkv < 1 or H % Hkv)
    if block_table is None:
        if k_cache.shape != (B, Hkv, Smax, D) or v_cache.shape != k_cache.shape or bad_heads:
            raise ValueError(f"shape mismatch: {name} {tuple(rows.shape)} k_cache {tuple(k_cache.shape)} v_cache {tuple(v_cache.shape)}")
    else:
        num_pages, page_size = k_cache.shape[0], k_cache.shape[2]
        if k_cache.shape != (num_pages, Hkv, page_size, D) or v_cache.shape != k_cache.shape or num_pages < 1 or bad_heads:
            raise ValueError(f"shape mismatch: {name} {tuple(rows.shape)} k pool {tuple(k_cache.shape)} v pool {tuple(v_cache.shape)}")
        if page_size < 64 or page_size % 64:
            raise ValueError(f"page size {page_size}: must be a multiple of 64 keys")
        if not isinstance(block_table, torch.Tensor) or block_table.dtype != torch.int32:
            raise ValueError("block_table must be an int32 tensor")
        if block_table.dim() != 2 or block_table.shape[0] != B or block_table.shape[1] < 1:
            raise ValueError(f"block_table must be [B, max_pages] with B = {B}, got {tuple(block_table.shape)}")
        if block_table.stride(1) != 1 and block_table.shape[1] != 1:
            raise ValueError("block_table: the last dim must be contiguous")
        Smax = block_table.shape[1] * page_size
    return Smax, page_size, num_pages


class _CacheOperands(NamedTuple):
    """``_cache_operands``' result."""
    Hkv: int
    Smax: int
    page_size: int
    num_pages: int
    odt: torch.dtype


def _rank4(*tensors) -> None:
    """The 4-D rule of the uniform calls over a KV cache, for the operands given."""
    for t in tensors:
        if t.dim() != 4:
            raise ValueError("q, k_cache, v_cache must be 4-D ([B,H,Sq,D], [B,Hkv,Smax,D])")


def _out_arg(out, shape, odt, device) -> None:
    """A caller's ``out=`` of the uniform calls over a KV cache against the result's shape, dtype and device."""
    if out.shape != shape or out.dtype != odt or out.device != device:
        raise ValueError("out must be a [B, H, Sq, D] tensor of the output dtype on the operands' device")


def _cache_operands(entry: str, q, B, H, D, k_cache, v_cache, out_dtype, block_table, fp8=False) -> _CacheOperands:
    """What the attention calls over a KV cache check about their caches against a query of B sequences, H heads and head dim D:
    ``_cache_geometry`` and what only the readers ask."""
    Hkv = k_cache.shape[1]
    Smax, page_size, num_pages = _cache_geometry("q", q, B, Hkv, D, k_cache, v_cache, block_table, H)
    if block_table is not None and (not block_table.is_cuda or block_table.device != q.device):
        raise ValueError("block_table must live on the operands' device (there is no CPU path)")
    if fp8:
        if q.dtype not in (torch.bfloat16, torch.float16) or k_cache.dtype != FP8 or v_cache.dtype != FP8:
            raise ValueError("q must be bf16 or fp16, k_cache and v_cache torch.float8_e4m3fn")
    elif q.dtype not in (torch.bfloat16, torch.float16) or k_cache.dtype != q.dtype or v_cache.dtype != q.dtype:
        raise ValueError("q, k_cache, v_cache must share dtype bf16 or fp16")
    if not (q.is_cuda and k_cache.is_cuda and v_cache.is_cuda) or k_cache.device != q.device or v_cache.device != q.device:
        raise ValueError(f"{entry} needs device tensors on one device (there is no CPU path)")
    odt = q.dtype if out_dtype is None else out_dtype
    if odt not in (q.dtype, torch.float32):
        raise ValueError("output dtype must be the input dtype or fp32")
    return _CacheOperands(Hkv, Smax, page_size, num_pages, odt)


def _cache_call_args(entry: str, q, k_cache, v_cache, causal, softmax_scale, out_dtype, out, block_table, fp8=False):
    """Validation and marshalling ``fa3_decode`` and ``fa3_prefill_cache`` share (both take ``pfa_fa3_decode_args``): the operands,
    the output buffer and the block table.  -> ``(args, out, Smax)``; ``entry`` names the C entry point in the messages."""
    _rank4(q, k_cache, v_cache)
    B, H, Sq, D = q.shape
    geo = _cache_operands(entry, q, B, H, D, k_cache, v_cache, out_dtype, block_table, fp8)
    if out is None:
        out = torch.empty((B, Sq, H, D), dtype=geo.odt, device=q.device).permute(0, 2, 1, 3)
    else:
        _out_arg(out, (B, H, Sq, D), geo.odt, q.device)
    a = _capi.make_decode_args(
        B=B, H=H, Hkv=geo.Hkv, Sq=Sq, Smax=geo.Smax, D=D, dtype_in=_DT[q.dtype], dtype_out=_DT[geo.odt], causal=1 if causal else 0,
        softmax_scale=_scale(softmax_scale, D),
        device_id=_device_index(q.device))
    _set_view(a, "q", q)
    _set_view(a, "k_cache", k_cache)
    _set_view(a, "v_cache", v_cache)
    _set_view(a, "o", out)
    _set_block_table(a, block_table, geo.page_size, geo.num_pages)
    return a, out, geo.Smax


def _set_cache_seqlens(a, cache_seqlens, q, keep, B=None) -> None:
    """``cache_seqlens`` (int32 ``[B]`` device tensor, or None) into the argument block; a converted copy is appended to ``keep``."""
    B = q.shape[0] if B is None else B
    if cache_seqlens is not None:
        if not isinstance(cache_seqlens, torch.Tensor) or not cache_seqlens.is_cuda or cache_seqlens.device != q.device:
            raise ValueError("cache_seqlens must be a [B] tensor on the operands' device")
        if cache_seqlens.shape != (B,):
            raise ValueError("cache_seqlens must have B entries")
        sl = cache_seqlens if cache_seqlens.dtype == torch.int32 and cache_seqlens.is_contiguous() else \
            cache_seqlens.to(torch.int32).contiguous()
        a.cache_seqlens = sl.data_ptr()
        keep.append(sl)


def _window_ext(window, causal):
    """``window`` (None, or an integer >= 1: each row sees its last ``window`` keys) as the ``*_ex`` calls' extension block, or None.
    Refused before anything is launched: any other value, and a window without ``causal``."""
    if window is None:
        return None
    w = _host_int(window)
    if w is None or w < 1:
        raise ValueError(f"window must be None or an integer >= 1, got {window!r}")
    if not causal:
        raise ValueError("a sliding window needs causal=True (it is cut from the causal diagonal)")
    return _capi.make_cache_ext(window=min(w, 0x7fffffff))


def _tree_mask_arg(tree_mask, q, causal, window, shared_prefix):
    """``tree_mask`` (None, or an int64 ``[B, Sq]`` tensor on q's device, last dim contiguous) as ``pfa_fa3_decode_tree``'s block
    (the caller's tensor is pointed into, not copied).  Refused before anything is launched: a wrong dtype, shape or device, ``causal=False``, a
    ``window`` and ``shared_prefix``."""
    if tree_mask is None:
        return None
    if not isinstance(tree_mask, torch.Tensor) or tree_mask.dtype != torch.int64:
        raise ValueError("tree_mask must be an int64 tensor (one 64-bit word per query row; the kernel reads it as unsigned)")
    _rank4(q)
    B, Sq = q.shape[0], q.shape[2]
    if tree_mask.shape != (B, Sq):
        raise ValueError(f"tree_mask must be [B, Sq] = [{B}, {Sq}], got {tuple(tree_mask.shape)}")
    if tree_mask.device != q.device:
        raise ValueError("tree_mask must live on the operands' device")
    if not causal:
        raise ValueError("tree_mask needs causal=True: the words replace the causal triangle over the step's own keys")
    if window is not None:
        raise ValueError("tree_mask does not combine with window: a node's window would be by depth, not by row index")
    if shared_prefix is not None:
        raise ValueError("tree_mask does not combine with shared_prefix yet")
    if (Sq > 1 and tree_mask.stride(1) != 1) or (B > 1 and tree_mask.stride(0) < Sq):
        raise ValueError("tree_mask: the last dim must be contiguous and the sequences' rows must not overlap")
    return _capi.make_tree_mask(words=tree_mask.data_ptr(), stride_b=max(tree_mask.stride(0), Sq))


def _sinks_arg(sinks, q, tree_mask=None):
    """``sinks`` (None, or a contiguous fp32 ``[H]`` tensor on q's device) as the ``pfa_fa3_sinks`` block of the ``*_sink`` calls, or None.
    Refused with ``tree_mask``; every refusal is a ``ValueError`` that names the argument, before anything is enqueued."""
    if sinks is None:
        return None
    if tree_mask is not None:
        raise ValueError("sinks is not supported with tree_mask: the tree kernels carry no sink")
    if not isinstance(sinks, torch.Tensor) or sinks.dtype != torch.float32:
        raise ValueError("sinks must be an fp32 tensor (one value per query head, in the units of the scaled scores)")
    H = q.shape[1] if isinstance(q, torch.Tensor) and q.dim() >= 2 else 0
    if sinks.shape != (H,):
        raise ValueError(f"sinks must be [H] = [{H}], got {tuple(sinks.shape)}")
    if not sinks.is_contiguous():
        raise ValueError("sinks must be contiguous")
    if sinks.device != q.device:
        raise ValueError("sinks must live on the operands' device")
    return _capi.make_sinks(sinks=sinks.data_ptr())


def tree_mask_from_parents(parents: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The ``tree_mask`` words of a drafted token tree given by parent links, and the nodes' depths.

    parents: integer ``[B, Sq]`` tensor on any device, Sq <= 64, nodes in an order that puts every parent in front of its children:
    ``parents[b, i]`` is in ``-1 .. i - 1``, -1 for a node that hangs off the cached prefix.  Returns ``(words, depths)`` on the same
    device: ``words[b, i]`` (int64) has bit i set plus the bits of the parent's word, i.e. the node and its ancestors -- what
    ``fa3_decode(tree_mask=)`` takes; bit 63 is the int64's sign bit, so the last node of a 64-node chain has the word -1.
    ``depths[b, i]`` (int32) is 0 for a child of the prefix, popcount - 1 in general.  A node's rotary position is

        ``len_b - Sq + depths[b, i]``

    with len_b the length after the step's Sq rows were appended.  Sq vectorised torch steps, no host synchronisation on device
    tensors: out-of-range parents are the caller's problem there (they are clamped into ``-1 .. i - 1``'s index range, never an
    out-of-range access); on CPU tensors they raise ``ValueError``, as do Sq > 64, a wrong rank and a non-integer dtype."""
    if not isinstance(parents, torch.Tensor) or parents.dim() != 2 or parents.dtype.is_floating_point or parents.dtype.is_complex \
            or parents.dtype == torch.bool:
        raise ValueError("parents must be an integer [B, Sq] tensor")
    B, Sq = parents.shape
    if Sq < 1 or Sq > 64:
        raise ValueError(f"parents: 1 .. 64 nodes per sequence (one bit of a 64-bit word each), got {Sq}")
    par = parents.to(torch.int64)
    if not par.is_cuda and B:
        idx = torch.arange(Sq, dtype=torch.int64, device=par.device)
        if bool(((par < -1) | (par >= idx)).any()):
            raise ValueError("parents[b, i] must be in -1 .. i - 1 (-1: the node hangs off the prefix)")
    # bit i as an int64: 1 << 63 wraps to the sign bit
    bits = torch.ones((), dtype=torch.int64, device=par.device) << torch.arange(Sq, dtype=torch.int64, device=par.device)
    words = torch.zeros((B, Sq), dtype=torch.int64, device=par.device)
    depths = torch.zeros((B, Sq), dtype=torch.int32, device=par.device)
    for i in range(Sq):
        p = par[:, i:i + 1]
        has = p >= 0
        at = p.clamp(0, max(i - 1, 0))
        words[:, i:i + 1] = torch.where(has, words.gather(1, at), torch.zeros_like(p)) | bits[i]
        depths[:, i:i + 1] = torch.where(has, depths.gather(1, at) + 1, torch.zeros_like(p, dtype=torch.int32))
    return words, depths


def _key_splits_arg(name: str, value):
    """``key_splits`` / ``prefix_key_splits`` (``name``) as the C value: None stays None, ``"auto"`` is 0 (the library's plan), an integer
    1 .. 8 is itself.  Any other value or type is refused before anything is launched."""
    if value is None:
        return None
    if isinstance(value, str) and value == "auto":
        return 0
    n = _host_int(value)
    if n is not None and 1 <= n <= _capi.PFA_PREFILL_MAX_SPLITS:
        return n
    raise ValueError(f'{name} must be None, "auto" or an integer 1 .. {_capi.PFA_PREFILL_MAX_SPLITS}, got {value!r}')


def _cu_seqlens_arg(cu_seqlens_q, *, layout: bool = True, contiguous: bool = True) -> int:
    """``cu_seqlens_q`` of the ragged calls over a KV cache -> B.  ``layout``: int32 and ``[B + 1]``; ``contiguous``: that too.  The append
    checks all of it at once; ``fa3_prefill_varlen`` has the caches' checks between the two halves."""
    if layout:
        if not isinstance(cu_seqlens_q, torch.Tensor) or cu_seqlens_q.dtype != torch.int32:
            raise ValueError("cu_seqlens_q must be an int32 tensor")
        if cu_seqlens_q.dim() != 1 or cu_seqlens_q.numel() < 2:
            raise ValueError(f"cu_seqlens_q must be [B + 1], got {tuple(cu_seqlens_q.shape)}")
    if contiguous and not cu_seqlens_q.is_contiguous():
        raise ValueError("cu_seqlens_q must be contiguous")
    return cu_seqlens_q.numel() - 1


class _AppendOperands(NamedTuple):
    """``_append_operands``' result."""
    ragged: bool
    B: int
    Hkv: int
    D: int
    total: int
    max_seqlen_q: int
    Smax: int
    page_size: int
    num_pages: int


def _append_operands(entry: str, k_new, v_new, k_cache, v_cache, cache_seqlens, cu_seqlens_q, max_seqlen_q, block_table, others=(),
                     fp8=False) -> _AppendOperands:
    """What ``kv_append`` and ``rope_append`` check about the step's rows, the caches and the device data they share (``others``: the
    further tensors that must live on k_new's device)."""
    ragged = cu_seqlens_q is not None
    if k_new.dim() != (3 if ragged else 4) or k_cache.dim() != 4 or v_cache.dim() != 4:
        raise ValueError("k_new must be 3-D ([total,Hkv,D]) with cu_seqlens_q, else 4-D ([B,Hkv,Sq,D]); k_cache, v_cache 4-D ([B,Hkv,Smax,D])")
    if v_new.shape != k_new.shape:
        raise ValueError(f"shape mismatch: k_new {tuple(k_new.shape)} v_new {tuple(v_new.shape)}")
    if ragged:
        B, (total, Hkv, D) = _cu_seqlens_arg(cu_seqlens_q), k_new.shape
        if max_seqlen_q is None:
            raise ValueError("cu_seqlens_q needs max_seqlen_q, the host bound on a sequence's rows (it sizes the grid)")
    else:
        B, Hkv, Sq, D = k_new.shape
        if max_seqlen_q is not None and int(max_seqlen_q) != Sq:
            raise ValueError(f"max_seqlen_q {max_seqlen_q}: without cu_seqlens_q every sequence brings k_new's {Sq} rows")
        max_seqlen_q, total = Sq, B * Sq
    max_seqlen_q = int(max_seqlen_q)
    Smax, page_size, num_pages = _cache_geometry("k_new", k_new, B, Hkv, D, k_cache, v_cache, block_table)
    if fp8:
        if k_new.dtype not in (torch.bfloat16, torch.float16) or v_new.dtype != k_new.dtype or k_cache.dtype != FP8 or v_cache.dtype != FP8:
            raise ValueError("k_new, v_new must share dtype bf16 or fp16, k_cache and v_cache be torch.float8_e4m3fn")
        if D % 16:
            raise ValueError(f"head dim {D}: the quantising append takes a multiple of 16 up to 256")
    elif k_new.dtype not in (torch.bfloat16, torch.float16) or any(t.dtype != k_new.dtype for t in (v_new, k_cache, v_cache)):
        raise ValueError("k_new, v_new, k_cache, v_cache must share dtype bf16 or fp16")
    if not isinstance(cache_seqlens, torch.Tensor) or cache_seqlens.shape != (B,):
        raise ValueError("cache_seqlens must be a [B] tensor (the lengths after the step)")
    if total < 1 or not 1 <= max_seqlen_q <= total:
        raise ValueError(f"max_seqlen_q {max_seqlen_q}: must lie in 1 .. {total}, the rows k_new holds")
    dev = k_new.device
    if any(t.device != dev for t in (v_new, k_cache, v_cache, cache_seqlens) + ((cu_seqlens_q,) if ragged else ())
           + ((block_table,) if block_table is not None else ()) + tuple(others)):
        raise ValueError(f"{entry} needs all its tensors on one device")
    return _AppendOperands(ragged, B, Hkv, D, total, max_seqlen_q, Smax, page_size, num_pages)


def _append_args(make, entry: str, k_new, v_new, k_cache, v_cache, geo: _AppendOperands, cu_seqlens_q, block_table, **more):
    """The argument block of ``pfa_kv_append`` / ``pfa_rope_append`` (``make``: its ``_capi`` constructor) with the fields the two
    share filled in from ``_append_operands``' ``geo``; ``more`` are further fields."""
    if not k_new.is_cuda:
        raise ValueError(f"{entry} needs device tensors (or CPU tensors for the torch model)")
    a = make(B=geo.B, Hkv=geo.Hkv, total_new=geo.total, max_seqlen_q=geo.max_seqlen_q, Smax=geo.Smax, D=geo.D, dtype=_DT[k_new.dtype],
             device_id=_device_index(k_new.device), **more)
    rows = "bsh"
    if geo.ragged:
        a.cu_seqlens_q, rows = cu_seqlens_q.data_ptr(), "sh"
    _set_view(a, "k_new", k_new, rows)
    _set_view(a, "v_new", v_new, rows)
    _set_view(a, "k_cache", k_cache)
    _set_view(a, "v_cache", v_cache)
    _set_block_table(a, block_table, geo.page_size, geo.num_pages)
    return a


def _append_launch(entry: str, a, cache_seqlens, k_new, B, quant=None) -> None:
    """``cache_seqlens`` into the block, then the one launch of ``entry`` (with ``quant``: of ``{entry}_q8``) on k_new's current stream."""
    keep = []
    _set_cache_seqlens(a, cache_seqlens, k_new, keep, B)
    stream = torch.cuda.current_stream(k_new.device)
    lib, s = _capi.load(), C.c_void_p(stream.cuda_stream)
    st = getattr(lib, entry)(C.byref(a), s) if quant is None else getattr(lib, entry + "_q8")(C.byref(a), C.byref(quant), s)
    _raise_status(entry, st, null_too=True)
    if keep:
        _hold(keep, stream)


def kv_append(k_new: torch.Tensor, v_new: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, *, cache_seqlens: torch.Tensor,
              cu_seqlens_q: Optional[torch.Tensor] = None, max_seqlen_q: Optional[int] = None,
              block_table: Optional[torch.Tensor] = None, k_descale: Optional[torch.Tensor] = None,
              v_descale: Optional[torch.Tensor] = None) -> None:
    """Device-side KV-cache append (``pfa_kv_append``): place a step's new K / V rows into the cache the calls over a KV cache read --
    the write side of ``fa3_decode`` / ``fa3_prefill_cache`` / ``fa3_prefill_varlen``, from device data alone.

    k_cache / v_cache (and ``block_table``) are passed exactly as to ``fa3_prefill_varlen``: ``[B,Hkv,Smax,D]``-shaped views, or with
    ``block_table`` (int32 ``[B, max_pages]``) pools ``[num_pages,Hkv,page_size,D]``-shaped, page_size a multiple of 64.  k_new / v_new:
    with ``cu_seqlens_q`` (int32 ``[B + 1]``, as in ``fa3_prefill_varlen``) the packed ``[total, Hkv, D]`` rows and ``max_seqlen_q`` the
    host bound on one sequence's rows; without it ``[B,Hkv,Sq,D]`` (any strides, head dim contiguous), ``max_seqlen_q`` being Sq.
    bf16 / fp16, D a multiple of 8 up to 256.  cache_seqlens: int32 ``[B]``, required, the lengths AFTER the step -- the tensor the
    attention call behind it takes.  With len_b = clamp(cache_seqlens[b], 0, Smax) and Sq_b the sequence's rows (clamped as
    ``fa3_prefill_varlen`` clamps them), row i goes to logical key ``len_b - Sq_b + i``.  Rows in front of key 0 (len_b < Sq_b) are
    dropped, and so is a row whose page id lies outside the pool: a write is never clamped into someone else's page.  Packed rows no
    sequence covers are never read; nothing but the destination rows is written, lengths and table included, so a replay is
    idempotent.  Two sequences given the same destination leave one of the two rows there (copy-on-write: ``page_copy`` in front of this
    call, as ``PagedKVCache(copy_on_write=True)`` does).

    On device tensors: one launch of a HIP copy kernel whose grid depends on host shapes only -- no host synchronisation, no tensor
    creation, capturable in ``torch.cuda.graph`` and valid while cu_seqlens_q, lengths, table and cache change between replays.  On CPU
    tensors the same rule runs in plain torch (the executable specification; ``PagedKVCache``'s bookkeeping is tested through it).

    FP8 cache: k_cache / v_cache of ``torch.float8_e4m3fn`` with ``k_descale=, v_descale=`` (contiguous fp32 ``[Hkv]`` or ``[B, Hkv]`` on the
    tensors' device; required then, refused otherwise) run the quantising append (``pfa_kv_append_q8``): the same placement, every
    16-bit source element x stored as ``e4m3fn(clamp(float(x) / descale[b, hk], -448, 448))`` -- an fp32 division, round to nearest
    even, NaN stays NaN; ``quantize_kv`` is the rule in plain torch, and what runs on CPU tensors.  D a multiple of 16 up to 256."""
    if not all(isinstance(t, torch.Tensor) for t in (k_new, v_new, k_cache, v_cache)):
        raise ValueError("k_new, v_new, k_cache, v_cache must be tensors")
    fp8 = k_cache.dtype == FP8 or v_cache.dtype == FP8
    geo = _append_operands("pfa_kv_append", k_new, v_new, k_cache, v_cache, cache_seqlens, cu_seqlens_q, max_seqlen_q, block_table,
                           fp8=fp8)
    quant = _kv_quant_arg("pfa_kv_append", k_cache, v_cache, k_descale, v_descale, geo.B, geo.Hkv, k_new.device)
    if k_new.device.type == "cpu":
        lens, cu = cache_seqlens.tolist(), cu_seqlens_q.tolist() if geo.ragged else None
        if fp8:
            _kv_append_q8_model(k_new, v_new, k_cache, v_cache, k_descale, v_descale, lens, cu, geo.max_seqlen_q, block_table)
        else:
            _kv_append_model(k_new, v_new, k_cache, v_cache, lens, cu, geo.max_seqlen_q, block_table)
        return
    a = _append_args(_capi.make_kv_append_args, "pfa_kv_append", k_new, v_new, k_cache, v_cache, geo, cu_seqlens_q, block_table)
    _append_launch("pfa_kv_append", a, cache_seqlens, k_new, geo.B, quant)


def page_copy(k_pool: torch.Tensor, v_pool: torch.Tensor, pairs: torch.Tensor, *, rows: Optional[torch.Tensor] = None) -> None:
    """Copy whole or partial pages inside the pools of a paged KV cache (``pfa_page_copy``): the data movement of copy-on-write, what
    vLLM's ``copy_blocks`` does.

    k_pool / v_pool are passed as everywhere else: ``[num_pages,Hkv,page_size,D]``-shaped views (head-major or token-major memory),
    bf16 / fp16, page_size a multiple of 64, D a multiple of 8 up to 256.  pairs: int32 ``[n, 2]`` of ``(src, dst)`` page ids on the
    pools' device (any row stride >= 2, the two ids adjacent); rows: int32 ``[n]`` contiguous, or None for whole pages.  A pair is
    empty -- nothing read, nothing written -- when an id lies outside ``[0, num_pages - 1]`` (-1 is the "no copy" marker) or
    ``src == dst``.  Otherwise tokens ``[0, r)`` of page src go to page dst in both pools, ``r = clamp(rows[i], 0, page_size)`` or
    page_size; tokens from r on are not written.  Bad device data loses a copy, it never reaches outside the pools.  The caller promises
    that no page is the destination of two non-empty pairs and that no destination is another pair's source: then a replay is
    idempotent.  ``n == 0`` returns without a launch.

    On device tensors: one launch of a HIP copy kernel on the current stream whose grid depends on host shapes only -- no host
    synchronisation, no tensor creation, capturable in ``torch.cuda.graph`` and valid while pairs, rows and the pools change between
    replays.  On CPU tensors the same rule runs in plain torch, pairs in order (the executable specification).  Wrong dtypes, shapes or
    devices raise ``ValueError`` before anything is enqueued."""
    if not all(isinstance(t, torch.Tensor) for t in (k_pool, v_pool, pairs)) or k_pool.dim() != 4 or v_pool.shape != k_pool.shape:
        raise ValueError("k_pool, v_pool must be 4-D tensors of one shape ([num_pages,Hkv,page_size,D])")
    num_pages, Hkv, page_size, D = k_pool.shape
    if k_pool.dtype not in (torch.bfloat16, torch.float16) or v_pool.dtype != k_pool.dtype:
        raise ValueError("k_pool, v_pool must share dtype bf16 or fp16")
    if num_pages < 1 or Hkv < 1:
        raise ValueError(f"shape mismatch: k pool {tuple(k_pool.shape)}")
    if page_size < 64 or page_size % 64:
        raise ValueError(f"page size {page_size}: must be a multiple of 64 keys")
    if D < 8 or D % 8 or D > 256:
        raise ValueError(f"head dim {D}: must be a multiple of 8 up to 256")
    if pairs.dtype != torch.int32 or pairs.dim() != 2 or pairs.shape[1] != 2:
        raise ValueError("pairs must be an int32 [n, 2] tensor of (src, dst) page ids")
    n = pairs.shape[0]
    if n > 1 and pairs.stride(0) < 2 or n > 0 and pairs.stride(1) != 1:
        raise ValueError("pairs: a row's two ids must be adjacent, rows at least 2 apart")
    if rows is not None:
        if not isinstance(rows, torch.Tensor) or rows.dtype != torch.int32 or rows.shape != (n,):
            raise ValueError("rows must be an int32 [n] tensor, one count per pair")
        if n > 1 and rows.stride(0) != 1:
            raise ValueError("rows must be contiguous")
    dev = k_pool.device
    if v_pool.device != dev or pairs.device != dev or (rows is not None and rows.device != dev):
        raise ValueError("pfa_page_copy needs all its tensors on one device")
    if n == 0:
        return
    if dev.type == "cpu":
        _page_copy_model(k_pool, v_pool, pairs.tolist(), None if rows is None else rows.tolist())
        return
    if not k_pool.is_cuda:
        raise ValueError("pfa_page_copy needs device tensors (or CPU tensors for the torch model)")
    a = _capi.make_page_copy_args(
        pairs=pairs.data_ptr(), rows=None if rows is None else rows.data_ptr(), pairs_stride=pairs.stride(0) if n > 1 else 2,
        n_pairs=n, Hkv=Hkv, D=D, page_size=page_size, num_pages=num_pages, dtype=_DT[k_pool.dtype], device_id=_device_index(dev))
    _set_view(a, "k_pool", k_pool)
    _set_view(a, "v_pool", v_pool)
    st = _capi.load().pfa_page_copy(C.byref(a), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    _raise_status("pfa_page_copy", st, null_too=True)


def rotary_tables(max_pos: int, rot_dim: int, base: float = 10000.0, device=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The standard rotary tables for ``rope_append``: ``(cos, sin)``, fp32 ``[max_pos, rot_dim // 2]``, of the angles
    ``pos * inv_freq[j]`` with ``inv_freq = base ** (-arange(0, rot_dim, 2) / rot_dim)``.  Computed in fp64 and rounded once."""
    max_pos, rot_dim = int(max_pos), int(rot_dim)
    if max_pos < 1 or rot_dim < 2 or rot_dim % 2:
        raise ValueError(f"rotary_tables: max_pos {max_pos} must be >= 1 and rot_dim {rot_dim} a positive even number")
    inv_freq = float(base) ** (-torch.arange(0, rot_dim, 2, dtype=torch.float64) / rot_dim)
    angle = torch.arange(max_pos, dtype=torch.float64)[:, None] * inv_freq[None, :]
    cos, sin = angle.cos().to(torch.float32), angle.sin().to(torch.float32)
    return (cos, sin) if device is None else (cos.to(device), sin.to(device))


def _fp32_tables(rotary_cos, rotary_sin) -> None:
    for t in (rotary_cos, rotary_sin):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise ValueError("rotary_cos / rotary_sin must be fp32 tensors (the tables are not converted per call)")


def _rotary_operands(rotary_cos, rotary_sin, D: int):
    """What ``rope_append`` checks about its fp32 tables against head dim D.  -> ``(rot_dim, max_pos)``."""
    if rotary_cos.dim() != 2 or rotary_sin.shape != rotary_cos.shape or rotary_cos.shape[0] < 1:
        raise ValueError(f"rotary_cos / rotary_sin must both be [max_pos, rot_dim / 2], got {tuple(rotary_cos.shape)} / {tuple(rotary_sin.shape)}")
    max_pos, half = rotary_cos.shape
    if D % 16 or not 16 <= D <= 256:
        raise ValueError(f"head dim {D}: rope_append takes a multiple of 16 in 16 .. 256")
    if (2 * half) % 16 or not 16 <= 2 * half <= D:
        raise ValueError(f"rot_dim {2 * half}: must be a multiple of 16 in 16 .. {D}, the head dim")
    if rotary_cos.stride(1) != 1 or rotary_sin.stride() != rotary_cos.stride():
        raise ValueError("rotary_cos / rotary_sin: the last dim must be contiguous and the two row strides equal")
    return 2 * half, max_pos


def _pos_offsets_operand(pos_offsets, B: int) -> None:
    if pos_offsets is not None and (not isinstance(pos_offsets, torch.Tensor) or pos_offsets.dtype != torch.int32
                                    or pos_offsets.shape != (B,) or not pos_offsets.is_contiguous()):
        raise ValueError("pos_offsets must be a contiguous int32 [B] tensor")


def _tables_given(rotary_cos, rotary_sin, **dependent) -> bool:
    """Are there rotary tables?  They are given together; without them every ``dependent`` keyword must be unset (None or False)."""
    if rotary_cos is None and rotary_sin is None:
        if any(v is not None and v is not False for v in dependent.values()):
            raise ValueError(f"{' / '.join(dependent)} need rotary_cos and rotary_sin")
        return False
    if rotary_cos is None or rotary_sin is None:
        raise ValueError("rotary_cos and rotary_sin go together")
    return True


def rope_append(k_new: torch.Tensor, v_new: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, *, cache_seqlens: torch.Tensor,
                rotary_cos: torch.Tensor, rotary_sin: torch.Tensor, q: Optional[torch.Tensor] = None, q_out: Optional[torch.Tensor] = None,
                rotary_interleaved: bool = False, pos_offsets: Optional[torch.Tensor] = None,
                cu_seqlens_q: Optional[torch.Tensor] = None, max_seqlen_q: Optional[int] = None,
                block_table: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """Rotary embedding fused into the KV-cache append (``pfa_rope_append``): ``kv_append`` that also rotates the step's Q and new K rows
    by each row's position -- flash-attn's ``flash_attn_with_kvcache(k=, v=, rotary_cos=, rotary_sin=, rotary_interleaved=)``.

    k_new / v_new, the caches, ``block_table``, ``cache_seqlens`` (the lengths AFTER the step), ``cu_seqlens_q`` and ``max_seqlen_q`` are
    ``kv_append``'s, with D a multiple of 16 in 16 .. 256.  New row i of sequence b belongs to logical key ``pos = len_b - Sq_b + i`` and
    is rotated at position ``clamp(pos + pos_offsets[b], 0, max_pos - 1)`` (``pos_offsets``: optional int32 ``[B]``, for a cache whose
    leading tokens were evicted or left-padded; an out-of-range position gives wrong numbers, never an address outside the tables).
    rotary_cos / rotary_sin: fp32 ``[max_pos, rot_dim / 2]`` (``rotary_tables``), rot_dim a multiple of 16 in 16 .. D; elements at and
    past rot_dim are copied.  The pair is ``(x[j], x[j + rot_dim / 2])`` -- Hugging Face's ``rotate_half``, NeoX, Llama -- or with
    ``rotary_interleaved`` ``(x[2j], x[2j + 1])`` (GPT-J), and ``y1 = x1 * cos - x2 * sin``, ``y2 = x2 * cos + x1 * sin`` with each
    product and the add / subtract rounded to fp32 separately, then once to the dtype.

    The rotated K goes where ``kv_append`` would put the row, with its drops; V is copied there.  q (optional): ``[total, H, D]`` with
    ``cu_seqlens_q``, else ``[B, H, Sq, D]``; every row a sequence covers is rotated into ``q_out``, which is returned: the given
    tensor (``q_out is q``: in place), or a fresh one in the layout the attention calls prefer, of which the packed rows no sequence
    covers are not written.  Without q, None.

    On device tensors one launch of a HIP kernel whose grid depends on host shapes only: no host synchronisation, capturable, and
    valid while cu_seqlens_q, lengths, offsets, tables and inputs change between replays.  On CPU tensors the same rule runs in plain
    torch, bit for bit (``_rope_append_model``, the executable specification)."""
    _fp32_tables(rotary_cos, rotary_sin)
    others = [rotary_cos, rotary_sin] + [t for t in (q, q_out, pos_offsets) if isinstance(t, torch.Tensor)]
    geo = _append_operands("pfa_rope_append", k_new, v_new, k_cache, v_cache, cache_seqlens, cu_seqlens_q, max_seqlen_q, block_table, others)
    ragged, B, D, total, max_seqlen_q = geo.ragged, geo.B, geo.D, geo.total, geo.max_seqlen_q
    rot_dim, max_pos = _rotary_operands(rotary_cos, rotary_sin, D)
    _pos_offsets_operand(pos_offsets, B)
    H = 0
    if q is None:
        if q_out is not None:
            raise ValueError("q_out without q")
    else:
        H = q.shape[1] if q.dim() >= 2 else 0
        want = (total, H, D) if ragged else (B, H, max_seqlen_q, D)
        if q.shape != want or H < 1:
            raise ValueError(f"shape mismatch: q {tuple(q.shape)} k_new {tuple(k_new.shape)}: q must be "
                             + ("[total, H, D]" if ragged else "[B, H, Sq, D]") + " over k_new's rows and head dim")
        if q.dtype != k_new.dtype:
            raise ValueError("q must have k_new's dtype")
        if q_out is None:
            q_out = torch.empty(want, dtype=q.dtype, device=q.device) if ragged else \
                torch.empty((B, max_seqlen_q, H, D), dtype=q.dtype, device=q.device).permute(0, 2, 1, 3)
        elif q_out.shape != q.shape or q_out.dtype != q.dtype:
            raise ValueError("q_out must have q's shape and dtype")
    if k_new.device.type == "cpu":
        _rope_append_model(k_new, v_new, k_cache, v_cache, rotary_cos, rotary_sin, cache_seqlens.tolist(),
                           cu_seqlens_q.tolist() if ragged else None, max_seqlen_q, block_table,
                           None if pos_offsets is None else pos_offsets.tolist(), bool(rotary_interleaved), q, q_out)
        return q_out
    a = _append_args(_capi.make_rope_append_args, "pfa_rope_append", k_new, v_new, k_cache, v_cache, geo, cu_seqlens_q, block_table,
                     flags=_capi.PFA_ROPE_INTERLEAVED if rotary_interleaved else 0, cos=rotary_cos.data_ptr(), sin=rotary_sin.data_ptr(),
                     cs_stride=rotary_cos.stride(0), rot_dim=rot_dim, max_pos=max_pos, H=H)
    if pos_offsets is not None:
        a.pos_offsets = pos_offsets.data_ptr()
    if q is not None:
        _set_view(a, "q", q, "sh" if ragged else "bsh")
        _set_view(a, "q_out", q_out, "sh" if ragged else "bsh")
    _append_launch("pfa_rope_append", a, cache_seqlens, k_new, B)
    return q_out


# ---------------------------------------------------------------------------------------------------------------------------------------
# Rotary embedding for the training calls (include/pfa_hip_rotary.h, pfa_rotary): flash-attn's apply_rotary_emb

class _RotaryGeo(NamedTuple):
    packed: bool
    B: int
    S: int            # rows of a sequence; packed: max_seqlen
    total: int        # packed rows (0 when dense)
    D: int
    rot_dim: int
    max_pos: int


def _rotary_geometry(q, k, rotary_cos, rotary_sin, cu_seqlens, max_seqlen, pos_offsets, position_ids, who: str = "apply_rotary") -> _RotaryGeo:
    """What ``apply_rotary`` checks about its operands, before anything is enqueued.  ``who``: the caller the messages name; ``qk_norm``
    passes no tables for the norm alone, and ``rot_dim`` and ``max_pos`` are then 0."""
    if rotary_cos is not None:
        _fp32_tables(rotary_cos, rotary_sin)
    if not isinstance(q, torch.Tensor) or q.dtype not in (torch.bfloat16, torch.float16):
        raise ValueError(f"{who} takes bf16 / fp16 operands (fp32 operands are not rotated here)")
    packed = cu_seqlens is not None
    if q.dim() != (3 if packed else 4):
        raise ValueError("q must be [total, H, D] with cu_seqlens, else [B, H, S, D]")
    D = q.shape[-1]
    if packed:
        if not isinstance(cu_seqlens, torch.Tensor) or cu_seqlens.dtype != torch.int32 or cu_seqlens.dim() != 1 or cu_seqlens.numel() < 2 \
                or not cu_seqlens.is_contiguous():
            raise ValueError("cu_seqlens must be a contiguous int32 [B + 1] tensor")
        B, total, H = cu_seqlens.numel() - 1, q.shape[0], q.shape[1]
        S = _host_int(max_seqlen)
        if S is None or total < 1 or not 1 <= S <= total:
            raise ValueError(f"max_seqlen {max_seqlen!r}: must be a host int in 1 .. {total}, the rows held")
    else:
        if max_seqlen is not None:
            raise ValueError("max_seqlen goes with cu_seqlens")
        (B, H, S, _), total = q.shape, 0
    if B < 1 or H < 1 or S < 1:
        raise ValueError(f"{who}: empty operand {tuple(q.shape)}")
    if k is not None:
        if not isinstance(k, torch.Tensor) or k.dtype != q.dtype or k.device != q.device or k.dim() != q.dim() or k.shape[1] < 1:
            raise ValueError("k must be a tensor of q's dtype, device and rank")
        same_rows = k.shape[0] == q.shape[0] and k.shape[-1] == D and (packed or k.shape[2] == S)
        if not same_rows:
            raise ValueError(f"k {tuple(k.shape)} does not share q's rows and head dim {tuple(q.shape)}: one launch rotates tensors over the "
                             "same rows; make two calls, one for q and one for k")
    rot_dim, max_pos = (0, 0) if rotary_cos is None else _rotary_operands(rotary_cos, rotary_sin, D)
    if pos_offsets is not None and position_ids is not None:
        raise ValueError("pos_offsets and position_ids exclude each other")
    _pos_offsets_operand(pos_offsets, B)
    if position_ids is not None and (not isinstance(position_ids, torch.Tensor) or position_ids.dtype != torch.int32
                                     or position_ids.shape != ((total,) if packed else (B, S))
                                     or (packed and not position_ids.is_contiguous())):
        raise ValueError("position_ids must be an int32 tensor, [B, S] for dense operands and contiguous [total] for packed ones")
    if any(t is not None and t.device != q.device for t in (rotary_cos, rotary_sin, cu_seqlens, pos_offsets, position_ids)):
        raise ValueError(f"{'pfa_rotary' if who == 'apply_rotary' else who} needs all its tensors on one device")
    return _RotaryGeo(packed, B, S, total, D, rot_dim, max_pos)


def _rotary_meets_abi(t: torch.Tensor) -> bool:
    """``pfa_rotary``'s rules for a 16-bit tensor: head dim contiguous, base 16-byte aligned, every other stride a multiple of 8."""
    return t.stride(-1) == 1 and t.data_ptr() % 16 == 0 and all(s % 8 == 0 for s in t.stride()[:-1])


def _rotary_out(x: torch.Tensor, packed: bool) -> torch.Tensor:
    """A fresh output for ``x``, in the layout the attention calls prefer: packed rows contiguous, dense a [B, S, H, D] buffer seen as
    [B, H, S, D]."""
    if packed:
        return torch.empty(x.shape, dtype=x.dtype, device=x.device)
    B, H, S, D = x.shape
    return torch.empty((B, S, H, D), dtype=x.dtype, device=x.device).permute(0, 2, 1, 3)


# The glue of the three calls over rows (pfa_rotary, pfa_qk_norm, pfa_qk_norm_bwd): their argument blocks name the shared fields alike.

def _rows_outs(who: str, xs, geo: _RotaryGeo, inplace, outs) -> list:
    """The outputs of ``who``: the caller's ``outs``, else in place ``xs`` themselves (refused unless they meet the ABI as they are: a
    copy would not be the caller's tensor), else fresh tensors."""
    if outs is not None:
        return list(outs)
    if not inplace:
        return [_rotary_out(x, geo.packed) for x in xs]
    if not all(_rotary_meets_abi(x) for x in xs):
        raise ValueError(f"{who}(inplace=True): the head dim must be contiguous, the base 16-byte aligned and every other stride "
                         "a multiple of 8 elements")
    return list(xs)


def _meeting_abi(ts, held: list, weights: bool = False) -> list:
    """``ts`` with a copy in place of every tensor that does not meet the ABI (16-bit row tensors: ``_rotary_meets_abi``; norm
    ``weights``: contiguous and 16-byte aligned).  The copies are added to ``held``: they must outlive the launch."""
    if weights:
        out = [w if w.is_contiguous() and w.data_ptr() % 16 == 0 else w.clone(memory_format=torch.contiguous_format) for w in ts]
    else:
        out = [t if _rotary_meets_abi(t) else t.contiguous() for t in ts]
    held += [o for o, t in zip(out, ts) if o is not t]
    return out


def _rows_shape(xs, geo: _RotaryGeo) -> dict:
    return dict(B=geo.B, S=geo.S, total=geo.total, H0=xs[0].shape[1], H1=xs[1].shape[1] if len(xs) > 1 else 0, D=geo.D, rot_dim=geo.rot_dim,
                max_pos=geo.max_pos, dtype=_DT[xs[0].dtype], device_id=_device_index(xs[0].device))


def _fwd_tensors(xs, outs) -> list:
    """``_qk_norm_fill``'s ``tensors`` of a forward block: x0, x1 and x0_out, x1_out (strides x0o, x1o)."""
    return [(pre, pre, x) for pre, x in zip(("x0", "x1"), xs)] + [(pre + "_out", pre + "o", o) for pre, o in zip(("x0", "x1"), outs)]


def _qk_norm_fill(a, geo: _RotaryGeo, tensors, rotary_cos, rotary_sin, cu_seqlens, pos_offsets, position_ids) -> None:
    """The fields all three argument blocks name alike; ``tensors``: (field prefix, stride prefix, tensor) of every 16-bit tensor."""
    for field, strides, t in tensors:
        setattr(a, field, t.data_ptr())
        for axis, st in zip("sh" if geo.packed else "bhs", t.stride()):
            setattr(a, f"{strides}_stride_{axis}", st)
    if rotary_cos is not None:
        a.cos, a.sin, a.cs_stride = rotary_cos.data_ptr(), rotary_sin.data_ptr(), rotary_cos.stride(0)
    if geo.packed:
        a.cu_seqlens = cu_seqlens.data_ptr()
    if pos_offsets is not None:
        a.pos_offsets = pos_offsets.data_ptr()
    if position_ids is not None:
        a.position_ids = position_ids.data_ptr()
        if not geo.packed:
            a.pid_stride_b, a.pid_stride_s = position_ids.stride()


def _rows_launch(name: str, binding, a, device, held) -> None:
    """Enqueue export ``name`` of ``binding`` on ``device``'s current stream; ``held`` is kept until the stream has passed the launch."""
    stream = torch.cuda.current_stream(device)
    _raise_status(name, getattr(binding.load(), name)(C.byref(a), C.c_void_p(stream.cuda_stream)), null_too=True)
    _hold(held, stream)


def _rotary_call(xs, geo: _RotaryGeo, rotary_cos, rotary_sin, interleaved, cu_seqlens, pos_offsets, position_ids, conjugate, inplace,
                 outs=None):
    """One ``pfa_rotary`` over the one or two tensors ``xs`` (checked by ``_rotary_geometry``) on their current stream, or on CPU tensors
    the plain-torch model.  -> the outputs: fresh tensors (or the caller's ``outs``, of the shapes and dtype of ``xs``), or ``xs``
    themselves in place."""
    outs = _rows_outs("apply_rotary", xs, geo, inplace, outs)
    if xs[0].device.type == "cpu":
        _rotary_model(xs, outs, rotary_cos, rotary_sin, bool(interleaved), bool(conjugate),
                      cu_seqlens.tolist() if geo.packed else None, geo.S, None if pos_offsets is None else pos_offsets.tolist(), position_ids)
        return outs
    held = []
    xs = _meeting_abi(xs, held)
    flags = (_capi_rotary.PFA_ROTARY_INTERLEAVED if interleaved else 0) | (_capi_rotary.PFA_ROTARY_CONJUGATE if conjugate else 0)
    a = _capi_rotary.make_rotary_args(flags=flags, **_rows_shape(xs, geo))
    _qk_norm_fill(a, geo, _fwd_tensors(xs, outs), rotary_cos, rotary_sin, cu_seqlens, pos_offsets, position_ids)
    _rows_launch("pfa_rotary", _capi_rotary, a, xs[0].device, held)
    return outs


class _RotaryFunction(torch.autograd.Function):
    """Differentiable ``apply_rotary``, out of place: saves no activation, only the tables and the position tensors.  The backward is
    one conjugate launch over the gradients that are asked for, into fresh tensors."""

    @staticmethod
    def forward(ctx, q, k, rotary_cos, rotary_sin, interleaved, cu_seqlens, pos_offsets, position_ids, conjugate, geo):
        ctx.save_for_backward(rotary_cos, rotary_sin, cu_seqlens, pos_offsets, position_ids)
        ctx.meta = (interleaved, conjugate, geo)
        outs = _rotary_call([q] if k is None else [q, k], geo, rotary_cos, rotary_sin, interleaved, cu_seqlens, pos_offsets, position_ids,
                            conjugate, False)
        return outs[0] if k is None else tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        rotary_cos, rotary_sin, cu_seqlens, pos_offsets, position_ids = ctx.saved_tensors
        interleaved, conjugate, geo = ctx.meta
        want = [i for i in range(len(grads)) if ctx.needs_input_grad[i] and grads[i] is not None]
        res = [None, None]
        if want:
            outs = _rotary_call([grads[i] for i in want], geo, rotary_cos, rotary_sin, interleaved, cu_seqlens, pos_offsets, position_ids,
                                not conjugate, False)
            for i, o in zip(want, outs):
                res[i] = o
        return res[0], res[1], None, None, None, None, None, None, None, None


def apply_rotary(q: torch.Tensor, k: Optional[torch.Tensor] = None, *, rotary_cos: torch.Tensor, rotary_sin: torch.Tensor,
                 rotary_interleaved: bool = False, cu_seqlens: Optional[torch.Tensor] = None, max_seqlen: Optional[int] = None,
                 pos_offsets: Optional[torch.Tensor] = None, position_ids: Optional[torch.Tensor] = None, conjugate: bool = False,
                 inplace: bool = False):
    """Rotary embedding of training tensors (``pfa_rotary``) -- flash-attn's ``apply_rotary_emb`` -- in ONE launch for q and, when given,
    k: ``[B, H, S, D]`` and ``[B, Hkv, S, D]`` (any strides with the head dim contiguous, so the views of a fused projection are read in
    place), or with ``cu_seqlens`` (int32 ``[B + 1]`` on the device) and ``max_seqlen`` (a host int) packed ``[total, H, D]`` and
    ``[total, Hkv, D]``.  bf16 / fp16, D a multiple of 16 in 16 .. 256.  Returns ``q_out`` or ``(q_out, k_out)``.

    The arithmetic, the tables and the pairing are ``rope_append``'s, bit for bit: rotary_cos / rotary_sin fp32 ``[max_pos, rot_dim / 2]``
    (``rotary_tables``), rot_dim a multiple of 16 in 16 .. D, the pair ``(x[j], x[j + rot_dim / 2])`` or with ``rotary_interleaved``
    ``(x[2j], x[2j + 1])``.  Row i of sequence b is rotated at ``clamp(p, 0, max_pos - 1)`` with ``p = position_ids[b, i]`` (int32
    ``[B, S]``, packed ``[total]``) when given, else ``i + pos_offsets[b]`` (int32 ``[B]``, optional): an out-of-range position gives
    wrong numbers, never an access outside the tables.  Packed rows no sequence covers, and a sequence's rows past ``max_seqlen``, are
    neither read nor written.  ``conjugate`` rotates the other way (by ``-sin``).

    Out of place (the default) the elements at and past rot_dim are copied into fresh tensors.  ``inplace=True`` rotates the given
    tensors, touching nothing at and past rot_dim, and returns them; refused on a tensor that requires grad.

    Differentiable: no activation is saved, only the tables and the position tensors, and the backward is one conjugate launch over
    both gradients into fresh tensors.  The grid depends on host shapes only: no host synchronisation, capturable, and valid while
    cu_seqlens, offsets, position_ids, tables and inputs change between replays.  On CPU tensors the same rule runs in plain torch,
    bit for bit (``_rotary_model``, the executable specification)."""
    geo = _rotary_geometry(q, k, rotary_cos, rotary_sin, cu_seqlens, max_seqlen, pos_offsets, position_ids)
    xs = [q] if k is None else [q, k]
    needs_grad = torch.is_grad_enabled() and any(x.requires_grad for x in xs)
    if inplace:
        if needs_grad:
            raise ValueError("apply_rotary(inplace=True) on a tensor that requires grad: the backward needs the call out of place")
        _rotary_call(xs, geo, rotary_cos, rotary_sin, rotary_interleaved, cu_seqlens, pos_offsets, position_ids, conjugate, True)
        return q if k is None else (q, k)
    if needs_grad:
        return _RotaryFunction.apply(q, k, rotary_cos, rotary_sin, bool(rotary_interleaved), cu_seqlens, pos_offsets, position_ids,
                                     bool(conjugate), geo)
    outs = _rotary_call(xs, geo, rotary_cos, rotary_sin, rotary_interleaved, cu_seqlens, pos_offsets, position_ids, conjugate, False)
    return outs[0] if k is None else tuple(outs)


def _train_rotary_kw(rotary_cos, rotary_sin, rotary_interleaved, pos_offsets, position_ids):
    """The rotary keywords of the training attention calls: None without tables (then the other three must be unset), else what
    ``apply_rotary`` takes."""
    kw = dict(rotary_interleaved=bool(rotary_interleaved), pos_offsets=pos_offsets, position_ids=position_ids)
    return dict(rotary_cos=rotary_cos, rotary_sin=rotary_sin, **kw) if _tables_given(rotary_cos, rotary_sin, **kw) else None


# ---------------------------------------------------------------------------------------------------------------------------------------
# QK-norm fused with the rotary embedding of the training calls (include/pfa_hip_qk_norm.h, pfa_qk_norm / pfa_qk_norm_bwd)

QKNORM_BWD_ROWS = _models.QKNORM_BWD_ROWS      # rows of one sequence a stage-1 workgroup of the backward walks


def _qk_norm_geometry(q, k, q_weight, k_weight, eps, rotary_cos, rotary_sin, cu_seqlens, max_seqlen, pos_offsets, position_ids) -> _RotaryGeo:
    """What ``qk_norm`` checks about its operands, before anything is enqueued.  Without tables ``rot_dim`` and ``max_pos`` are 0."""
    if not isinstance(q, torch.Tensor) or q.dtype not in (torch.bfloat16, torch.float16):
        raise ValueError("qk_norm takes bf16 / fp16 operands (fp32 operands are not normalised here)")
    D = q.shape[-1]
    if D not in (64, 128):
        raise ValueError(f"head dim {D}: qk_norm takes 64 or 128, the attention's head dims")
    _tables_given(rotary_cos, rotary_sin, pos_offsets=pos_offsets, position_ids=position_ids)
    geo = _rotary_geometry(q, k, rotary_cos, rotary_sin, cu_seqlens, max_seqlen, pos_offsets, position_ids, who="qk_norm")
    if (k is None) != (k_weight is None):
        raise ValueError("k and k_weight go together")
    ws = [w for w in (q_weight, k_weight) if w is not None]
    for w in ws:
        if not isinstance(w, torch.Tensor) or w.shape != (D,) or w.dtype not in (torch.float32, q.dtype) or w.device != q.device:
            raise ValueError(f"a norm weight must be a [{D}] tensor on q's device, fp32 or of q's dtype")
    if len(ws) == 2 and ws[0].dtype != ws[1].dtype:
        raise ValueError("q_weight and k_weight must share a dtype")
    eps = float(eps)
    if not (eps >= 0.0 and math.isfinite(eps)):
        raise ValueError(f"eps {eps!r}: must be finite and not negative")
    return geo


def _qk_norm_block(make, xs, ws, geo: _RotaryGeo, eps, unit_offset, interleaved):
    flags = (_capi_qk_norm.PFA_QKNORM_INTERLEAVED if interleaved else 0) | (_capi_qk_norm.PFA_QKNORM_UNIT_OFFSET if unit_offset else 0)
    return make(flags=flags, eps=eps, w_dtype=_DT[ws[0].dtype], **_rows_shape(xs, geo))


def _qk_norm_call(xs, ws, geo: _RotaryGeo, eps, unit_offset, rotary_cos, rotary_sin, interleaved, cu_seqlens, pos_offsets, position_ids,
                  inplace, outs=None):
    """One ``pfa_qk_norm`` over the one or two tensors ``xs`` with the weights ``ws`` (checked by ``_qk_norm_geometry``) on their current
    stream, or on CPU tensors the plain-torch model.  -> the outputs: fresh tensors (or the caller's ``outs``), or ``xs`` in place."""
    outs = _rows_outs("qk_norm", xs, geo, inplace, outs)
    if xs[0].device.type == "cpu":
        _qk_norm_model(xs, outs, ws, float(eps), bool(unit_offset), rotary_cos, rotary_sin, bool(interleaved),
                       cu_seqlens.tolist() if geo.packed else None, geo.S, None if pos_offsets is None else pos_offsets.tolist(), position_ids)
        return outs
    held = []
    xs, ws = _meeting_abi(xs, held), _meeting_abi(ws, held, weights=True)
    a = _qk_norm_block(_capi_qk_norm.make_qk_norm_args, xs, ws, geo, eps, unit_offset, interleaved)
    _qk_norm_fill(a, geo, _fwd_tensors(xs, outs), rotary_cos, rotary_sin, cu_seqlens, pos_offsets, position_ids)
    for pre, w in zip(("w0", "w1"), ws):
        setattr(a, pre, w.data_ptr())
    _rows_launch("pfa_qk_norm", _capi_qk_norm, a, xs[0].device, held)
    return outs


def _qk_norm_bwd_call(xs, dys, ws, geo: _RotaryGeo, eps, unit_offset, rotary_cos, rotary_sin, interleaved, cu_seqlens, pos_offsets,
                      position_ids, dxs=None):
    """One ``pfa_qk_norm_bwd`` (two launches) on the current stream, or on CPU tensors the plain-torch model.  -> (``dxs`` in the
    tensors' dtype -- fresh, or the caller's --, ``dws`` fp32 ``[D]``)."""
    dxs = [_rotary_out(x, geo.packed) for x in xs] if dxs is None else list(dxs)
    dws = [torch.empty(geo.D, dtype=torch.float32, device=xs[0].device) for _ in xs]
    if xs[0].device.type == "cpu":
        _qk_norm_bwd_model(xs, dys, dxs, ws, dws, float(eps), bool(unit_offset), rotary_cos, rotary_sin, bool(interleaved),
                           cu_seqlens.tolist() if geo.packed else None, geo.S, None if pos_offsets is None else pos_offsets.tolist(), position_ids)
        return dxs, dws
    held = []
    xs, dys, ws = _meeting_abi(xs, held), _meeting_abi(dys, held), _meeting_abi(ws, held, weights=True)
    a = _qk_norm_block(_capi_qk_norm.make_qk_norm_bwd_args, xs, ws, geo, eps, unit_offset, interleaved)
    tensors = [(f"{n}{i}", f"{n}{i}", t) for n, ts in (("x", xs), ("dy", dys), ("dx", dxs)) for i, t in enumerate(ts)]
    _qk_norm_fill(a, geo, tensors, rotary_cos, rotary_sin, cu_seqlens, pos_offsets, position_ids)
    for i, (w, dw) in enumerate(zip(ws, dws)):
        setattr(a, f"w{i}", w.data_ptr())
        setattr(a, f"dw{i}", dw.data_ptr())
    nbytes = _capi_qk_norm.bwd_workspace_bytes(a)
    if nbytes == 0:
        raise ValueError("pfa_qk_norm_bwd: the shape is refused")
    workspace = torch.empty(nbytes // 4, dtype=torch.float32, device=xs[0].device)
    a.workspace, a.workspace_bytes = workspace.data_ptr(), nbytes
    _rows_launch("pfa_qk_norm_bwd", _capi_qk_norm, a, xs[0].device, held + [workspace])
    return dxs, dws


class _QkNormFunction(torch.autograd.Function):
    """Differentiable ``qk_norm``, out of place: saves q, k, the weights, the tables and the position tensors -- nothing computed.  The
    backward is ``pfa_qk_norm_bwd``'s two launches; the weight gradients are cast to the weights' dtype."""

    @staticmethod
    def forward(ctx, q, k, q_weight, k_weight, rotary_cos, rotary_sin, cu_seqlens, pos_offsets, position_ids, meta):
        ctx.save_for_backward(q, k, q_weight, k_weight, rotary_cos, rotary_sin, cu_seqlens, pos_offsets, position_ids)
        ctx.meta = meta
        eps, unit_offset, interleaved, geo = meta
        xs, ws = ([q], [q_weight]) if k is None else ([q, k], [q_weight, k_weight])
        outs = _qk_norm_call(xs, ws, geo, eps, unit_offset, rotary_cos, rotary_sin, interleaved, cu_seqlens, pos_offsets, position_ids, False)
        return outs[0] if k is None else tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        q, k, q_weight, k_weight, rotary_cos, rotary_sin, cu_seqlens, pos_offsets, position_ids = ctx.saved_tensors
        eps, unit_offset, interleaved, geo = ctx.meta
        xs, ws = ([q], [q_weight]) if k is None else ([q, k], [q_weight, k_weight])
        dys = [torch.zeros_like(x) if g is None else g.to(x.dtype) for x, g in zip(xs, grads)]      # an output nobody used
        dxs, dws = _qk_norm_bwd_call(xs, dys, ws, geo, eps, unit_offset, rotary_cos, rotary_sin, interleaved, cu_seqlens, pos_offsets,
                                     position_ids)
        dws = [dw.to(w.dtype) for dw, w in zip(dws, ws)]
        if k is None:
            dxs, dws = dxs + [None], dws + [None]
        need = ctx.needs_input_grad
        return (dxs[0] if need[0] else None, dxs[1] if need[1] else None, dws[0] if need[2] else None, dws[1] if need[3] else None,
                None, None, None, None, None, None)


def qk_norm(q: torch.Tensor, k: Optional[torch.Tensor] = None, *, q_weight: torch.Tensor, k_weight: Optional[torch.Tensor] = None,
            eps: float = 1e-6, unit_offset: bool = False, rotary_cos: Optional[torch.Tensor] = None,
            rotary_sin: Optional[torch.Tensor] = None, rotary_interleaved: bool = False, cu_seqlens: Optional[torch.Tensor] = None,
            max_seqlen: Optional[int] = None, pos_offsets: Optional[torch.Tensor] = None, position_ids: Optional[torch.Tensor] = None,
            inplace: bool = False):
    """QK-norm -- an RMSNorm over the head dim of every head of q and, when given, k (Qwen3's ``q_norm`` / ``k_norm``) -- and, with
    ``rotary_cos`` / ``rotary_sin``, the rotary embedding behind it, in ONE launch (``pfa_qk_norm``).  Operands, layouts, tables,
    positions, ``cu_seqlens`` / ``max_seqlen`` and ``inplace`` are ``apply_rotary``'s; the head dim is 64 or 128.  ``q_weight`` /
    ``k_weight``: ``[D]``, fp32 or of the operands' dtype, shared by the heads of a tensor.  Returns ``q_out`` or ``(q_out, k_out)``.

    Per head, all in fp32 with every product and sum rounded on its own: ``r = 1 / sqrt(sum(x^2) / D + eps)`` (the sum in the fixed
    tree of ``_models._qkn_head_sum``), ``n = (x * r) * w`` -- with ``unit_offset`` (Gemma) ``(x * r) * (1 + w)`` --, the elements
    under rot_dim rotated as ``apply_rotary`` rotates them but on the fp32 ``n``, one rounding to the dtype.  Without tables: the norm
    alone.

    Differentiable: q, k and the weights are saved (nothing computed), the backward is ``pfa_qk_norm_bwd`` -- ``r`` recomputed, dq and
    dk in one launch together with the partial weight gradients, a second small launch adds those in a fixed order: no atomics,
    bitwise reproducible -- and the weight gradients come back in the weights' dtype.  ``inplace=True`` is refused on a tensor that
    requires grad.  The grids depend on host shapes only: no host synchronisation, capturable.  On CPU tensors the same rule runs in
    plain torch, bit for bit (``_models._qk_norm_model`` / ``_qk_norm_bwd_model``, the executable specification)."""
    geo = _qk_norm_geometry(q, k, q_weight, k_weight, eps, rotary_cos, rotary_sin, cu_seqlens, max_seqlen, pos_offsets, position_ids)
    xs, ws = ([q], [q_weight]) if k is None else ([q, k], [q_weight, k_weight])
    needs_grad = torch.is_grad_enabled() and any(t.requires_grad for t in xs + ws)
    if inplace:
        if needs_grad:
            raise ValueError("qk_norm(inplace=True) on a tensor that requires grad: the backward needs the input")
        _qk_norm_call(xs, ws, geo, eps, unit_offset, rotary_cos, rotary_sin, rotary_interleaved, cu_seqlens, pos_offsets, position_ids, True)
        return q if k is None else (q, k)
    if needs_grad:
        return _QkNormFunction.apply(q, k, q_weight, k_weight, rotary_cos, rotary_sin, cu_seqlens, pos_offsets, position_ids,
                                     (float(eps), bool(unit_offset), bool(rotary_interleaved), geo))
    outs = _qk_norm_call(xs, ws, geo, eps, unit_offset, rotary_cos, rotary_sin, rotary_interleaved, cu_seqlens, pos_offsets, position_ids, False)
    return outs[0] if k is None else tuple(outs)


def _train_qk_norm_kw(q_norm_weight, k_norm_weight, qk_norm_eps, qk_norm_unit_offset):
    """The QK-norm keywords of the training attention calls: None without weights, else what ``qk_norm`` takes."""
    if q_norm_weight is None and k_norm_weight is None:
        if qk_norm_unit_offset:
            raise ValueError("qk_norm_unit_offset needs q_norm_weight and k_norm_weight")
        return None
    if q_norm_weight is None or k_norm_weight is None:
        raise ValueError("q_norm_weight and k_norm_weight go together")
    return dict(eps=qk_norm_eps, unit_offset=bool(qk_norm_unit_offset))


def _rotary_kw(rotary_cos, rotary_sin, rotary_interleaved, pos_offsets, k_new, v_new, cache_seqlens):
    """The rotary keywords of the attention calls over a KV cache: None without them, else what ``rope_append`` takes.  Refused before
    anything else is looked at: one table without the other, ``rotary_interleaved`` / ``pos_offsets`` without tables, tables that are
    not fp32, and rotary without ``k_new`` / ``v_new`` and ``cache_seqlens`` (the positions are those of the appended rows)."""
    if not _tables_given(rotary_cos, rotary_sin, rotary_interleaved=bool(rotary_interleaved), pos_offsets=pos_offsets):
        return None
    _fp32_tables(rotary_cos, rotary_sin)
    if k_new is None or v_new is None or cache_seqlens is None:
        raise ValueError("rotary_cos / rotary_sin need k_new, v_new and cache_seqlens: rows are rotated at the positions they are appended at")
    return dict(rotary_cos=rotary_cos, rotary_sin=rotary_sin, rotary_interleaved=bool(rotary_interleaved), pos_offsets=pos_offsets)


def _append_first(k_new, v_new, k_cache, v_cache, cache_seqlens, block_table, q=None, rotary=None, descales=None, **ragged):
    """The ``k_new=, v_new=`` form of the calls over a KV cache: ``kv_append`` enqueued in front of the attention launch, on the
    same stream, with the same lengths, ``cu_seqlens_q`` and table.  With ``rotary`` (``_rotary_kw``) it is ``rope_append`` instead, and
    q rotated into a fresh buffer is returned; otherwise None."""
    if k_new is None and v_new is None:
        return None
    if k_new is None or v_new is None:
        raise ValueError("k_new and v_new go together")
    if cache_seqlens is None:
        raise ValueError("k_new / v_new need cache_seqlens: the lengths after the step say where the rows go")
    if rotary is not None:
        return rope_append(k_new, v_new, k_cache, v_cache, cache_seqlens=cache_seqlens, block_table=block_table, q=q, **rotary, **ragged)
    kd, vd = descales if descales is not None else (None, None)       # an FP8 cache: the quantising append
    kv_append(k_new, v_new, k_cache, v_cache, cache_seqlens=cache_seqlens, block_table=block_table, k_descale=kd, v_descale=vd, **ragged)
    return None


def _finish_cache_call(entry: str, a, ext, q, lse_shape, keep, new_rows, rotary=None, key_splits=None, tree=None, quant=None, descales=None,
                       sinks=None, **ragged):
    """The tail the attention calls over a KV cache share, behind all their validation: the optional LSE (``lse_shape`` or None),
    ``_append_first`` of ``new_rows`` = (k_new, v_new, k_cache, v_cache, cache_seqlens, block_table), the launch of ``{entry}_ex`` on
    the current stream right behind it, the status, and the kept tensors' hold on the stream.  With ``rotary`` the launch reads the
    rotated copy of q that ``rope_append`` wrote; the caller's q is not modified.  ``key_splits`` (the C value, ``pfa_fa3_prefill`` only)
    launches ``pfa_fa3_prefill_split`` instead, which takes no extension; ``tree`` (``pfa_fa3_decode`` only) launches
    ``pfa_fa3_decode_tree``, which takes it behind the extension; ``quant`` (``pfa_fa3_decode`` over an FP8 cache, with the caller's
    ``descales`` for the append) launches ``pfa_fa3_decode_q8``; with the prefill entries it launches ``{entry}_q8``; ``sinks`` (a
    ``pfa_fa3_sinks`` block; with neither a tree nor an FP8 cache) launches ``{entry}_sink``, or ``{entry}_split_sink`` with ``key_splits``.
    -> lse or None."""
    lse = None
    if lse_shape is not None:
        lse = torch.empty(lse_shape, dtype=torch.float32, device=q.device)
        a.lse = lse.data_ptr()
    q_rot = _append_first(*new_rows, q=q, rotary=rotary, descales=descales, **ragged)
    if q_rot is not None:
        _set_view(a, "q", q_rot, "sh" if q_rot.dim() == 3 else "bhs")
        keep.append(q_rot)
    stream = torch.cuda.current_stream(q.device)
    e = None if ext is None else C.byref(ext)
    # the export that serves the call, and what it takes between the argument block and the stream
    suffix, middle = (("_split", (key_splits,)) if key_splits is not None else ("_q8", (e, C.byref(quant))) if quant is not None
                      else ("_tree", (e, C.byref(tree))) if tree is not None else ("_ex", (e,)))
    if sinks is not None:
        suffix, middle = ("_split_sink", (key_splits, C.byref(sinks))) if key_splits is not None else ("_sink", (e, C.byref(sinks)))
    st = getattr(_capi.load(), entry + suffix)(C.byref(a), *middle, C.c_void_p(stream.cuda_stream))
    _raise_status(entry, st, null_too=True)
    if keep:
        _hold(keep, stream)
    return lse


def attn_merge(outs, lses, *, out: Optional[torch.Tensor] = None, out_dtype: Optional[torch.dtype] = None,
               return_lse: bool = False) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """Merge of partial attention results (``pfa_attn_merge``): N results over DISJOINT key sets -- each an O and the natural-log LSE
    the calls over a KV cache return -- into the result over the union of the keys (FlashInfer's ``merge_state``, vLLM's
    ``merge_attn_states``).  For every row, in fp32 and in part order::

        m = max_n lse_n  (over the parts with lse_n > -inf)     w_n = exp(lse_n - m)     s = sum_n w_n
        O = (sum_n w_n * O_n) / s                               LSE = m + log(s)

    outs: 2 .. 8 ``[B,H,Sq,D]``-shaped views of one dtype (bf16, fp16 or fp32; any strides, head dim contiguous, D a multiple of 8 up
    to 256) -- the layout the cache calls return.  lses: as many ``[B,H,Sq]``-shaped fp32 views, ANY strides: the LSE of one call over
    all ``B * Sq`` rows as one sequence goes in as ``lse.view(H, B, Sq).transpose(0, 1)`` without a copy.  The result has ``out_dtype``
    (default: the parts' dtype; 16-bit parts give their own dtype or fp32, fp32 parts any of the three; 16-bit output is rounded to
    nearest even) or is written into ``out`` (``[B,H,Sq,D]``-shaped, not overlapping a part).  Returns ``(o, lse [B,H,Sq] or None)``.

    A part whose LSE is -inf (a row that saw no key there) is skipped, not multiplied by zero: its O may hold anything, NaN included.
    If every part is -inf the row is O = 0, LSE = -inf, the calls' own "row with no visible key".  A NaN LSE gives a NaN row.  Rows
    are independent.  Merging one finite part with parts that are all -inf returns that part's LSE bit for bit and its O bit for bit
    (fp32 output) or rounded once (16-bit output).  Fixed order, no atomics: two runs give the same bits.

    On device tensors one launch of a memory-bound HIP kernel on the current stream, its grid from host shapes only: no host
    synchronisation, no workspace, no cached allocation, capturable in ``torch.cuda.graph``.  On CPU tensors the same rule runs in plain
    fp32 torch ops (``_attn_merge_model``, the executable specification)."""
    outs, lses = list(outs), list(lses)
    N = len(outs)
    if not 2 <= N <= _capi.PFA_MERGE_MAX_PARTS or len(lses) != N:
        raise ValueError(f"attn_merge takes 2 .. {_capi.PFA_MERGE_MAX_PARTS} parts and as many LSEs, got {N} and {len(lses)}")
    o0 = outs[0]
    if any(not isinstance(t, torch.Tensor) for t in outs + lses) or o0.dim() != 4:
        raise ValueError("outs must be [B,H,Sq,D]-shaped tensors and lses [B,H,Sq]-shaped tensors")
    B, H, Sq, D = o0.shape
    if o0.dtype not in _DT or any(t.shape != o0.shape or t.dtype != o0.dtype for t in outs):
        raise ValueError("outs must share one shape and one dtype, bf16, fp16 or fp32")
    if any(t.shape != (B, H, Sq) or t.dtype != torch.float32 for t in lses):
        raise ValueError(f"lses must be fp32 [B,H,Sq] = {(B, H, Sq)}-shaped views")
    if D % 8 or not 8 <= D <= 256:
        raise ValueError(f"head dim {D}: attn_merge takes a multiple of 8 in 8 .. 256")
    if min(B, H, Sq) < 1:
        raise ValueError(f"attn_merge: empty shape {tuple(o0.shape)}")
    if out is not None and not isinstance(out, torch.Tensor):
        raise ValueError("out must be a tensor")
    odt = out_dtype if out_dtype is not None else (out.dtype if out is not None else o0.dtype)
    if odt not in _DT or (o0.dtype != torch.float32 and odt not in (o0.dtype, torch.float32)):
        raise ValueError("output dtype must be bf16, fp16 or fp32, and with 16-bit parts the parts' dtype or fp32")
    dev = o0.device
    if any(t.device != dev for t in outs + lses) or (out is not None and out.device != dev):
        raise ValueError("attn_merge needs all its tensors on one device")
    if out is None:
        out = torch.empty((B, Sq, H, D), dtype=odt, device=dev).permute(0, 2, 1, 3)
    elif out.shape != o0.shape or out.dtype != odt:
        raise ValueError("out must be a [B, H, Sq, D] tensor of the output dtype")
    lse_out = torch.empty((B, H, Sq), dtype=torch.float32, device=dev) if return_lse else None
    if dev.type == "cpu":
        _attn_merge_model(outs, lses, out, lse_out)
        return out, lse_out
    if dev.type != "cuda":
        raise ValueError("attn_merge needs device tensors (or CPU tensors for the torch model)")
    ostr = [_bhsd_strides(t) for t in outs]       # the per-part fields are arrays: they stay with make_attn_merge_args
    a = _capi.make_attn_merge_args(
        n_parts=N, B=B, H=H, Sq=Sq, D=D, dtype_part=_DT[o0.dtype], dtype_out=_DT[odt], device_id=_device_index(dev),
        o_part=[t.data_ptr() for t in outs], lse_part=[t.data_ptr() for t in lses],
        op_stride_b=[x[0] for x in ostr], op_stride_h=[x[1] for x in ostr], op_stride_s=[x[2] for x in ostr],
        lp_stride_b=[t.stride(0) for t in lses], lp_stride_h=[t.stride(1) for t in lses], lp_stride_s=[t.stride(2) for t in lses])
    _set_view(a, "o", out)
    if lse_out is not None:
        a.lse_out = lse_out.data_ptr()
        a.lo_stride_b, a.lo_stride_h, a.lo_stride_s = lse_out.stride()
    st = _capi.load().pfa_attn_merge(C.byref(a), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    _raise_status("pfa_attn_merge", st, null_too=True)
    return out, lse_out


def _shared_prefix_step(call, entry: str, shared_prefix, q, k_cache, v_cache, *, cache_seqlens, key_mask, window, causal, softmax_scale,
                        out_dtype, return_lse, out, block_table, k_new, v_new, rotary, prefix_key_splits=None, sinks=None):
    """``shared_prefix=P`` of ``fa3_decode`` / ``fa3_prefill_cache`` (``call``; ``entry`` names its C entry point in the messages): the
    attention cut at logical key P.  All ``B * Sq`` rows go as ONE sequence against sequence 0's first P keys (``causal=False``; every
    row lies behind the prefix), each sequence goes against its own keys from P on (``call`` unchanged on the cache view that starts
    at P, lengths ``max(len_b - P, 0)``), and ``attn_merge`` joins the two fp32 parts through their LSEs into the caller's ``out`` /
    ``out_dtype``.  The optional append runs once, first, on the whole cache, and both passes read the rotated q.  Everything is
    enqueued on the current stream with no host synchronisation; every ``ValueError`` is raised before the first launch.
    ``prefix_key_splits`` (as the caller gave it, already validated) is the prefix pass's ``key_splits`` when that pass is
    ``fa3_prefill_cache``; the decode kernel splits by itself.  ``sinks`` (already validated) go to the own-keys pass ONLY: its LSE then
    contains the sink, and the merge with the sink-less prefix part is the sink-carrying result over all keys."""
    P = _host_int(shared_prefix)
    if P is None:
        raise ValueError(f"shared_prefix must be None or a host integer, got {shared_prefix!r}")
    if key_mask is not None or window is not None:
        raise ValueError("shared_prefix does not combine with key_mask or window: their indices are over the unshifted keys")
    if cache_seqlens is None:
        raise ValueError("shared_prefix needs cache_seqlens: each sequence's own keys are those from the prefix up to its length")
    _rank4(q, k_cache, v_cache)
    B, H, Sq, D = q.shape
    # the geometry first and the readers' other checks (_cache_operands, which repeats it) behind P's own: the order the refusals have
    Smax, page_size, _ = _cache_geometry("q", q, B, k_cache.shape[1], D, k_cache, v_cache, block_table, H)
    if P < 64 or P % 64:
        raise ValueError(f"shared_prefix {P}: must be a positive multiple of 64 keys")
    if block_table is not None and P % page_size:
        raise ValueError(f"shared_prefix {P}: with a block table it must be a multiple of the page size {page_size}")
    if P >= Smax:
        raise ValueError(f"shared_prefix {P}: must be below the cache capacity {Smax} (the sequences' own keys lie behind it)")
    if entry == "pfa_fa3_decode" and Sq > 64:
        raise ValueError(f"{entry}: at most 64 query rows per sequence, got {Sq} (fa3_prefill_cache takes any number)")
    # not _set_cache_seqlens' check: here a wrong shape has the device message, and the two passes repeat that check anyway
    if not isinstance(cache_seqlens, torch.Tensor) or cache_seqlens.device != q.device or cache_seqlens.shape != (B,):
        raise ValueError("cache_seqlens must be a [B] tensor on the operands' device")
    odt = _cache_operands(entry, q, B, H, D, k_cache, v_cache, out_dtype, block_table).odt
    if out is not None:
        _out_arg(out, (B, H, Sq, D), odt, q.device)

    q_rot = _append_first(k_new, v_new, k_cache, v_cache, cache_seqlens, block_table, q=q, rotary=rotary, max_seqlen_q=Sq)
    if q_rot is not None:
        q = q_rot
    rows = B * Sq
    # the prefix pass: B' = 1, Sq' = B * Sq.  A view when q's batch stride is Sq token strides (the layout the calls return), else one copy
    q_all = q.transpose(1, 2).reshape(1, rows, H, D).transpose(1, 2)
    if block_table is None:
        pre = (k_cache[:1, :, :P], v_cache[:1, :, :P], None)
        own = (k_cache[:, :, P:], v_cache[:, :, P:], None)
    else:
        pre = (k_cache, v_cache, block_table[:1, :P // page_size])
        own = (k_cache, v_cache, block_table[:, P // page_size:])              # the row stride stays
    # the decode kernel packs a K/V head's rows and splits the keys over workgroups: it fills the chip at few rows; past 64 the MFMA forward.
    # No length tensor: the prefix views hold exactly P keys, and without cache_seqlens the kernels take the capacity.
    prefix_call = fa3_decode if rows <= 64 else fa3_prefill_cache
    split_kw = {} if rows <= 64 or prefix_key_splits is None else dict(key_splits=prefix_key_splits)
    o_pre, lse_pre = prefix_call(q_all, pre[0], pre[1], block_table=pre[2], causal=False, softmax_scale=softmax_scale,
                                 out_dtype=torch.float32, return_lse=True, **split_kw)
    own_lens = (cache_seqlens.to(torch.int32) - P).clamp_(min=0)
    o_own, lse_own = call(q, own[0], own[1], block_table=own[2], cache_seqlens=own_lens, causal=causal, softmax_scale=softmax_scale,
                          out_dtype=torch.float32, return_lse=True, sinks=sinks)
    return attn_merge([o_pre.transpose(1, 2).reshape(B, Sq, H, D).transpose(1, 2), o_own],
                      [lse_pre.view(H, B, Sq).transpose(0, 1), lse_own], out=out, out_dtype=odt, return_lse=return_lse)


def fa3_decode(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, *, cache_seqlens: Optional[torch.Tensor] = None,
               key_mask: Optional[torch.Tensor] = None, causal: bool = True, softmax_scale: Optional[float] = None,
               out_dtype: Optional[torch.dtype] = None, return_lse: bool = False,
               out: Optional[torch.Tensor] = None,
               block_table: Optional[torch.Tensor] = None, window: Optional[int] = None,
               k_new: Optional[torch.Tensor] = None, v_new: Optional[torch.Tensor] = None,
               rotary_cos: Optional[torch.Tensor] = None, rotary_sin: Optional[torch.Tensor] = None, rotary_interleaved: bool = False,
               pos_offsets: Optional[torch.Tensor] = None, shared_prefix: Optional[int] = None,
               prefix_key_splits=None, tree_mask: Optional[torch.Tensor] = None, k_descale: Optional[torch.Tensor] = None,
               v_descale: Optional[torch.Tensor] = None, sinks: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """Decode attention over a KV cache (``pfa_fa3_decode_ex``): a few new query rows per batch against the cached keys.  Inference only.

    q: ``[B,H,Sq,D]`` (1 <= Sq <= 64, D 64 or 128, bf16 / fp16; any strides, head dim contiguous) as in ``fa3_forward``.
    k_cache / v_cache: ``[B,Hkv,Smax,D]``-shaped views, H a multiple of Hkv (a flash-attn ``[B,Smax,Hkv,D]`` buffer is passed as
    ``.transpose(1, 2)``; a slice of a larger preallocated cache is just a view).  cache_seqlens: optional int32 ``[B]`` DEVICE tensor of
    valid keys per batch.  key_mask: optional ``[B,Smax]`` (0 / False = masked); given alone, each batch's length is derived from it
    on the device, so a static cache's unfilled tail is never read.  ``causal`` is bottom-right aligned: row i sees key j iff
    j <= len_b - Sq + i (for Sq = 1 it changes nothing).  Returns ``(o [B,H,Sq,D] view of a [B,Sq,H,D] buffer, lse [B,H,Sq] or None)``.
    No host synchronisation and no cached allocation: capturable in ``torch.cuda.graph``.

    Paged cache: with ``block_table`` (int32 ``[B, max_pages]`` DEVICE tensor, last dim contiguous) k_cache / v_cache are pools,
    ``[num_pages,Hkv,page_size,D]``-shaped views (a flash-attn ``[num_pages,page_size,Hkv,D]`` pool is passed as ``.transpose(1, 2)``),
    page_size a multiple of 64: logical key j of batch b lives in page ``block_table[b, j // page_size]`` at token ``j % page_size``.
    Smax is then ``max_pages * page_size``; cache_seqlens, key_mask (``[B, max_pages * page_size]``) and causal are over logical keys.
    Table entries at and past ``ceil(len_b / page_size)`` are never read; page ids are clamped into the pool by the kernel.  The
    result is bit for bit that of the contiguous call on the gathered cache.

    Sliding window: ``window=W`` (an integer >= 1, with ``causal=True``; Hugging Face's ``sliding_window``, flash-attn's
    ``window_size=(W - 1, 0)``): a row sees at most W keys, its own diagonal key included -- row i sees key j iff j < len_b,
    j <= len_b - Sq + i and j > len_b - Sq + i - W.  A key_mask combines with it (AND).  Only the windowed span is streamed, and it
    alone is split over workgroups.  With lo_b = max(0, len_b - Sq - W + 1), keys below lo_b rounded down to a multiple of 64 and
    table entries below ``lo_b // page_size`` are never read, so the pages behind the window can be given away
    (``PagedKVCache.release_behind_window``); keys between that boundary and a row's own bound are read and masked.  ``None``: no window.

    ``k_new=, v_new=`` (``[B,Hkv,Sq,D]``; needs ``cache_seqlens``, the lengths after the step): ``kv_append`` of these rows is enqueued on the
    same stream in front of the attention launch, with the same lengths and table -- flash-attn's ``flash_attn_with_kvcache(k=, v=)``.
    ``None``: nothing is appended.

    ``rotary_cos=, rotary_sin=`` (fp32 ``[max_pos, rot_dim / 2]``, with ``rotary_interleaved`` and ``pos_offsets`` as in ``rope_append``; they
    need ``k_new`` / ``v_new`` and ``cache_seqlens``): ``rope_append`` is enqueued instead of ``kv_append`` -- the new K rows are rotated at
    the positions they are appended at, and the attention launch reads q rotated into a fresh buffer; the caller's q is not modified.

    ``shared_prefix=P`` (a host integer; ``None``: the call above, unchanged): the caller promises that (a) the first P logical keys of
    every sequence have the same contents -- with a block table normally the same page ids -- and (b) every row of the step lies
    behind the prefix, ``len_b - Sq >= P``.  The attention is then cut at key P: all ``B * Sq`` rows go as one sequence against sequence
    0's first P keys (``fa3_decode`` up to 64 rows, else ``fa3_prefill_cache``; the prefix is streamed once instead of B times), each
    sequence goes against its own keys from P on, and ``attn_merge`` joins the two fp32 parts through their LSEs into ``out`` /
    ``out_dtype`` (and the merged LSE).  ``k_new`` / ``v_new`` and rotary run once, first, as above.  P must be a multiple of 64, with a
    block table of the page size, and below Smax; ``cache_seqlens`` is required; ``key_mask`` and ``window`` do not combine with it (their
    indices are over the unshifted keys).  All of these raise ``ValueError`` before anything is enqueued.  A broken promise gives wrong
    numbers, never a wrong address: every clamp of the underlying calls stays in force.  No host synchronisation: the whole step
    (append, prefix pass, own-keys pass, merge) is capturable and replays while lengths, table and cache contents change.

    When it pays (one MI355X, H 32 / Hkv 8, D 128, 256 private keys, ``profiles/shared_prefix.md``): the step is two attention calls
    and a merge instead of one call, so a captured step costs about 40 us at the least against 25 us.  With the prefix in shared
    pages -- where the plain call already gets its B re-reads from L2 / the Infinity Cache -- a captured step wins from B 32 at
    P 8192 (1.5 x) and from B 8 at P 32768 (1.4 x; 2.5 x at B 32), and loses at P 2048 for every B (0.64 - 0.94) and at B 8, P 8192
    (0.77).  When every sequence holds its own copy of the prefix it wins 1.25 - 5.6 x from B 32 at P 2048 and from B 8 at P 8192.
    Eager calls add a host floor of about 100 us per step and win only where the plain call is slower than that (B 32 at P 32768):
    capture the step.  Past ``B * Sq`` = 64 rows the prefix pass is the MFMA forward over ONE sequence, 32 - 64 workgroups, and
    without a split over keys the gain shrinks to 1.1 - 1.2 x (B 128; Sq 16 at B 32).

    ``prefix_key_splits`` (``None``, ``"auto"`` or 1 .. 8; only with ``shared_prefix``, else ``ValueError``): the ``key_splits`` of that
    prefix pass when it is ``fa3_prefill_cache``, i.e. for ``B * Sq`` > 64 -- the P keys are cut over that many workgroups per q block
    and merged (``profiles/prefill_split.md``).  With 64 rows or fewer the decode kernel splits by itself and the value is only
    validated.  ``None``: exactly the calls made without the argument.

    ``tree_mask`` (int64 ``[B, Sq]`` DEVICE tensor, last dim contiguous; ``pfa_fa3_decode_tree``): the verification of a drafted token
    TREE.  The step's Sq rows are the tree's nodes, appended like any step's rows, and word ``tree_mask[b, i]`` replaces the causal
    triangle over them: with off_b = len_b - Sq, row i sees key j iff j < len_b and (j < off_b or bit (j - off_b) of the word is set).
    The kernel reads the word as unsigned: bit 63 is the sign bit of the int64.  Bits at and above Sq are ignored and nothing is
    required of the pattern (no self bit, no order); the chain (bits 0 .. i) returns the bits of the plain causal call, all-ones
    those of ``causal=False``.  A row whose word is empty and that has no prefix gets O = 0 and LSE = -inf.  Hidden keys of the step
    are read and masked, so they must be finite.  ``tree_mask_from_parents`` builds the words from parent links.  It needs
    ``causal=True`` and combines with neither ``window`` nor ``shared_prefix`` (``ValueError`` before any launch, as for a wrong dtype,
    shape or device); ``key_mask`` (AND), ``block_table``, ``k_new`` / ``v_new``, ``out``, ``out_dtype`` and ``return_lse`` work as above.  The
    number of key splits and the workspace do not depend on it: a captured step replays while the words change.  The fused rotary
    arguments rotate by ROW INDEX (row i at ``len_b - Sq + i``), which is a chain's position and not a tree's: for a tree the caller
    rotates Q and K itself at ``len_b - Sq + depth`` (``tree_mask_from_parents`` returns the depths) and passes no rotary tables.
    ``None``: exactly the calls made without the argument.

    FP8 cache (``pfa_fa3_decode_q8``): k_cache / v_cache of ``torch.float8_e4m3fn`` (contiguous or pools), with ``k_descale=, v_descale=``
    -- contiguous fp32 DEVICE tensors ``[Hkv]`` or ``[B, Hkv]``, required then and refused with 16-bit caches.  A cache element stands
    for ``e4m3(byte) * descale[b, hk]``; the bytes are converted to q's dtype in registers (exact) in front of the same MFMA, k_descale
    multiplies the softmax scale and v_descale the output once, so the call streams half the bytes and returns the attention over
    ``dequantize_kv`` of the cache.  With all descales 1 it returns the bits of the 16-bit call on ``k_cache.to(q.dtype)``.  ``key_mask``,
    ``cache_seqlens``, ``block_table``, ``causal``, ``out``, ``out_dtype``, ``return_lse`` work as above; ``k_new=, v_new=`` (16-bit rows) go
    through the quantising ``kv_append`` first.  Splits and workspace are those of the 16-bit call, and a captured step replays while
    the descales' contents change.  ``window``, ``tree_mask``, ``shared_prefix`` and the rotary arguments are not built for an FP8 cache
    and raise ``ValueError``; bytes at and past a length are never read into a result (NaN bytes there are harmless).

    Attention sinks: ``sinks`` (contiguous fp32 ``[H]`` DEVICE tensor, one value per QUERY head; ``pfa_fa3_decode_sink``) adds
    ``exp(sinks[h])`` to every row's softmax denominator -- one extra key with score ``sinks[h]`` and a zero value row.  The values are in
    the units of the scaled scores (natural log) and are NOT multiplied by ``softmax_scale``.  The sink is inside the returned LSE; a row
    with no visible key gets O = 0 and LSE = ``sinks[h]`` (not -inf); ``sinks[h] = -inf`` gives head h the O bits of the call without
    sinks; +inf or NaN is the caller's error (that head's rows are unspecified).  ``window``, ``block_table``, ``cache_seqlens``,
    ``key_mask``, ``causal``, ``out``, ``out_dtype``, ``return_lse``, ``k_new`` / ``v_new`` and rotary work as above, and with
    ``shared_prefix`` the sinks go to the own-keys pass only.  Splits and workspace are those of the call without sinks, and a captured step
    replays while the sink values change.  A wrong dtype, shape, layout or device raises ``ValueError`` naming ``sinks`` before anything is
    enqueued, and so do ``tree_mask`` and an FP8 cache, which take no sinks.  ``None``: exactly the calls made without the argument."""
    fp8 = _fp8_caches(k_cache, v_cache, k_descale, v_descale)
    quant = _fp8_quant("pfa_fa3_decode", "decode takes key_mask, cache_seqlens", q, k_cache, v_cache, k_descale, v_descale, None, (
        ("window", window is not None), ("tree_mask", tree_mask is not None), ("shared_prefix", shared_prefix is not None),
        ("rotary_cos / rotary_sin", rotary_cos is not None or rotary_sin is not None), ("sinks", sinks is not None)), q_too=True) if fp8 else None
    snk = _sinks_arg(sinks, q, tree_mask)
    ext = _window_ext(window, causal)
    rotary = _rotary_kw(rotary_cos, rotary_sin, rotary_interleaved, pos_offsets, k_new, v_new, cache_seqlens)
    _key_splits_arg("prefix_key_splits", prefix_key_splits)
    tree = _tree_mask_arg(tree_mask, q, causal, window, shared_prefix)
    _prefix_splits_need_prefix(prefix_key_splits, shared_prefix)
    if shared_prefix is not None:
        return _shared_prefix_step(fa3_decode, "pfa_fa3_decode", shared_prefix, q, k_cache, v_cache, cache_seqlens=cache_seqlens,
                                   key_mask=key_mask, window=window, causal=causal, softmax_scale=softmax_scale, out_dtype=out_dtype,
                                   return_lse=return_lse, out=out, block_table=block_table, k_new=k_new, v_new=v_new, rotary=rotary,
                                   prefix_key_splits=prefix_key_splits, sinks=sinks)
    if k_new is not None and cache_seqlens is None:
        raise ValueError("k_new / v_new need cache_seqlens: the lengths after the step say where the rows go")
    a, out, Smax = _cache_call_args("pfa_fa3_decode", q, k_cache, v_cache, causal, softmax_scale, out_dtype, out, block_table, fp8)
    B, H, Sq, _ = q.shape
    keep = []
    if key_mask is not None:
        if key_mask.shape != (B, Smax):
            raise ValueError("key_mask must be [B, Smax]")
        if not key_mask.is_cuda or key_mask.device != q.device:
            raise ValueError("key_mask must live on the operands' device")
        km = key_mask.view(torch.uint8) if key_mask.dtype in (torch.bool, torch.uint8) else (key_mask != 0).view(torch.uint8)
        if km.stride(1) != 1:
            km = km.contiguous()
        a.key_mask, a.key_mask_stride_b = km.data_ptr(), km.stride(0)
        keep.append(km)
        if cache_seqlens is None:
            cache_seqlens = _mask_bound(km)
    _set_cache_seqlens(a, cache_seqlens, q, keep)
    if snk is not None:
        keep.append(sinks)
    # neither a tree nor an FP8 cache nor sinks change the workspace
    _attach_workspace(a, _capi.load().pfa_fa3_decode_workspace_bytes_ex(C.byref(a), None if ext is None else C.byref(ext)), q.device, keep)
    lse = _finish_cache_call("pfa_fa3_decode", a, ext, q, (B, H, Sq) if return_lse else None, keep,
                             (k_new, v_new, k_cache, v_cache, cache_seqlens, block_table), rotary, tree=tree, quant=quant,
                             descales=(k_descale, v_descale) if fp8 else None, sinks=snk, max_seqlen_q=Sq)
    return out, lse


def _fp8_caches(k_cache, v_cache, k_descale, v_descale) -> bool:
    """What the attention calls over a KV cache ask first: is this an FP8 cache?  16-bit caches refuse descales."""
    if isinstance(k_cache, torch.Tensor) and isinstance(v_cache, torch.Tensor) and (k_cache.dtype == FP8 or v_cache.dtype == FP8):
        return True
    if k_descale is not None or v_descale is not None:
        raise ValueError("k_descale / v_descale go with torch.float8_e4m3fn caches only")
    return False


def _fp8_quant(entry: str, takes: str, q, k_cache, v_cache, k_descale, v_descale, B, refused, q_too=False):
    """... and then, over an FP8 cache: -> the ``pfa_fa3_kv_quant`` block.  ``refused``: (name, given) of the arguments the FP8 kernels
    are not built for; a given one raises ``ValueError`` naming it and what the family ``takes``, before anything is enqueued.  ``B``:
    the sequences, None for q's first dim.  ``q_too``: the decode asks 4-D of q here."""
    for name, given in refused:
        if given:
            raise ValueError(f"{name} is not supported with an FP8 (torch.float8_e4m3fn) KV cache: the FP8 {takes}, "
                             "block_table, causal and k_new / v_new only")
    if q_too:
        _rank4(q, k_cache, v_cache)
    elif k_cache.dim() != 4 or v_cache.dim() != 4:
        raise ValueError("k_cache, v_cache must be 4-D ([B,Hkv,Smax,D])")
    if B is None:
        B = q.shape[0] if q.dim() else 0
    return _kv_quant_arg(entry, k_cache, v_cache, k_descale, v_descale, B, k_cache.shape[1], q.device)


def _prefix_splits_need_prefix(prefix_key_splits, shared_prefix) -> None:
    if prefix_key_splits is not None and shared_prefix is None:
        raise ValueError("prefix_key_splits needs shared_prefix: it splits the keys of the prefix pass")


def fa3_prefill_cache(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, *, cache_seqlens: Optional[torch.Tensor] = None,
                      causal: bool = True, softmax_scale: Optional[float] = None, out_dtype: Optional[torch.dtype] = None,
                      return_lse: bool = False, out: Optional[torch.Tensor] = None,
                      block_table: Optional[torch.Tensor] = None, window: Optional[int] = None,
                      k_new: Optional[torch.Tensor] = None, v_new: Optional[torch.Tensor] = None,
                      rotary_cos: Optional[torch.Tensor] = None, rotary_sin: Optional[torch.Tensor] = None, rotary_interleaved: bool = False,
                      pos_offsets: Optional[torch.Tensor] = None, shared_prefix: Optional[int] = None,
                      key_splits=None, prefix_key_splits=None, k_descale: Optional[torch.Tensor] = None,
                      v_descale: Optional[torch.Tensor] = None, sinks: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """Forward over a KV cache (``pfa_fa3_prefill_ex``): ANY number of new query rows per batch against the cached keys -- the later
    chunks of a chunked prefill, the suffix of a prefix-cached prompt, speculative verification.  Inference only.

    The tensor conventions are those of ``fa3_decode``: q ``[B,H,Sq,D]`` (Sq >= 1, D 64 or 128, bf16 / fp16), k_cache / v_cache
    ``[B,Hkv,Smax,D]``-shaped views, or with ``block_table`` (int32 ``[B, max_pages]`` device tensor) pools
    ``[num_pages,Hkv,page_size,D]``-shaped, page_size a multiple of 64.  cache_seqlens: optional int32 ``[B]`` DEVICE tensor of valid
    keys per batch, the query rows' own keys included (append first, then call); keys at and past it are never read.  ``causal`` is
    bottom-right aligned: row i sees key j iff j <= len_b - Sq + i; with len_b < Sq the first Sq - len_b rows see nothing (O = 0, LSE =
    -inf).  There is no key mask (``fa3_decode`` takes one).  By default the call is one launch of the 8-wave MFMA kernel, 256 query
    rows per workgroup, each walking every key its rows see: it wants B * H * ceil(Sq / 256) of the order of the CU count to fill the
    chip (``key_splits`` below is for the calls that have fewer).
    Returns ``(o [B,H,Sq,D] view of a [B,Sq,H,D] buffer, lse [B,H,Sq] or None)``.  No host synchronisation, no workspace and no cached
    allocation: capturable in ``torch.cuda.graph`` and valid while lengths, table and cache change between replays.  A paged call
    returns the bits of the contiguous call on the gathered cache.

    ``key_splits`` (``None``: the call above through ``pfa_fa3_prefill_ex``, untouched; an integer 1 .. 8; or ``"auto"``, the library's
    plan from (B, H, Sq, Smax) alone) goes through ``pfa_fa3_prefill_split``: every q block's 64-key tiles are cut into N ranges
    (split s of n tiles runs ``[s * per, min(n, (s + 1) * per))``, ``per = ceil(n / N)``), one workgroup per range writes an fp32 partial
    result into a fresh workspace of ``N * B * Sq * H * (D + 1) * 4`` bytes, and ``pfa_attn_merge`` joins them in split order: two
    launches, no atomics, the same bits every run, still capturable.  A count that resolves to 1 is the call above bit for bit.  For a
    short chunk of few sequences over a long cache (chunked prefill at B = 1; ``profiles/prefill_split.md``).  It does not combine with
    ``window`` or ``shared_prefix`` (``ValueError`` before anything is enqueued, as for a bad value), and with a 16-bit ``out`` the
    merge wants strides that are multiples of 8 elements.

    Sliding window: ``window=W`` (an integer >= 1, with ``causal=True``) as in ``fa3_decode``: row i sees key j iff j < len_b,
    j <= len_b - Sq + i and j > len_b - Sq + i - W.  A workgroup starts at the first 64-key tile its rows can see.  With
    lo_b = max(0, len_b - Sq - W + 1), keys below lo_b rounded down to a multiple of 64 and table entries below ``lo_b // page_size``
    are never read; keys between that boundary and a row's own bound are read and masked.  ``None``: no window.

    ``k_new=, v_new=`` (``[B,Hkv,Sq,D]``; needs ``cache_seqlens``, the lengths after the step): ``kv_append`` of these rows is enqueued on the
    same stream in front of the attention launch, with the same lengths and table -- flash-attn's ``flash_attn_with_kvcache(k=, v=)``.
    ``None``: nothing is appended.

    ``rotary_cos=, rotary_sin=`` (fp32 ``[max_pos, rot_dim / 2]``, with ``rotary_interleaved`` and ``pos_offsets`` as in ``rope_append``; they
    need ``k_new`` / ``v_new`` and ``cache_seqlens``): ``rope_append`` is enqueued instead of ``kv_append`` -- the new K rows are rotated at
    the positions they are appended at, and the attention launch reads q rotated into a fresh buffer; the caller's q is not modified.

    ``shared_prefix=P``: as in ``fa3_decode`` -- the first P keys of every sequence are the same and every row lies behind them
    (``len_b - Sq >= P``); all ``B * Sq`` rows go once against sequence 0's first P keys, each sequence against its own keys from P on
    with ``causal`` as given, and ``attn_merge`` joins the two.  Same restrictions (a multiple of 64 and of the page size, below Smax,
    ``cache_seqlens`` required, no ``window``), raised as ``ValueError`` before anything is enqueued.  Past 64 rows the prefix pass is
    this call over one sequence of ``B * Sq`` rows, H * ceil(B * Sq / 256) workgroups; ``prefix_key_splits`` (``None``, ``"auto"`` or
    1 .. 8; only with ``shared_prefix``) is that pass's ``key_splits``, as in ``fa3_decode``.  ``key_splits`` itself is refused with
    ``shared_prefix``: the own-keys pass is short.  Measured (``profiles/shared_prefix.md``, ``profiles/prefill_split.md``): the 512-row
    speculative step through ``fa3_decode``, 1.09 x shared pages, 2.3 x own copies, without a split of the prefix pass.

    FP8 cache (``pfa_fa3_prefill_q8``): k_cache / v_cache of ``torch.float8_e4m3fn`` (contiguous or pools), with ``k_descale=, v_descale=``
    -- contiguous fp32 DEVICE tensors ``[Hkv]`` or ``[B, Hkv]``, required then and refused with 16-bit caches -- as in ``fa3_decode``.  A
    cache element stands for ``e4m3(byte) * descale[b, hk]``; the bytes are converted to q's dtype on their way into the same LDS tile
    images, k_descale multiplies the softmax scale and v_descale the output once, so the call returns the attention over
    ``dequantize_kv`` of the cache, and with all descales 1 the bits of the 16-bit call on ``k_cache.to(q.dtype)``.  ``cache_seqlens``,
    ``block_table``, ``causal``, ``out``, ``out_dtype``, ``return_lse`` work as above; ``k_new=, v_new=`` (16-bit rows) go through the
    quantising ``kv_append`` first.  Still one launch from host shapes: a captured step replays while lengths, table, cache and the
    descales' contents change.  ``window``, ``shared_prefix``, ``key_splits`` / ``prefix_key_splits`` and the rotary arguments are not
    built for an FP8 cache and raise ``ValueError`` naming the argument before anything is enqueued; bytes at and past a length are
    never read into a result (NaN bytes there are harmless).  Over a ``PagedKVCache``:
    ``k, v, kw = cache.operands(slots); fa3_prefill_cache(q, k, v, **kw)``.

    Attention sinks: ``sinks`` (contiguous fp32 ``[H]`` DEVICE tensor; ``pfa_fa3_prefill_sink``, with ``key_splits``
    ``pfa_fa3_prefill_split_sink``) as in ``fa3_decode``: ``exp(sinks[h])`` joins every row's softmax denominator, in the units of the scaled
    scores, inside the LSE; a row with no visible key gets O = 0 and LSE = ``sinks[h]``; ``-inf`` gives the O bits of the call without
    sinks.  It works with ``window``, ``block_table``, ``cache_seqlens``, ``causal=False``, both output types, ``return_lse``, ``out``,
    ``k_new`` / ``v_new``, rotary, ``key_splits`` (split 0 of every q block carries the sink into the merge; a count of 1 is the unsplit
    call with sinks bit for bit) and ``shared_prefix`` / ``prefix_key_splits`` (the own-keys pass carries it).  Grid and workspace are
    those of the call without sinks; a captured step replays while the values change.  An FP8 cache takes no sinks (``ValueError``).
    ``None``: exactly the calls made without the argument."""
    fp8 = _fp8_caches(k_cache, v_cache, k_descale, v_descale)
    quant = _fp8_quant("pfa_fa3_prefill", "prefill takes cache_seqlens", q, k_cache, v_cache, k_descale, v_descale, None, (
        ("window", window is not None), ("shared_prefix", shared_prefix is not None), ("key_splits", key_splits is not None),
        ("prefix_key_splits", prefix_key_splits is not None),
        ("rotary_cos / rotary_sin", rotary_cos is not None or rotary_sin is not None or bool(rotary_interleaved) or pos_offsets is not None),
        ("sinks", sinks is not None))
    ) if fp8 else None
    snk = _sinks_arg(sinks, q)
    ext = _window_ext(window, causal)
    rotary = _rotary_kw(rotary_cos, rotary_sin, rotary_interleaved, pos_offsets, k_new, v_new, cache_seqlens)
    splits = _key_splits_arg("key_splits", key_splits)
    _key_splits_arg("prefix_key_splits", prefix_key_splits)
    _prefix_splits_need_prefix(prefix_key_splits, shared_prefix)
    if splits is not None and window is not None:
        raise ValueError("key_splits does not combine with window: the windowed kernel has no split over keys")
    if shared_prefix is not None:
        if splits is not None:
            raise ValueError("key_splits does not combine with shared_prefix (the own-keys pass is short): use prefix_key_splits")
        return _shared_prefix_step(fa3_prefill_cache, "pfa_fa3_prefill", shared_prefix, q, k_cache, v_cache, cache_seqlens=cache_seqlens,
                                   key_mask=None, window=window, causal=causal, softmax_scale=softmax_scale, out_dtype=out_dtype,
                                   return_lse=return_lse, out=out, block_table=block_table, k_new=k_new, v_new=v_new, rotary=rotary,
                                   prefix_key_splits=prefix_key_splits, sinks=sinks)
    a, out, _ = _cache_call_args("pfa_fa3_prefill", q, k_cache, v_cache, causal, softmax_scale, out_dtype, out, block_table, fp8)
    keep = [] if snk is None else [sinks]
    _set_cache_seqlens(a, cache_seqlens, q, keep)
    if splits is not None:
        _attach_workspace(a, _capi.load().pfa_fa3_prefill_split_workspace_bytes(C.byref(a), splits), q.device, keep)
    lse = _finish_cache_call("pfa_fa3_prefill", a, ext, q, q.shape[:3] if return_lse else None, keep,
                             (k_new, v_new, k_cache, v_cache, cache_seqlens, block_table), rotary, key_splits=splits, quant=quant,
                             descales=(k_descale, v_descale) if fp8 else None, sinks=snk, max_seqlen_q=q.shape[2])
    return out, lse


def fa3_prefill_varlen(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, *, cu_seqlens_q: torch.Tensor, max_seqlen_q: int,
                       cache_seqlens: Optional[torch.Tensor] = None, causal: bool = True, softmax_scale: Optional[float] = None,
                       out_dtype: Optional[torch.dtype] = None, return_lse: bool = False, out: Optional[torch.Tensor] = None,
                       block_table: Optional[torch.Tensor] = None, window: Optional[int] = None,
                       k_new: Optional[torch.Tensor] = None, v_new: Optional[torch.Tensor] = None,
                       rotary_cos: Optional[torch.Tensor] = None, rotary_sin: Optional[torch.Tensor] = None, rotary_interleaved: bool = False,
                       pos_offsets: Optional[torch.Tensor] = None, k_descale: Optional[torch.Tensor] = None,
                       v_descale: Optional[torch.Tensor] = None, sinks: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """Ragged forward over a KV cache (``pfa_fa3_prefill_varlen_ex``): ``fa3_prefill_cache`` for sequences that bring DIFFERENT numbers
    of query rows -- one step of continuous batching (a prompt chunk, a suffix behind shared prefix pages, a speculative
    verification, one-token decode rows) in one launch.  The packed form flash-attn calls varlen.  Inference only.

    q: ``[total_q, H, D]`` (D 64 or 128, bf16 / fp16; any token / head strides, head dim contiguous), the sequences' rows one after
    the other.  cu_seqlens_q: int32 ``[B + 1]`` DEVICE tensor, non-decreasing, within ``[0, total_q]``: sequence b owns the packed rows
    ``cu[b] .. cu[b+1] - 1`` (none is fine).  max_seqlen_q: host bound on the rows of one sequence (1 .. total_q); it alone sizes the
    grid, ``B * H * ceil(max_seqlen_q / 256)`` workgroups, and of a longer sequence only the first max_seqlen_q rows are computed.
    k_cache / v_cache, ``block_table`` and ``cache_seqlens`` are passed as in ``fa3_prefill_cache`` with ``B = cu_seqlens_q.numel() - 1``:
    the lengths count each sequence's own new rows (append first, then call), and ``causal`` is bottom-right aligned per sequence
    (row i of sequence b sees key j iff j <= len_b - Sq_b + i).  A row with no visible key gets O = 0 and LSE = -inf.  Packed rows no
    sequence covers (gaps, the tail behind ``cu[B]``) are never written; device values out of range are clamped by the kernel.
    Returns ``(o [total_q, H, D], lse [H, total_q] or None)``.  The result is bit for bit that of ``fa3_prefill_cache`` called per
    sequence.  No host synchronisation, no workspace and no cached allocation: capturable in ``torch.cuda.graph`` and valid while
    cu_seqlens_q, lengths, table and cache change between replays.

    Sliding window: ``window=W`` (an integer >= 1, with ``causal=True``), per sequence as in ``fa3_prefill_cache``: row i of sequence b
    sees key j iff j < len_b, j <= len_b - Sq_b + i and j > len_b - Sq_b + i - W.  With lo_b = max(0, len_b - Sq_b - W + 1), keys below
    lo_b rounded down to a multiple of 64 and table entries below ``lo_b // page_size`` are never read; keys between that boundary and a
    row's own bound are read and masked.  The bits are still those of per-sequence ``fa3_prefill_cache(window=W)`` calls.  ``None``: no window.

    ``k_new=, v_new=`` (packed ``[total_q,Hkv,D]``; needs ``cache_seqlens``, the lengths after the step): ``kv_append`` of these rows is enqueued on the
    same stream in front of the attention launch, with the same lengths, ``cu_seqlens_q``, ``max_seqlen_q`` and table -- flash-attn's ``flash_attn_with_kvcache(k=, v=)``.
    ``None``: nothing is appended.

    ``rotary_cos=, rotary_sin=`` (fp32 ``[max_pos, rot_dim / 2]``, with ``rotary_interleaved`` and ``pos_offsets`` as in ``rope_append``; they
    need ``k_new`` / ``v_new`` and ``cache_seqlens``): ``rope_append`` is enqueued instead of ``kv_append`` -- the new K rows are rotated at
    the positions they are appended at, and the attention launch reads q rotated into a fresh buffer; the caller's q is not modified.

    FP8 cache (``pfa_fa3_prefill_varlen_q8``): ``torch.float8_e4m3fn`` caches or pools with ``k_descale=, v_descale=`` (contiguous fp32
    DEVICE tensors ``[Hkv]`` or ``[B, Hkv]``; refused with 16-bit caches), exactly as in ``fa3_prefill_cache``: the attention over
    ``dequantize_kv`` of the cache, the bits of the 16-bit call at descales 1, and of per-sequence ``fa3_prefill_cache`` calls over
    the FP8 cache at any descales.  ``k_new=, v_new=`` go through the quantising ``kv_append``; ``window`` and the rotary arguments raise
    ``ValueError`` naming the argument before anything is enqueued.

    Attention sinks: ``sinks`` (contiguous fp32 ``[H]`` DEVICE tensor; ``pfa_fa3_prefill_varlen_sink``) exactly as in ``fa3_prefill_cache``,
    with and without ``window``; the result is still bit for bit that of per-sequence ``fa3_prefill_cache(sinks=)`` calls.  An FP8
    cache takes no sinks (``ValueError``).  ``None``: exactly the calls made without the argument."""
    B_cu = cu_seqlens_q.numel() - 1 if isinstance(cu_seqlens_q, torch.Tensor) else 0
    fp8 = _fp8_caches(k_cache, v_cache, k_descale, v_descale)
    quant = _fp8_quant("pfa_fa3_prefill_varlen", "prefill takes cache_seqlens", q, k_cache, v_cache, k_descale, v_descale, B_cu, (
        ("window", window is not None),
        ("rotary_cos / rotary_sin", rotary_cos is not None or rotary_sin is not None or bool(rotary_interleaved) or pos_offsets is not None),
        ("sinks", sinks is not None))
    ) if fp8 else None
    snk = _sinks_arg(sinks, q)
    ext = _window_ext(window, causal)
    rotary = _rotary_kw(rotary_cos, rotary_sin, rotary_interleaved, pos_offsets, k_new, v_new, cache_seqlens)
    if q.dim() != 3 or k_cache.dim() != 4 or v_cache.dim() != 4:
        raise ValueError("q must be 3-D ([total_q,H,D]) and k_cache, v_cache 4-D ([B,Hkv,Smax,D])")
    B = _cu_seqlens_arg(cu_seqlens_q, contiguous=False)
    total_q, H, D = q.shape
    geo = _cache_operands("pfa_fa3_prefill_varlen", q, B, H, D, k_cache, v_cache, out_dtype, block_table, fp8)
    if not cu_seqlens_q.is_cuda or cu_seqlens_q.device != q.device:
        raise ValueError("cu_seqlens_q must live on the operands' device (there is no CPU path)")
    _cu_seqlens_arg(cu_seqlens_q, layout=False)
    if q.stride(2) != 1 and D != 1:      # (ahead of out's own message; _set_view asks again)
        raise ValueError("last (head_dim) stride must be 1")
    if out is None:
        out = torch.empty((total_q, H, D), dtype=geo.odt, device=q.device)
    elif out.shape != (total_q, H, D) or out.dtype != geo.odt or out.device != q.device or (out.stride(2) != 1 and D != 1):
        raise ValueError("out must be a [total_q, H, D] tensor of the output dtype on the operands' device, head dim contiguous")
    a = _capi.make_prefill_varlen_args(
        cu_seqlens_q=cu_seqlens_q.data_ptr(), B=B, H=H, Hkv=geo.Hkv, total_q=total_q, max_seqlen_q=int(max_seqlen_q), Smax=geo.Smax, D=D,
        dtype_in=_DT[q.dtype], dtype_out=_DT[geo.odt], causal=1 if causal else 0, softmax_scale=_scale(softmax_scale, D),
        device_id=_device_index(q.device))
    _set_view(a, "q", q, "sh")
    _set_view(a, "o", out, "sh")
    _set_view(a, "k_cache", k_cache)
    _set_view(a, "v_cache", v_cache)
    _set_block_table(a, block_table, geo.page_size, geo.num_pages)
    keep = [] if snk is None else [sinks]
    _set_cache_seqlens(a, cache_seqlens, q, keep, B)
    lse = _finish_cache_call("pfa_fa3_prefill_varlen", a, ext, q, (H, total_q) if return_lse else None, keep,
                             (k_new, v_new, k_cache, v_cache, cache_seqlens, block_table), rotary, quant=quant,
                             descales=(k_descale, v_descale) if fp8 else None, sinks=snk, cu_seqlens_q=cu_seqlens_q,
                             max_seqlen_q=int(max_seqlen_q))
    return out, lse


# ---------------------------------------------------------------------------------------------------------------------------------------
# Packed variable-length attention for training (include/pfa_hip.h, pfa_fa3_varlen_args): flash-attn's flash_attn_varlen_func

def _varlen_operands(entry: str, q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k):
    """What the packed calls check about their operands -> ``(B, H, Hkv, D, total_q, total_k, max_seqlen_q, max_seqlen_k)``."""
    if q.dim() != 3 or k.dim() != 3 or v.dim() != 3:
        raise ValueError("q must be [total_q, H, D] and k, v [total_k, Hkv, D]")
    (total_q, H, D), (total_k, Hkv, _) = q.shape, k.shape
    if Hkv < 1 or H % Hkv or k.shape != (total_k, Hkv, D) or v.shape != k.shape:
        raise ValueError(f"shape mismatch: q {tuple(q.shape)} k {tuple(k.shape)} v {tuple(v.shape)}")
    if q.dtype not in (torch.bfloat16, torch.float16) or k.dtype != q.dtype or v.dtype != q.dtype:
        raise ValueError("q, k, v must share dtype bf16 or fp16")
    for name, cu in (("cu_seqlens_q", cu_seqlens_q), ("cu_seqlens_k", cu_seqlens_k)):
        if not isinstance(cu, torch.Tensor) or cu.dtype != torch.int32:
            raise ValueError(f"{name} must be an int32 tensor")
        if cu.dim() != 1 or cu.numel() < 2 or not cu.is_contiguous():
            raise ValueError(f"{name} must be a contiguous [B + 1] tensor, got {tuple(cu.shape)}")
    if cu_seqlens_k.numel() != cu_seqlens_q.numel():
        raise ValueError("cu_seqlens_q and cu_seqlens_k must both be [B + 1]")
    if any(t.device != q.device for t in (k, v, cu_seqlens_q, cu_seqlens_k)):
        raise ValueError(f"{entry} needs all its tensors on one device")
    max_seqlen_q, max_seqlen_k = operator.index(max_seqlen_q), operator.index(max_seqlen_k)      # host ints: they size the grids
    if total_q < 1 or total_k < 1 or not 1 <= max_seqlen_q <= total_q or not 1 <= max_seqlen_k <= total_k:
        raise ValueError(f"max_seqlen_q {max_seqlen_q} / max_seqlen_k {max_seqlen_k}: must lie in 1 .. {total_q} / 1 .. {total_k}, the rows held")
    return cu_seqlens_q.numel() - 1, H, Hkv, D, total_q, total_k, max_seqlen_q, max_seqlen_k


def _varlen_fwd_launch(q, k, v, out, lse, cu_seqlens_q, cu_seqlens_k, geo, causal, softmax_scale, snk=None) -> None:
    """One ``pfa_fa3_varlen_fwd`` on q's current stream into the caller's ``out`` (``[total_q, H, D]``-shaped, any row / head strides)
    and ``lse`` (contiguous fp32 ``[H, total_q]`` or None)."""
    B, H, Hkv, D, total_q, total_k, max_q, max_k = geo
    if D not in SUPPORTED_HEAD_DIMS:
        raise ValueError(f"head_dim {D}: the packed kernels exist for {SUPPORTED_HEAD_DIMS}")
    if out.shape != (total_q, H, D) or out.dtype not in (q.dtype, torch.float32) or out.device != q.device:
        raise ValueError("out must be a [total_q, H, D] tensor of the input dtype or fp32 on the operands' device")
    a = _capi.make_varlen_args(
        cu_seqlens_q=cu_seqlens_q.data_ptr(), cu_seqlens_k=cu_seqlens_k.data_ptr(), B=B, H=H, Hkv=Hkv, total_q=total_q, total_k=total_k,
        max_seqlen_q=max_q, max_seqlen_k=max_k, D=D, dtype_in=_DT[q.dtype], dtype_out=_DT[out.dtype], causal=1 if causal else 0,
        softmax_scale=_scale(softmax_scale, D), device_id=_device_index(q.device))
    for name, t in (("q", q), ("k", k), ("v", v), ("o", out)):
        _set_view(a, name, t, "sh")
    if lse is not None:
        if lse.shape != (H, total_q) or lse.dtype != torch.float32 or not lse.is_contiguous():
            raise ValueError("lse must be contiguous fp32 [H, total_q]")
        a.lse = lse.data_ptr()
    stream = C.c_void_p(torch.cuda.current_stream(q.device).cuda_stream)
    if snk is None:
        _raise_status("pfa_fa3_varlen_fwd", _capi.load().pfa_fa3_varlen_fwd(C.byref(a), stream), null_too=True)
    else:
        _raise_status("pfa_fa3_varlen_fwd_sink", _capi_sinks.load().pfa_fa3_varlen_fwd_sink(C.byref(a), C.byref(snk), stream), null_too=True)


def fa3_varlen_forward(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, *, cu_seqlens_q: torch.Tensor, cu_seqlens_k: torch.Tensor,
                       max_seqlen_q: int, max_seqlen_k: int, causal: bool = False, softmax_scale: Optional[float] = None,
                       out_dtype: Optional[torch.dtype] = None, return_lse: bool = False,
                       out: Optional[torch.Tensor] = None,
                       sinks: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """Packed variable-length attention forward (``pfa_fa3_varlen_fwd``): ``fa3_forward`` for a batch of sequences of different
    lengths that is not padded -- the operand layout of flash-attn's ``flash_attn_varlen_func``.

    q: ``[total_q, H, D]``, k / v: ``[total_k, Hkv, D]`` (bf16 / fp16, D 64 or 128, ``H % Hkv == 0``; any row / head strides that are
    multiples of 8 elements, head dim contiguous), the sequences' rows one after the other.  cu_seqlens_q / cu_seqlens_k: int32
    ``[B + 1]`` DEVICE tensors, non-decreasing, ``cu[0] >= 0``; the caller's contract is ``cu[B] == total``.  Sequence b owns the packed
    rows ``cu[b] .. cu[b + 1] - 1`` (none is fine).  max_seqlen_q / max_seqlen_k: HOST ints, bounds on the rows / keys of one sequence
    (1 .. total); they alone size the grid, and of a longer sequence only the first max_seqlen rows / keys take part.  Device values out
    of range are clamped by the kernel as in ``fa3_prefill_varlen``: wrong numbers, never an access outside the packed tensors.

    ``causal`` is the DENSE rule, top-left aligned per sequence: row i of sequence b sees key j iff ``j <= i``.  It is not the
    bottom-right rule of the calls over a KV cache; for packed self-attention (``cu_seqlens_k is cu_seqlens_q``) the two coincide.
    A row with no key (``Sk_b == 0``) gets O = 0 and LSE = -inf.  Packed rows no sequence covers are never written.

    Returns ``(out [total_q, H, D], lse [H, total_q] fp32 or None)``.  ``out_dtype=torch.float32`` selects the parity variant (fp32
    store, split P) as in ``fa3_forward``.  The result is bit for bit that of ``fa3_forward(..., _variant=44)`` per sequence: the
    8-wave kernel in its packed mode (no masks, no ``seqlens_k``, no dropout, no fp32 operands here).  Nothing synchronises with the
    device and nothing is cached: capturable in ``torch.cuda.graph`` and valid while the cu_seqlens contents change between replays.

    ``sinks``: fp32 ``[H]`` attention sinks as in ``fa3_forward`` (``pfa_fa3_varlen_fwd_sink``): a row of a sequence without keys gets
    O = 0 and LSE = the sink, and the result is bit for bit ``fa3_forward(..., sinks=)`` per sequence.  Device tensors only.

    On CPU tensors the same rule runs in plain torch per sequence in fp32 (the executable specification)."""
    geo = _varlen_operands("pfa_fa3_varlen_fwd", q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k)
    snk = _sinks_arg(sinks, q.unsqueeze(0).transpose(1, 2))      # (as [1, H, total_q, D]: the helper reads H from dim 1)
    if snk is not None and q.device.type == "cpu":
        raise ValueError("sinks need device tensors: the plain-torch model of the packed forward carries no sink")
    _, H, _, D, total_q = geo[:5]
    odt = q.dtype if out_dtype is None else out_dtype
    if out is None:
        out = torch.empty((total_q, H, D), dtype=odt, device=q.device)
    elif out.shape != (total_q, H, D) or out.dtype != odt or out.device != q.device:
        raise ValueError("out must be a [total_q, H, D] tensor of the output dtype on the operands' device")
    lse = torch.empty((H, total_q), dtype=torch.float32, device=q.device) if return_lse else None
    if q.device.type == "cpu":
        _varlen_forward_model(q, k, v, out, lse, cu_seqlens_q.tolist(), cu_seqlens_k.tolist(), geo[6], geo[7], causal, _scale(softmax_scale, D))
    else:
        _varlen_fwd_launch(q, k, v, out, lse, cu_seqlens_q, cu_seqlens_k, geo, causal, softmax_scale, snk)
    return out, lse


def _packed_meets_abi(t: torch.Tensor) -> bool:
    """The packed calls' rules for a 16-bit operand: head dim contiguous, base 16-byte aligned, row / head strides multiples of 8."""
    return t.stride(2) == 1 and t.data_ptr() % 16 == 0 and t.stride(0) % 8 == 0 and t.stride(1) % 8 == 0 and t.stride(0) >= 0


def _varlen_bwd_launch(q, k, v, out, dout, lse, dq, dk, dv, cu_seqlens_q, cu_seqlens_k, geo, causal, softmax_scale) -> torch.Tensor:
    """One ``pfa_fa3_varlen_bwd`` (two launches) on q's current stream into the caller's ``dq`` / ``dk`` / ``dv``; returns the ``delta``
    scratch ``[H, total_q]`` the launches leave."""
    B, H, Hkv, D, total_q, total_k, max_q, max_k = geo
    if D not in SUPPORTED_HEAD_DIMS:
        raise ValueError(f"head_dim {D}: the packed kernels exist for {SUPPORTED_HEAD_DIMS}")
    if lse.shape != (H, total_q) or lse.dtype != torch.float32 or not lse.is_contiguous() or lse.device != q.device:
        raise ValueError("lse must be the forward's contiguous fp32 [H, total_q]")
    delta = torch.empty((H, total_q), dtype=torch.float32, device=q.device)
    a = _capi.make_varlen_bwd_args(
        lse=lse.data_ptr(), delta=delta.data_ptr(), cu_seqlens_q=cu_seqlens_q.data_ptr(), cu_seqlens_k=cu_seqlens_k.data_ptr(),
        B=B, H=H, Hkv=Hkv, total_q=total_q, total_k=total_k, max_seqlen_q=max_q, max_seqlen_k=max_k, D=D, dtype=_DT[q.dtype],
        dtype_grad=_DT[dq.dtype], causal=1 if causal else 0, softmax_scale=_scale(softmax_scale, D), device_id=_device_index(q.device))
    for name, t in (("q", q), ("k", k), ("v", v), ("o", out), ("dout", dout), ("dq", dq), ("dk", dk), ("dv", dv)):
        _set_view(a, name, t, "sh")
    stream = torch.cuda.current_stream(q.device)
    st = _capi.load().pfa_fa3_varlen_bwd(C.byref(a), C.c_void_p(stream.cuda_stream))
    _raise_status("pfa_fa3_varlen_bwd", st, null_too=True)
    delta.record_stream(stream)      # made here: must outlive the enqueued kernels
    return delta


def fa3_varlen_backward(q, k, v, out, dout, lse, *, cu_seqlens_q: torch.Tensor, cu_seqlens_k: torch.Tensor, max_seqlen_q: int,
                        max_seqlen_k: int, causal: bool = False, softmax_scale: Optional[float] = None,
                        grad_dtype: Optional[torch.dtype] = None, sinks: Optional[torch.Tensor] = None):
    """dQ, dK, dV of ``fa3_varlen_forward`` (``pfa_fa3_varlen_bwd``).  q / out / dout ``[total_q, H, D]``, k / v ``[total_k, Hkv, D]``,
    ``lse`` the forward's fp32 ``[H, total_q]``; ``out`` and ``dout`` in the operand dtype.  Returns ``(dq [total_q, H, D], dk, dv
    [total_k, Hkv, D])`` in ``grad_dtype`` (the input dtype by default, or fp32); grouped-query heads are summed inside the dK/dV kernel.
    Every row of dq / dk / dv a sequence covers is written exactly once (rows without a key get dq = 0, keys no row sees -- a sequence
    without rows, under causal the keys ``j >= Sq_b`` -- get exact zeros); rows no sequence covers are left as ``torch.empty`` made them.
    ``causal`` is the dense top-left rule, as in ``fa3_varlen_forward``.  The gradients are bit for bit those of ``fa3_backward`` per
    sequence; no atomics.  A ``dout`` that fails the alignment or stride rules is copied, as ``fa3_backward`` does; nothing
    synchronises with the device.  On CPU tensors: the plain-torch model, fp32 per sequence.

    ``sinks``: the forward's sinks (device tensors only); the packed backward runs unchanged, ``fa3_sink_grad`` follows on its ``delta``, and
    the result is ``(dq, dk, dv, d_sinks)``."""
    geo = _varlen_operands("pfa_fa3_varlen_bwd", q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k)
    if _sinks_arg(sinks, q.unsqueeze(0).transpose(1, 2)) is not None and q.device.type == "cpu":
        raise ValueError("sinks need device tensors: the plain-torch model of the packed backward carries no sink")
    _, H, Hkv, D, total_q, total_k = geo[:6]
    if out.shape != q.shape or dout.shape != q.shape or out.dtype != q.dtype or dout.dtype != q.dtype:
        raise ValueError("out and dout must be [total_q, H, D] tensors of the operand dtype")
    if any(t.device != q.device for t in (out, dout, lse)):
        raise ValueError("pfa_fa3_varlen_bwd needs all its tensors on one device")
    gdt = q.dtype if grad_dtype is None else grad_dtype
    if gdt not in (q.dtype, torch.float32):
        raise ValueError("grad_dtype must be the input dtype or fp32")
    dq = torch.empty((total_q, H, D), dtype=gdt, device=q.device)
    dk = torch.empty((total_k, Hkv, D), dtype=gdt, device=q.device)
    dv = torch.empty((total_k, Hkv, D), dtype=gdt, device=q.device)
    if q.device.type == "cpu":
        _varlen_backward_model(q, k, v, out, dout, lse, dq, dk, dv, cu_seqlens_q.tolist(), cu_seqlens_k.tolist(), geo[6], geo[7], causal,
                               _scale(softmax_scale, D))
        return dq, dk, dv
    if not _packed_meets_abi(dout):
        dout = dout.contiguous()
    delta = _varlen_bwd_launch(q, k, v, out, dout, lse, dq, dk, dv, cu_seqlens_q, cu_seqlens_k, geo, causal, softmax_scale)
    if sinks is not None:
        return dq, dk, dv, fa3_sink_grad(lse, delta, sinks, cu_seqlens_q=cu_seqlens_q, max_seqlen_q=geo[6])
    return dq, dk, dv


class _FA3VarlenFunction(torch.autograd.Function):
    """Differentiable ``fa3_varlen_forward``: saves q, k, v, a 16-bit O, the LSE and the two cu_seqlens tensors."""

    @staticmethod
    def forward(ctx, q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, causal, softmax_scale, out_dtype):
        out, lse = fa3_varlen_forward(q, k, v, cu_seqlens_q=cu_seqlens_q, cu_seqlens_k=cu_seqlens_k, max_seqlen_q=max_seqlen_q,
                                      max_seqlen_k=max_seqlen_k, causal=causal, softmax_scale=softmax_scale, out_dtype=out_dtype,
                                      return_lse=True)
        o16 = out if out.dtype == q.dtype else out.to(q.dtype)
        ctx.save_for_backward(q, k, v, o16, lse, cu_seqlens_q, cu_seqlens_k)
        ctx.meta = (max_seqlen_q, max_seqlen_k, causal, softmax_scale)
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, out, lse, cu_q, cu_k = ctx.saved_tensors
        max_q, max_k, causal, softmax_scale = ctx.meta
        dq, dk, dv = fa3_varlen_backward(q, k, v, out, dout.to(q.dtype), lse, cu_seqlens_q=cu_q, cu_seqlens_k=cu_k, max_seqlen_q=max_q,
                                         max_seqlen_k=max_k, causal=causal, softmax_scale=softmax_scale)
        return dq, dk, dv, None, None, None, None, None, None, None


class _FA3VarlenSinkFunction(torch.autograd.Function):
    """``_FA3VarlenFunction`` with attention sinks: a sibling that also saves the sinks (see ``_FA3SinkFunction``)."""

    @staticmethod
    def forward(ctx, q, k, v, sinks, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, causal, softmax_scale, out_dtype):
        out, lse = fa3_varlen_forward(q, k, v, cu_seqlens_q=cu_seqlens_q, cu_seqlens_k=cu_seqlens_k, max_seqlen_q=max_seqlen_q,
                                      max_seqlen_k=max_seqlen_k, causal=causal, softmax_scale=softmax_scale, out_dtype=out_dtype,
                                      return_lse=True, sinks=sinks)
        o16 = out if out.dtype == q.dtype else out.to(q.dtype)
        ctx.save_for_backward(q, k, v, o16, lse, cu_seqlens_q, cu_seqlens_k, sinks)
        ctx.meta = (max_seqlen_q, max_seqlen_k, causal, softmax_scale)
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, out, lse, cu_q, cu_k, sinks = ctx.saved_tensors
        max_q, max_k, causal, softmax_scale = ctx.meta
        grads = fa3_varlen_backward(q, k, v, out, dout.to(q.dtype), lse, cu_seqlens_q=cu_q, cu_seqlens_k=cu_k, max_seqlen_q=max_q,
                                    max_seqlen_k=max_k, causal=causal, softmax_scale=softmax_scale,
                                    sinks=sinks if ctx.needs_input_grad[3] else None)
        return grads[0], grads[1], grads[2], (grads[3] if len(grads) > 3 else None), None, None, None, None, None, None, None


def fa3_varlen_attention(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, dropout_p: float = 0.0,
                         softmax_scale: Optional[float] = None, causal: bool = False, *, out_dtype: Optional[torch.dtype] = None,
                         sinks: Optional[torch.Tensor] = None, q_norm_weight: Optional[torch.Tensor] = None,
                         k_norm_weight: Optional[torch.Tensor] = None, qk_norm_eps: float = 1e-6, qk_norm_unit_offset: bool = False,
                         rotary_cos: Optional[torch.Tensor] = None,
                         rotary_sin: Optional[torch.Tensor] = None, rotary_interleaved: bool = False,
                         pos_offsets: Optional[torch.Tensor] = None, position_ids: Optional[torch.Tensor] = None):
    """Autograd-aware packed variable-length attention, arguments in the order of flash-attn's ``flash_attn_varlen_func``: q
    ``[total_q, H, D]``, k / v ``[total_k, Hkv, D]``, int32 device ``cu_seqlens_*`` ``[B + 1]``, host ints ``max_seqlen_*``.  Forward
    and backward on the packed HIP kernels (``fa3_varlen_forward`` / ``fa3_varlen_backward``: their conventions hold, the dense
    top-left ``causal`` rule among them); returns ``out [total_q, H, D]``.  ``dropout_p`` must be 0: there is no dropout here.
    Rows no sequence covers get whatever ``torch.empty`` left, in the output and in the gradients (``cu[B] == total`` leaves none).
    ``rotary_cos`` / ``rotary_sin`` (with ``rotary_interleaved``, ``pos_offsets``, ``position_ids``): q and k are rotated first by
    ``apply_rotary`` at their row in the sequence -- one launch for packed self-attention (``cu_seqlens_k is cu_seqlens_q``), else one
    each over their own ``cu_seqlens`` -- and the call is the one without them on the rotated operands, in both directions.
    ``q_norm_weight`` / ``k_norm_weight`` (with ``qk_norm_eps``, ``qk_norm_unit_offset``): ``qk_norm`` takes the place of that step,
    the rotation (if any) fused into its launch, under the same one-launch rule."""
    if dropout_p:
        raise NotImplementedError("attention dropout is not implemented on the packed path (dropout_p must be 0)")
    rot = _train_rotary_kw(rotary_cos, rotary_sin, rotary_interleaved, pos_offsets, position_ids)
    qkn = _train_qk_norm_kw(q_norm_weight, k_norm_weight, qk_norm_eps, qk_norm_unit_offset)
    if qkn is not None:
        qkn.update(rot or {})
        if cu_seqlens_q is cu_seqlens_k and _host_int(max_seqlen_q) == _host_int(max_seqlen_k):
            q, k = qk_norm(q, k, q_weight=q_norm_weight, k_weight=k_norm_weight, cu_seqlens=cu_seqlens_q, max_seqlen=max_seqlen_q, **qkn)
        else:
            q = qk_norm(q, q_weight=q_norm_weight, cu_seqlens=cu_seqlens_q, max_seqlen=max_seqlen_q, **qkn)
            k = qk_norm(k, q_weight=k_norm_weight, cu_seqlens=cu_seqlens_k, max_seqlen=max_seqlen_k, **qkn)
    elif rot is not None:
        if cu_seqlens_q is cu_seqlens_k and _host_int(max_seqlen_q) == _host_int(max_seqlen_k):
            q, k = apply_rotary(q, k, cu_seqlens=cu_seqlens_q, max_seqlen=max_seqlen_q, **rot)
        else:
            q = apply_rotary(q, cu_seqlens=cu_seqlens_q, max_seqlen=max_seqlen_q, **rot)
            k = apply_rotary(k, cu_seqlens=cu_seqlens_k, max_seqlen=max_seqlen_k, **rot)
    if sinks is not None:      # fp32 [H] attention sinks (fa3_varlen_forward), differentiable
        return _FA3VarlenSinkFunction.apply(q, k, v, sinks, cu_seqlens_q, cu_seqlens_k, operator.index(max_seqlen_q),
                                            operator.index(max_seqlen_k), bool(causal), softmax_scale, out_dtype)
    return _FA3VarlenFunction.apply(q, k, v, cu_seqlens_q, cu_seqlens_k, operator.index(max_seqlen_q), operator.index(max_seqlen_k),
                                    bool(causal), softmax_scale, out_dtype)

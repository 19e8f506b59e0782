"""ctypes binding of the part of ``libpfa_hip.so``'s C ABI that ``include/pfa_hip_qk_norm.h`` declares: QK-norm fused with the rotary
embedding of the training calls (``pfa_qk_norm*``, ``pfa_qk_norm_bwd*``).  The counterpart of ``_capi`` for that header, arranged as
``_capi_rotary`` is: the library is the one ``_capi.load()`` loads, and ``load()`` here types these exports on it."""

from __future__ import annotations

import ctypes as C

from . import _capi

PFA_QKNORM_INTERLEAVED = 1
PFA_QKNORM_UNIT_OFFSET = 2

_STRIDES = [(n, C.c_int64) for n in ("pid_stride_b", "pid_stride_s", "cs_stride")]
_TAIL = [("eps", C.c_float)] + [(n, C.c_int32) for n in ("B", "S", "total", "H0", "H1", "D", "rot_dim", "max_pos", "dtype", "w_dtype", "device_id")]


class PfaQkNormArgs(C.Structure):
    """Mirror of ``struct pfa_qk_norm_args`` (include/pfa_hip_qk_norm.h)."""
    _fields_ = (
        [("size", C.c_uint32), ("flags", C.c_uint32)]
        + [(n, C.c_void_p) for n in ("x0", "x0_out", "x1", "x1_out", "w0", "w1", "cos", "sin", "cu_seqlens", "pos_offsets", "position_ids")]
        + [(f"{t}_stride_{x}", C.c_int64) for t in ("x0", "x0o", "x1", "x1o") for x in "bsh"]
        + _STRIDES + _TAIL
    )


class PfaQkNormBwdArgs(C.Structure):
    """Mirror of ``struct pfa_qk_norm_bwd_args`` (include/pfa_hip_qk_norm.h)."""
    _fields_ = (
        [("size", C.c_uint32), ("flags", C.c_uint32)]
        + [(n, C.c_void_p) for n in ("x0", "dy0", "dx0", "w0", "dw0", "x1", "dy1", "dx1", "w1", "dw1", "cos", "sin", "cu_seqlens", "pos_offsets",
                                     "position_ids", "workspace")]
        + [("workspace_bytes", C.c_size_t)]
        + [(f"{t}_stride_{x}", C.c_int64) for t in ("x0", "dy0", "dx0", "x1", "dy1", "dx1") for x in "bsh"]
        + _STRIDES + _TAIL
    )


def _prototypes():
    """Export name -> ``(restype, argtypes)``, one row per symbol ``include/pfa_hip_qk_norm.h`` declares."""
    i, vp, buf = C.c_int, C.c_void_p, [C.c_char_p, C.c_size_t]
    fwd, bwd = C.POINTER(PfaQkNormArgs), C.POINTER(PfaQkNormBwdArgs)
    return {
        "pfa_qk_norm_check": (i, [fwd]),
        "pfa_qk_norm": (i, [fwd, vp]),
        "pfa_qk_norm_describe": (i, [fwd] + buf),
        "pfa_qk_norm_bwd_workspace_bytes": (C.c_size_t, [bwd]),
        "pfa_qk_norm_bwd_check": (i, [bwd]),
        "pfa_qk_norm_bwd": (i, [bwd, vp]),
        "pfa_qk_norm_bwd_describe": (i, [bwd] + buf),
    }


_PROTOTYPES = _prototypes()
EXPORTS = tuple(_PROTOTYPES)

load = _capi.bind(_PROTOTYPES)      # ``_capi.load()``'s library with the exports of this header typed (once)


def make_qk_norm_args(**kw) -> PfaQkNormArgs:
    return _capi._make(PfaQkNormArgs, kw)


def make_qk_norm_bwd_args(**kw) -> PfaQkNormBwdArgs:
    return _capi._make(PfaQkNormBwdArgs, kw)


def describe_qk_norm(args: PfaQkNormArgs):
    """-> (kernel name ``qk_norm_{bf16|fp16}_d{64|128}[_packed][_interleaved][_rot][_unit][_w32][_inplace]``, workgroups
    ``B * ceil(S * units / 256)``) of ``pfa_qk_norm``, from host shapes only."""
    load()
    return _capi._describe("pfa_qk_norm_describe", args)


def describe_qk_norm_bwd(args: PfaQkNormBwdArgs):
    """-> (kernel names ``qk_norm_bwd_..._r32+dw``, stage-1 workgroups ``T * B * ceil(S / 32)``) of ``pfa_qk_norm_bwd``."""
    load()
    return _capi._describe("pfa_qk_norm_bwd_describe", args)


def bwd_workspace_bytes(args: PfaQkNormBwdArgs) -> int:
    """The workspace ``pfa_qk_norm_bwd`` needs for the block's shape, in bytes (0: the shape is refused)."""
    return int(load().pfa_qk_norm_bwd_workspace_bytes(C.byref(args)))

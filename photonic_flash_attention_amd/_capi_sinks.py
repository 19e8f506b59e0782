"""ctypes binding of the part of ``libpfa_hip.so``'s C ABI that ``include/pfa_hip_train_sinks.h`` declares: attention sinks for
training (``pfa_fa3_fwd_sink*``, ``pfa_fa3_varlen_fwd_sink*``, ``pfa_fa3_sink_grad*``).  The counterpart of ``_capi`` for that header:
the argument blocks of ``include/pfa_hip.h`` (``PfaFa3Args``, ``PfaFa3VarlenArgs``, ``PfaFa3Sinks``) are ``_capi``'s, the library is
the one ``_capi.load()`` loads, and ``load()`` here types these exports on it."""

from __future__ import annotations

import ctypes as C
from typing import Optional

from . import _capi
from ._capi import PfaFa3Args, PfaFa3Sinks, PfaFa3VarlenArgs


class PfaFa3SinkGradArgs(C.Structure):
    """Mirror of ``struct pfa_fa3_sink_grad_args`` (include/pfa_hip_train_sinks.h): the gradient of the training forward's attention sinks."""
    _fields_ = (
        [("size", C.c_uint32), ("flags", C.c_uint32)]
        + [(n, C.c_void_p) for n in ("lse", "delta", "sinks", "d_sinks", "cu_seqlens_q", "workspace")]
        + [("workspace_bytes", C.c_size_t)]
        + [(n, C.c_int64) for n in ("lse_stride_b", "lse_stride_h", "delta_stride_b", "delta_stride_h")]
        + [(n, C.c_int32) for n in ("B", "H", "Sq", "total_q", "device_id", "reserved0")]
    )


def _prototypes():
    """Export name -> ``(restype, argtypes)``, one row per symbol ``include/pfa_hip_train_sinks.h`` declares."""
    i, sz, vp, buf = C.c_int, C.c_size_t, C.c_void_p, [C.c_char_p, C.c_size_t]
    fa3, vl, snk, sgr = (C.POINTER(t) for t in (PfaFa3Args, PfaFa3VarlenArgs, PfaFa3Sinks, PfaFa3SinkGradArgs))
    return {
        "pfa_fa3_fwd_sink_check": (i, [fa3, snk]),
        "pfa_fa3_fwd_sink": (i, [fa3, snk, vp]),
        "pfa_fa3_fwd_sink_describe": (i, [fa3, snk] + buf),
        "pfa_fa3_varlen_fwd_sink_check": (i, [vl, snk]),
        "pfa_fa3_varlen_fwd_sink": (i, [vl, snk, vp]),
        "pfa_fa3_varlen_fwd_sink_describe": (i, [vl, snk] + buf),
        "pfa_fa3_sink_grad_workspace_bytes": (sz, [sgr]),
        "pfa_fa3_sink_grad_check": (i, [sgr]),
        "pfa_fa3_sink_grad": (i, [sgr, vp]),
        "pfa_fa3_sink_grad_describe": (i, [sgr] + buf),
    }


_PROTOTYPES = _prototypes()
EXPORTS = tuple(_PROTOTYPES)

load = _capi.bind(_PROTOTYPES)      # ``_capi.load()``'s library with the exports of this header typed (once)


def make_sink_grad_args(**kw) -> PfaFa3SinkGradArgs:
    return _capi._make(PfaFa3SinkGradArgs, kw)


def describe_fwd_sink(args: PfaFa3Args, sinks: Optional[PfaFa3Sinks]):
    """``_capi.describe`` of ``pfa_fa3_fwd_sink`` (``sinks`` None: ``pfa_fa3_fwd``): the 8-wave kernel's name with "_sink" in front of its tag."""
    load()
    return _capi._describe("pfa_fa3_fwd_sink_describe", args, sinks)


def describe_varlen_fwd_sink(args: PfaFa3VarlenArgs, sinks: Optional[PfaFa3Sinks]):
    """``_capi.describe_varlen`` of ``pfa_fa3_varlen_fwd_sink``."""
    load()
    return _capi._describe("pfa_fa3_varlen_fwd_sink_describe", args, sinks)


def describe_sink_grad(args: PfaFa3SinkGradArgs):
    """-> (kernel names, stage-1 workgroups ``H * B * ceil(Sq / 2048)``) of ``pfa_fa3_sink_grad``, from host shapes only."""
    load()
    return _capi._describe("pfa_fa3_sink_grad_describe", args)

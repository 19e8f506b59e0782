"""ctypes binding of the part of ``libpfa_hip.so``'s C ABI that ``include/pfa_hip_mla_prefill.h`` declares: the non-absorbed MLA prefill
over packed sequences (``pfa_mla_prefill*``).  The counterpart of ``_capi`` for that header, arranged as ``_capi_mla`` is: the library is
the one ``_capi.load()`` loads, and ``load()`` here types these exports on it.  The header declares one struct, mirrored here."""

from __future__ import annotations

import ctypes as C

from . import _capi

D_NOPE, D_ROPE, D_V = 128, 64, 128      # PFA_MLA_PREFILL_D_NOPE, _D_ROPE, _D_V
D_QK = D_NOPE + D_ROPE
BLOCK_M = 256                           # query rows per workgroup: the grid is ceil(max_seqlen_q / 256) * B * H


class PfaMlaPrefillArgs(C.Structure):
    """Mirror of ``struct pfa_mla_prefill_args`` (include/pfa_hip_mla_prefill.h)."""
    _fields_ = (
        [("size", C.c_uint32), ("flags", C.c_uint32)]
        + [(n, C.c_void_p) for n in ("q", "k_nope", "k_rope", "v", "o", "lse", "cu_seqlens_q", "cu_seqlens_k")]
        + [(f"{t}_stride_{a}", C.c_int64) for t in ("q", "kn", "kr", "v", "o") for a in "sh"]
        + [(n, C.c_int32) for n in ("B", "H", "rope_heads", "total_q", "total_k", "max_seqlen_q", "max_seqlen_k", "dtype_in", "dtype_out",
                                    "causal")]
        + [("softmax_scale", C.c_float), ("device_id", C.c_int32), ("reserved", C.c_int32)]
    )


def _prototypes():
    """Export name -> ``(restype, argtypes)``, one row per symbol ``include/pfa_hip_mla_prefill.h`` declares."""
    i, a = C.c_int, C.POINTER(PfaMlaPrefillArgs)
    return {
        "pfa_mla_prefill_check": (i, [a]),
        "pfa_mla_prefill": (i, [a, C.c_void_p]),
        "pfa_mla_prefill_describe": (i, [a, C.c_char_p, C.c_size_t]),
    }


_PROTOTYPES = _prototypes()
EXPORTS = tuple(_PROTOTYPES)

load = _capi.bind(_PROTOTYPES)      # ``_capi.load()``'s library with the exports of this header typed (once)


def make_mla_prefill_args(**kw) -> PfaMlaPrefillArgs:
    return _capi._make(PfaMlaPrefillArgs, kw)


def describe_mla_prefill(args: PfaMlaPrefillArgs):
    """-> (kernel name ``mla_prefill_{bf16|fp16}_{o16|o32}_{causal|full}_{rope1|ropeH}``, workgroups of the launch) of
    ``pfa_mla_prefill``, from host shapes only."""
    load()
    return _capi._describe("pfa_mla_prefill_describe", args)

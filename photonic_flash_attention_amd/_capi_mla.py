"""ctypes binding of the part of ``libpfa_hip.so``'s C ABI that ``include/pfa_hip_mla.h`` declares: the MLA decode over a latent KV cache
(``pfa_mla_decode*``).  The counterpart of ``_capi`` for that header, arranged as ``_capi_decode_d256`` is: the library is the one
``_capi.load()`` loads, and ``load()`` here types these exports on it.  The header declares one struct, mirrored here."""

from __future__ import annotations

import ctypes as C

from . import _capi

D_QK, D_V = 576, 512        # PFA_MLA_D_QK, PFA_MLA_D_V


class PfaMlaDecodeArgs(C.Structure):
    """Mirror of ``struct pfa_mla_decode_args`` (include/pfa_hip_mla.h)."""
    _fields_ = (
        [("size", C.c_uint32), ("flags", C.c_uint32)]
        + [(n, C.c_void_p) for n in ("q", "kv_cache", "o", "lse", "cache_seqlens")]
        + [(f"{t}_stride_{a}", C.c_int64) for t in "qo" for a in "bhs"]
        + [("kv_stride_b", C.c_int64), ("kv_stride_s", C.c_int64)]
        + [("block_table", C.c_void_p), ("block_table_stride_b", C.c_int64), ("page_size", C.c_int32), ("num_pages", C.c_int32)]
        + [(n, C.c_int32) for n in ("B", "H", "Sq", "Smax", "dtype_in", "dtype_out", "causal")]
        + [("softmax_scale", C.c_float), ("device_id", C.c_int32), ("reserved", C.c_int32)]
        + [("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t)]
    )


def _prototypes():
    """Export name -> ``(restype, argtypes)``, one row per symbol ``include/pfa_hip_mla.h`` declares."""
    i, a = C.c_int, C.POINTER(PfaMlaDecodeArgs)
    return {
        "pfa_mla_decode_workspace_bytes": (C.c_size_t, [a]),
        "pfa_mla_decode_check": (i, [a]),
        "pfa_mla_decode": (i, [a, C.c_void_p]),
        "pfa_mla_decode_describe": (i, [a, C.c_char_p, C.c_size_t, C.POINTER(C.c_int32)]),
    }


_PROTOTYPES = _prototypes()
EXPORTS = tuple(_PROTOTYPES)

load = _capi.bind(_PROTOTYPES)      # ``_capi.load()``'s library with the exports of this header typed (once)


def make_mla_decode_args(**kw) -> PfaMlaDecodeArgs:
    return _capi._make(PfaMlaDecodeArgs, kw)


def describe_mla_decode(args: PfaMlaDecodeArgs):
    """-> (kernel name ``mla_decode_{bf16|fp16}_{o16|o32}[+combine][_paged]``, workgroups of the main launch, number of key splits) of
    ``pfa_mla_decode``, from host shapes only."""
    load()
    return _capi._describe("pfa_mla_decode_describe", args, nsplit=True)

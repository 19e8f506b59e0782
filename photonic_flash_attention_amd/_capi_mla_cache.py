"""ctypes binding of the part of ``libpfa_hip.so``'s C ABI that ``include/pfa_hip_mla_cache.h`` declares: the MLA decode over an FP8
(e4m3fn) latent cache (``pfa_mla_decode_q8*``) and the latent-cache append at width 576 (``pfa_mla_append*``).  Arranged as ``_capi_mla``
is, whose argument block the decode takes: the library is the one ``_capi.load()`` loads, and ``load()`` here types these exports on it.
The header declares two structs, mirrored here."""

from __future__ import annotations

import ctypes as C
from typing import Optional

from . import _capi
from ._capi_mla import PfaMlaDecodeArgs


class PfaMlaKvQuant(C.Structure):
    """Mirror of ``struct pfa_mla_kv_quant`` (include/pfa_hip_mla_cache.h)."""
    _fields_ = [("size", C.c_uint32), ("flags", C.c_uint32), ("kv_dtype", C.c_int32), ("reserved", C.c_int32), ("kv_descale", C.c_void_p),
                ("descale_stride_b", C.c_int64)]


class PfaMlaAppendArgs(C.Structure):
    """Mirror of ``struct pfa_mla_append_args`` (include/pfa_hip_mla_cache.h)."""
    _fields_ = (
        [("size", C.c_uint32), ("flags", C.c_uint32)]
        + [(n, C.c_void_p) for n in ("kv_c", "k_pe", "kv_cache", "cache_seqlens", "cu_seqlens_q")]
        + [(f"{t}_stride_{a}", C.c_int64) for t in ("kvc", "kpe", "kv") for a in "bs"]
        + [("block_table", C.c_void_p), ("block_table_stride_b", C.c_int64), ("page_size", C.c_int32), ("num_pages", C.c_int32)]
        + [(n, C.c_int32) for n in ("B", "Smax", "total_new", "max_seqlen_q", "dtype", "device_id", "reserved", "reserved1")]
    )


def _prototypes():
    """Export name -> ``(restype, argtypes)``, one row per symbol ``include/pfa_hip_mla_cache.h`` declares."""
    i, d, q, a = C.c_int, C.POINTER(PfaMlaDecodeArgs), C.POINTER(PfaMlaKvQuant), C.POINTER(PfaMlaAppendArgs)
    return {
        "pfa_mla_decode_q8_workspace_bytes": (C.c_size_t, [d, q]),
        "pfa_mla_decode_q8_check": (i, [d, q]),
        "pfa_mla_decode_q8": (i, [d, q, C.c_void_p]),
        "pfa_mla_decode_q8_describe": (i, [d, q, C.c_char_p, C.c_size_t, C.POINTER(C.c_int32)]),
        "pfa_mla_append_check": (i, [a, q]),
        "pfa_mla_append": (i, [a, q, C.c_void_p]),
        "pfa_mla_append_describe": (i, [a, q, C.c_char_p, C.c_size_t]),
    }


_PROTOTYPES = _prototypes()
EXPORTS = tuple(_PROTOTYPES)

load = _capi.bind(_PROTOTYPES)      # ``_capi.load()``'s library with the exports of this header typed (once)


def make_mla_kv_quant(**kw) -> PfaMlaKvQuant:
    """A ``pfa_mla_kv_quant`` block; ``kv_dtype`` defaults to e4m3."""
    kw.setdefault("kv_dtype", _capi.PFA_DTYPE_FP8_E4M3)
    return _capi._make(PfaMlaKvQuant, kw)


def make_mla_append_args(**kw) -> PfaMlaAppendArgs:
    return _capi._make(PfaMlaAppendArgs, kw)


def describe_mla_decode_q8(args: PfaMlaDecodeArgs, quant: Optional[PfaMlaKvQuant]):
    """-> (kernel name ``mla_decode_q8_{bf16|fp16}_{o16|o32}[+combine][_paged]``, workgroups of the main launch, number of key splits) of
    ``pfa_mla_decode_q8``: workgroups and splits are the 16-bit call's."""
    load()
    return _capi._describe("pfa_mla_decode_q8_describe", args, quant, nsplit=True)


def describe_mla_append(args: PfaMlaAppendArgs, quant: Optional[PfaMlaKvQuant]):
    """-> (kernel name ``mla_append[_q8_{bf16|fp16}][_varlen][_paged]``, workgroups) of ``pfa_mla_append``, from host shapes only."""
    load()
    return _capi._describe("pfa_mla_append_describe", args, quant)

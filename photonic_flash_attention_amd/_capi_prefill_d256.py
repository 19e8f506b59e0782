"""ctypes binding of the part of ``libpfa_hip.so``'s C ABI that ``include/pfa_hip_prefill_d256.h`` declares: the forward over a KV cache
at head dim 256, uniform and ragged (``pfa_fa3_prefill_d256*``, ``pfa_fa3_prefill_varlen_d256*``).  Arranged as ``_capi_decode_d256`` is:
the library is the one ``_capi.load()`` loads, and ``load()`` here types these exports on it.  The header declares no struct: the calls
take ``_capi``'s ``PfaFa3DecodeArgs``, ``PfaFa3PrefillVarlenArgs`` and ``PfaFa3CacheExt``."""

from __future__ import annotations

import ctypes as C
from typing import Optional

from . import _capi


def _prototypes():
    """Export name -> ``(restype, argtypes)``, one row per symbol ``include/pfa_hip_prefill_d256.h`` declares."""
    i, ext = C.c_int, C.POINTER(_capi.PfaFa3CacheExt)
    rows = {}
    for name, args in (("pfa_fa3_prefill_d256", C.POINTER(_capi.PfaFa3DecodeArgs)),
                       ("pfa_fa3_prefill_varlen_d256", C.POINTER(_capi.PfaFa3PrefillVarlenArgs))):
        rows[name + "_check"] = (i, [args, ext])
        rows[name] = (i, [args, ext, C.c_void_p])
        rows[name + "_describe"] = (i, [args, ext, C.c_char_p, C.c_size_t])
    return rows


_PROTOTYPES = _prototypes()
EXPORTS = tuple(_PROTOTYPES)

load = _capi.bind(_PROTOTYPES)      # ``_capi.load()``'s library with the exports of this header typed (once)


def describe_prefill_d256(args: _capi.PfaFa3DecodeArgs, ext: Optional[_capi.PfaFa3CacheExt] = None):
    """-> (kernel name ``fa3_prefill_{bf16|fp16}_d256_{o16|o32}[_causal][_win][_paged]``, workgroups ``B * H * ceil(Sq / 128)``) of
    ``pfa_fa3_prefill_d256``, from host shapes only."""
    load()
    return _capi._describe("pfa_fa3_prefill_d256_describe", args, ext)


def describe_prefill_varlen_d256(args: _capi.PfaFa3PrefillVarlenArgs, ext: Optional[_capi.PfaFa3CacheExt] = None):
    """-> (kernel name with ``_varlen``, workgroups ``B * H * ceil(max_seqlen_q / 128)``) of ``pfa_fa3_prefill_varlen_d256``."""
    load()
    return _capi._describe("pfa_fa3_prefill_varlen_d256_describe", args, ext)

"""ctypes binding of the part of ``libpfa_hip.so``'s C ABI that ``include/pfa_hip_decode_d256.h`` declares: decode attention over a KV
cache at head dim 256 (``pfa_fa3_decode_d256*``).  The counterpart of ``_capi`` for that header, arranged as ``_capi_rotary`` is: the
library is the one ``_capi.load()`` loads, and ``load()`` here types these exports on it.  The header declares no struct: the calls take
``_capi``'s ``PfaFa3DecodeArgs`` and ``PfaFa3CacheExt``."""

from __future__ import annotations

import ctypes as C
from typing import Optional

from . import _capi


def _prototypes():
    """Export name -> ``(restype, argtypes)``, one row per symbol ``include/pfa_hip_decode_d256.h`` declares."""
    i, dec, ext = C.c_int, C.POINTER(_capi.PfaFa3DecodeArgs), C.POINTER(_capi.PfaFa3CacheExt)
    return {
        "pfa_fa3_decode_d256_workspace_bytes": (C.c_size_t, [dec, ext]),
        "pfa_fa3_decode_d256_check": (i, [dec, ext]),
        "pfa_fa3_decode_d256": (i, [dec, ext, C.c_void_p]),
        "pfa_fa3_decode_d256_describe": (i, [dec, ext, C.c_char_p, C.c_size_t, C.POINTER(C.c_int32)]),
    }


_PROTOTYPES = _prototypes()
EXPORTS = tuple(_PROTOTYPES)

load = _capi.bind(_PROTOTYPES)      # ``_capi.load()``'s library with the exports of this header typed (once)


def describe_decode_d256(args: _capi.PfaFa3DecodeArgs, ext: Optional[_capi.PfaFa3CacheExt] = None):
    """-> (kernel name ``fa3_decode_{bf16|fp16}_d256_{o16|o32}[_win][+combine][_paged]``, workgroups of the main launch, number of key
    splits) of ``pfa_fa3_decode_d256``, from host shapes only."""
    load()
    return _capi._describe("pfa_fa3_decode_d256_describe", args, ext, nsplit=True)

"""ctypes binding of the part of ``libpfa_hip.so``'s C ABI that ``include/pfa_hip_rotary.h`` declares: rotary embedding for the
training calls (``pfa_rotary*``).  The counterpart of ``_capi`` for that header, arranged as ``_capi_sinks`` is: the library is the one
``_capi.load()`` loads, and ``load()`` here types these exports on it."""

from __future__ import annotations

import ctypes as C

from . import _capi

PFA_ROTARY_INTERLEAVED = 1
PFA_ROTARY_CONJUGATE = 2


class PfaRotaryArgs(C.Structure):
    """Mirror of ``struct pfa_rotary_args`` (include/pfa_hip_rotary.h)."""
    _fields_ = (
        [("size", C.c_uint32), ("flags", C.c_uint32)]
        + [(n, C.c_void_p) for n in ("x0", "x0_out", "x1", "x1_out", "cos", "sin", "cu_seqlens", "pos_offsets", "position_ids")]
        + [(f"{t}_stride_{x}", C.c_int64) for t in ("x0", "x0o", "x1", "x1o") for x in "bsh"]
        + [(n, C.c_int64) for n in ("pid_stride_b", "pid_stride_s", "cs_stride")]
        + [(n, C.c_int32) for n in ("B", "S", "total", "H0", "H1", "D", "rot_dim", "max_pos", "dtype", "device_id")]
    )


def _prototypes():
    """Export name -> ``(restype, argtypes)``, one row per symbol ``include/pfa_hip_rotary.h`` declares."""
    i, vp, rot = C.c_int, C.c_void_p, C.POINTER(PfaRotaryArgs)
    return {
        "pfa_rotary_check": (i, [rot]),
        "pfa_rotary": (i, [rot, vp]),
        "pfa_rotary_describe": (i, [rot, C.c_char_p, C.c_size_t]),
    }


_PROTOTYPES = _prototypes()
EXPORTS = tuple(_PROTOTYPES)

load = _capi.bind(_PROTOTYPES)      # ``_capi.load()``'s library with the exports of this header typed (once)


def make_rotary_args(**kw) -> PfaRotaryArgs:
    return _capi._make(PfaRotaryArgs, kw)


def describe_rotary(args: PfaRotaryArgs):
    """-> (kernel name ``rotary_{bf16|fp16}[_packed][_interleaved][_conj][_inplace]``, workgroups ``B * ceil(S * units / 256)``) of
    ``pfa_rotary``, from host shapes only."""
    load()
    return _capi._describe("pfa_rotary_describe", args)

"""ctypes binding of the part of ``libpfa_hip.so``'s C ABI that ``include/pfa_hip_norm_rope_append.h`` declares: QK-norm, rotary
embedding and the FP8 store fused into the KV-cache append (``pfa_norm_rope_append*``).  The counterpart of ``_capi`` for that header,
arranged as ``_capi_rotary`` and ``_capi_qk_norm`` are: the library is the one ``_capi.load()`` loads, and ``load()`` here types these
exports on it."""

from __future__ import annotations

import ctypes as C

from . import _capi

PFA_NRA_INTERLEAVED = 1
PFA_NRA_UNIT_OFFSET = 2


class PfaNormRopeAppendArgs(C.Structure):
    """Mirror of ``struct pfa_norm_rope_append_args`` (include/pfa_hip_norm_rope_append.h)."""
    _fields_ = (
        [("size", C.c_uint32), ("flags", C.c_uint32)]
        + [(n, C.c_void_p) for n in ("q", "q_out", "k_new", "v_new", "k_cache", "v_cache", "cos", "sin", "cu_seqlens_q", "cache_seqlens",
                                     "pos_offsets", "q_weight", "k_weight", "k_descale", "v_descale")]
        + [(f"{t}_stride_{a}", C.c_int64) for t in ("q", "qo", "kn", "vn") for a in "bsh"]
        + [(f"{t}_stride_{a}", C.c_int64) for t in "kv" for a in "bhs"]
        + [("cs_stride", C.c_int64), ("ds_sb", C.c_int64), ("eps", C.c_float)]
        + [(n, C.c_int32) for n in ("B", "H", "Hkv", "total_new", "max_seqlen_q", "Smax", "D", "rot_dim", "max_pos", "dtype", "weight_dtype",
                                    "kv_dtype", "device_id")]
        + [("block_table", C.c_void_p), ("block_table_stride_b", C.c_int64), ("page_size", C.c_int32), ("num_pages", C.c_int32)]
        + [("reserved0", C.c_int32), ("reserved1", C.c_int32)]
    )


def _prototypes():
    """Export name -> ``(restype, argtypes)``, one row per symbol ``include/pfa_hip_norm_rope_append.h`` declares."""
    a = C.POINTER(PfaNormRopeAppendArgs)
    return {
        "pfa_norm_rope_append_check": (C.c_int, [a]),
        "pfa_norm_rope_append": (C.c_int, [a, C.c_void_p]),
        "pfa_norm_rope_append_describe": (C.c_int, [a, C.c_char_p, C.c_size_t]),
    }


_PROTOTYPES = _prototypes()
EXPORTS = tuple(_PROTOTYPES)

load = _capi.bind(_PROTOTYPES)      # ``_capi.load()``'s library with the exports of this header typed (once)


def make_norm_rope_append_args(**kw) -> PfaNormRopeAppendArgs:
    return _capi._make(PfaNormRopeAppendArgs, kw)


def describe_norm_rope_append(args: PfaNormRopeAppendArgs):
    """-> (kernel name ``norm_rope_append_{bf16|fp16}_d{64|128}[_varlen][_paged][_il][_rot][_qn][_kn][_unit][_w32][_q8]``, workgroups
    ``B * ceil(max_seqlen_q * (H + 2 * Hkv) * (D / 16) / 256)``) of ``pfa_norm_rope_append``, from host shapes only."""
    load()
    return _capi._describe("pfa_norm_rope_append_describe", args)

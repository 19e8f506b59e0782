"""ctypes binding of ``libpfa_hip.so`` (C ABI declared in ``include/pfa_hip.h``).

PyTorch is plumbing here: it owns device memory and streams; the library gets raw device
pointers, element strides and the current ``hipStream_t``.  There is NO CPU or eager
fallback in this module: if the native library is missing or refuses the arguments the
call raises.
"""

from __future__ import annotations

import ctypes as C
import os
import threading
from typing import Optional

PFA_ABI_VERSION = 9
PFA_DTYPE_BF16, PFA_DTYPE_FP16, PFA_DTYPE_FP32, PFA_DTYPE_FP8_E4M3 = 0, 1, 2, 3
PFA_FLAG_SPLIT_P = 0x1
PFA_FLAG_NO_XCD_MAP = 0x2
PFA_ROPE_INTERLEAVED = 0x1
PFA_MERGE_MAX_PARTS = 8
PFA_PREFILL_MAX_SPLITS = 8

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG_DIR, "libpfa_hip.so")

class PfaFa3Args(C.Structure):
    """Mirror of ``struct pfa_fa3_args`` (include/pfa_hip.h)."""
    _fields_ = [
        ("size", C.c_uint32), ("flags", C.c_uint32),
        ("q", C.c_void_p), ("k", C.c_void_p), ("v", C.c_void_p), ("o", C.c_void_p),
        ("lse", C.c_void_p), ("seqlens_k", C.c_void_p), ("key_mask", C.c_void_p),
        ("q_stride_b", C.c_int64), ("q_stride_h", C.c_int64), ("q_stride_s", C.c_int64),
        ("k_stride_b", C.c_int64), ("k_stride_h", C.c_int64), ("k_stride_s", C.c_int64),
        ("v_stride_b", C.c_int64), ("v_stride_h", C.c_int64), ("v_stride_s", C.c_int64),
        ("o_stride_b", C.c_int64), ("o_stride_h", C.c_int64), ("o_stride_s", C.c_int64),
        ("key_mask_stride_b", C.c_int64),
        ("B", C.c_int32), ("H", C.c_int32), ("Sq", C.c_int32), ("Sk", C.c_int32), ("D", C.c_int32),
        ("dtype_in", C.c_int32), ("dtype_out", C.c_int32), ("causal", C.c_int32),
        ("softmax_scale", C.c_float), ("device_id", C.c_int32),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
        ("mask", C.c_void_p),
        ("mask_stride_b", C.c_int64), ("mask_stride_h", C.c_int64), ("mask_stride_q", C.c_int64),
        ("mask_stride_k", C.c_int64),
        ("kv_group", C.c_int32), ("reserve_cus", C.c_int32),
        ("drop_mask", C.c_void_p), ("drop_scale", C.c_float), ("reserved1", C.c_int32),
    ]


class PfaFa3BwdArgs(C.Structure):
    """Mirror of ``struct pfa_fa3_bwd_args`` (include/pfa_hip.h)."""
    _fields_ = (
        [("size", C.c_uint32), ("flags", C.c_uint32)]
        + [(n, C.c_void_p) for n in ("q", "k", "v", "o", "dout", "lse", "dq", "dk", "dv", "delta", "seqlens_k")]
        + [(f"{t}_stride_{a}", C.c_int64) for t in ("q", "k", "v", "o", "do", "dq", "dk", "dv") for a in "bhs"]
        + [(n, C.c_int32) for n in ("B", "H", "Sq", "Sk", "D", "dtype", "dtype_grad", "causal")]
        + [("softmax_scale", C.c_float), ("device_id", C.c_int32)]
        + [("mask", C.c_void_p)] + [(f"mask_stride_{a}", C.c_int64) for a in "bhqk"]
        + [("drop_mask", C.c_void_p), ("drop_scale", C.c_float), ("kv_group", C.c_int32)]
        + [("mask_workspace", C.c_void_p), ("mask_workspace_bytes", C.c_size_t)]
    )


class PfaFa3DecodeArgs(C.Structure):
    """Mirror of ``struct pfa_fa3_decode_args`` (include/pfa_hip.h, ABI v9: the paging fields are appended)."""
    _fields_ = (
        [("size", C.c_uint32), ("flags", C.c_uint32)]
        + [(n, C.c_void_p) for n in ("q", "k_cache", "v_cache", "o", "lse", "cache_seqlens", "key_mask")]
        + [(f"{t}_stride_{a}", C.c_int64) for t in "qkvo" for a in "bhs"]
        + [("key_mask_stride_b", C.c_int64)]
        + [(n, C.c_int32) for n in ("B", "H", "Hkv", "Sq", "Smax", "D", "dtype_in", "dtype_out", "causal")]
        + [("softmax_scale", C.c_float), ("device_id", C.c_int32), ("reserved0", C.c_int32)]
        + [("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t)]
        + [("block_table", C.c_void_p), ("block_table_stride_b", C.c_int64), ("page_size", C.c_int32), ("num_pages", C.c_int32)]
    )


class PfaFa3PrefillVarlenArgs(C.Structure):
    """Mirror of ``struct pfa_fa3_prefill_varlen_args`` (include/pfa_hip.h): packed query rows, no batch stride on q / o."""
    _fields_ = (
        [("size", C.c_uint32), ("flags", C.c_uint32)]
        + [(n, C.c_void_p) for n in ("q", "k_cache", "v_cache", "o", "lse", "cu_seqlens_q", "cache_seqlens")]
        + [(f"{t}_stride_{a}", C.c_int64) for t in "qo" for a in "sh"]
        + [(f"{t}_stride_{a}", C.c_int64) for t in "kv" for a in "bhs"]
        + [(n, C.c_int32) for n in ("B", "H", "Hkv", "total_q", "max_seqlen_q", "Smax", "D", "dtype_in", "dtype_out", "causal")]
        + [("softmax_scale", C.c_float), ("device_id", C.c_int32), ("reserved0", C.c_int32)]
        + [("block_table", C.c_void_p), ("block_table_stride_b", C.c_int64), ("page_size", C.c_int32), ("num_pages", C.c_int32)]
    )


class PfaFa3VarlenArgs(C.Structure):
    """Mirror of ``struct pfa_fa3_varlen_args`` (include/pfa_hip.h): the packed variable-length forward, no batch strides."""
    _fields_ = (
        [("size", C.c_uint32), ("flags", C.c_uint32)]
        + [(n, C.c_void_p) for n in ("q", "k", "v", "o", "lse", "cu_seqlens_q", "cu_seqlens_k")]
        + [(f"{t}_stride_{a}", C.c_int64) for t in "qkvo" for a in "sh"]
        + [(n, C.c_int32) for n in ("B", "H", "Hkv", "total_q", "total_k", "max_seqlen_q", "max_seqlen_k", "D", "dtype_in", "dtype_out",
                                    "causal")]
        + [("softmax_scale", C.c_float), ("device_id", C.c_int32), ("reserved0", C.c_int32)]
    )


class PfaFa3VarlenBwdArgs(C.Structure):
    """Mirror of ``struct pfa_fa3_varlen_bwd_args`` (include/pfa_hip.h): the packed variable-length backward."""
    _fields_ = (
        [("size", C.c_uint32), ("flags", C.c_uint32)]
        + [(n, C.c_void_p) for n in ("q", "k", "v", "o", "dout", "lse", "dq", "dk", "dv", "delta", "cu_seqlens_q", "cu_seqlens_k")]
        + [(f"{t}_stride_{a}", C.c_int64) for t in ("q", "k", "v", "o", "do", "dq", "dk", "dv") for a in "sh"]
        + [(n, C.c_int32) for n in ("B", "H", "Hkv", "total_q", "total_k", "max_seqlen_q", "max_seqlen_k", "D", "dtype", "dtype_grad",
                                    "causal")]
        + [("softmax_scale", C.c_float), ("device_id", C.c_int32), ("reserved0", C.c_int32)]
    )


class PfaFa3CacheExt(C.Structure):
    """Mirror of ``struct pfa_fa3_cache_ext`` (include/pfa_hip.h): per-call options of the ``*_ex`` calls over a KV cache."""
    _fields_ = [("size", C.c_uint32), ("flags", C.c_uint32), ("window", C.c_int32), ("reserved", C.c_int32)]


class PfaFa3TreeMask(C.Structure):
    """Mirror of ``struct pfa_fa3_tree_mask`` (include/pfa_hip.h): a 64-bit visibility word per query row of ``pfa_fa3_decode_tree``."""
    _fields_ = [("size", C.c_uint32), ("flags", C.c_uint32), ("words", C.c_void_p), ("stride_b", C.c_int64)]


class PfaFa3KvQuant(C.Structure):
    """Mirror of ``struct pfa_fa3_kv_quant`` (include/pfa_hip.h): the element type and the descales of an FP8 KV cache."""
    _fields_ = [("size", C.c_uint32), ("flags", C.c_uint32), ("kv_dtype", C.c_int32), ("reserved", C.c_int32),
                ("k_descale", C.c_void_p), ("v_descale", C.c_void_p), ("descale_stride_b", C.c_int64)]


class PfaFa3Sinks(C.Structure):
    """Mirror of ``struct pfa_fa3_sinks`` (include/pfa_hip.h): one fp32 attention sink per query head, for the ``*_sink`` calls."""
    _fields_ = [("size", C.c_uint32), ("flags", C.c_uint32), ("sinks", C.c_void_p)]


class PfaKvAppendArgs(C.Structure):
    """Mirror of ``struct pfa_kv_append_args`` (include/pfa_hip.h): the device-side KV-cache append."""
    _fields_ = (
        [("size", C.c_uint32), ("flags", C.c_uint32)]
        + [(n, C.c_void_p) for n in ("k_new", "v_new", "k_cache", "v_cache", "cu_seqlens_q", "cache_seqlens")]
        + [(f"{t}_stride_{a}", C.c_int64) for t in ("kn", "vn") for a in "bsh"]
        + [(f"{t}_stride_{a}", C.c_int64) for t in "kv" for a in "bhs"]
        + [(n, C.c_int32) for n in ("B", "Hkv", "total_new", "max_seqlen_q", "Smax", "D", "dtype", "device_id")]
        + [("block_table", C.c_void_p), ("block_table_stride_b", C.c_int64), ("page_size", C.c_int32), ("num_pages", C.c_int32)]
        + [("reserved0", C.c_int32), ("reserved1", C.c_int32)]
    )


class PfaRopeAppendArgs(C.Structure):
    """Mirror of ``struct pfa_rope_append_args`` (include/pfa_hip.h): rotary embedding fused into the KV-cache append."""
    _fields_ = (
        [("size", C.c_uint32), ("flags", C.c_uint32)]
        + [(n, C.c_void_p) for n in ("q", "q_out", "k_new", "v_new", "k_cache", "v_cache", "cos", "sin", "cu_seqlens_q", "cache_seqlens",
                                     "pos_offsets")]
        + [(f"{t}_stride_{a}", C.c_int64) for t in ("q", "qo", "kn", "vn") for a in "bsh"]
        + [(f"{t}_stride_{a}", C.c_int64) for t in "kv" for a in "bhs"]
        + [("cs_stride", C.c_int64)]
        + [(n, C.c_int32) for n in ("B", "H", "Hkv", "total_new", "max_seqlen_q", "Smax", "D", "rot_dim", "max_pos", "dtype", "device_id",
                                    "reserved0")]
        + [("block_table", C.c_void_p), ("block_table_stride_b", C.c_int64), ("page_size", C.c_int32), ("num_pages", C.c_int32)]
        + [("reserved1", C.c_int32)]
    )


class PfaAttnMergeArgs(C.Structure):
    """Mirror of ``struct pfa_attn_merge_args`` (include/pfa_hip.h): the merge of partial attention results."""
    _fields_ = (
        [("size", C.c_uint32), ("flags", C.c_uint32)]
        + [("o_part", C.c_void_p * PFA_MERGE_MAX_PARTS), ("lse_part", C.c_void_p * PFA_MERGE_MAX_PARTS)]
        + [("o", C.c_void_p), ("lse_out", C.c_void_p)]
        + [(f"{t}_stride_{a}", C.c_int64 * PFA_MERGE_MAX_PARTS) for t in ("op", "lp") for a in "bhs"]
        + [(f"{t}_stride_{a}", C.c_int64) for t in ("o", "lo") for a in "bhs"]
        + [(n, C.c_int32) for n in ("n_parts", "B", "H", "Sq", "D", "dtype_part", "dtype_out", "device_id", "reserved0", "reserved1")]
    )


class PfaPageCopyArgs(C.Structure):
    """Mirror of ``struct pfa_page_copy_args`` (include/pfa_hip.h): the page copy inside a paged cache's pools."""
    _fields_ = (
        [("size", C.c_uint32), ("flags", C.c_uint32)]
        + [(n, C.c_void_p) for n in ("k_pool", "v_pool", "pairs", "rows")]
        + [("pairs_stride", C.c_int64)]
        + [(f"{t}_stride_{a}", C.c_int64) for t in "kv" for a in "bhs"]
        + [(n, C.c_int32) for n in ("n_pairs", "Hkv", "D", "page_size", "num_pages", "dtype", "device_id", "reserved0")]
    )


def _prototypes():
    """Export name -> ``(restype, argtypes)``, one row per symbol ``include/pfa_hip.h`` declares (argtypes None: left untyped)."""
    i, sz, vp, buf = C.c_int, C.c_size_t, C.c_void_p, [C.c_char_p, C.c_size_t]
    fa3, bwd, dec, var, app, ext, rope, mrg = (C.POINTER(t) for t in (PfaFa3Args, PfaFa3BwdArgs, PfaFa3DecodeArgs, PfaFa3PrefillVarlenArgs,
                                                                      PfaKvAppendArgs, PfaFa3CacheExt, PfaRopeAppendArgs, PfaAttnMergeArgs))
    ns = [C.POINTER(C.c_int32)]
    pcp = C.POINTER(PfaPageCopyArgs)
    tree = C.POINTER(PfaFa3TreeMask)
    vl, vlb = C.POINTER(PfaFa3VarlenArgs), C.POINTER(PfaFa3VarlenBwdArgs)
    quant = C.POINTER(PfaFa3KvQuant)
    snk = C.POINTER(PfaFa3Sinks)
    return {
        "pfa_abi_version": (i, None),
        "pfa_status_string": (C.c_char_p, [i]),
        "pfa_device_supported": (i, [i]),
        "pfa_last_hip_error": (i, None),
        "pfa_fa3_workspace_bytes": (sz, [fa3]),
        "pfa_fa3_check": (i, [fa3]),
        "pfa_fa3_fwd": (i, [fa3, vp]),
        "pfa_fa3_describe": (i, [fa3] + buf),
        "pfa_fa3_weights": (i, [fa3, vp, C.c_int32, C.c_int64, C.c_int64, C.c_int64, vp]),
        "pfa_fa3_bwd": (i, [bwd, vp]),
        "pfa_fa3_bwd_workspace_bytes": (sz, [bwd]),
        "pfa_fa3_bwd_mask_workspace_bytes": (sz, [bwd]),
        "pfa_fa3_prepare": (i, [i]),
        "pfa_probe_mfma": (i, [vp, vp, i, i, vp, C.POINTER(C.c_double)]),
        "pfa_fa3_decode_workspace_bytes": (sz, [dec]),
        "pfa_fa3_decode_check": (i, [dec]),
        "pfa_fa3_decode": (i, [dec, vp]),
        "pfa_fa3_decode_describe": (i, [dec] + buf + ns),
        "pfa_fa3_prefill_check": (i, [dec]),
        "pfa_fa3_prefill": (i, [dec, vp]),
        "pfa_fa3_prefill_describe": (i, [dec] + buf),
        "pfa_fa3_prefill_varlen_check": (i, [var]),
        "pfa_fa3_prefill_varlen": (i, [var, vp]),
        "pfa_fa3_prefill_varlen_describe": (i, [var] + buf),
        "pfa_fa3_decode_workspace_bytes_ex": (sz, [dec, ext]),
        "pfa_fa3_decode_check_ex": (i, [dec, ext]),
        "pfa_fa3_decode_ex": (i, [dec, ext, vp]),
        "pfa_fa3_decode_describe_ex": (i, [dec, ext] + buf + ns),
        "pfa_fa3_decode_tree_workspace_bytes": (sz, [dec, ext, tree]),
        "pfa_fa3_decode_tree_check": (i, [dec, ext, tree]),
        "pfa_fa3_decode_tree": (i, [dec, ext, tree, vp]),
        "pfa_fa3_decode_tree_describe": (i, [dec, ext, tree] + buf + ns),
        "pfa_fa3_prefill_check_ex": (i, [dec, ext]),
        "pfa_fa3_prefill_ex": (i, [dec, ext, vp]),
        "pfa_fa3_prefill_describe_ex": (i, [dec, ext] + buf),
        "pfa_fa3_prefill_varlen_check_ex": (i, [var, ext]),
        "pfa_fa3_prefill_varlen_ex": (i, [var, ext, vp]),
        "pfa_fa3_prefill_varlen_describe_ex": (i, [var, ext] + buf),
        "pfa_fa3_prefill_split_plan": (i, [dec, C.c_int32]),
        "pfa_fa3_prefill_split_workspace_bytes": (sz, [dec, C.c_int32]),
        "pfa_fa3_prefill_split_check": (i, [dec, C.c_int32]),
        "pfa_fa3_prefill_split": (i, [dec, C.c_int32, vp]),
        "pfa_fa3_prefill_split_describe": (i, [dec, C.c_int32] + buf + ns),
        "pfa_kv_append_check": (i, [app]),
        "pfa_kv_append": (i, [app, vp]),
        "pfa_kv_append_describe": (i, [app] + buf),
        "pfa_rope_append_check": (i, [rope]),
        "pfa_rope_append": (i, [rope, vp]),
        "pfa_rope_append_describe": (i, [rope] + buf),
        "pfa_attn_merge_check": (i, [mrg]),
        "pfa_attn_merge": (i, [mrg, vp]),
        "pfa_attn_merge_describe": (i, [mrg] + buf),
        "pfa_page_copy_check": (i, [pcp]),
        "pfa_page_copy": (i, [pcp, vp]),
        "pfa_page_copy_describe": (i, [pcp] + buf),
        "pfa_fa3_varlen_check": (i, [vl]),
        "pfa_fa3_varlen_fwd": (i, [vl, vp]),
        "pfa_fa3_varlen_describe": (i, [vl] + buf),
        "pfa_fa3_varlen_bwd_workspace_bytes": (sz, [vlb]),
        "pfa_fa3_varlen_bwd_check": (i, [vlb]),
        "pfa_fa3_varlen_bwd": (i, [vlb, vp]),
        "pfa_fa3_varlen_bwd_describe": (i, [vlb] + buf + ns),
        "pfa_fa3_decode_q8_workspace_bytes": (sz, [dec, ext, quant]),
        "pfa_fa3_decode_q8_check": (i, [dec, ext, quant]),
        "pfa_fa3_decode_q8": (i, [dec, ext, quant, vp]),
        "pfa_fa3_decode_q8_describe": (i, [dec, ext, quant] + buf + ns),
        "pfa_kv_append_q8_check": (i, [app, quant]),
        "pfa_kv_append_q8": (i, [app, quant, vp]),
        "pfa_fa3_prefill_q8_check": (i, [dec, ext, quant]),
        "pfa_fa3_prefill_q8": (i, [dec, ext, quant, vp]),
        "pfa_fa3_prefill_q8_describe": (i, [dec, ext, quant] + buf),
        "pfa_fa3_prefill_varlen_q8_check": (i, [var, ext, quant]),
        "pfa_fa3_prefill_varlen_q8": (i, [var, ext, quant, vp]),
        "pfa_fa3_prefill_varlen_q8_describe": (i, [var, ext, quant] + buf),
        "pfa_fa3_decode_sink_workspace_bytes": (sz, [dec, ext, snk]),
        "pfa_fa3_decode_sink_check": (i, [dec, ext, snk]),
        "pfa_fa3_decode_sink": (i, [dec, ext, snk, vp]),
        "pfa_fa3_decode_sink_describe": (i, [dec, ext, snk] + buf + ns),
        "pfa_fa3_prefill_sink_check": (i, [dec, ext, snk]),
        "pfa_fa3_prefill_sink": (i, [dec, ext, snk, vp]),
        "pfa_fa3_prefill_sink_describe": (i, [dec, ext, snk] + buf),
        "pfa_fa3_prefill_varlen_sink_check": (i, [var, ext, snk]),
        "pfa_fa3_prefill_varlen_sink": (i, [var, ext, snk, vp]),
        "pfa_fa3_prefill_varlen_sink_describe": (i, [var, ext, snk] + buf),
        "pfa_fa3_prefill_split_sink_workspace_bytes": (sz, [dec, C.c_int32, snk]),
        "pfa_fa3_prefill_split_sink_check": (i, [dec, C.c_int32, snk]),
        "pfa_fa3_prefill_split_sink": (i, [dec, C.c_int32, snk, vp]),
        "pfa_fa3_prefill_split_sink_describe": (i, [dec, C.c_int32, snk] + buf + ns),
    }


_PROTOTYPES = _prototypes()
EXPORTS = tuple(_PROTOTYPES)


class PfaError(RuntimeError):
    """A non-zero ``pfa_status`` from the native library."""

    def __init__(self, status: int, text: str):
        super().__init__(f"libpfa_hip: {text} (status {status})")
        self.status = status


_lib = None
_lock = threading.Lock()


def load(path: Optional[str] = None):
    """Load (once) and type the library.  Raises ``OSError`` if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        p = path or os.environ.get("PFA_HIP_LIB", LIB_PATH)
        if not os.path.exists(p):
            raise OSError(
                f"{p} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                f"or `make -C photonic_flash_attention_amd/csrc` (there is no CPU fallback)")
        lib = C.CDLL(p)
        _type(lib, _PROTOTYPES)
        v = lib.pfa_abi_version()
        if v != PFA_ABI_VERSION:
            raise OSError(f"{p}: ABI version {v}, binding expects {PFA_ABI_VERSION}")
        _lib = lib
    return _lib


def _type(lib, prototypes) -> None:
    for name, (restype, argtypes) in prototypes.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes


def bind(prototypes):
    """The ``load`` of a side header's binding module (``_capi_sinks``, ``_capi_rotary``, ``_capi_qk_norm``): -> a function that returns
    ``load()``'s library with the exports of ``prototypes`` typed on it (once).  It raises ``OSError`` if the library has not been built."""
    typed = []

    def load_typed():
        lib = load()
        if not typed:
            with _lock:
                _type(lib, prototypes)
                typed.append(True)
        return lib
    return load_typed


def status_string(status: int) -> str:
    return load().pfa_status_string(int(status)).decode()


def check_status(status: int) -> None:
    if status != 0:
        extra = ""
        if status == -9:
            extra = f" [hipError {load().pfa_last_hip_error()}]"
        raise PfaError(status, status_string(status) + extra)


def _make(cls, kw):
    """A zeroed argument block of type ``cls`` with its ``size`` field set, then the given fields."""
    a = cls()
    a.size = C.sizeof(cls)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _describe(export: str, args, *mid, nsplit: bool = False):
    """One ``*_describe`` export: -> ``(kernel name, workgroups)``, with ``nsplit`` also the call's int32 out-parameter.
    ``mid``: what the call takes between its argument block and the buffer -- an option block goes by reference (None: the NULL block),
    a plain value such as ``key_splits`` as it is."""
    buf = C.create_string_buffer(128)
    ns = C.c_int32(0)
    refs = [C.byref(m) if isinstance(m, C.Structure) else m for m in mid] + [buf, 128] + ([C.byref(ns)] if nsplit else [])
    n = getattr(load(), export)(C.byref(args), *refs)
    if n < 0:
        check_status(n)
    return (buf.value.decode(), n, ns.value) if nsplit else (buf.value.decode(), n)


def make_args(**kw) -> PfaFa3Args:
    return _make(PfaFa3Args, kw)


def describe(args: PfaFa3Args):
    """-> (kernel variant name, number of workgroups) the library would launch."""
    return _describe("pfa_fa3_describe", args)


def make_decode_args(**kw) -> PfaFa3DecodeArgs:
    return _make(PfaFa3DecodeArgs, kw)


def describe_decode(args: PfaFa3DecodeArgs):
    """-> (kernel name, workgroups of the main launch, number of key splits) of ``pfa_fa3_decode``."""
    return _describe("pfa_fa3_decode_describe", args, nsplit=True)


def describe_prefill(args: PfaFa3DecodeArgs):
    """-> (kernel name, workgroups) of ``pfa_fa3_prefill`` (the forward over a KV cache takes the decode's argument block)."""
    return _describe("pfa_fa3_prefill_describe", args)


def make_prefill_varlen_args(**kw) -> PfaFa3PrefillVarlenArgs:
    return _make(PfaFa3PrefillVarlenArgs, kw)


def describe_prefill_varlen(args: PfaFa3PrefillVarlenArgs):
    """-> (kernel name, workgroups) of ``pfa_fa3_prefill_varlen``: ``B * H * ceil(max_seqlen_q / 256)``, from host shapes only."""
    return _describe("pfa_fa3_prefill_varlen_describe", args)


def make_cache_ext(**kw) -> PfaFa3CacheExt:
    return _make(PfaFa3CacheExt, kw)


def describe_decode_ex(args: PfaFa3DecodeArgs, ext: Optional[PfaFa3CacheExt]):
    """``describe_decode`` of ``pfa_fa3_decode_ex`` (``ext`` None: the NULL extension); "_win" marks a windowed kernel."""
    return _describe("pfa_fa3_decode_describe_ex", args, ext, nsplit=True)


def make_tree_mask(**kw) -> PfaFa3TreeMask:
    return _make(PfaFa3TreeMask, kw)


def describe_decode_tree(args: PfaFa3DecodeArgs, ext: Optional[PfaFa3CacheExt], tree: Optional[PfaFa3TreeMask]):
    """``describe_decode_ex`` of ``pfa_fa3_decode_tree`` (``tree`` None: the NULL tree, i.e. ``pfa_fa3_decode_ex``); "_tree" marks a
    kernel that takes the words."""
    return _describe("pfa_fa3_decode_tree_describe", args, ext, tree, nsplit=True)


def make_kv_quant(**kw) -> PfaFa3KvQuant:
    """A ``pfa_fa3_kv_quant`` block; ``kv_dtype`` defaults to e4m3."""
    kw.setdefault("kv_dtype", PFA_DTYPE_FP8_E4M3)
    return _make(PfaFa3KvQuant, kw)


def describe_decode_q8(args: PfaFa3DecodeArgs, ext: Optional[PfaFa3CacheExt], quant: Optional[PfaFa3KvQuant]):
    """``describe_decode_ex`` of ``pfa_fa3_decode_q8``: "_kv8" marks a kernel over an FP8 cache; workgroups and splits are the 16-bit call's."""
    return _describe("pfa_fa3_decode_q8_describe", args, ext, quant, nsplit=True)


def describe_prefill_q8(args: PfaFa3DecodeArgs, ext: Optional[PfaFa3CacheExt], quant: Optional[PfaFa3KvQuant]):
    """``describe_prefill_ex`` of ``pfa_fa3_prefill_q8``: "_kv8" marks a kernel over an FP8 cache; the workgroups are the 16-bit call's."""
    return _describe("pfa_fa3_prefill_q8_describe", args, ext, quant)


def describe_prefill_varlen_q8(args: PfaFa3PrefillVarlenArgs, ext: Optional[PfaFa3CacheExt], quant: Optional[PfaFa3KvQuant]):
    """``describe_prefill_varlen_ex`` of ``pfa_fa3_prefill_varlen_q8``."""
    return _describe("pfa_fa3_prefill_varlen_q8_describe", args, ext, quant)


def make_sinks(**kw) -> PfaFa3Sinks:
    return _make(PfaFa3Sinks, kw)


def describe_decode_sink(args: PfaFa3DecodeArgs, ext: Optional[PfaFa3CacheExt], sinks: Optional[PfaFa3Sinks]):
    """``describe_decode_ex`` of ``pfa_fa3_decode_sink`` (``sinks`` None: the NULL block, i.e. ``pfa_fa3_decode_ex``): "_sink" marks a kernel
    that takes the sinks; workgroups and splits are the sink-less call's."""
    return _describe("pfa_fa3_decode_sink_describe", args, ext, sinks, nsplit=True)


def describe_prefill_sink(args: PfaFa3DecodeArgs, ext: Optional[PfaFa3CacheExt], sinks: Optional[PfaFa3Sinks]):
    """``describe_prefill_ex`` of ``pfa_fa3_prefill_sink``."""
    return _describe("pfa_fa3_prefill_sink_describe", args, ext, sinks)


def describe_prefill_varlen_sink(args: PfaFa3PrefillVarlenArgs, ext: Optional[PfaFa3CacheExt], sinks: Optional[PfaFa3Sinks]):
    """``describe_prefill_varlen_ex`` of ``pfa_fa3_prefill_varlen_sink``."""
    return _describe("pfa_fa3_prefill_varlen_sink_describe", args, ext, sinks)


def describe_prefill_split_sink(args: PfaFa3DecodeArgs, key_splits: int, sinks: Optional[PfaFa3Sinks]):
    """``describe_prefill_split`` of ``pfa_fa3_prefill_split_sink``."""
    return _describe("pfa_fa3_prefill_split_sink_describe", args, int(key_splits), sinks, nsplit=True)


def describe_prefill_ex(args: PfaFa3DecodeArgs, ext: Optional[PfaFa3CacheExt]):
    """``describe_prefill`` of ``pfa_fa3_prefill_ex``."""
    return _describe("pfa_fa3_prefill_describe_ex", args, ext)


def describe_prefill_varlen_ex(args: PfaFa3PrefillVarlenArgs, ext: Optional[PfaFa3CacheExt]):
    """``describe_prefill_varlen`` of ``pfa_fa3_prefill_varlen_ex``."""
    return _describe("pfa_fa3_prefill_varlen_describe_ex", args, ext)


def describe_prefill_split(args: PfaFa3DecodeArgs, key_splits: int):
    """-> (kernel name, workgroups of the main launch, resolved number of key splits) of ``pfa_fa3_prefill_split`` (``key_splits`` 0:
    the library's plan); "_split{N}+merge" marks a split call."""
    return _describe("pfa_fa3_prefill_split_describe", args, int(key_splits), nsplit=True)


def make_kv_append_args(**kw) -> PfaKvAppendArgs:
    return _make(PfaKvAppendArgs, kw)


def describe_kv_append(args: PfaKvAppendArgs):
    """-> (kernel name, workgroups) of ``pfa_kv_append``: ``B * ceil(max_seqlen_q * Hkv * (D / 8) / 256)``, from host shapes only."""
    return _describe("pfa_kv_append_describe", args)


def make_rope_append_args(**kw) -> PfaRopeAppendArgs:
    return _make(PfaRopeAppendArgs, kw)


def describe_rope_append(args: PfaRopeAppendArgs):
    """-> (kernel name, workgroups) of ``pfa_rope_append``: ``B * ceil(max_seqlen_q * (H + 2 * Hkv) * (D / 16) / 256)``, from host
    shapes only."""
    return _describe("pfa_rope_append_describe", args)


def make_attn_merge_args(**kw) -> PfaAttnMergeArgs:
    """A zeroed ``pfa_attn_merge_args``; the per-part arrays (``o_part``, ``lse_part``, ``op_stride_*``, ``lp_stride_*``) are given as
    sequences of up to ``PFA_MERGE_MAX_PARTS`` values."""
    a = _make(PfaAttnMergeArgs, {k: v for k, v in kw.items() if not isinstance(v, (list, tuple))})
    for k, v in kw.items():
        if isinstance(v, (list, tuple)):
            arr = getattr(a, k)
            for n, x in enumerate(v):
                arr[n] = x
    return a


def describe_attn_merge(args: PfaAttnMergeArgs):
    """-> (kernel name, workgroups) of ``pfa_attn_merge``: ``ceil(B * Sq * H * (D / 8) / 256)``, from host shapes only."""
    return _describe("pfa_attn_merge_describe", args)


def make_page_copy_args(**kw) -> PfaPageCopyArgs:
    return _make(PfaPageCopyArgs, kw)


def describe_page_copy(args: PfaPageCopyArgs):
    """-> (kernel name, workgroups) of ``pfa_page_copy``: ``n_pairs * ceil(page_size * Hkv * (D / 8) / 1024)``, from host shapes only."""
    return _describe("pfa_page_copy_describe", args)


def make_varlen_args(**kw) -> PfaFa3VarlenArgs:
    return _make(PfaFa3VarlenArgs, kw)


def describe_varlen(args: PfaFa3VarlenArgs):
    """-> (kernel name, workgroups) of ``pfa_fa3_varlen_fwd``: ``B * H * ceil(max_seqlen_q / 256)``, from host shapes only."""
    return _describe("pfa_fa3_varlen_describe", args)


def make_varlen_bwd_args(**kw) -> PfaFa3VarlenBwdArgs:
    return _make(PfaFa3VarlenBwdArgs, kw)


def describe_varlen_bwd(args: PfaFa3VarlenBwdArgs):
    """-> (kernel names "dq+dkdv", workgroups of the dQ launch ``B * H * ceil(max_seqlen_q / 256)``, workgroups of the dK/dV launch
    ``B * Hkv * ceil(max_seqlen_k / 128)``) of ``pfa_fa3_varlen_bwd``."""
    return _describe("pfa_fa3_varlen_bwd_describe", args, nsplit=True)

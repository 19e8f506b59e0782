"""What the host-side (no GPU) tests of the C ABI share.  Plain functions, constants and one fixture; pytest collects nothing from here.

A new ``test_*_host.py`` imports from here instead of typing it again:

  ``lib``                      the module-scoped fixture: the built library through ctypes (``from capi_testlib import lib``)
  ``OK, NULL, SIZE, ...``      the values of ``pfa_status``
  ``ref(x)``                   None -> NULL, else ``byref(x)``
  ``name_of(fn, a, *mid)``     a raw ``*_describe`` export -> (return value, name, nsplit)
  ``decode_args`` / ``decode_paged``                     a valid ``pfa_fa3_decode_args`` (decode, prefill, split prefill)
  ``prefill_varlen_args`` / ``prefill_varlen_paged``     a valid ``pfa_fa3_prefill_varlen_args``
  ``kv_append_args`` / ``kv_append_uniform`` / ``kv_append_paged``     a valid ``pfa_kv_append_args`` (ragged, uniform, paged)
  ``rope_append_args`` / ``rope_append_uniform`` / ``rope_append_paged``     a valid ``pfa_rope_append_args``, the same three ways
  ``fa3_args``, ``attn_merge_args``, ``page_copy_args``, ``varlen_args``, ``varlen_bwd_args``     a valid block of the struct each names
  ``ext`` / ``tree`` / ``quant`` / ``sinks``             the option blocks of the ``*_ex``, ``*_tree``, ``*_q8`` and ``*_sink`` calls

Layout, sizes, prototypes, exported symbols and the ABI version are tests/test_capi_conformance.py's: a new struct or export is covered
there without new code, and no other file pins them.

Every builder derives its strides from the overridden shape and then lets the overrides replace whatever they name, so a rule table
is a list of ``(override, expected status)``.  The blocks with one default shape take the overrides as keywords.  ``decode_args`` and
``prefill_varlen_args`` (and their paged forms) take them as a dict, in front of the choices the older files made differently, which a
file states once in a two-line alias such as ``def _dargs(**over): return decode_args(over, Sq=4)``: ``Sq`` and ``Smax``; ``ws``, the
workspace; ``pages``, a fixed number of pages a sequence or as many as ``Smax`` holds; and ``follow``, the shape fields an override of
which moves the derived strides too (an override of another field leaves the strides of the default shape in place, which every
check takes all the same)."""

from __future__ import annotations

import ctypes as C
import os
import subprocess

import pytest

from conftest import REPO
from photonic_flash_attention_amd import _capi

OK, NULL, SIZE, SHAPE, HEAD_DIM, DTYPE, STRIDE, ALIGN, DEVICE, LAUNCH, FLAGS = 0, -1, -2, -3, -4, -5, -6, -7, -8, -9, -10     # pfa_status


def built_lib():
    """The native library through ctypes, built first if it is missing."""
    if not os.path.exists(_capi.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(REPO, "photonic_flash_attention_amd", "csrc")], check=True)
    return _capi.load()


@pytest.fixture(scope="module")
def lib():
    return built_lib()


def ref(x):
    return None if x is None else C.byref(x)


def name_of(fn, a, *mid, nsplit=False):
    """(status or workgroups, name, nsplit) of a raw describe export; ``mid``: what goes between the block and the buffer."""
    buf, ns = C.create_string_buffer(128), C.c_int32(-1)
    n = fn(C.byref(a), *mid, buf, 128, *([C.byref(ns)] if nsplit else []))
    return n, buf.value.decode(), ns.value


# --- option blocks ----------------------------------------------------------------------------------------------------------------------

def ext(**kw):
    return _capi.make_cache_ext(**kw)


def tree(**kw):
    return _capi.make_tree_mask(**{"words": 0x7000, "stride_b": 5, **kw})


def quant(**kw):
    return _capi.make_kv_quant(**{"k_descale": 0x7000, "v_descale": 0x7400, **kw})


def sinks(**kw):
    return _capi.make_sinks(**{"sinks": 0xA000, **kw})


# --- argument blocks --------------------------------------------------------------------------------------------------------------------

SHAPE_FIELDS = "D Sq H Hkv Smax"


def _shape(over, follow, **default):
    """The shape the strides are derived from: the default one, with the overrides of the fields named in ``follow``."""
    return {**default, **{k: over[k] for k in follow.split() if k in over}}


def _pages(over, s, pages):
    """The paging fields over a pool [num_pages 100, page_size, Hkv, D]; ``_page=`` in ``over`` is the page size (128).  ``pages``: that
    many pages a sequence whatever ``Smax`` says (and ``Smax`` defaults to all of them); None: as many as ``Smax`` holds."""
    ps = over.pop("_page", 128)
    base = dict(k_stride_b=ps * s["Hkv"] * s["D"], v_stride_b=ps * s["Hkv"] * s["D"], block_table=0x8000,
                block_table_stride_b=pages or s["Smax"] // ps, page_size=ps, num_pages=100)
    if pages:
        base["Smax"] = pages * ps
    return {**base, **over}


def decode_args(over, *, Sq, Smax=4096, ws=True, follow=SHAPE_FIELDS, min_rows=0):
    """A valid contiguous ``pfa_fa3_decode_args``: B 2, H 8, Hkv 2, D 128, [B, S, H, D] q, o and caches.  ``ws``: True, a workspace
    large enough for any plan; False, none; "asked", the bytes ``pfa_fa3_decode_workspace_bytes`` asks for, unless ``over`` names a
    workspace.  ``min_rows``: the rows q's and o's batch stride counts at least."""
    s = _shape(over, follow, D=128, Sq=Sq, H=8, Hkv=2, Smax=Smax)
    d, h, hkv, rows = s["D"], s["H"], s["Hkv"], max(s["Sq"], min_rows)
    base = dict(q=0x1000, k_cache=0x1000000, v_cache=0x2000000, o=0x800000, B=2, H=8, Hkv=2, Sq=Sq, Smax=Smax, D=128,
                q_stride_b=rows * h * d, q_stride_h=d, q_stride_s=h * d, k_stride_b=s["Smax"] * hkv * d, k_stride_h=d, k_stride_s=hkv * d,
                v_stride_b=s["Smax"] * hkv * d, v_stride_h=d, v_stride_s=hkv * d, o_stride_b=rows * h * d, o_stride_h=d, o_stride_s=h * d,
                dtype_in=0, dtype_out=0, causal=1, softmax_scale=d ** -0.5)
    if ws is True:
        base.update(workspace=0x4000000, workspace_bytes=1 << 40)
    base.update(over)
    a = _capi.make_decode_args(**base)
    if ws == "asked" and "workspace" not in over:
        a.workspace_bytes = _capi.load().pfa_fa3_decode_workspace_bytes(C.byref(a))
        a.workspace = 0x40000000 if a.workspace_bytes else None
    return a


def decode_paged(over, *, Sq, Smax=4096, pages=None, follow=SHAPE_FIELDS, **how):
    """``decode_args`` of the same logical shape over a pool of pages (``_pages``)."""
    s = _shape(over, follow, D=128, Hkv=2, Smax=Smax)
    return decode_args(_pages(dict(over), s, pages), Sq=Sq, Smax=Smax, follow=follow, **how)


def prefill_varlen_args(over, *, Smax=4096, follow="D"):
    """A valid contiguous ``pfa_fa3_prefill_varlen_args``: B 5, H 8, Hkv 2, 640 packed rows of which a sequence has at most 300, D 128."""
    s = _shape(over, follow, D=128, H=8, Hkv=2, Smax=Smax)
    d, h, hkv = s["D"], s["H"], s["Hkv"]
    base = dict(q=0x1000, k_cache=0x1000000, v_cache=0x2000000, o=0x800000, cu_seqlens_q=0x9000, B=5, H=8, Hkv=2, total_q=640,
                max_seqlen_q=300, Smax=Smax, D=128, q_stride_s=h * d, q_stride_h=d, o_stride_s=h * d, o_stride_h=d,
                k_stride_b=s["Smax"] * hkv * d, k_stride_h=d, k_stride_s=hkv * d, v_stride_b=s["Smax"] * hkv * d, v_stride_h=d, v_stride_s=hkv * d,
                dtype_in=0, dtype_out=0, causal=1, softmax_scale=d ** -0.5)
    base.update(over)
    return _capi.make_prefill_varlen_args(**base)


def prefill_varlen_paged(over, *, Smax=4096, pages=None, follow="D"):
    """``prefill_varlen_args`` of the same logical shape over a pool of pages (``_pages``)."""
    s = _shape(over, follow, D=128, Hkv=2, Smax=Smax)
    return prefill_varlen_args(_pages(dict(over), s, pages), Smax=Smax, follow=follow)


# The blocks below have one default shape: they take the overrides as keywords, and a file imports them under the name it uses.

def fa3_args(**over):
    """A valid ``pfa_fa3_args``: B 1, H 2, Sq 64, Sk 64, D 64, bf16, [B, S, H, D] buffers."""
    base = dict(q=0x1000, k=0x2000, v=0x3000, o=0x4000, B=1, H=2, Sq=64, Sk=64, D=64,
                q_stride_b=8192, q_stride_h=64, q_stride_s=128, k_stride_b=8192, k_stride_h=64, k_stride_s=128,
                v_stride_b=8192, v_stride_h=64, v_stride_s=128, o_stride_b=8192, o_stride_h=64, o_stride_s=128,
                dtype_in=0, dtype_out=0, softmax_scale=0.125)
    base.update(over)
    return _capi.make_args(**base)


def kv_append_args(**over):
    """A valid ragged contiguous ``pfa_kv_append_args``: B 5, Hkv 2, 640 packed rows of which a sequence has at most 300, Smax 4096, D 128."""
    d = over.get("D", 128)
    base = dict(k_new=0x1000, v_new=0x3000, k_cache=0x1000000, v_cache=0x2000000, cu_seqlens_q=0x9000, cache_seqlens=0x5000,
                B=5, Hkv=2, total_new=640, max_seqlen_q=300, Smax=4096, D=d, dtype=0,
                kn_stride_s=2 * d, kn_stride_h=d, vn_stride_s=2 * d, vn_stride_h=d,
                k_stride_b=4096 * 2 * d, k_stride_h=d, k_stride_s=2 * d, v_stride_b=4096 * 2 * d, v_stride_h=d, v_stride_s=2 * d)
    base.update(over)
    return _capi.make_kv_append_args(**base)


def kv_append_uniform(**over):
    """The uniform call of the same cache: [B, Sq, Hkv, D] rows, Sq 300, no cu_seqlens_q."""
    d = over.get("D", 128)
    return kv_append_args(**{**dict(cu_seqlens_q=0, total_new=1500, kn_stride_b=300 * 2 * d, vn_stride_b=300 * 2 * d), **over})


def kv_append_paged(**over):
    """The ragged call over a pool of pages (``_pages``), 32 pages a sequence."""
    return kv_append_args(**_pages(over, dict(D=over.get("D", 128), Hkv=2), 32))


def rope_append_args(**over):
    """A valid ragged contiguous ``pfa_rope_append_args`` with Q: B 5, H 4, Hkv 2, 640 packed rows of which a sequence has at most 300,
    Smax 4096, D 128, rot_dim 64, tables of 4096 positions."""
    d = over.get("D", 128)
    base = dict(q=0x100000, q_out=0x200000, k_new=0x1000, v_new=0x3000, k_cache=0x1000000, v_cache=0x2000000, cos=0x400000, sin=0x500000,
                cu_seqlens_q=0x9000, cache_seqlens=0x5000, pos_offsets=0x6000,
                B=5, H=4, Hkv=2, total_new=640, max_seqlen_q=300, Smax=4096, D=d, rot_dim=min(64, d), max_pos=4096, dtype=0, cs_stride=32,
                q_stride_s=4 * d, q_stride_h=d, qo_stride_s=4 * d, qo_stride_h=d,
                kn_stride_s=2 * d, kn_stride_h=d, vn_stride_s=2 * d, vn_stride_h=d,
                k_stride_b=4096 * 2 * d, k_stride_h=d, k_stride_s=2 * d, v_stride_b=4096 * 2 * d, v_stride_h=d, v_stride_s=2 * d)
    base.update(over)
    return _capi.make_rope_append_args(**base)


def rope_append_uniform(**over):
    """The uniform call of the same cache: [B, Sq, heads, D] rows, Sq 300, no cu_seqlens_q."""
    d = over.get("D", 128)
    return rope_append_args(**{**dict(cu_seqlens_q=0, total_new=1500, kn_stride_b=300 * 2 * d, vn_stride_b=300 * 2 * d,
                                      q_stride_b=300 * 4 * d, qo_stride_b=300 * 4 * d), **over})


def rope_append_paged(**over):
    """The ragged call over a pool of pages (``_pages``), 32 pages a sequence."""
    return rope_append_args(**_pages(over, dict(D=over.get("D", 128), Hkv=2), 32))


def attn_merge_args(**over):
    """A valid ``pfa_attn_merge_args``: ``_n`` (3) fp32 parts of B 3, Sq 5, H 4, D 128 in [B, Sq, H, D] buffers, [B, H, Sq] LSEs, fp32
    output and an output LSE."""
    n = over.pop("_n", 3)
    d = over.get("D", 128)
    base = dict(n_parts=n, B=3, H=4, Sq=5, D=d, dtype_part=2, dtype_out=2,
                o_part=[0x100000 * (k + 1) for k in range(n)], lse_part=[0x10000 * (k + 1) for k in range(n)], o=0x9000000, lse_out=0x8000,
                op_stride_b=[5 * 4 * d] * n, op_stride_h=[d] * n, op_stride_s=[4 * d] * n,
                lp_stride_b=[20] * n, lp_stride_h=[5] * n, lp_stride_s=[1] * n,
                o_stride_b=5 * 4 * d, o_stride_h=d, o_stride_s=4 * d, lo_stride_b=20, lo_stride_h=5, lo_stride_s=1)
    base.update(over)
    return _capi.make_attn_merge_args(**base)


def page_copy_args(**over):
    """A valid ``pfa_page_copy_args``: 8 pairs with row counts over token-major pools of 100 pages of 128 keys, Hkv 2, D 128."""
    ps, d, hkv = over.get("page_size", 128), over.get("D", 128), over.get("Hkv", 2)
    base = dict(k_pool=0x1000000, v_pool=0x2000000, pairs=0x9000, rows=0x5000, pairs_stride=2,
                k_stride_b=ps * hkv * d, k_stride_h=d, k_stride_s=hkv * d, v_stride_b=ps * hkv * d, v_stride_h=d, v_stride_s=hkv * d,
                n_pairs=8, Hkv=hkv, D=d, page_size=ps, num_pages=100, dtype=0)
    base.update(over)
    return _capi.make_page_copy_args(**base)


def varlen_args(**over):
    """A valid ``pfa_fa3_varlen_args``: B 3, H 4, Hkv 2, D 128, 1000 packed rows and 900 packed keys, bf16 in and out."""
    base = dict(q=0x100000, k=0x200000, v=0x300000, o=0x400000, lse=0x500000, cu_seqlens_q=0x600000, cu_seqlens_k=0x700000,
                q_stride_s=512, q_stride_h=128, k_stride_s=256, k_stride_h=128, v_stride_s=256, v_stride_h=128, o_stride_s=512, o_stride_h=128,
                B=3, H=4, Hkv=2, total_q=1000, total_k=900, max_seqlen_q=300, max_seqlen_k=257, D=128, dtype_in=0, dtype_out=0,
                causal=1, softmax_scale=128 ** -0.5)
    base.update(over)
    return _capi.make_varlen_args(**base)


def varlen_bwd_args(**over):
    """The ``pfa_fa3_varlen_bwd_args`` of the same problem, 16-bit gradients."""
    base = dict(q=0x100000, k=0x200000, v=0x300000, o=0x400000, dout=0x800000, lse=0x500000, dq=0x900000, dk=0xA00000, dv=0xB00000,
                delta=0xC00000, cu_seqlens_q=0x600000, cu_seqlens_k=0x700000,
                q_stride_s=512, q_stride_h=128, k_stride_s=256, k_stride_h=128, v_stride_s=256, v_stride_h=128, o_stride_s=512, o_stride_h=128,
                do_stride_s=512, do_stride_h=128, dq_stride_s=512, dq_stride_h=128, dk_stride_s=256, dk_stride_h=128, dv_stride_s=256,
                dv_stride_h=128, B=3, H=4, Hkv=2, total_q=1000, total_k=900, max_seqlen_q=300, max_seqlen_k=257, D=128, dtype=0,
                dtype_grad=0, causal=1, softmax_scale=128 ** -0.5)
    base.update(over)
    return _capi.make_varlen_bwd_args(**base)

"""CPU-side tests (no GPU) of the address widths the C ABI admits: one test per argument block of include/pfa_hip.h, through the
``*_check`` / ``*_describe`` exports with made-up pointers and the block builders of tests/capi_testlib.py.

Batch, head and page strides are 64-bit without limit: ``2^31 + 2^20`` elements (does not fit an int) and ``2^40`` must pass wherever a
block has such a stride -- the tensors', ``block_table_stride_b``, the key mask's, the tree words', the descales' and ``pairs_stride``.
Row strides are limited, because the kernels address the rows of one slab, tile or page with 32-bit offsets; the limits are the source's,
at their boundary values -- the largest admitted multiple of 8 (fp32: of 4) passes, the next one is refused with the status the source
gives:

  ``slab_fits32`` (csrc/pfa_host.h)                                    ``((S - 1) * stride + D) * bytes <= 0x7fffffff``, else PFA_ERR_SHAPE
  ``k_stride_s * 64 > 0x3fffffff`` (csrc/pfa_capi.hip, csrc/pfa_varlen_host.h)       PFA_ERR_STRIDE
  ``k_stride_s * 2 * 64 + 256 > 0x7fffffff`` (``check_cache_args``, csrc/pfa_host.h)   PFA_ERR_STRIDE

The persistent forward (``p4_eligible``, csrc/pfa_p4.hip) takes a block while every q / k / v stride times 2 and every o stride times
its element size fits 32 unsigned bits.  Without a device ``pfa_fa3_describe`` never names it, so what holds on both machines is asserted
here -- at the limit the name is that of the same block with ordinary strides, one unit more and the name carries no ``p4`` while the
status stays OK -- and tests/test_hip_far_dense.py asserts on the device that the limit itself runs the persistent kernel.

``pfa_fa3_bwd`` has no check export, and an accepted block would be launched on the made-up pointers wherever a GPU is present: its far
strides ride on a block that the LAST rule (the slab) refuses, which shows that every stride rule in front of it took them.

The GPU side of the same contract -- that the kernels compute the same bits at these strides -- is tests/test_hip_far_cache.py and
tests/test_hip_far_dense.py."""

from __future__ import annotations

import ctypes as C

import pytest

from capi_testlib import (OK, SHAPE, STRIDE, attn_merge_args, decode_args, decode_paged, ext, fa3_args, kv_append_args, kv_append_paged,
                          kv_append_uniform, lib, name_of, page_copy_args, prefill_varlen_args, prefill_varlen_paged, quant, ref,  # noqa: F401
                          rope_append_paged, rope_append_uniform, tree, varlen_args, varlen_bwd_args)
from photonic_flash_attention_amd import _capi

FAR = (2 ** 31 + 2 ** 20, 2 ** 40)
MAX31 = 0x7fffffff


def slab_limit(S, D, elem_bytes, unit):
    """The largest row stride (a multiple of ``unit``) ``slab_fits32`` admits for S rows of D elements"""
    return (MAX31 // elem_bytes - D) // (S - 1) // unit * unit


TILE_LIMIT_DENSE = 0x3fffffff // 64 // 8 * 8           # k_stride_s * 64 <= 0x3fffffff
TILE_LIMIT_CACHE = (MAX31 - 256) // 128 // 8 * 8       # k_stride_s * 2 * 64 + 256 <= 0x7fffffff


def _accepts(check, make, fields, *mid):
    """Every field alone, and all together, at both far strides"""
    for s in FAR:
        for f in fields:
            assert check(C.byref(make({f: s})), *mid) == OK, (f, s)
        assert check(C.byref(make({f: s for f in fields})), *mid) == OK, s


def test_fa3_args(lib):
    big = dict(Sq=256, Sk=256, D=128, **{f"{t}_stride_{x}": n for t in "qkvo" for x, n in (("s", 256), ("h", 128), ("b", 65536))})
    make = lambda over, base=big: fa3_args(**{**base, **over})
    _accepts(lib.pfa_fa3_check, make, [f"{t}_stride_{x}" for t in "qkvo" for x in "bh"])
    _accepts(lib.pfa_fa3_check, lambda over: make({"key_mask": 0x7000, **over}), ["key_mask_stride_b"])
    _accepts(lib.pfa_fa3_check, lambda over: make({"mask": 0x7000, "mask_stride_q": 256, "mask_stride_k": 1, **over}), ["mask_stride_b", "mask_stride_h"])
    # the persistent forward: every q / k / v stride x 2 and every o stride x its element size inside 32 unsigned bits
    plain = name_of(lib.pfa_fa3_describe, make({}))[1]
    for f in [f"{t}_stride_{x}" for t in "qkvo" for x in "bh"]:
        at, n = name_of(lib.pfa_fa3_describe, make({f: 2 ** 31 - 8}))[1], name_of(lib.pfa_fa3_describe, make({f: 2 ** 31}))[1]
        assert at == plain, (f, at, plain)                       # at the limit: the kernel of the ordinary strides
        assert "p4" not in n and lib.pfa_fa3_check(C.byref(make({f: 2 ** 31}))) == OK, (f, n)
    o32 = dict(dtype_out=2, flags=1)                             # the parity variant stores fp32: o's limit is 2^30 - 4 elements
    assert name_of(lib.pfa_fa3_describe, make({**o32, "o_stride_b": 2 ** 30 - 4}))[1] == name_of(lib.pfa_fa3_describe, make(o32))[1]
    assert "p4" not in name_of(lib.pfa_fa3_describe, make({**o32, "o_stride_b": 2 ** 30}))[1]
    # row strides: the slab of Sk = 256 keys (and of Sq rows), then 64 keys of a tile
    lim = slab_limit(256, 128, 2, 8)
    for f in ("k_stride_s", "v_stride_s", "q_stride_s"):
        assert lib.pfa_fa3_check(C.byref(make({f: lim}))) == OK and lib.pfa_fa3_check(C.byref(make({f: lim + 8}))) == SHAPE, f
    small = dict(big, Sq=64, Sk=64)                              # 64 keys: the slab admits more than a tile does
    assert slab_limit(64, 128, 2, 8) > TILE_LIMIT_DENSE
    for f in ("k_stride_s", "v_stride_s"):
        assert lib.pfa_fa3_check(C.byref(make({f: TILE_LIMIT_DENSE}, small))) == OK, f
        assert lib.pfa_fa3_check(C.byref(make({f: TILE_LIMIT_DENSE + 8}, small))) == STRIDE, f
    # the exact fp32 kernel: 4-byte elements, multiples of 4, all four tensors
    f32 = dict(big, dtype_in=2, dtype_out=2)
    lim = slab_limit(256, 128, 4, 4)
    for f in ("q_stride_s", "k_stride_s", "v_stride_s", "o_stride_s"):
        assert lib.pfa_fa3_check(C.byref(make({f: lim}, f32))) == OK and lib.pfa_fa3_check(C.byref(make({f: lim + 4}, f32))) == SHAPE, f
    _accepts(lib.pfa_fa3_check, lambda over: make(over, f32), [f"{t}_stride_{x}" for t in "qkvo" for x in "bh"])


def test_fa3_bwd_args(lib):
    tensors = ("q", "k", "v", "o", "do", "dq", "dk", "dv")
    base = dict(q=0x1000, k=0x2000, v=0x3000, o=0x4000, dout=0x5000, lse=0x6000, dq=0x7000, dk=0x8000, dv=0x9000, delta=0xa000,
                B=1, H=2, Sq=256, Sk=256, D=128, dtype=0, dtype_grad=0, softmax_scale=0.125)
    for t in tensors:
        base.update({f"{t}_stride_b": 65536, f"{t}_stride_h": 128, f"{t}_stride_s": 256})

    def refused(over):
        st = lib.pfa_fa3_bwd(C.byref(_capi._make(_capi.PfaFa3BwdArgs, {**base, **over})), None)
        assert st < 0                                            # (0 would mean the block went on to the device)
        return st

    lim = slab_limit(256, 128, 2, 8)
    far = lambda s: {f"{t}_stride_{x}": s for t in tensors for x in "bh"}
    for f in ("k_stride_s", "v_stride_s", "q_stride_s", "do_stride_s"):
        for s in FAR:                                            # the last rule refuses; every stride rule in front of it took the far strides
            assert refused({**far(s), f: lim + 8}) == SHAPE, (f, s)
    assert refused({**far(FAR[0]), "dq_stride_b": FAR[0] + 4}) == STRIDE                    # (the stride rules do look at them)
    f32 = dict(dtype=2, dtype_grad=2)
    lim = slab_limit(256, 128, 4, 4)
    for f in (f"{t}_stride_s" for t in tensors):
        assert refused({**f32, **far(FAR[1]), f: lim + 4}) == SHAPE, f


def _decode(over=None, **kw):
    return decode_args(dict(over or {}), Sq=4, **kw)


def _paged(over=None, **kw):
    return decode_paged(dict(over or {}), Sq=4, **kw)


def test_decode_args(lib):
    tensor_strides = [f"{t}_stride_{x}" for t in "qkvo" for x in "bh"]
    for check in (lib.pfa_fa3_decode_check, lib.pfa_fa3_prefill_check):
        _accepts(check, _decode, tensor_strides)
        _accepts(check, _paged, ["k_stride_b", "v_stride_b", "block_table_stride_b"])              # the PAGE strides, the table's rows
        for make in (_decode, _paged):
            for f in ("k_stride_s", "v_stride_s"):
                assert check(C.byref(make({f: TILE_LIMIT_CACHE}))) == OK and check(C.byref(make({f: TILE_LIMIT_CACHE + 8}))) == STRIDE, f
    _accepts(lib.pfa_fa3_decode_check, lambda over: _decode({"key_mask": 0x7000, **over}), ["key_mask_stride_b"])
    _accepts(lib.pfa_fa3_decode_check_ex, _paged, tensor_strides + ["block_table_stride_b"], ref(ext(window=100)))
    _accepts(lib.pfa_fa3_prefill_check_ex, _paged, tensor_strides + ["block_table_stride_b"], ref(ext(window=100)))
    _accepts(lib.pfa_fa3_prefill_split_check, lambda over: _paged({"Sq": 300, **over}), tensor_strides + ["block_table_stride_b"], 2)
    for s in FAR:
        assert lib.pfa_fa3_decode_tree_check(C.byref(_paged({f: s for f in tensor_strides})), None, C.byref(tree(stride_b=s))) == OK, s
        q8 = dict(k_cache=0x1000000, v_cache=0x2000000)
        assert lib.pfa_fa3_decode_q8_check(C.byref(_decode({**q8, **{f: s for f in tensor_strides}})), None, C.byref(quant(descale_stride_b=s))) == OK, s
        assert lib.pfa_fa3_prefill_q8_check(C.byref(_paged({**q8, "block_table_stride_b": s})), None, C.byref(quant(descale_stride_b=s))) == OK, s
    assert lib.pfa_fa3_decode_q8_check(C.byref(_decode({"k_stride_s": TILE_LIMIT_CACHE + 8})), None, C.byref(quant())) == STRIDE


def test_prefill_varlen_args(lib):
    fields = ["q_stride_h", "o_stride_h"] + [f"{t}_stride_{x}" for t in "kv" for x in "bh"]
    _accepts(lib.pfa_fa3_prefill_varlen_check, lambda over: prefill_varlen_args(dict(over)), fields)
    _accepts(lib.pfa_fa3_prefill_varlen_check, lambda over: prefill_varlen_paged(dict(over)), fields + ["block_table_stride_b"])
    _accepts(lib.pfa_fa3_prefill_varlen_check_ex, lambda over: prefill_varlen_paged(dict(over)), fields + ["block_table_stride_b"], ref(ext(window=100)))
    for make in (prefill_varlen_args, prefill_varlen_paged):
        for f in ("k_stride_s", "v_stride_s"):
            assert lib.pfa_fa3_prefill_varlen_check(C.byref(make({f: TILE_LIMIT_CACHE}))) == OK, f
            assert lib.pfa_fa3_prefill_varlen_check(C.byref(make({f: TILE_LIMIT_CACHE + 8}))) == STRIDE, f
    for s in FAR:
        a = prefill_varlen_paged({"block_table_stride_b": s, "k_stride_b": s, "v_stride_b": s})
        assert lib.pfa_fa3_prefill_varlen_q8_check(C.byref(a), None, C.byref(quant(descale_stride_b=s))) == OK, s


def test_kv_append_args(lib):
    cache = [f"{t}_stride_{x}" for t in "kv" for x in "bh"]
    _accepts(lib.pfa_kv_append_check, lambda over: kv_append_args(**over), cache + ["kn_stride_h", "vn_stride_h"])
    _accepts(lib.pfa_kv_append_check, lambda over: kv_append_uniform(**over), cache + [f"{t}_stride_{x}" for t in ("kn", "vn") for x in "bh"])
    _accepts(lib.pfa_kv_append_check, lambda over: kv_append_paged(**over), cache + ["block_table_stride_b"])
    for s in FAR:
        a = kv_append_paged(block_table_stride_b=s, k_stride_b=s, v_stride_b=s)
        assert lib.pfa_kv_append_q8_check(C.byref(a), C.byref(quant(descale_stride_b=s))) == OK, s


def test_rope_append_args(lib):
    cache = [f"{t}_stride_{x}" for t in "kv" for x in "bh"]
    rows = [f"{t}_stride_{x}" for t in ("q", "qo", "kn", "vn") for x in "bh"]
    _accepts(lib.pfa_rope_append_check, lambda over: rope_append_uniform(**over), cache + rows + ["cs_stride"])
    _accepts(lib.pfa_rope_append_check, lambda over: rope_append_paged(**over), cache + ["block_table_stride_b", "cs_stride", "q_stride_h", "qo_stride_h"])


def test_attn_merge_args(lib):
    for s in FAR:
        for f in ("op_stride_b", "op_stride_h", "lp_stride_b", "lp_stride_h", "lp_stride_s"):
            assert lib.pfa_attn_merge_check(C.byref(attn_merge_args(**{f: [s] * 3}))) == OK, (f, s)
        for f in ("o_stride_b", "o_stride_h", "lo_stride_b", "lo_stride_h", "lo_stride_s"):
            assert lib.pfa_attn_merge_check(C.byref(attn_merge_args(**{f: s}))) == OK, (f, s)
        every = {f: [s] * 3 for f in ("op_stride_b", "op_stride_h", "lp_stride_b", "lp_stride_h")}
        assert lib.pfa_attn_merge_check(C.byref(attn_merge_args(o_stride_b=s, o_stride_h=s, lo_stride_b=s, lo_stride_h=s, **every))) == OK, s


def test_page_copy_args(lib):
    _accepts(lib.pfa_page_copy_check, lambda over: page_copy_args(**over), ["k_stride_b", "v_stride_b", "k_stride_h", "v_stride_h", "pairs_stride"])
    assert lib.pfa_page_copy_check(C.byref(page_copy_args(num_pages=2 ** 18 + 64, k_stride_b=FAR[0], v_stride_b=FAR[1], pairs_stride=FAR[1]))) == OK


@pytest.mark.parametrize("make,check,heads", [
    (varlen_args, "pfa_fa3_varlen_check", [f"{t}_stride_h" for t in "qkvo"]),
    (varlen_bwd_args, "pfa_fa3_varlen_bwd_check", [f"{t}_stride_h" for t in ("q", "k", "v", "o", "do", "dq", "dk", "dv")])],
    ids=["varlen_args", "varlen_bwd_args"])
def test_varlen_args(lib, make, check, heads):
    """The packed blocks have no batch strides: head strides far, and the row-stride limits over one sequence's ``max_seqlen`` rows."""
    check = getattr(lib, check)
    _accepts(check, lambda over: make(**over), heads)
    lim_q, lim_k = slab_limit(300, 128, 2, 8), slab_limit(257, 128, 2, 8)
    slabs = [("q_stride_s", lim_q), ("k_stride_s", lim_k), ("v_stride_s", lim_k)] + ([("do_stride_s", lim_q)] if make is varlen_bwd_args else [])
    for f, lim in slabs:
        assert check(C.byref(make(**{f: lim}))) == OK and check(C.byref(make(**{f: lim + 8}))) == SHAPE, f
    short = dict(max_seqlen_q=64, max_seqlen_k=64)               # 64 rows: the slab admits more than a tile does
    for f in ("k_stride_s", "v_stride_s"):
        assert check(C.byref(make(**short, **{f: TILE_LIMIT_DENSE}))) == OK and check(C.byref(make(**short, **{f: TILE_LIMIT_DENSE + 8}))) == STRIDE, f
    # the packed rows of the far-address GPU tests: 2^22 + 8 elements between rows, at most 255 rows a sequence
    rows = {f.replace("_h", "_s"): 2 ** 22 + 8 for f in heads}
    assert check(C.byref(make(max_seqlen_q=255, max_seqlen_k=255, total_q=1064, total_k=1064, B=6, **rows))) == OK
    assert check(C.byref(make(max_seqlen_q=257, max_seqlen_k=257, total_q=1064, total_k=1064, B=6, **rows))) == SHAPE

"""Host-side (no GPU) tests of the decode at head dim 256 (include/pfa_hip_decode_d256.h): the check's codes in their order, the describe
names, the workspace against the plan of ``pfa_fa3_decode`` for the same shapes, the older call's refusal of D 256, and the ``ValueError``s
of the keywords ``ops.fa3_decode`` refuses at this head dim."""

from __future__ import annotations

import ctypes as C

import pytest
import torch

from capi_testlib import ALIGN, DTYPE, FLAGS, HEAD_DIM, NULL, OK, SHAPE, SIZE, STRIDE, decode_args, decode_paged, ext, name_of, ref
from capi_testlib import lib as base_lib  # noqa: F401  (the fixture)
from photonic_flash_attention_amd import _capi_decode_d256, ops


@pytest.fixture(scope="module")
def lib(base_lib):  # noqa: F811
    return _capi_decode_d256.load()


def _args(**over):
    return decode_args({"D": 256, **over}, Sq=4)


# in the order the errors are reported: each row breaks one rule and every rule in front of it holds
RULES = [({}, OK), ({"size": 8}, SIZE), ({"flags": 1}, FLAGS), ({"reserved0": 1}, FLAGS), ({"q": 0}, NULL), ({"Sq": 65}, SHAPE),
         ({"H": 7}, SHAPE), ({"D": 128}, HEAD_DIM), ({"D": 64}, HEAD_DIM), ({"D": 192}, HEAD_DIM), ({"D": 512}, HEAD_DIM),
         ({"dtype_in": 2}, DTYPE), ({"dtype_out": 1}, DTYPE), ({"softmax_scale": 0.0}, SHAPE), ({"k_stride_s": 516}, STRIDE),
         ({"o_stride_h": 258}, STRIDE), ({"v_cache": 0x2000008}, ALIGN), ({"cache_seqlens": 0x5002}, ALIGN), ({"k_stride_s": -512}, STRIDE),
         ({"page_size": 64}, FLAGS), ({"workspace": 0}, NULL), ({"workspace": 0x4000008}, ALIGN)]


@pytest.mark.parametrize("over,want", RULES, ids=[f"{next(iter(o), 'valid')}-{n}" for n, (o, _) in enumerate(RULES)])
def test_check_codes_in_order(lib, over, want):
    assert lib.pfa_fa3_decode_d256_check(C.byref(_args(**over)), None) == want


def test_null_block_paging_and_extension_rules(lib):
    assert lib.pfa_fa3_decode_d256_check(None, None) == NULL
    assert lib.pfa_fa3_decode_d256_check(C.byref(decode_paged({"D": 256}, Sq=4)), None) == OK
    for over, want in (({"_page": 96}, SHAPE), ({"block_table": 0x8002}, ALIGN), ({"num_pages": 0}, SHAPE)):
        assert lib.pfa_fa3_decode_d256_check(C.byref(decode_paged({"D": 256, **over}, Sq=4)), None) == want
    for e, over, want in ((ext(window=100), {}, OK), (ext(window=-1), {}, SHAPE), (ext(window=5, flags=1), {}, FLAGS),
                          (ext(window=5), {"causal": 0}, FLAGS), (ext(window=5, size=8), {}, SIZE)):
        assert lib.pfa_fa3_decode_d256_check(C.byref(_args(**over)), C.byref(e)) == want


@pytest.mark.parametrize("dtype_in,dtype_out,window,Smax,paged,want", [
    (0, 0, None, 4096, False, "fa3_decode_bf16_d256_o16+combine"), (1, 2, None, 4096, True, "fa3_decode_fp16_d256_o32+combine_paged"),
    (0, 0, 100, 4096, True, "fa3_decode_bf16_d256_o16_win_paged"), (1, 1, None, 128, False, "fa3_decode_fp16_d256_o16"),
    (0, 2, 1000, 4096, False, "fa3_decode_bf16_d256_o32_win+combine")])
def test_describe_names_and_workspace_follow_the_shared_plan(lib, dtype_in, dtype_out, window, Smax, paged, want):
    make = decode_paged if paged else decode_args
    a = make({"D": 256, "dtype_in": dtype_in, "dtype_out": dtype_out}, Sq=4, Smax=Smax)
    a128 = make({"dtype_in": dtype_in, "dtype_out": dtype_out}, Sq=4, Smax=Smax)
    e = None if window is None else ext(window=window)
    n, name, ns = name_of(lib.pfa_fa3_decode_d256_describe, a, ref(e), nsplit=True)
    n128, _, ns128 = name_of(lib.pfa_fa3_decode_describe_ex, a128, ref(e), nsplit=True)
    assert name == want and (n, ns) == (n128, ns128) and ns >= 1               # the plan does not depend on D
    assert ("+combine" in want) == (ns > 1)
    assert lib.pfa_fa3_decode_d256_workspace_bytes(C.byref(a), ref(e)) == (ns * a.B * a.H * a.Sq * (256 + 2) * 4 if ns > 1 else 0)
    assert lib.pfa_fa3_decode_d256_workspace_bytes(C.byref(a128), ref(e)) == 0  # no plan at another head dim


def test_the_older_entry_points_still_refuse_head_dim_256(lib):
    a = _args()
    assert lib.pfa_fa3_decode_check(C.byref(a)) == HEAD_DIM and lib.pfa_fa3_decode_check_ex(C.byref(a), None) == HEAD_DIM
    assert lib.pfa_fa3_prefill_check(C.byref(a)) == HEAD_DIM and lib.pfa_fa3_decode_workspace_bytes(C.byref(a)) == 0


@pytest.mark.parametrize("name,kw", [("tree_mask", dict(tree_mask=torch.zeros(2, 1, dtype=torch.int64))), ("sinks", dict(sinks=torch.zeros(8))),
                                     ("shared_prefix", dict(shared_prefix=64)), ("prefix_key_splits", dict(prefix_key_splits=2)),
                                     ("FP8", dict(k_descale=torch.ones(2), v_descale=torch.ones(2)))])
def test_refused_keywords_name_the_argument_and_the_head_dim(name, kw):
    q, k = torch.zeros(2, 8, 1, 256, dtype=torch.bfloat16), torch.zeros(2, 2, 128, 256, dtype=torch.bfloat16)
    if name == "FP8":
        k = k.to(torch.float8_e4m3fn)
    with pytest.raises(ValueError, match=f"{name}.*head dim 256"):
        ops.fa3_decode(q, k, k, cache_seqlens=torch.tensor([5, 6], dtype=torch.int32), **kw)

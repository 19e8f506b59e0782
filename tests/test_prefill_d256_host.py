"""Host-side (no GPU) tests of the forward over a KV cache at head dim 256 (include/pfa_hip_prefill_d256.h): the checks' codes in their
order for the uniform and the ragged entry point, the describe names with their workgroups (128 query rows each), and the ``ValueError``s
of the keywords ``ops.fa3_prefill_cache`` / ``ops.fa3_prefill_varlen`` refuse at this head dim."""

from __future__ import annotations

import ctypes as C

import pytest
import torch

from capi_testlib import ALIGN, DTYPE, FLAGS, HEAD_DIM, NULL, OK, SHAPE, SIZE, STRIDE, decode_args, decode_paged, ext, name_of
from capi_testlib import prefill_varlen_args, prefill_varlen_paged, ref
from capi_testlib import lib as base_lib  # noqa: F401  (the fixture)
from photonic_flash_attention_amd import _capi_prefill_d256, ops


@pytest.fixture(scope="module")
def lib(base_lib):  # noqa: F811
    return _capi_prefill_d256.load()


def _uniform(paged=False, **over):
    return (decode_paged if paged else decode_args)({"D": 256, **over}, Sq=300, ws=False)


def _ragged(paged=False, **over):
    return (prefill_varlen_paged if paged else prefill_varlen_args)({"D": 256, **over})


# in the order the errors are reported: each row breaks one rule and every rule in front of it holds
SHARED = [({}, OK), ({"size": 8}, SIZE), ({"flags": 1}, FLAGS), ({"reserved0": 1}, FLAGS), ({"q": 0}, NULL), ({"H": 7}, SHAPE),
          ({"D": 128}, HEAD_DIM), ({"D": 64}, HEAD_DIM), ({"D": 192}, HEAD_DIM), ({"dtype_in": 2}, DTYPE), ({"dtype_out": 1}, DTYPE),
          ({"softmax_scale": 0.0}, SHAPE), ({"k_stride_s": 516}, STRIDE), ({"o_stride_h": 258}, STRIDE), ({"v_cache": 0x2000008}, ALIGN),
          ({"cache_seqlens": 0x5002}, ALIGN), ({"k_stride_s": -512}, STRIDE), ({"page_size": 64}, FLAGS)]
RULES = [("pfa_fa3_prefill_d256_check", _uniform, over, want) for over, want in SHARED + [({"Sq": 0}, SHAPE), ({"key_mask": 0x6000}, FLAGS)]] \
    + [("pfa_fa3_prefill_varlen_d256_check", _ragged, over, want) for over, want in SHARED + [
        ({"cu_seqlens_q": 0}, NULL), ({"cu_seqlens_q": 0x9002}, ALIGN), ({"max_seqlen_q": 641}, SHAPE), ({"total_q": 0}, SHAPE)]]


@pytest.mark.parametrize("export,make,over,want", RULES, ids=[f"{e[11:-6]}-{next(iter(o), 'valid')}-{n}" for n, (e, _, o, _) in enumerate(RULES)])
def test_check_codes_in_order(lib, export, make, over, want):
    assert getattr(lib, export)(C.byref(make(**over)), None) == want


@pytest.mark.parametrize("export,make", [("pfa_fa3_prefill_d256_check", _uniform), ("pfa_fa3_prefill_varlen_d256_check", _ragged)])
def test_null_block_paging_and_extension_rules(lib, export, make):
    check = getattr(lib, export)
    assert check(None, None) == NULL and check(C.byref(make(paged=True)), None) == OK
    for over, want in (({"_page": 96}, SHAPE), ({"block_table": 0x8002}, ALIGN), ({"num_pages": 0}, SHAPE)):
        assert check(C.byref(make(paged=True, **over)), None) == want
    for e, over, want in ((ext(window=100), {}, OK), (ext(window=-1), {}, SHAPE), (ext(window=5, flags=1), {}, FLAGS),
                          (ext(window=5), {"causal": 0}, FLAGS), (ext(window=5, size=8), {}, SIZE)):
        assert check(C.byref(make(**over)), C.byref(e)) == want
    # the grid rule counts 128 rows a workgroup: B * H * ceil(rows / 128) must fit a grid
    rows = {"Sq": 1 << 30, "q_stride_b": 0, "o_stride_b": 0} if make is _uniform else {"max_seqlen_q": 1 << 30, "total_q": 1 << 30}
    assert check(C.byref(make(B=64, H=8, Hkv=8, **rows)), None) == SHAPE and check(C.byref(make(B=1, H=8, Hkv=8, **rows)), None) == OK


@pytest.mark.parametrize("ragged,dtype_in,dtype_out,causal,window,paged,want", [
    (False, 0, 0, 1, None, False, "fa3_prefill_bf16_d256_o16_causal"), (False, 1, 2, 0, None, True, "fa3_prefill_fp16_d256_o32_paged"),
    (False, 0, 2, 1, 100, True, "fa3_prefill_bf16_d256_o32_causal_win_paged"), (True, 1, 1, 1, None, False, "fa3_prefill_fp16_d256_o16_causal_varlen"),
    (True, 0, 0, 1, 64, True, "fa3_prefill_bf16_d256_o16_causal_win_varlen_paged"), (True, 0, 2, 0, None, False, "fa3_prefill_bf16_d256_o32_varlen")])
def test_describe_names_and_workgroups(lib, ragged, dtype_in, dtype_out, causal, window, paged, want):
    a = (_ragged if ragged else _uniform)(paged, dtype_in=dtype_in, dtype_out=dtype_out, causal=causal)
    e = None if window is None else ext(window=window)
    export = lib.pfa_fa3_prefill_varlen_d256_describe if ragged else lib.pfa_fa3_prefill_d256_describe
    n, name, _ = name_of(export, a, ref(e))
    assert (name, n) == (want, a.B * a.H * 3)           # 300 rows: three blocks of 128 (two of fa3_prefill_kernel's 256)
    helper = _capi_prefill_d256.describe_prefill_varlen_d256 if ragged else _capi_prefill_d256.describe_prefill_d256
    assert helper(a, e) == (want, n)


@pytest.mark.parametrize("name,kw", [("key_splits", dict(key_splits=2)), ("shared_prefix", dict(shared_prefix=64)),
                                     ("prefix_key_splits", dict(prefix_key_splits=2)), ("sinks", dict(sinks=torch.zeros(8))),
                                     ("FP8", dict(k_descale=torch.ones(2), v_descale=torch.ones(2)))])
def test_refused_keywords_name_the_argument_and_the_head_dim(name, kw):
    q, k = torch.zeros(2, 8, 200, 256, dtype=torch.bfloat16), torch.zeros(2, 2, 256, 256, dtype=torch.bfloat16)
    if name == "FP8":
        k = k.to(torch.float8_e4m3fn)
    sl = torch.tensor([200, 256], dtype=torch.int32)
    with pytest.raises(ValueError, match=f"{name}.*head dim 256"):
        ops.fa3_prefill_cache(q, k, k, cache_seqlens=sl, **kw)
    if name in ("sinks", "FP8"):        # the ragged call has no other of these keywords
        with pytest.raises(ValueError, match=f"{name}.*head dim 256"):
            ops.fa3_prefill_varlen(q.transpose(1, 2).reshape(400, 8, 256), k, k, cu_seqlens_q=torch.tensor([0, 200, 400], dtype=torch.int32),
                                   max_seqlen_q=200, cache_seqlens=sl, **kw)

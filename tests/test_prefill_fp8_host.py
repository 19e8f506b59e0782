"""CPU-side tests (no GPU) of the forward over an FP8 (e4m3fn) KV cache: the ``pfa_fa3_prefill_q8*`` / ``pfa_fa3_prefill_varlen_q8*`` entry
points (ABI v9 additive) -- every field rule of ``pfa_fa3_kv_quant`` in its documented order through both ``_check``
calls, the rules of one-byte caches, the window, everything else equal to the 16-bit call's status, names and workgroups equal to the
16-bit ``describe_ex`` -- then the refusals of ``ops.fa3_prefill_cache`` / ``ops.fa3_prefill_varlen`` and ``PagedKVCache.operands`` on
CPU tensors."""

from __future__ import annotations

import ctypes as C
import os

import pytest
import torch

from capi_testlib import (ALIGN, DTYPE, FLAGS, NULL, SHAPE, SIZE, STRIDE, decode_args, decode_paged, lib,  # noqa: F401
                          prefill_varlen_args, prefill_varlen_paged, quant, ref)
from conftest import REPO
from photonic_flash_attention_amd import _capi, ops

FP8 = torch.float8_e4m3fn
KD, VD = 0x7000, 0x7400


def _uargs(**over):
    """A valid contiguous block of the uniform call over one-byte caches: B 2, H 8, Hkv 2, Sq 300, Smax 1024, D 128."""
    return decode_args(over, Sq=300, Smax=1024, ws=False)


def _upaged(**over):
    return decode_paged(over, Sq=300, Smax=1024, ws=False)


def _vargs(**over):
    """A valid contiguous block of the ragged call: B 5, H 8, Hkv 2, 640 packed rows, at most 300 a sequence, Smax 1024, D 128."""
    return prefill_varlen_args(over, Smax=1024, follow="D H Hkv Smax")


def _vpaged(**over):
    return prefill_varlen_paged(over, Smax=1024, follow="D H Hkv Smax")


# (check, 16-bit check_ex, launch, q8 describe, 16-bit describe_ex, blocks)
def _calls(lib):
    return (
        (lib.pfa_fa3_prefill_q8_check, lib.pfa_fa3_prefill_check_ex, lib.pfa_fa3_prefill_q8, _capi.describe_prefill_q8,
         _capi.describe_prefill_ex, (_uargs, _upaged)),
        (lib.pfa_fa3_prefill_varlen_q8_check, lib.pfa_fa3_prefill_varlen_check_ex, lib.pfa_fa3_prefill_varlen_q8,
         _capi.describe_prefill_varlen_q8, _capi.describe_prefill_varlen_ex, (_vargs, _vpaged)),
    )


def test_the_abi_history_names_the_entry_points():
    header = open(os.path.join(REPO, "include", "pfa_hip.h")).read()
    assert "pfa_fa3_prefill_q8*" in header.split("Reference seam")[0]


def _quant_rules(chk, make):
    """The rules of pfa_fa3_kv_quant and of one-byte caches, each alone and in their documented order, for ``chk(a, quant)``."""
    ok = make()
    assert chk(ok, quant()) == 0
    assert chk(ok, quant(descale_stride_b=2)) == 0 and chk(ok, quant(descale_stride_b=64)) == 0
    assert chk(None, quant()) == NULL
    short = make()
    short.size -= 8
    assert chk(short, quant()) == SIZE
    assert chk(ok, None) == NULL
    wrong = quant()
    for size in (32, 48):
        wrong.size = size
        assert chk(ok, wrong) == SIZE
    assert chk(ok, quant(flags=1)) == FLAGS
    assert chk(ok, quant(reserved=1)) == FLAGS
    for dt in (0, 1, 2, 4, -1):
        assert chk(ok, quant(kv_dtype=dt)) == DTYPE
    assert chk(ok, quant(k_descale=0)) == NULL and chk(ok, quant(v_descale=0)) == NULL
    assert chk(ok, quant(k_descale=KD + 2)) == ALIGN and chk(ok, quant(v_descale=VD + 1)) == ALIGN
    assert chk(ok, quant(descale_stride_b=1)) == STRIDE and chk(ok, quant(descale_stride_b=-2)) == STRIDE
    # a one-byte stride that is no multiple of 16: a multiple of 8 passes the 16-bit rule, not this one
    for f in ("k_stride_b", "k_stride_h", "k_stride_s", "v_stride_b", "v_stride_h", "v_stride_s"):
        a = make()
        setattr(a, f, getattr(a, f) + 8)
        assert chk(a, quant()) == STRIDE, f
    assert chk(make(k_stride_s=-256), quant()) == STRIDE and chk(make(v_stride_s=-256), quant()) == STRIDE
    # a misaligned cache
    assert chk(make(k_cache=0x1000008), quant()) == ALIGN and chk(make(v_cache=0x2000004), quant()) == ALIGN
    # the order: each rule wins over all that follow it
    bad = make(k_stride_s=264, k_cache=0x1000008)
    every = dict(flags=1, kv_dtype=0, k_descale=0, v_descale=VD + 2, descale_stride_b=1)
    q = quant(**every)
    q.size = 8
    assert chk(bad, q) == SIZE
    assert chk(bad, quant(**every)) == FLAGS
    del every["flags"]
    assert chk(bad, quant(**every)) == DTYPE
    del every["kv_dtype"]
    assert chk(bad, quant(**every)) == NULL
    del every["k_descale"]
    assert chk(bad, quant(**every)) == ALIGN
    del every["v_descale"]
    assert chk(bad, quant(**every)) == STRIDE                                   # descale_stride_b
    assert chk(bad, quant()) == STRIDE                                          # the cache stride in front of the cache base
    short = make(k_stride_s=264)
    short.size -= 8
    assert chk(short, quant(flags=1)) == SIZE                                   # the block's own size comes first of all
    return ok


def test_field_rules_in_their_order_through_both_checks(lib):
    for check, check16, launch, describe, _, makes in _calls(lib):
        for make in makes:
            def chk(a, q, ext=None):
                return check(ref(a), ref(ext), ref(q))
            ok = _quant_rules(chk, make)
            # a window does not combine; window = 0 and a NULL extension are the plain call
            assert chk(ok, quant(), _capi.make_cache_ext(window=4)) == FLAGS
            assert chk(ok, quant(), _capi.make_cache_ext(window=0)) == 0
            assert chk(make(k_cache=0x1000008), quant(), _capi.make_cache_ext(window=4)) == ALIGN   # the cache base in front of the window
            assert chk(make(D=96), quant(), _capi.make_cache_ext(window=4)) == FLAGS                # ... which is in front of the old rules
            # then the 16-bit call's rules: the same status for every block the quant rules pass
            overs = [dict(q=0), dict(B=0), dict(D=96), dict(dtype_out=1), dict(dtype_in=2), dict(dtype_in=3), dict(o=0x800008), dict(flags=1),
                     dict(reserved0=1), dict(softmax_scale=0.0), dict(q_stride_s=4), dict(o_stride_s=6), dict(H=7), dict(causal=0),
                     dict(dtype_out=2), dict(D=64), dict(Smax=1000) if ok.block_table else dict(Smax=1000, k_stride_b=16, v_stride_b=16)]
            overs += [dict(cu_seqlens_q=0), dict(cu_seqlens_q=0x9002), dict(total_q=0), dict(max_seqlen_q=641)] if hasattr(ok, "total_q") else \
                [dict(key_mask=0x6000, key_mask_stride_b=1024), dict(Sq=65), dict(Sq=1), dict(Sq=0)]
            for over in overs:
                a = make(**over)
                assert chk(a, quant()) == check16(C.byref(a), None), over
            bad_ext = _capi.make_cache_ext(window=-1)
            assert chk(ok, quant(), bad_ext) == check16(C.byref(ok), C.byref(bad_ext)) == SHAPE
            assert chk(ok, quant(), _capi.make_cache_ext(flags=1)) == FLAGS
            # describe and the launch entry refuse the same way (nothing is launched: the status comes first)
            with pytest.raises(_capi.PfaError) as e:
                describe(ok, None, quant(kv_dtype=1))
            assert e.value.status == DTYPE
            assert launch(C.byref(ok), None, C.byref(quant(k_descale=0)), None) == NULL
            assert launch(C.byref(ok), None, None, None) == NULL
            assert launch(C.byref(ok), C.byref(_capi.make_cache_ext(window=4)), C.byref(quant()), None) == FLAGS


def test_a_key_mask_gives_the_16_bit_calls_error_and_any_row_count_is_accepted(lib):
    chk = lib.pfa_fa3_prefill_q8_check
    for make in (_uargs, _upaged):
        a = make(key_mask=0x6000, key_mask_stride_b=1024)
        assert chk(C.byref(a), None, C.byref(quant())) == lib.pfa_fa3_prefill_check_ex(C.byref(a), None) == FLAGS
        for sq in (1, 64, 65, 257, 5000):                                        # no 64-row limit: that is the decode's
            assert chk(C.byref(make(Sq=sq)), None, C.byref(quant())) == 0, sq


def test_describe_is_the_16_bit_describe_with_kv8_in_the_name(lib):
    for _, _, _, describe, describe16, makes in _calls(lib):
        for make in makes:
            for over in (dict(), dict(D=64, dtype_in=1, dtype_out=1), dict(dtype_out=2), dict(causal=0), dict(B=8, H=32, Hkv=8)):
                a = make(**over)
                name0, items0 = describe16(a, None)
                for q in (quant(), quant(descale_stride_b=a.Hkv), quant(k_descale=0x123450)):
                    for ext in (None, _capi.make_cache_ext()):
                        name, items = describe(a, ext, q)
                        assert items == items0 > 0
                        assert "_kv8" in name and "_kv8" not in name0 and name.replace("_kv8", "") == name0
    assert _capi.describe_prefill_q8(_uargs(), None, quant()) == ("fa3_prefill_bf16_d128_o16_causal_kv8", 2 * 8 * 2)
    assert _capi.describe_prefill_q8(_upaged(D=64, dtype_in=1, dtype_out=2, causal=0), None, quant())[0] == "fa3_prefill_fp16_d64_o32_kv8_paged"
    assert _capi.describe_prefill_varlen_q8(_vargs(), None, quant()) == ("fa3_prefill_bf16_d128_o16_causal_kv8_varlen", 5 * 8 * 2)
    assert _capi.describe_prefill_varlen_q8(_vpaged(dtype_out=2), None, quant())[0] == "fa3_prefill_bf16_d128_o32_causal_kv8_varlen_paged"
    # a short buffer is truncated and terminated, a NULL buffer only counts
    buf = C.create_string_buffer(b"x" * 16, 16)
    assert lib.pfa_fa3_prefill_q8_describe(C.byref(_uargs()), None, C.byref(quant()), buf, 12) == 32 and buf.value == b"fa3_prefill"
    assert lib.pfa_fa3_prefill_q8_describe(C.byref(_uargs()), None, C.byref(quant()), None, 0) == 32


# --- ops: refusals --------------------------------------------------------------------------------------------------------------------

def _operands(B=2, H=8, Hkv=2, Sq=70, Smax=512, D=128):
    q = torch.zeros(B, H, Sq, D, dtype=torch.bfloat16)
    k8 = torch.zeros(B, Hkv, Smax, D, dtype=FP8)
    return q, k8, k8.clone(), torch.ones(Hkv), torch.ones(Hkv)


def _refusals(call, extra):
    rot = dict(rotary_cos=torch.zeros(8, 64), rotary_sin=torch.zeros(8, 64))
    cases = [(dict(window=16), "window"), (rot, "rotary_cos / rotary_sin"), (dict(rotary_cos=rot["rotary_cos"]), "rotary_cos / rotary_sin"),
             (dict(pos_offsets=torch.zeros(2, dtype=torch.int32)), "rotary_cos / rotary_sin")] + extra
    for kw, name in cases:
        with pytest.raises(ValueError, match=f"{name} is not supported with an FP8"):
            call(**kw)
    for kw in (dict(k_descale=None), dict(v_descale=None), dict(k_descale=None, v_descale=None)):
        with pytest.raises(ValueError, match="caches need k_descale and v_descale"):
            call(**kw)
    for bad in (torch.ones(3), torch.ones(2, 3), torch.ones(2, dtype=torch.float64), torch.ones(2, 4)[:, ::2], [1.0, 1.0], torch.ones(1, 2)):
        with pytest.raises(ValueError, match="k_descale must be a contiguous fp32 tensor"):
            call(k_descale=bad)
    with pytest.raises(ValueError, match="must have one shape"):
        call(v_descale=torch.ones(2, 2))
    with pytest.raises(ValueError, match="v_descale must live on the operands' device"):
        call(v_descale=torch.ones(2, device="meta"))


def test_fa3_prefill_cache_refuses_what_an_fp8_cache_does_not_take():
    q, k8, v8, kd, vd = _operands()
    lens = torch.tensor([100, 100], dtype=torch.int32)

    def call(**kw):
        return ops.fa3_prefill_cache(q, k8, v8, **{"k_descale": kd, "v_descale": vd, **kw})

    _refusals(call, [(dict(shared_prefix=64, cache_seqlens=lens), "shared_prefix"), (dict(key_splits=2), "key_splits"),
                     (dict(key_splits="auto"), "key_splits"), (dict(prefix_key_splits=2), "prefix_key_splits")])
    kb = torch.zeros(2, 2, 512, 128, dtype=torch.bfloat16)
    for kw in (dict(k_descale=kd), dict(v_descale=vd), dict(k_descale=kd, v_descale=vd)):
        with pytest.raises(ValueError, match="go with torch.float8_e4m3fn caches only"):
            ops.fa3_prefill_cache(q, kb, kb.clone(), **kw)
    with pytest.raises(ValueError, match="must both be torch.float8_e4m3fn"):
        ops.fa3_prefill_cache(q, k8, kb, k_descale=kd, v_descale=vd)
    with pytest.raises(ValueError, match="q must be bf16 or fp16"):
        ops.fa3_prefill_cache(q.float(), k8, v8, k_descale=kd, v_descale=vd)
    # good arguments: the next refusal is the usual one (there is no CPU path)
    for kw in (dict(), dict(k_descale=torch.ones(2, 2), v_descale=torch.ones(2, 2)), dict(causal=False, out_dtype=torch.float32),
               dict(cache_seqlens=lens, return_lse=True)):
        with pytest.raises(ValueError, match="device tensors"):
            call(**kw)


def test_fa3_prefill_varlen_refuses_what_an_fp8_cache_does_not_take():
    _, k8, v8, kd, vd = _operands()
    q = torch.zeros(90, 8, 128, dtype=torch.bfloat16)
    cu = torch.tensor([0, 70, 90], dtype=torch.int32)

    def call(**kw):
        return ops.fa3_prefill_varlen(q, k8, v8, **{"cu_seqlens_q": cu, "max_seqlen_q": 70, "k_descale": kd, "v_descale": vd, **kw})

    _refusals(call, [])
    kb = torch.zeros(2, 2, 512, 128, dtype=torch.bfloat16)
    for kw in (dict(k_descale=kd), dict(v_descale=vd), dict(k_descale=kd, v_descale=vd)):
        with pytest.raises(ValueError, match="go with torch.float8_e4m3fn caches only"):
            ops.fa3_prefill_varlen(q, kb, kb.clone(), cu_seqlens_q=cu, max_seqlen_q=70, **kw)
    with pytest.raises(ValueError, match="q must be bf16 or fp16"):
        ops.fa3_prefill_varlen(q.float(), k8, v8, cu_seqlens_q=cu, max_seqlen_q=70, k_descale=kd, v_descale=vd)
    for kw in (dict(), dict(k_descale=torch.ones(2, 2), v_descale=torch.ones(2, 2)), dict(causal=False, out_dtype=torch.float32)):
        with pytest.raises(ValueError, match="device tensors"):
            call(**kw)


# --- PagedKVCache.operands on CPU tensors ---------------------------------------------------------------------------------------------

def _same_storage(a, b):
    return a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr()


def test_paged_cache_operands_are_views_of_the_cache():
    from photonic_flash_attention_amd.integration.pytorch import PagedKVCache
    kd, vd = torch.tensor([0.5, 0.031]), torch.tensor([1.0, 0.7])
    base = dict(num_pages=12, page_size=64, Hkv=2, D=64, device="cpu", max_batch=4, max_pages_per_seq=8)
    c8 = PagedKVCache(dtype=FP8, k_descale=kd, v_descale=vd, **base)
    c16 = PagedKVCache(dtype=torch.bfloat16, **base)
    for c, fp8 in ((c8, True), (c16, False)):
        for slots, rows in ((None, 4), (slice(1, 3), 2), ([1, 2], 2), (2, 1)):
            k, v, kw = c.operands(slots)
            assert k.shape == v.shape == (12, 2, 64, 64) and k.dtype == c.k_pool.dtype
            assert _same_storage(k, c.k_pool) and _same_storage(v, c.v_pool) and k.stride() == c.k_pool.transpose(1, 2).stride()
            assert _same_storage(kw["block_table"], c.block_table) and _same_storage(kw["cache_seqlens"], c.cache_seqlens)
            assert kw["block_table"].shape == (rows, 8) and kw["cache_seqlens"].shape == (rows,)
            if fp8:
                assert set(kw) == {"cache_seqlens", "block_table", "k_descale", "v_descale"}
                assert kw["k_descale"] is kd and kw["v_descale"] is vd
            else:
                assert set(kw) == {"cache_seqlens", "block_table"}
        # the views follow the cache: a later allocation shows through them
        _, _, kw = c.operands(None)
        s = c.allocate(70)
        c.advance([s], [70])
        assert int(kw["cache_seqlens"][s]) == 70 and kw["block_table"][s, :2].tolist() == list(c.pages(s))
        # a list that is no run of consecutive slots is a copy of its rows, as in decode
        _, _, kw2 = c.operands([2, 0])
        assert kw2["block_table"].shape == (2, 8) and not _same_storage(kw2["block_table"], c.block_table)
        with pytest.raises(ValueError, match="no slots"):
            c.operands([])
    # the methods keep refusing an FP8 cache; operands is the way in
    with pytest.raises(ValueError, match="prefill over an FP8 cache is not built"):
        c8.prefill(torch.zeros(4, 8, 4, 64, dtype=torch.bfloat16))
    k, v, kw = c8.operands(None)
    with pytest.raises(ValueError, match="device"):
        ops.fa3_prefill_cache(torch.zeros(4, 8, 70, 64, dtype=torch.bfloat16), k, v, **kw)

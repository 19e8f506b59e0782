"""CPU-side tests (no GPU) of the forward over a KV cache (``pfa_fa3_prefill*``, ABI v9 additive): argument
validation on the decode's argument block, the launch description, host-tensor refusal and ``PagedKVCache.prefill``'s plumbing."""

from __future__ import annotations

import ctypes as C

import pytest
import torch

from capi_testlib import decode_args, decode_paged, lib  # noqa: F401
from photonic_flash_attention_amd import _capi, ops


def _args(**over):
    """A valid contiguous call: B 2, H 8, Hkv 2, Sq 300, Smax 4096, D 128, [B, S, H, D] q and cache, no workspace.  The derived strides
    move with Sq and D only: an override of H, Hkv or Smax leaves those of the default shape in place."""
    return decode_args(over, Sq=300, ws=False, follow="D Sq", min_rows=1)


def _pargs(**over):
    """A valid paged call of the same logical shape: 32 pages of ``_page`` keys per sequence out of a pool of 100 pages laid out
    [num_pages, page_size, Hkv, D]."""
    return decode_paged(over, Sq=300, pages=32, ws=False, follow="D Sq", min_rows=1)


def test_the_decode_row_limit_is_unchanged(lib):
    a = _args(Sq=65)
    n = lib.pfa_fa3_decode_workspace_bytes(C.byref(a))
    a.workspace, a.workspace_bytes = 0x40000000, n
    assert lib.pfa_fa3_decode_check(C.byref(a)) == -3
    assert lib.pfa_fa3_prefill_check(C.byref(a)) == 0


@pytest.mark.parametrize("Sq", [1, 64, 65, 300, 4096])
def test_prefill_takes_any_number_of_rows(lib, Sq):
    assert lib.pfa_fa3_prefill_check(C.byref(_args(Sq=Sq))) == 0
    assert lib.pfa_fa3_prefill_check(C.byref(_pargs(Sq=Sq))) == 0


def test_prefill_argument_validation(lib):
    assert lib.pfa_fa3_prefill_check(C.byref(_args())) == 0
    assert lib.pfa_fa3_prefill_check(None) == -1
    bad = _args()
    bad.size = 16
    assert lib.pfa_fa3_prefill_check(C.byref(bad)) == -2
    short = _args()
    short.size = 232                       # an ABI v8 caller's struct
    assert lib.pfa_fa3_prefill_check(C.byref(short)) == -2
    # a key mask over the cache is out of scope for this entry point
    assert lib.pfa_fa3_prefill_check(C.byref(_args(key_mask=0x6000, key_mask_stride_b=4096))) == -10
    assert lib.pfa_fa3_prefill_check(C.byref(_pargs(key_mask=0x6000, key_mask_stride_b=4096))) == -10
    # the table of test_decode_argument_validation, without its Sq = 65 and workspace rows
    cases = [
        (dict(q=0), -1), (dict(k_cache=0), -1), (dict(o=0), -1),
        (dict(D=96), -4), (dict(Sq=0), -3), (dict(H=8, Hkv=3), -3), (dict(B=0), -3), (dict(Smax=0), -3),
        (dict(softmax_scale=0.0), -3), (dict(k_cache=0x1000008), -7), (dict(q=0x1004), -7), (dict(k_stride_s=2 * 128 + 1), -6),
        (dict(q_stride_h=129), -6), (dict(o_stride_s=6), -6), (dict(flags=1), -10), (dict(flags=0x100), -10),
        (dict(dtype_in=2, dtype_out=2), -5), (dict(dtype_out=1), -5), (dict(reserved0=1), -10),
    ]
    for over, want in cases:
        assert lib.pfa_fa3_prefill_check(C.byref(_args(**over))) == want, over
    for ok in (dict(D=64), dict(H=64, Hkv=1), dict(dtype_in=1, dtype_out=1), dict(dtype_out=2), dict(Smax=1), dict(causal=0),
               dict(cache_seqlens=0x5000), dict(lse=0x7000),
               dict(workspace=0, workspace_bytes=0), dict(workspace=0x1234, workspace_bytes=3)):      # the workspace is ignored
        assert lib.pfa_fa3_prefill_check(C.byref(_args(**ok))) == 0, ok
    # more workgroups than a grid holds
    assert lib.pfa_fa3_prefill_check(C.byref(_args(B=1 << 20, H=1 << 10, Hkv=1 << 10, Sq=1024))) == -3


def test_prefill_paged_argument_validation(lib):
    for ok in (dict(), dict(_page=64), dict(_page=1024), dict(_page=192), dict(block_table_stride_b=40), dict(num_pages=1),
               dict(Smax=128, block_table_stride_b=1), dict(D=64), dict(dtype_out=2)):
        assert lib.pfa_fa3_prefill_check(C.byref(_pargs(**ok))) == 0, ok
    SHAPE, ALIGN, FLAGS = -3, -7, -10
    cases = [
        (dict(page_size=96), SHAPE), (dict(page_size=32), SHAPE), (dict(page_size=0), SHAPE), (dict(num_pages=0), SHAPE),
        (dict(Smax=32 * 128 + 64), SHAPE),              # Smax != max_pages * page_size: not a whole number of pages
        (dict(Smax=33 * 128), SHAPE),                   # ... or more pages than a table row holds
        (dict(block_table_stride_b=31), SHAPE),
        (dict(block_table=0x8002), ALIGN),
        (dict(block_table=0), FLAGS), (dict(block_table=0, block_table_stride_b=0, num_pages=0), FLAGS),
    ]
    for over, want in cases:
        assert lib.pfa_fa3_prefill_check(C.byref(_pargs(**over))) == want, over


@pytest.mark.parametrize("B,H,Hkv,Sq", [(2, 8, 2, 1), (2, 8, 2, 256), (2, 8, 2, 257), (1, 32, 8, 512), (8, 32, 32, 2048), (3, 16, 1, 300)])
def test_prefill_describe_counts_workgroups_from_shapes(lib, B, H, Hkv, Sq):
    want = B * H * -(-Sq // 256)
    for make in (_args, _pargs):
        a = make(B=B, H=H, Hkv=Hkv, Sq=Sq, q_stride_b=Sq * H * 128, q_stride_s=H * 128, o_stride_b=Sq * H * 128, o_stride_s=H * 128,
                 k_stride_h=128, k_stride_s=Hkv * 128, v_stride_h=128, v_stride_s=Hkv * 128)
        name, wgs = _capi.describe_prefill(a)
        assert wgs == want
        assert name.startswith("fa3_prefill_bf16_d128_o16") and name.endswith("_paged") == (make is _pargs)
        # device-side inputs do not change the launch
        a.cache_seqlens = 0x5000
        assert _capi.describe_prefill(a) == (name, wgs)


def test_prefill_describe_names_dtype_head_dim_and_paging(lib):
    assert _capi.describe_prefill(_args(dtype_in=1, dtype_out=1, D=64))[0].startswith("fa3_prefill_fp16_d64_o16")
    assert _capi.describe_prefill(_args(dtype_out=2))[0].startswith("fa3_prefill_bf16_d128_o32")
    paged, plain = _capi.describe_prefill(_pargs())[0], _capi.describe_prefill(_args())[0]
    assert paged == plain + "_paged"
    with pytest.raises(_capi.PfaError):
        _capi.describe_prefill(_args(D=96))
    buf = C.create_string_buffer(8)                       # truncated, NUL terminated
    assert lib.pfa_fa3_prefill_describe(C.byref(_args()), buf, 8) == 2 * 8 * 2 and buf.value == b"fa3_pre"
    assert lib.pfa_fa3_prefill_describe(C.byref(_args()), None, 0) == 2 * 8 * 2


def test_fa3_prefill_cache_refuses_host_tensors_and_bad_shapes():
    q = torch.zeros(1, 8, 300, 128, dtype=torch.bfloat16)
    k = torch.zeros(1, 2, 512, 128, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="pfa_fa3_prefill needs device tensors"):
        ops.fa3_prefill_cache(q, k, k.clone())
    with pytest.raises(ValueError, match="shape mismatch"):
        ops.fa3_prefill_cache(q, k, k[:, :1].clone())
    with pytest.raises(ValueError, match="4-D"):
        ops.fa3_prefill_cache(q[0], k, k.clone())
    with pytest.raises(ValueError, match="dtype"):
        ops.fa3_prefill_cache(q.float(), k, k.clone())
    pool = torch.zeros(12, 2, 96, 128, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="multiple of 64"):
        ops.fa3_prefill_cache(q, pool, pool.clone(), block_table=torch.zeros(1, 4, dtype=torch.int32))
    with pytest.raises(TypeError):
        ops.fa3_prefill_cache(q, k, k.clone(), key_mask=torch.ones(1, 512, dtype=torch.bool))     # no key masks here
    # the decode keeps its own message
    with pytest.raises(ValueError, match="pfa_fa3_decode needs device tensors"):
        ops.fa3_decode(q[:, :, :1], k, k.clone())


def test_paged_cache_prefill_hands_its_own_table_and_lengths_to_ops(monkeypatch):
    from photonic_flash_attention_amd.integration.pytorch import PagedKVCache, paged_cache
    calls = []

    def spy(q, k, v, **kw):
        calls.append((q, k, v, kw))
        return "o", "lse"

    monkeypatch.setattr(paged_cache.ops, "fa3_prefill_cache", spy)
    c = PagedKVCache(num_pages=8, page_size=64, Hkv=2, D=64, dtype=torch.bfloat16, device="cpu", max_batch=3, max_pages_per_seq=4)
    for _ in range(3):
        c.allocate()
    q = torch.zeros(3, 8, 100, 64, dtype=torch.bfloat16)
    assert c.prefill(q, causal=False, return_lse=True) == ("o", "lse")
    q_, k_, v_, kw = calls.pop()
    assert q_ is q and k_.shape == (8, 2, 64, 64) and v_.shape == (8, 2, 64, 64)
    assert k_.data_ptr() == c.k_pool.data_ptr() and v_.data_ptr() == c.v_pool.data_ptr() and k_.stride() == c.k_pool.transpose(1, 2).stride()
    assert kw["block_table"] is c.block_table and kw["cache_seqlens"] is c.cache_seqlens
    assert kw["causal"] is False and kw["return_lse"] is True
    # a run of consecutive slots: views of the cache's own tensors (capturable); any other list: copies of its rows
    c.prefill(q[:2], slots=[1, 2])
    kw = calls.pop()[3]
    assert kw["block_table"].data_ptr() == c.block_table[1:].data_ptr() and kw["cache_seqlens"].data_ptr() == c.cache_seqlens[1:].data_ptr()
    assert kw["block_table"].shape == (2, 4)
    c.prefill(q[:2], slots=[2, 0])
    kw = calls.pop()[3]
    assert torch.equal(kw["block_table"], c.block_table[[2, 0]]) and torch.equal(kw["cache_seqlens"], c.cache_seqlens[[2, 0]])
    # and without the spy the CPU cache is refused by ops: there is no CPU path
    monkeypatch.undo()
    with pytest.raises(ValueError, match="device"):
        c.prefill(q)

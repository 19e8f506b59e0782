"""CPU-side tests (no GPU) of the forward over a KV cache with the keys split over workgroups (``pfa_fa3_prefill_split*``, ABI v9
additive): the plan and its invariance, the workspace size, validation on the decode's argument block, the launch
description, and the refusals of ``ops.fa3_prefill_cache(key_splits=)`` / ``prefix_key_splits=`` before any launch."""

from __future__ import annotations

import ctypes as C
import os

import pytest
import torch

from capi_testlib import ALIGN, FLAGS, NULL, SHAPE, STRIDE, decode_args, decode_paged, lib  # noqa: F401
from conftest import REPO
from photonic_flash_attention_amd import _capi, ops


def _args(**over):
    """A valid contiguous call: B 2, H 8, Hkv 2, Sq 300, Smax 4096, D 128, [B, S, H, D] q and cache, no workspace.  The derived strides
    move with Sq and D only: an override of H, Hkv or Smax leaves those of the default shape in place."""
    return decode_args(over, Sq=300, ws=False, follow="D Sq", min_rows=1)


def _pargs(**over):
    """A valid paged call of the same logical shape: 32 pages of ``_page`` keys per sequence out of a pool of 100 pages laid out
    [num_pages, page_size, Hkv, D]."""
    return decode_paged(over, Sq=300, pages=32, ws=False, follow="D Sq", min_rows=1)


def _with_ws(lib, a, n, ptr=0x40000000):
    a.workspace, a.workspace_bytes = ptr, lib.pfa_fa3_prefill_split_workspace_bytes(C.byref(a), n)
    return a


def test_the_split_limit_is_the_merge_limit():
    header = open(os.path.join(REPO, "include", "pfa_hip.h")).read()
    assert "#define PFA_PREFILL_MAX_SPLITS 8" in header and _capi.PFA_PREFILL_MAX_SPLITS == _capi.PFA_MERGE_MAX_PARTS == 8


def test_plan_returns_an_explicit_count_and_refuses_the_rest(lib):
    a = _args()
    for n in range(1, 9):
        assert lib.pfa_fa3_prefill_split_plan(C.byref(a), n) == n
    for bad in (-1, 9, 100, -(1 << 31)):
        assert lib.pfa_fa3_prefill_split_plan(C.byref(a), bad) == SHAPE
        assert lib.pfa_fa3_prefill_split_workspace_bytes(C.byref(a), bad) == 0
        assert lib.pfa_fa3_prefill_split_check(C.byref(a), bad) == SHAPE
    assert lib.pfa_fa3_prefill_split_plan(None, 2) == NULL
    short = _args()
    short.size = 232
    assert lib.pfa_fa3_prefill_split_plan(C.byref(short), 2) == -2
    assert lib.pfa_fa3_prefill_split_plan(C.byref(_args(D=96)), 2) == -4
    assert lib.pfa_fa3_prefill_split_plan(C.byref(_args(B=0)), 0) == SHAPE


SHAPES = [(B, H, Sq, Smax) for B in (1, 2, 16, 128) for H in (1, 8, 32) for Sq in (1, 255, 256, 257, 2048, 5000)
          for Smax in (1, 64, 128, 4096, 32768, 131072)]


def test_the_library_plan_keeps_its_three_properties(lib):
    seen = set()
    for B, H, Sq, Smax in SHAPES:
        n = lib.pfa_fa3_prefill_split_plan(C.byref(_args(B=B, H=H, Hkv=1, Sq=Sq, Smax=Smax)), 0)
        assert 1 <= n <= 8, (B, H, Sq, Smax, n)
        base = B * H * -(-Sq // 256)
        if base >= 512:                      # two workgroups on each of the 256 CUs already
            assert n == 1, (B, H, Sq, Smax)
        if Smax <= 64:                       # a second split could never hold a tile
            assert n == 1, (B, H, Sq, Smax)
        seen.add(n)
    assert len(seen) > 1                     # the plan does split somewhere
    # chunked prefill at B = 1 over a long cache is where it must
    assert lib.pfa_fa3_prefill_split_plan(C.byref(_args(B=1, H=32, Hkv=8, Sq=256, Smax=131072)), 0) > 1
    # monotone: more base workgroups never ask for more splits
    a = [lib.pfa_fa3_prefill_split_plan(C.byref(_args(B=b, H=32, Hkv=8, Sq=256, Smax=131072)), 0) for b in (1, 2, 4, 8, 16)]
    assert a == sorted(a, reverse=True) and a[-1] == 1


@pytest.mark.parametrize("ks", [0, 1, 2, 8])
def test_plan_and_workspace_ignore_pointers_lengths_table_and_page_size(lib, ks):
    shape = dict(B=1, H=32, Hkv=8, Sq=512, q_stride_b=512 * 32 * 128, q_stride_s=32 * 128, o_stride_b=512 * 32 * 128, o_stride_s=32 * 128,
                 k_stride_s=8 * 128, v_stride_s=8 * 128)
    ref = _args(Smax=8192, **shape)
    plan, ws = lib.pfa_fa3_prefill_split_plan(C.byref(ref), ks), lib.pfa_fa3_prefill_split_workspace_bytes(C.byref(ref), ks)
    others = [_args(Smax=8192, cache_seqlens=0x5000, **shape), _args(Smax=8192, q=0x777000, o=0, k_cache=0, lse=0x30, **shape),
              _pargs(_page=256, **shape), _pargs(_page=64, Smax=8192, block_table_stride_b=128, **shape),
              _pargs(_page=1024, Smax=8192, block_table=0x9000, num_pages=8, **shape)]
    for a in others:
        assert a.Smax == 8192
        assert lib.pfa_fa3_prefill_split_plan(C.byref(a), ks) == plan
        assert lib.pfa_fa3_prefill_split_workspace_bytes(C.byref(a), ks) == ws


@pytest.mark.parametrize("B,H,Hkv,Sq,D", [(2, 8, 2, 300, 128), (1, 32, 8, 1, 64), (3, 16, 1, 257, 128)])
def test_workspace_bytes_follow_the_formula(lib, B, H, Hkv, Sq, D):
    a = _args(B=B, H=H, Hkv=Hkv, Sq=Sq, D=D)
    assert lib.pfa_fa3_prefill_split_workspace_bytes(C.byref(a), 1) == 0
    for n in range(2, 9):
        assert lib.pfa_fa3_prefill_split_workspace_bytes(C.byref(a), n) == n * B * Sq * H * (D + 1) * 4
    n = lib.pfa_fa3_prefill_split_plan(C.byref(a), 0)
    assert lib.pfa_fa3_prefill_split_workspace_bytes(C.byref(a), 0) == (n * B * Sq * H * (D + 1) * 4 if n > 1 else 0)


def test_one_split_checks_exactly_as_pfa_fa3_prefill(lib):
    cases = [dict(), dict(q=0), dict(k_cache=0), dict(o=0), dict(D=96), dict(Sq=0), dict(H=8, Hkv=3), dict(B=0), dict(Smax=0),
             dict(softmax_scale=0.0), dict(k_cache=0x1000008), dict(q=0x1004), dict(k_stride_s=2 * 128 + 1), dict(q_stride_h=129),
             dict(o_stride_s=6), dict(o_stride_s=8 * 128 + 4), dict(flags=1), dict(dtype_in=2, dtype_out=2), dict(dtype_out=1), dict(reserved0=1),
             dict(key_mask=0x6000, key_mask_stride_b=4096), dict(D=64), dict(H=64, Hkv=1), dict(dtype_in=1, dtype_out=1), dict(dtype_out=2),
             dict(Smax=1), dict(causal=0), dict(cache_seqlens=0x5000), dict(lse=0x7000), dict(lse=0x7002),
             dict(workspace=0, workspace_bytes=0), dict(workspace=0x1234, workspace_bytes=3),          # the workspace is ignored
             dict(B=1 << 20, H=1 << 10, Hkv=1 << 10, Sq=1024)]
    for over in cases:
        want = lib.pfa_fa3_prefill_check(C.byref(_args(**over)))
        assert lib.pfa_fa3_prefill_split_check(C.byref(_args(**over)), 1) == want, over
    paged = [dict(), dict(_page=64), dict(page_size=96), dict(num_pages=0), dict(Smax=33 * 128), dict(block_table=0x8002),
             dict(block_table=0), dict(key_mask=0x6000, key_mask_stride_b=4096)]
    for over in paged:
        want = lib.pfa_fa3_prefill_check(C.byref(_pargs(**dict(over))))
        assert lib.pfa_fa3_prefill_split_check(C.byref(_pargs(**dict(over))), 1) == want, over
    assert lib.pfa_fa3_prefill_split_check(None, 1) == NULL
    # a shape the plan leaves unsplit is that call too
    full = _args(B=64, H=8, Hkv=2)
    assert lib.pfa_fa3_prefill_split_plan(C.byref(full), 0) == 1 and lib.pfa_fa3_prefill_split_check(C.byref(full), 0) == 0


@pytest.mark.parametrize("n", [2, 5, 8])
def test_split_validation(lib, n):
    for make in (_args, _pargs):
        assert lib.pfa_fa3_prefill_split_check(C.byref(_with_ws(lib, make(), n)), n) == 0
        assert lib.pfa_fa3_prefill_split_check(C.byref(_with_ws(lib, make(lse=0x7000, dtype_out=2, causal=0), n)), n) == 0
        # the workspace: missing, short, misaligned -- the decode's rules
        assert lib.pfa_fa3_prefill_split_check(C.byref(make()), n) == NULL
        a = _with_ws(lib, make(), n)
        a.workspace_bytes -= 1
        assert lib.pfa_fa3_prefill_split_check(C.byref(a), n) == NULL
        a = _with_ws(lib, make(), n)
        a.workspace = 0
        assert lib.pfa_fa3_prefill_split_check(C.byref(a), n) == NULL
        assert lib.pfa_fa3_prefill_split_check(C.byref(_with_ws(lib, make(), n, ptr=0x40000008)), n) == ALIGN
        # the prefill's own rules come first
        assert lib.pfa_fa3_prefill_split_check(C.byref(make(q=0)), n) == NULL
        assert lib.pfa_fa3_prefill_split_check(C.byref(make(D=96)), n) == -4
        assert lib.pfa_fa3_prefill_split_check(C.byref(make(o_stride_s=6)), n) == STRIDE
        # key masks stay with pfa_fa3_decode
        assert lib.pfa_fa3_prefill_split_check(C.byref(_with_ws(lib, make(key_mask=0x6000, key_mask_stride_b=4096), n)), n) == FLAGS
        # the merge writes a 16-bit o in rows of 8 elements; an fp32 o keeps the prefill's multiple of 4
        for st in (dict(o_stride_s=8 * 128 + 4), dict(o_stride_h=132), dict(o_stride_b=300 * 8 * 128 + 4)):
            assert lib.pfa_fa3_prefill_check(C.byref(make(**st))) == 0
            assert lib.pfa_fa3_prefill_split_check(C.byref(_with_ws(lib, make(**st), n)), n) == STRIDE, st
            assert lib.pfa_fa3_prefill_split_check(C.byref(_with_ws(lib, make(dtype_out=2, **st), n)), n) == 0, st


def test_the_planned_count_needs_its_workspace(lib):
    a = _args(B=1, H=32, Hkv=8, Sq=256, Smax=131072, q_stride_s=32 * 128, o_stride_s=32 * 128, k_stride_s=8 * 128, v_stride_s=8 * 128,
              k_stride_b=131072 * 8 * 128, v_stride_b=131072 * 8 * 128)
    n = lib.pfa_fa3_prefill_split_plan(C.byref(a), 0)
    assert n > 1
    assert lib.pfa_fa3_prefill_split_check(C.byref(a), 0) == NULL
    assert lib.pfa_fa3_prefill_split_check(C.byref(_with_ws(lib, a, 0)), 0) == 0
    assert a.workspace_bytes == n * 256 * 32 * 129 * 4


@pytest.mark.parametrize("B,H,Hkv,Sq", [(2, 8, 2, 1), (2, 8, 2, 257), (1, 32, 8, 512), (3, 16, 1, 300)])
def test_describe_names_the_split_and_counts_its_workgroups(lib, B, H, Hkv, Sq):
    over = dict(B=B, H=H, Hkv=Hkv, Sq=Sq, q_stride_b=Sq * H * 128, q_stride_s=H * 128, o_stride_b=Sq * H * 128, o_stride_s=H * 128,
                k_stride_h=128, k_stride_s=Hkv * 128, v_stride_h=128, v_stride_s=Hkv * 128)
    for make in (_args, _pargs):
        plain = _capi.describe_prefill(make(**over))
        assert _capi.describe_prefill_split(make(**over), 1) == plain + (1,)
        for n in (2, 3, 8):
            a = _with_ws(lib, make(**over), n)
            name, wgs, ns = _capi.describe_prefill_split(a, n)
            assert ns == n and wgs == B * H * -(-Sq // 256) * n
            tail = "_paged" if make is _pargs else ""
            assert name == plain[0][:len(plain[0]) - len(tail)] + f"_split{n}+merge" + tail
            a.cache_seqlens = 0x5000                          # device-side inputs do not change the launch
            assert _capi.describe_prefill_split(a, n) == (name, wgs, ns)
    # the planned count is reported too
    a = _with_ws(lib, _args(**over), 0)
    name, wgs, ns = _capi.describe_prefill_split(a, 0)
    assert ns == lib.pfa_fa3_prefill_split_plan(C.byref(a), 0) and wgs == B * H * -(-Sq // 256) * ns
    assert ("_split" in name) == (ns > 1)
    buf = C.create_string_buffer(8)                           # truncated, NUL terminated; NULL out-parameters
    assert lib.pfa_fa3_prefill_split_describe(C.byref(_with_ws(lib, _args(), 2)), 2, buf, 8, None) == 2 * 8 * 2 * 2 and buf.value == b"fa3_pre"


def test_the_grid_limit_counts_the_splits(lib):
    # 2^28 base workgroups: fine unsplit and 7-fold, past 2^31 - 1 with 8 splits
    big = dict(B=1 << 18, H=1 << 10, Hkv=1 << 10, Sq=1)
    assert lib.pfa_fa3_prefill_split_check(C.byref(_args(**big)), 1) == 0
    assert lib.pfa_fa3_prefill_split_check(C.byref(_args(**big)), 8) == SHAPE
    assert lib.pfa_fa3_prefill_split_describe(C.byref(_args(**big)), 8, None, 0, None) == SHAPE
    assert lib.pfa_fa3_prefill_split_check(C.byref(_args(B=1 << 20, H=1 << 10, Hkv=1 << 10, Sq=1024)), 2) == SHAPE


def test_key_splits_refusals_come_before_any_launch():
    q = torch.zeros(1, 8, 300, 128, dtype=torch.bfloat16)
    k = torch.zeros(1, 2, 2048, 128, dtype=torch.bfloat16)
    lens = torch.full((1,), 1500, dtype=torch.int32)
    for bad in (0, 9, -1, True, False, 2.0, "8", "AUTO", (2,), [4]):
        with pytest.raises(ValueError, match="key_splits must be"):
            ops.fa3_prefill_cache(q, k, k.clone(), key_splits=bad)
        with pytest.raises(ValueError, match="prefix_key_splits must be"):
            ops.fa3_prefill_cache(q, k, k.clone(), cache_seqlens=lens, shared_prefix=1024, prefix_key_splits=bad)
        with pytest.raises(ValueError, match="prefix_key_splits must be"):
            ops.fa3_decode(q[:, :, :1], k, k.clone(), cache_seqlens=lens, shared_prefix=1024, prefix_key_splits=bad)
    for ok in (1, 4, 8, "auto"):
        with pytest.raises(ValueError, match="key_splits does not combine with window"):
            ops.fa3_prefill_cache(q, k, k.clone(), key_splits=ok, window=128)
        with pytest.raises(ValueError, match="key_splits does not combine with shared_prefix"):
            ops.fa3_prefill_cache(q, k, k.clone(), cache_seqlens=lens, key_splits=ok, shared_prefix=1024)
        with pytest.raises(ValueError, match="prefix_key_splits needs shared_prefix"):
            ops.fa3_prefill_cache(q, k, k.clone(), prefix_key_splits=ok)
        with pytest.raises(ValueError, match="prefix_key_splits needs shared_prefix"):
            ops.fa3_decode(q[:, :, :1], k, k.clone(), prefix_key_splits=ok)
        # a legal value on host tensors reaches the usual refusal: there is no CPU path
        with pytest.raises(ValueError, match="pfa_fa3_prefill needs device tensors"):
            ops.fa3_prefill_cache(q, k, k.clone(), key_splits=ok)
        with pytest.raises(ValueError, match="needs device tensors"):
            ops.fa3_prefill_cache(q, k, k.clone(), cache_seqlens=lens, shared_prefix=1024, prefix_key_splits=ok)
        with pytest.raises(ValueError, match="needs device tensors"):
            ops.fa3_decode(q[:, :, :1], k, k.clone(), cache_seqlens=lens, shared_prefix=1024, prefix_key_splits=ok)
    # meta tensors: nothing can have been launched
    qm, km = q.to("meta"), k.to("meta")
    with pytest.raises(ValueError, match="key_splits must be"):
        ops.fa3_prefill_cache(qm, km, km, key_splits=16)
    with pytest.raises(ValueError, match="does not combine with window"):
        ops.fa3_prefill_cache(qm, km, km, key_splits=2, window=64)


def test_paged_cache_prefill_passes_key_splits_through(monkeypatch):
    from photonic_flash_attention_amd.integration.pytorch import PagedKVCache, paged_cache
    calls = []
    monkeypatch.setattr(paged_cache.ops, "fa3_prefill_cache", lambda q, k, v, **kw: calls.append(kw) or ("o", None))
    c = PagedKVCache(num_pages=8, page_size=64, Hkv=2, D=64, dtype=torch.bfloat16, device="cpu", max_batch=2, max_pages_per_seq=4)
    c.allocate()
    c.allocate()
    c.prefill(torch.zeros(2, 8, 100, 64, dtype=torch.bfloat16), key_splits="auto")
    assert calls.pop()["key_splits"] == "auto"
    c.prefill(torch.zeros(2, 8, 100, 64, dtype=torch.bfloat16), shared_prefix=64, prefix_key_splits=4)
    kw = calls.pop()
    assert kw["prefix_key_splits"] == 4 and kw["shared_prefix"] == 64

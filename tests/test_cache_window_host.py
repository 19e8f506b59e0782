"""CPU-side tests (no GPU) of sliding-window attention over the KV cache (``pfa_fa3_cache_ext`` and the ``*_ex`` entry points, ABI v9
additive): old and new entry points agreeing without a window, the new field rules,
the decode's split plan under a window, ``ops``' refusals and ``PagedKVCache.release_behind_window``."""

from __future__ import annotations

import ctypes as C

import pytest
import torch

from capi_testlib import FLAGS, HEAD_DIM, NULL, SHAPE, SIZE, decode_args, decode_paged, ext, lib, prefill_varlen_args, ref  # noqa: F401
from photonic_flash_attention_amd import _capi, ops

MIN_SPLIT_KEYS = 256                # kMinSplitKeys of pfa_decode_capi.hip


def _dargs(**over):
    """A valid contiguous block of the decode / prefill calls: B 2, H 8, Hkv 2, Sq 4, Smax 4096, D 128, with a workspace."""
    return decode_args(over, Sq=4)


def _paged(**over):
    return decode_paged(over, Sq=4)


def _vargs(**over):
    """A valid block of the ragged call: B 5, H 8, Hkv 2, 640 packed rows, Smax 4096, D 128."""
    return prefill_varlen_args(over)


def _entries(lib):
    """(name, old check, new check, block maker) of the three calls."""
    return [("decode", lib.pfa_fa3_decode_check, lib.pfa_fa3_decode_check_ex, _dargs),
            ("prefill", lib.pfa_fa3_prefill_check, lib.pfa_fa3_prefill_check_ex, lambda **kw: _dargs(**{"Sq": 300, **kw})),
            ("varlen", lib.pfa_fa3_prefill_varlen_check, lib.pfa_fa3_prefill_varlen_check_ex, _vargs)]


def test_old_and_new_entry_points_agree_without_a_window(lib):
    bad = [dict(), dict(q=0), dict(B=0), dict(D=96), dict(dtype_out=1), dict(k_stride_s=257), dict(o=0x800008), dict(flags=1),
           dict(reserved0=1), dict(page_size=64), dict(causal=0), dict(dtype_out=2), dict(D=64)]
    for name, old, new, make in _entries(lib):
        for over in bad:
            a = make(**over)
            want = old(C.byref(a))
            for e in (None, ext(), ext(window=0)):
                assert new(C.byref(a), ref(e)) == want, (name, over)
        assert old(None) == NULL and new(None, None) == NULL and new(None, C.byref(ext(window=4))) == NULL
        short = make()
        short.size = 16
        assert old(C.byref(short)) == SIZE and new(C.byref(short), C.byref(ext(window=4))) == SIZE
    # decode: key_mask, a missing workspace
    for over in (dict(key_mask=0x6000, key_mask_stride_b=4096), dict(workspace=0), dict(workspace_bytes=16), dict(Sq=65),
                 dict(B=8, H=32, Hkv=8, Sq=1, Smax=32768)):
        a = _dargs(**over)
        for e in (None, ext(window=0)):
            assert lib.pfa_fa3_decode_check_ex(C.byref(a), ref(e)) == lib.pfa_fa3_decode_check(C.byref(a)), over
    # describe / workspace
    for make in (_dargs, _paged):
        for over in (dict(), dict(B=1, H=32, Hkv=8, Sq=1, Smax=32768), dict(Sq=64, dtype_out=2), dict(D=64, dtype_in=1, dtype_out=1, causal=0)):
            a = make(**over)
            for e in (None, ext(window=0)):
                assert _capi.describe_decode_ex(a, e) == _capi.describe_decode(a)
                assert lib.pfa_fa3_decode_workspace_bytes_ex(C.byref(a), ref(e)) == lib.pfa_fa3_decode_workspace_bytes(C.byref(a))
            p = make(Sq=300, **{k: v for k, v in over.items() if k != "Sq"})
            for e in (None, ext(window=0)):
                assert _capi.describe_prefill_ex(p, e) == _capi.describe_prefill(p)
    for over in (dict(), dict(causal=0), dict(dtype_out=2), dict(D=64)):
        for e in (None, ext(window=0)):
            assert _capi.describe_prefill_varlen_ex(_vargs(**over), e) == _capi.describe_prefill_varlen(_vargs(**over))


def test_extension_field_rules(lib):
    for name, _, new, make in _entries(lib):
        ok = make()
        assert new(C.byref(ok), C.byref(ext(window=1))) == 0, name
        assert new(C.byref(ok), C.byref(ext(window=4096))) == 0
        assert new(C.byref(ok), C.byref(ext(window=2 ** 31 - 1))) == 0              # larger than the cache: hides nothing
        wrong = ext(window=4)
        wrong.size = 12
        assert new(C.byref(ok), C.byref(wrong)) == SIZE
        wrong.size = 24
        assert new(C.byref(ok), C.byref(wrong)) == SIZE
        assert new(C.byref(ok), C.byref(ext(window=4, flags=1))) == FLAGS
        assert new(C.byref(ok), C.byref(ext(flags=0x100))) == FLAGS
        assert new(C.byref(ok), C.byref(ext(window=4, reserved=1))) == FLAGS
        assert new(C.byref(ok), C.byref(ext(reserved=-1))) == FLAGS
        assert new(C.byref(ok), C.byref(ext(window=-1))) == SHAPE
        assert new(C.byref(ok), C.byref(ext(window=-(2 ** 31)))) == SHAPE
        full = make(causal=0)
        assert new(C.byref(full), C.byref(ext(window=4))) == FLAGS                  # a window needs the causal flag
        assert new(C.byref(full), C.byref(ext(window=0))) == 0
        # the block's own rules come first
        assert new(C.byref(make(D=96)), C.byref(ext(window=-1))) == HEAD_DIM
        assert new(C.byref(make(reserved0=1)), C.byref(ext(window=4))) == FLAGS
    # prefill still refuses a key mask, decode combines it with the window
    km = dict(key_mask=0x6000, key_mask_stride_b=4096)
    assert lib.pfa_fa3_prefill_check_ex(C.byref(_dargs(Sq=300, **km)), C.byref(ext(window=4))) == FLAGS
    assert lib.pfa_fa3_decode_check_ex(C.byref(_dargs(**km)), C.byref(ext(window=4))) == 0
    assert lib.pfa_fa3_decode_workspace_bytes_ex(C.byref(_dargs(causal=0)), C.byref(ext(window=4))) == 0       # refused: 0


def test_describe_marks_windowed_kernels(lib):
    w = ext(window=1024)
    assert _capi.describe_decode_ex(_dargs(Smax=256), w)[0] == "fa3_decode_bf16_d128_o16_win"
    assert _capi.describe_decode_ex(_dargs(), w)[0] == "fa3_decode_bf16_d128_o16_win+combine"
    assert _capi.describe_decode_ex(_paged(D=64, dtype_in=1, dtype_out=2), w)[0] == "fa3_decode_fp16_d64_o32_win+combine_paged"
    assert _capi.describe_prefill_ex(_dargs(Sq=300), w) == ("fa3_prefill_bf16_d128_o16_causal_win", 2 * 8 * 2)
    assert _capi.describe_prefill_ex(_paged(Sq=300, dtype_out=2), w) == ("fa3_prefill_bf16_d128_o32_causal_win_paged", 2 * 8 * 2)
    assert _capi.describe_prefill_varlen_ex(_vargs(), w) == ("fa3_prefill_bf16_d128_o16_causal_win_varlen", 5 * 8 * 2)
    assert _capi.describe_prefill_varlen_ex(_vargs(D=64), None)[0] == "fa3_prefill_bf16_d64_o16_causal_varlen"
    with pytest.raises(_capi.PfaError):
        _capi.describe_prefill_ex(_dargs(Sq=300, causal=0), w)
    # the grid of the prefill calls does not depend on the window
    for win in (1, 64, 5000):
        assert _capi.describe_prefill_ex(_dargs(Sq=300), ext(window=win))[1] == 32
        assert _capi.describe_prefill_varlen_ex(_vargs(), ext(window=win))[1] == 80


def test_decode_plan_under_a_window(lib):
    shape = dict(B=1, H=32, Hkv=8, Sq=1, Smax=32768, D=128)
    for make in (_dargs, _paged):
        a = make(**shape)
        _, items0, ns0 = _capi.describe_decode(a)
        ws0 = lib.pfa_fa3_decode_workspace_bytes(C.byref(a))
        assert ns0 > 1 and ws0 > 0
        w = ext(window=256)
        _, items, ns = _capi.describe_decode_ex(a, w)
        ws = lib.pfa_fa3_decode_workspace_bytes_ex(C.byref(a), C.byref(w))
        assert ns < ns0 and ws < ws0 and items < items0
        span = -(-(256 + 1 - 1) // 64) * 64
        assert span // ns >= MIN_SPLIT_KEYS                     # no split covers fewer than kMinSplitKeys keys of the span
        for win in (1, 63, 1000, 4096, 20000):
            _, _, n = _capi.describe_decode_ex(a, ext(window=win))
            sp = min(32768, -(-win // 64) * 64)
            assert n == 1 or sp // n >= MIN_SPLIT_KEYS, win
            assert n <= ns0
        for win in (32768, 32769, 2 ** 31 - 1):                 # a window the cache fits in: the plan without a window
            e = ext(window=win)
            assert _capi.describe_decode_ex(a, e)[1:] == (items0, ns0)
            assert lib.pfa_fa3_decode_workspace_bytes_ex(C.byref(a), C.byref(e)) == ws0
    # a 4096-key window over a 128K cache is not cut into 128 splits of a few tiles
    big = _dargs(B=1, H=32, Hkv=8, Sq=1, Smax=131072)
    assert _capi.describe_decode(big)[2] == 64
    assert _capi.describe_decode_ex(big, ext(window=4096))[2] == 16
    # paged and contiguous plans are equal, and device-side inputs do not enter
    for win in (256, 4096):
        c, p = _dargs(**shape), _paged(**shape)
        e = ext(window=win)
        assert _capi.describe_decode_ex(c, e)[1:] == _capi.describe_decode_ex(p, e)[1:]
        assert lib.pfa_fa3_decode_workspace_bytes_ex(C.byref(c), C.byref(e)) == lib.pfa_fa3_decode_workspace_bytes_ex(C.byref(p), C.byref(e))
        before = _capi.describe_decode_ex(p, e)
        p.cache_seqlens, p.block_table, p.lse = 0x5000, 0xB000, 0x7000
        assert _capi.describe_decode_ex(p, e) == before
    # Sq enters the span: 64 rows behind a 193-key window reach 256 keys back
    a = _dargs(B=1, H=8, Hkv=8, Sq=64, Smax=32768)
    assert _capi.describe_decode_ex(a, ext(window=193))[2] == 1
    assert _capi.describe_decode_ex(a, ext(window=512 - 63))[2] == 2


def test_ops_refuse_a_bad_window_before_any_launch():
    q = torch.zeros(2, 8, 4, 128, dtype=torch.bfloat16)
    k = torch.zeros(2, 2, 512, 128, dtype=torch.bfloat16)
    qp = torch.zeros(12, 8, 128, dtype=torch.bfloat16)
    cu = torch.tensor([0, 4, 12], dtype=torch.int32)
    calls = [lambda **kw: ops.fa3_decode(q, k, k.clone(), **kw),
             lambda **kw: ops.fa3_prefill_cache(q, k, k.clone(), **kw),
             lambda **kw: ops.fa3_prefill_varlen(qp, k, k.clone(), cu_seqlens_q=cu, max_seqlen_q=8, **kw)]
    for call in calls:
        for bad in (0, -3, 2.5, "4", True):
            with pytest.raises(ValueError, match="window must be None or an integer >= 1"):
                call(window=bad)
        with pytest.raises(ValueError, match="needs causal=True"):
            call(window=4, causal=False)
        with pytest.raises(ValueError, match="device tensors"):       # a good window: the next refusal is the usual one (no CPU path)
            call(window=4)
        with pytest.raises(ValueError, match="device tensors"):
            call(window=None)


def _cache(**kw):
    from photonic_flash_attention_amd.integration.pytorch import PagedKVCache
    base = dict(num_pages=12, page_size=64, Hkv=2, D=64, dtype=torch.bfloat16, device="cpu", max_batch=2, max_pages_per_seq=8)
    base.update(kw)
    return PagedKVCache(**base)


def _tok(n, val=1.0):
    return torch.full((1, 2, n, 64), val, dtype=torch.bfloat16)


@pytest.mark.parametrize("window", [1, 64, 65, 1000])
@pytest.mark.parametrize("length", [0, 63, 64, 65, 300])
def test_release_behind_window_counts_and_bookkeeping(length, window):
    c = _cache()
    s = c.allocate()
    if length:
        c.append(s, _tok(length), _tok(length))
    held = -(-length // 64)
    assert c.free_pages == 12 - held
    before = c.pages(s)
    want = max(0, length - window + 1) // 64                        # pages p with (p + 1) * 64 <= max(0, length - window + 1)
    assert c.release_behind_window(s, window) == want
    assert c.free_pages == 12 - held + want
    assert c.length(s) == length and int(c.cache_seqlens[s]) == length
    assert c.pages(s) == (-1,) * want + before[want:]
    assert c.block_table[s, :want].tolist() == [-1] * want
    assert c.block_table[s, want:held].tolist() == list(before[want:])
    assert c.release_behind_window(s, window) == 0                  # a second call releases nothing
    assert c.free_pages == 12 - held + want
    if want:
        with pytest.raises(ValueError, match="released"):
            c.gather(s)
        with pytest.raises(ValueError, match="released"):
            c.swap_pages(s, 0, held - 1)
        with pytest.raises(ValueError, match="released"):
            c.swap_pages(s, held - 1, want - 1)
    elif length:
        assert c.gather(s)[0].shape == (2, length, 64)
    # a later append continues at the right logical position and takes fresh pages
    c.append(s, _tok(70, 2.0), _tok(70, 3.0))
    assert c.length(s) == length + 70
    pages = c.pages(s)
    assert len(pages) == -(-(length + 70) // 64) and pages[:want] == (-1,) * want
    live = [p for p in pages if p >= 0]
    assert len(set(live)) == len(live) and c.free_pages == 12 - len(live)
    for j in (length, length + 69):                                 # first and last appended token, where the table says they are
        pg = int(c.block_table[s, j // 64])
        assert pg == pages[j // 64] >= 0
        assert float(c.k_pool[pg, j % 64, 0, 0]) == 2.0 and float(c.v_pool[pg, j % 64, 1, 5]) == 3.0
    # free returns only the live pages: the pool ends full, no page twice
    c.free(s)
    assert c.free_pages == 12 and sorted(c._free_pages) == list(range(12))


def test_release_behind_window_arguments_and_growth():
    c = _cache()
    s, t = c.allocate(), c.allocate()
    c.append([s, t], torch.ones(2, 2, 200, 64, dtype=torch.bfloat16), torch.ones(2, 2, 200, 64, dtype=torch.bfloat16))
    for bad in (0, -1, 2.5, None, True):
        with pytest.raises(ValueError, match="window must be an integer >= 1"):
            c.release_behind_window(s, bad)
    with pytest.raises(ValueError, match="not allocated"):
        _cache().release_behind_window(0, 4)
    assert c.release_behind_window(s, 100) == 1                     # the other slot is untouched
    assert -1 not in c.pages(t) and c.gather(t)[0].shape == (2, 200, 64)
    # as the sequence grows, more pages fall behind; a wider window releases nothing more
    c.append(s, _tok(100), _tok(100))
    assert c.release_behind_window(s, 1000) == 0
    assert c.release_behind_window(s, 100) == 2 and c.pages(s)[:3] == (-1, -1, -1)
    assert c.block_table[s, :3].tolist() == [-1, -1, -1]
    # reserve counts logical positions: 300 tokens hold 5 pages, 3 of them released
    c.reserve(s, 6 * 64)
    assert len(c.pages(s)) == 6 and c.pages(s)[:3] == (-1, -1, -1) and all(p >= 0 for p in c.pages(s)[3:])
    c.free(s)
    c.free(t)
    assert c.free_pages == 12 and sorted(c._free_pages) == list(range(12))


def test_paged_cache_passes_window_through(monkeypatch):
    from photonic_flash_attention_amd.integration.pytorch import paged_cache
    seen = []
    for name in ("fa3_decode", "fa3_prefill_cache", "fa3_prefill_varlen"):
        monkeypatch.setattr(paged_cache.ops, name, lambda q, k, v, _n=name, **kw: seen.append((_n, kw)) or ("o", None))
    c = _cache()
    c.allocate()
    c.allocate()
    c.decode(torch.zeros(2, 8, 1, 64, dtype=torch.bfloat16), window=128)
    c.prefill(torch.zeros(2, 8, 40, 64, dtype=torch.bfloat16), window=128)
    c.prefill_varlen(torch.zeros(41, 8, 64, dtype=torch.bfloat16), [40, 1], window=128)
    assert [n for n, _ in seen] == ["fa3_decode", "fa3_prefill_cache", "fa3_prefill_varlen"]
    assert all(kw["window"] == 128 and kw["block_table"] is c.block_table for _, kw in seen)

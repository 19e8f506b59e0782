"""CPU-side tests (no GPU) of the page copy inside a paged KV cache's pools (``pfa_page_copy*``, ABI v9 additive):
every validation rule and the order the rules are reported in, the launch description,
``ops.page_copy``'s refusals, and the plain-torch model of the rule (``ops.page_copy`` on CPU tensors: the executable specification the
GPU tests compare the kernel with) against a token-by-token loop written here.

Every pool holds a sentinel outside its random pages, so a stray write, a missing write and a wrong source all show.  Every comparison
is ``torch.equal``: a copy is bit-exact."""

from __future__ import annotations

import ctypes as C

import pytest
import torch

from capi_testlib import ALIGN, DTYPE, FLAGS, HEAD_DIM, NULL, SHAPE, SIZE, STRIDE, lib  # noqa: F401
from capi_testlib import page_copy_args as _args
from photonic_flash_attention_amd import _capi, ops

SENTINEL = -7.0


def _check(lib, a):
    return lib.pfa_page_copy_check(C.byref(a))


def test_page_copy_argument_validation(lib):
    assert _check(lib, _args()) == 0
    assert lib.pfa_page_copy_check(None) == NULL
    bad = _args()
    bad.size = 16
    assert _check(lib, bad) == SIZE
    other = _args()
    other.size = C.sizeof(_capi.PfaKvAppendArgs)
    assert _check(lib, other) == SIZE
    cases = [
        (dict(flags=1), FLAGS), (dict(flags=0x100), FLAGS), (dict(reserved0=1), FLAGS), (dict(reserved0=-1), FLAGS),
        (dict(k_pool=0), NULL), (dict(v_pool=0), NULL), (dict(pairs=0), NULL),
        (dict(n_pairs=0), SHAPE), (dict(n_pairs=-3), SHAPE), (dict(Hkv=0), SHAPE), (dict(num_pages=0), SHAPE), (dict(num_pages=-1), SHAPE),
        (dict(page_size=0), SHAPE), (dict(page_size=-64), SHAPE), (dict(page_size=32), SHAPE), (dict(page_size=96), SHAPE),
        (dict(D=0), HEAD_DIM), (dict(D=4), HEAD_DIM), (dict(D=100), HEAD_DIM), (dict(D=264), HEAD_DIM), (dict(D=512), HEAD_DIM),
        (dict(dtype=2), DTYPE), (dict(dtype=7), DTYPE), (dict(dtype=-1), DTYPE),
        (dict(k_stride_b=128 * 256 + 2), STRIDE), (dict(k_stride_h=129), STRIDE), (dict(k_stride_s=257), STRIDE),
        (dict(v_stride_b=7), STRIDE), (dict(v_stride_h=132), STRIDE), (dict(v_stride_s=-3), STRIDE),
        (dict(k_stride_s=-256), STRIDE), (dict(v_stride_s=-256), STRIDE),
        (dict(pairs_stride=1), STRIDE), (dict(pairs_stride=0), STRIDE), (dict(pairs_stride=-2), STRIDE),
        (dict(k_pool=0x1000008), ALIGN), (dict(v_pool=0x2000002), ALIGN), (dict(pairs=0x9002), ALIGN), (dict(rows=0x5001), ALIGN),
        # more workgroups than a grid holds; a page's 16-byte pieces past 32 bits
        (dict(n_pairs=1 << 24, page_size=1 << 12), SHAPE), (dict(n_pairs=1, Hkv=1 << 10, page_size=1 << 20, D=256), SHAPE),
    ]
    for over, want in cases:
        assert _check(lib, _args(**over)) == want, over
    # the launch refuses what the check refuses, before it touches a device
    assert lib.pfa_page_copy(C.byref(_args(D=100)), None) == HEAD_DIM and lib.pfa_page_copy(None, None) == NULL


def test_page_copy_rules_are_reported_in_the_documented_order(lib):
    """Each rule's violation next to one of every later rule: the earlier rule's status comes back."""
    ladder = [(dict(flags=1), FLAGS), (dict(pairs=0), NULL), (dict(page_size=96), SHAPE), (dict(D=100), HEAD_DIM), (dict(dtype=2), DTYPE),
              (dict(pairs_stride=1), STRIDE), (dict(rows=0x5002), ALIGN), (dict(n_pairs=1 << 30), SHAPE)]
    for i, (first, want) in enumerate(ladder):
        for later, _ in ladder[i + 1:]:
            over = dict(later)
            over.update(first)
            if set(first) & set(later):
                continue
            assert _check(lib, _args(**over)) == want, over
        everything = {}
        for later, _ in reversed(ladder[i:]):
            everything.update(later)
        assert _check(lib, _args(**everything)) == want, everything
        broken = _args(**everything)
        broken.size = 24                                     # and the size rule in front of them all
        assert _check(lib, broken) == SIZE


def test_page_copy_accepted_variants(lib):
    for ok in (dict(D=8), dict(D=64), dict(D=96), dict(D=256), dict(dtype=1), dict(Hkv=1), dict(Hkv=64), dict(n_pairs=1), dict(num_pages=1),
               dict(page_size=64), dict(page_size=192), dict(page_size=1024), dict(rows=0), dict(pairs_stride=3), dict(pairs_stride=64),
               dict(k_stride_h=128 * 128, k_stride_s=128, v_stride_h=128 * 128, v_stride_s=128),        # head-major pools
               dict(k_stride_b=3 * 128 * 256, v_stride_b=5 * 128 * 256)):                               # pages with gaps between them
        assert _check(lib, _args(**ok)) == 0, ok


@pytest.mark.parametrize("page_size", [64, 256, 1024])
@pytest.mark.parametrize("n_pairs,Hkv,D", [(1, 2, 128), (8, 8, 128), (512, 8, 128), (3, 1, 64), (2, 2, 96), (5, 3, 8)])
def test_page_copy_describe_counts_workgroups_from_host_shapes(lib, n_pairs, Hkv, D, page_size):
    want = n_pairs * -(-page_size * Hkv * (D // 8) // 1024)
    for rows in (0x5000, 0):
        a = _args(n_pairs=n_pairs, Hkv=Hkv, D=D, page_size=page_size, rows=rows)
        name, wgs = _capi.describe_page_copy(a)
        assert wgs == want
        # device-side inputs and the pool's size change neither the name nor the count
        a.pairs, a.k_pool, a.num_pages, a.pairs_stride = 0xA000, 0x3000000, 7, 4
        if rows:
            a.rows = 0xB000
        assert _capi.describe_page_copy(a) == (name, wgs)


def test_page_copy_describe_names(lib):
    assert _capi.describe_page_copy(_args())[0] == "page_copy_bf16_d128_rows"
    assert _capi.describe_page_copy(_args(rows=0))[0] == "page_copy_bf16_d128"
    assert _capi.describe_page_copy(_args(rows=0, dtype=1, D=96))[0] == "page_copy_fp16_d96"
    with pytest.raises(_capi.PfaError):
        _capi.describe_page_copy(_args(D=100))
    buf = C.create_string_buffer(8)                       # truncated, NUL terminated
    wgs = 8 * -(-128 * 2 * 16 // 1024)
    assert lib.pfa_page_copy_describe(C.byref(_args()), buf, 8) == wgs and buf.value == b"page_co"
    assert lib.pfa_page_copy_describe(C.byref(_args()), None, 0) == wgs


def test_page_copy_refusals():
    bf = torch.bfloat16
    pool = torch.zeros(6, 2, 64, 64, dtype=bf)
    pairs = torch.tensor([[0, 1], [2, 3]], dtype=torch.int32)
    rows = torch.tensor([5, 64], dtype=torch.int32)
    ops.page_copy(pool, pool.clone(), pairs)                                             # the CPU model takes it
    ops.page_copy(pool, pool.clone(), pairs, rows=rows)
    ops.page_copy(pool, pool.clone(), pairs[:0])                                         # no pairs: nothing to do
    ops.page_copy(pool, pool.clone(), pairs[:0], rows=rows[:0])
    with pytest.raises(TypeError):
        ops.page_copy(pool, pool.clone(), pairs, rows)                                   # rows is keyword-only
    with pytest.raises(ValueError, match="4-D"):
        ops.page_copy(pool[0], pool[0].clone(), pairs)
    with pytest.raises(ValueError, match="4-D"):
        ops.page_copy(pool, pool[:, :1].clone(), pairs)
    with pytest.raises(ValueError, match="4-D"):
        ops.page_copy(pool, pool.clone(), pairs.tolist())
    with pytest.raises(ValueError, match="dtype"):
        ops.page_copy(pool.float(), pool.float(), pairs)
    with pytest.raises(ValueError, match="dtype"):
        ops.page_copy(pool, pool.half(), pairs)
    with pytest.raises(ValueError, match="multiple of 64"):
        ops.page_copy(pool[:, :, :32], pool[:, :, :32].clone(), pairs)
    with pytest.raises(ValueError, match="multiple of 64"):
        ops.page_copy(torch.zeros(6, 2, 96, 64, dtype=bf), torch.zeros(6, 2, 96, 64, dtype=bf), pairs)
    with pytest.raises(ValueError, match="head dim"):
        ops.page_copy(pool[..., :4], pool[..., :4].clone(), pairs)
    with pytest.raises(ValueError, match="head dim"):
        ops.page_copy(torch.zeros(2, 1, 64, 264, dtype=bf), torch.zeros(2, 1, 64, 264, dtype=bf), pairs)
    with pytest.raises(ValueError, match=r"int32 \[n, 2\]"):
        ops.page_copy(pool, pool.clone(), pairs.long())
    with pytest.raises(ValueError, match=r"int32 \[n, 2\]"):
        ops.page_copy(pool, pool.clone(), pairs.reshape(-1))
    with pytest.raises(ValueError, match=r"int32 \[n, 2\]"):
        ops.page_copy(pool, pool.clone(), torch.zeros(2, 3, dtype=torch.int32))
    with pytest.raises(ValueError, match="adjacent"):
        ops.page_copy(pool, pool.clone(), torch.zeros(2, 4, dtype=torch.int32)[:, ::2])
    with pytest.raises(ValueError, match="adjacent"):
        ops.page_copy(pool, pool.clone(), torch.zeros(2, 2, dtype=torch.int32).t())
    with pytest.raises(ValueError, match=r"rows must be an int32 \[n\]"):
        ops.page_copy(pool, pool.clone(), pairs, rows=rows.long())
    with pytest.raises(ValueError, match=r"rows must be an int32 \[n\]"):
        ops.page_copy(pool, pool.clone(), pairs, rows=rows[:1])
    with pytest.raises(ValueError, match=r"rows must be an int32 \[n\]"):
        ops.page_copy(pool, pool.clone(), pairs, rows=rows.tolist())
    with pytest.raises(ValueError, match="rows must be contiguous"):
        ops.page_copy(pool, pool.clone(), pairs, rows=torch.zeros(4, dtype=torch.int32)[::2])
    with pytest.raises(ValueError, match="one device"):
        ops.page_copy(pool, pool.clone(), pairs.to("meta"))
    with pytest.raises(ValueError, match="one device"):
        ops.page_copy(pool, pool.clone(), pairs, rows=rows.to("meta"))
    with pytest.raises(ValueError, match="one device"):
        ops.page_copy(pool, pool.to("meta"), pairs)


# ---- the CPU model against a token-by-token loop --------------------------------------------------------------------------------

def _pools(num_pages, page_size, Hkv, D, random_pages, token_major, seed, dtype=torch.bfloat16):
    """K and V pools as ``[num_pages, Hkv, page_size, D]``-shaped views of head-major or token-major (flash-attn) memory: the pages
    in ``random_pages`` hold random numbers, every other page the sentinel."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(2):
        shape = (num_pages, page_size, Hkv, D) if token_major else (num_pages, Hkv, page_size, D)
        pool = torch.full(shape, SENTINEL, dtype=dtype)
        if token_major:
            pool = pool.transpose(1, 2)
        for pg in random_pages:
            pool[pg] = torch.randn(Hkv, page_size, D, generator=g).to(dtype)
        out.append(pool)
    return out


def _loop(k_pool, v_pool, pairs, rows):
    """The issue's rule one token at a time, pairs in order."""
    num_pages, page_size = k_pool.shape[0], k_pool.shape[2]
    for i, (s, d) in enumerate(pairs):
        if s < 0 or s > num_pages - 1 or d < 0 or d > num_pages - 1 or s == d:
            continue
        r = page_size if rows is None else min(max(rows[i], 0), page_size)
        for pool in (k_pool, v_pool):
            for t in range(r):
                for h in range(pool.shape[1]):
                    pool[d, h, t] = pool[s, h, t].clone()


def _both(kp, vp, pairs, rows=None, pairs_tensor=None):
    """Run the model and the loop on copies -> (model k, model v), after asserting they equal the loop's."""
    mk, mv, lk, lv = kp.clone(), vp.clone(), kp.clone(), vp.clone()
    pt = torch.tensor(pairs, dtype=torch.int32).reshape(-1, 2) if pairs_tensor is None else pairs_tensor
    ops.page_copy(mk, mv, pt, rows=None if rows is None else torch.tensor(rows, dtype=torch.int32))
    _loop(lk, lv, pairs, rows)
    assert torch.equal(mk, lk) and torch.equal(mv, lv)
    return mk, mv


@pytest.mark.parametrize("token_major", [False, True])
def test_model_whole_pages_in_both_layouts(token_major):
    kp, vp = _pools(9, 64, 2, 64, (0, 2, 5), token_major, 3)
    mk, mv = _both(kp, vp, [(0, 1), (2, 7), (5, 3)])
    for s, d in ((0, 1), (2, 7), (5, 3)):
        assert torch.equal(mk[d], kp[s]) and torch.equal(mv[d], vp[s])
    for same in (0, 2, 5, 4, 6, 8):                                              # sources and bystanders are what they were
        assert torch.equal(mk[same], kp[same]) and torch.equal(mv[same], vp[same])
    assert bool((mk[[4, 6, 8]] == SENTINEL).all()) and bool((mv[[4, 6, 8]] == SENTINEL).all())


@pytest.mark.parametrize("token_major", [False, True])
def test_model_row_counts_clamp_and_leave_the_tail_alone(token_major):
    kp, vp = _pools(13, 64, 2, 64, (0, 1, 2, 3, 4), token_major, 4)
    pairs, rows = [(0, 5), (1, 6), (2, 7), (3, 8), (4, 9)], [0, 1, 63, 64, 200]
    mk, mv = _both(kp, vp, pairs, rows)
    for (s, d), r in zip(pairs, [0, 1, 63, 64, 64]):
        for m, p in ((mk, kp), (mv, vp)):
            assert torch.equal(m[d, :, :r], p[s, :, :r]) and bool((m[d, :, r:] == SENTINEL).all())
    assert bool((mk[10:] == SENTINEL).all()) and torch.equal(mk[:5], kp[:5]) and torch.equal(mv[:5], vp[:5])
    # a negative count is an empty copy
    mk, _ = _both(kp, vp, [(0, 5)], [-4])
    assert torch.equal(mk, kp)


def test_model_empty_pairs_read_and_write_nothing():
    kp, vp = _pools(9, 64, 2, 64, (0, 1, 2), False, 5)
    # -1 on either side, ids at and past num_pages, far outside, s == d: all empty; the one live pair in the middle goes through
    pairs = [(-1, -1), (-1, 4), (0, -1), (9, 4), (0, 9), (1, 6), (1000, 4), (0, -(1 << 31)), (2, 2), ((1 << 31) - 1, 5)]
    mk, mv = _both(kp, vp, pairs)
    want_k, want_v = kp.clone(), vp.clone()
    want_k[6], want_v[6] = kp[1], vp[1]
    assert torch.equal(mk, want_k) and torch.equal(mv, want_v)
    mk, mv = _both(kp, vp, pairs, [64, 64, 64, 64, 64, 10, 64, 64, 64, 64])
    assert torch.equal(mk[6, :, :10], kp[1, :, :10]) and bool((mk[6, :, 10:] == SENTINEL).all()) and bool((mk[[3, 4, 5, 7, 8]] == SENTINEL).all())


def test_model_takes_a_strided_pair_view_and_larger_pages():
    kp, vp = _pools(11, 256, 2, 96, (0, 3), True, 6, dtype=torch.float16)
    wide = torch.full((3, 6), 7, dtype=torch.int32)                              # the pairs are columns 2:4 of a wider table
    wide[:, 2:4] = torch.tensor([[0, 5], [-1, 1], [3, 9]])
    view = wide[:, 2:4]
    assert not view.is_contiguous()
    mk, mv = _both(kp, vp, [(0, 5), (-1, 1), (3, 9)], [200, 256, 300], pairs_tensor=view)
    assert torch.equal(mk[5, :, :200], kp[0, :, :200]) and bool((mk[5, :, 200:] == SENTINEL).all()) and torch.equal(mv[9], vp[3])
    assert bool((mk[[1, 2, 4, 6, 7, 8, 10]] == SENTINEL).all())
    # every other row of a pair list
    every = torch.tensor([[0, 5], [0, 6], [3, 9], [3, 10]], dtype=torch.int32)[::2]
    mk, _ = _both(kp, vp, [(0, 5), (3, 9)], pairs_tensor=every)
    assert torch.equal(mk[5], kp[0]) and torch.equal(mk[9], kp[3]) and bool((mk[[6, 10]] == SENTINEL).all())


def test_model_processes_pairs_in_order():
    """Outside the caller's promise the model is still defined: pairs run in order, so a chain moves the first page down the chain."""
    kp, vp = _pools(4, 64, 1, 8, (0, 1), False, 7)
    mk, _ = _both(kp, vp, [(0, 2), (2, 3), (1, 2)])
    assert torch.equal(mk[3], kp[0]) and torch.equal(mk[2], kp[1])

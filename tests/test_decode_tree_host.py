"""CPU-side tests (no GPU) of tree attention masks in the decode (``pfa_fa3_tree_mask`` and the ``pfa_fa3_decode_tree*`` entry points,
ABI v9 additive): a NULL tree agreeing with ``pfa_fa3_decode_ex``, the field rules in their
stated order, the plan not depending on a tree, ``ops.fa3_decode``'s refusals, ``ops.tree_mask_from_parents`` against an ancestor walk,
``PagedKVCache.truncate`` and the accept flow of a speculative step."""

from __future__ import annotations

import ctypes as C
import os

import pytest
import torch

from capi_testlib import ALIGN, FLAGS, HEAD_DIM, NULL, SHAPE, SIZE, decode_args, decode_paged, ext, lib, ref, tree  # noqa: F401
from conftest import REPO
from photonic_flash_attention_amd import _capi, ops

WORDS = 0x7000


def _dargs(**over):
    """A valid contiguous block of the decode: B 2, H 8, Hkv 2, Sq 5, Smax 1024, D 128, with a workspace."""
    return decode_args(over, Sq=5, Smax=1024)


def _paged(**over):
    return decode_paged(over, Sq=5, Smax=1024)


def test_the_abi_history_entry_and_the_tree_block_default_size():
    header = open(os.path.join(REPO, "include", "pfa_hip.h")).read()
    assert "pfa_fa3_decode_tree*" in header.split("Reference seam")[0]          # the ABI history names it
    assert _capi.make_tree_mask().size == 24


def test_a_null_tree_is_the_ex_call(lib):
    bad = [dict(), dict(q=0), dict(B=0), dict(D=96), dict(dtype_out=1), dict(k_stride_s=257), dict(o=0x800008), dict(flags=1),
           dict(reserved0=1), dict(page_size=64), dict(causal=0), dict(dtype_out=2), dict(D=64), dict(Sq=65), dict(workspace=0),
           dict(workspace_bytes=16), dict(key_mask=0x6000, key_mask_stride_b=1024), dict(B=8, H=32, Hkv=8, Sq=1, Smax=32768)]
    exts = (None, ext(), ext(window=4), ext(window=300), ext(window=-1), ext(flags=1))
    for make in (_dargs, _paged):
        for over in bad:
            a = make(**over)
            for e in exts:
                assert lib.pfa_fa3_decode_tree_check(C.byref(a), ref(e), None) == lib.pfa_fa3_decode_check_ex(C.byref(a), ref(e)), over
                assert lib.pfa_fa3_decode_tree_workspace_bytes(C.byref(a), ref(e), None) == \
                    lib.pfa_fa3_decode_workspace_bytes_ex(C.byref(a), ref(e)), over
                if lib.pfa_fa3_decode_check_ex(C.byref(a), ref(e)) == 0:
                    assert _capi.describe_decode_tree(a, e, None) == _capi.describe_decode_ex(a, e), over
                else:
                    with pytest.raises(_capi.PfaError):
                        _capi.describe_decode_tree(a, e, None)
    assert lib.pfa_fa3_decode_tree_check(None, None, None) == NULL
    assert lib.pfa_fa3_decode_tree_check(None, None, C.byref(tree())) == NULL
    assert lib.pfa_fa3_decode_tree_workspace_bytes(None, None, C.byref(tree())) == 0
    assert _capi.describe_decode_tree(_dargs(), ext(window=300), None)[0] == "fa3_decode_bf16_d128_o16_win"
    assert _capi.describe_decode_tree(_dargs(), ext(window=800), None)[0] == "fa3_decode_bf16_d128_o16_win+combine"
    assert _capi.describe_decode_tree(_paged(Smax=128), None, None)[0] == "fa3_decode_bf16_d128_o16_paged"


def test_tree_field_rules_in_their_order(lib):
    chk = lib.pfa_fa3_decode_tree_check
    for make in (_dargs, _paged):
        ok = make()
        assert chk(C.byref(ok), None, C.byref(tree())) == 0
        assert chk(C.byref(ok), C.byref(ext()), C.byref(tree(stride_b=64))) == 0
        assert chk(C.byref(make(key_mask=0x6000, key_mask_stride_b=1024)), None, C.byref(tree())) == 0      # a key mask combines
        assert chk(C.byref(make(Sq=64)), None, C.byref(tree(stride_b=64))) == 0
        # each rule alone
        wrong = tree()
        wrong.size = 16
        assert chk(C.byref(ok), None, C.byref(wrong)) == SIZE
        wrong.size = 32
        assert chk(C.byref(ok), None, C.byref(wrong)) == SIZE
        assert chk(C.byref(ok), None, C.byref(tree(flags=1))) == FLAGS
        assert chk(C.byref(ok), None, C.byref(tree(words=0))) == NULL
        assert chk(C.byref(ok), None, C.byref(tree(words=WORDS + 4))) == ALIGN
        assert chk(C.byref(ok), None, C.byref(tree(stride_b=4))) == SHAPE
        assert chk(C.byref(ok), None, C.byref(tree(stride_b=-8))) == SHAPE
        assert chk(C.byref(make(causal=0)), None, C.byref(tree())) == FLAGS
        assert chk(C.byref(ok), C.byref(ext(window=4)), C.byref(tree())) == FLAGS
        assert chk(C.byref(ok), C.byref(ext(window=0)), C.byref(tree())) == 0
        # the order: each rule wins over all that follow it
        every = dict(flags=1, words=0, stride_b=4)                              # + causal = 0 and a window, below
        full, win = make(causal=0), ext(window=4)
        t = tree(**every)
        t.size = 8
        assert chk(C.byref(ok), None, C.byref(t)) == SIZE
        assert chk(C.byref(ok), None, C.byref(tree(**every))) == FLAGS
        assert chk(C.byref(ok), None, C.byref(tree(words=0, stride_b=4))) == NULL
        assert chk(C.byref(ok), None, C.byref(tree(words=WORDS + 1, stride_b=4))) == ALIGN
        assert chk(C.byref(full), None, C.byref(tree(words=0))) == NULL           # NULL (3) in front of causal == 0 (6)
        assert chk(C.byref(full), None, C.byref(tree(words=WORDS + 2))) == ALIGN
        assert chk(C.byref(full), None, C.byref(tree(stride_b=4))) == SHAPE       # stride (5) in front of causal == 0 (6)
        assert chk(C.byref(ok), C.byref(win), C.byref(tree(stride_b=4))) == SHAPE  # ... and in front of the window (7)
        assert chk(C.byref(ok), C.byref(win), C.byref(tree(words=0))) == NULL
        # the argument block's and the extension's rules come first
        assert chk(C.byref(make(D=96)), None, C.byref(wrong)) == HEAD_DIM
        assert chk(C.byref(make(Sq=65)), None, C.byref(tree(stride_b=4))) == SHAPE
        assert chk(C.byref(make(q=0)), None, C.byref(tree(flags=1))) == NULL
        assert chk(C.byref(ok), C.byref(ext(window=-1)), C.byref(tree(flags=1))) == SHAPE
        short = ext()
        short.size = 12
        assert chk(C.byref(ok), C.byref(short), C.byref(tree(flags=1))) == SIZE
        assert chk(C.byref(ok), C.byref(ext(reserved=1)), C.byref(wrong)) == FLAGS
        # ... and the workspace rules behind the tree's
        assert chk(C.byref(make(workspace=0)), None, C.byref(tree())) == NULL
        assert chk(C.byref(make(workspace=0)), None, C.byref(tree(words=WORDS + 4))) == ALIGN
        assert chk(C.byref(make(Smax=128, workspace=0)), None, C.byref(tree())) == 0
        # describe and the launch entry refuse the same way (nothing is launched: the status comes first)
        with pytest.raises(_capi.PfaError) as e:
            _capi.describe_decode_tree(ok, None, tree(flags=2))
        assert e.value.status == FLAGS
        assert lib.pfa_fa3_decode_tree(C.byref(ok), None, C.byref(tree(words=0)), None) == NULL
        assert lib.pfa_fa3_decode_tree(C.byref(full), None, C.byref(tree()), None) == FLAGS
        # the workspace query takes no pointers; what the other rules refuse is 0
        assert lib.pfa_fa3_decode_tree_workspace_bytes(C.byref(ok), None, C.byref(tree(words=0))) > 0
        assert lib.pfa_fa3_decode_tree_workspace_bytes(C.byref(ok), None, C.byref(tree(stride_b=4))) == 0
        assert lib.pfa_fa3_decode_tree_workspace_bytes(C.byref(full), None, C.byref(tree())) == 0
        assert lib.pfa_fa3_decode_tree_workspace_bytes(C.byref(ok), C.byref(win), C.byref(tree())) == 0


@pytest.mark.parametrize("smax, want_ns", [(128, 1), (1024, 4)])
def test_the_plan_does_not_depend_on_the_tree(lib, smax, want_ns):
    for make in (_dargs, _paged):
        for over in (dict(), dict(D=64, dtype_in=1, dtype_out=1), dict(dtype_out=2)):
            a = make(Smax=smax, **over)                                         # B 2, H 8, Hkv 2, Sq 5
            name0, items0, ns0 = _capi.describe_decode_ex(a, None)
            ws0 = lib.pfa_fa3_decode_workspace_bytes_ex(C.byref(a), None)
            assert ns0 == want_ns and (ws0 > 0) == (want_ns > 1)
            for t in (tree(), tree(stride_b=4096), tree(words=0x123458)):
                name, items, ns = _capi.describe_decode_tree(a, None, t)
                assert (items, ns) == (items0, ns0)
                assert lib.pfa_fa3_decode_tree_workspace_bytes(C.byref(a), None, C.byref(t)) == ws0
                assert lib.pfa_fa3_decode_tree_workspace_bytes(C.byref(a), C.byref(ext()), C.byref(t)) == ws0
            # device-side inputs do not enter
            before = _capi.describe_decode_tree(a, None, tree())
            a.cache_seqlens, a.lse = 0x5000, 0x7000
            assert _capi.describe_decode_tree(a, None, tree()) == before


def test_describe_marks_tree_kernels(lib):
    t = tree()
    assert _capi.describe_decode_tree(_dargs(Smax=128), None, t)[0] == "fa3_decode_bf16_d128_o16_tree"
    assert _capi.describe_decode_tree(_dargs(), None, t)[0] == "fa3_decode_bf16_d128_o16_tree+combine"
    assert _capi.describe_decode_tree(_dargs(), ext(window=0), t)[0] == "fa3_decode_bf16_d128_o16_tree+combine"
    assert _capi.describe_decode_tree(_paged(D=64, dtype_in=1, dtype_out=2), None, t)[0] == "fa3_decode_fp16_d64_o32_tree+combine_paged"
    assert _capi.describe_decode_tree(_paged(Smax=128), None, t)[0] == "fa3_decode_bf16_d128_o16_tree_paged"


def test_ops_refuse_a_bad_tree_mask_before_any_launch():
    q = torch.zeros(2, 8, 4, 128, dtype=torch.bfloat16)
    k = torch.zeros(2, 2, 512, 128, dtype=torch.bfloat16)
    good = torch.ones(2, 4, dtype=torch.int64)

    def call(**kw):
        return ops.fa3_decode(q, k, k.clone(), **kw)

    for bad in (good.to(torch.int32), good.to(torch.uint8), good.double(), good.bool(), [[1] * 4] * 2):
        with pytest.raises(ValueError, match="tree_mask must be an int64 tensor"):
            call(tree_mask=bad)
    for bad in (torch.ones(2, 5, dtype=torch.int64), torch.ones(4, 2, dtype=torch.int64), torch.ones(8, dtype=torch.int64),
                torch.ones(2, 4, 1, dtype=torch.int64)):
        with pytest.raises(ValueError, match=r"tree_mask must be \[B, Sq\]"):
            call(tree_mask=bad)
    with pytest.raises(ValueError, match="tree_mask must live on the operands' device"):
        call(tree_mask=torch.ones(2, 4, dtype=torch.int64, device="meta"))
    with pytest.raises(ValueError, match="tree_mask needs causal=True"):
        call(tree_mask=good, causal=False)
    with pytest.raises(ValueError, match="tree_mask does not combine with window"):
        call(tree_mask=good, window=16)
    with pytest.raises(ValueError, match="tree_mask does not combine with shared_prefix yet"):
        call(tree_mask=good, shared_prefix=64, cache_seqlens=torch.tensor([100, 100], dtype=torch.int32))
    with pytest.raises(ValueError, match="last dim must be contiguous"):
        call(tree_mask=torch.ones(2, 8, dtype=torch.int64)[:, ::2])
    with pytest.raises(ValueError, match="must not overlap"):
        call(tree_mask=torch.ones(1, 4, dtype=torch.int64).expand(2, 4))
    # a good mask: the next refusal is the usual one (there is no CPU path); without one nothing changes
    with pytest.raises(ValueError, match="device tensors"):
        call(tree_mask=good)
    with pytest.raises(ValueError, match="device tensors"):
        call(tree_mask=torch.ones(2, 64, dtype=torch.int64)[:, :4])              # a row stride above Sq is fine
    with pytest.raises(ValueError, match="device tensors"):
        call(tree_mask=None)


@pytest.mark.gpu
def test_ops_refuse_a_tree_mask_on_another_device_than_q():
    dev = torch.device("cuda:0")
    q = torch.zeros(2, 8, 4, 128, dtype=torch.bfloat16, device=dev)
    k = torch.zeros(2, 2, 512, 128, dtype=torch.bfloat16, device=dev)
    with pytest.raises(ValueError, match="tree_mask must live on the operands' device"):
        ops.fa3_decode(q, k, k.clone(), tree_mask=torch.ones(2, 4, dtype=torch.int64))


# --- tree_mask_from_parents ----------------------------------------------------------------------------------------------------------

def _walk(parents):
    """Words and depths by walking every node's ancestors: unsigned Python integers, folded to int64 by the caller."""
    words, depths = [], []
    for row in parents:
        w, d = [], []
        for i in range(len(row)):
            bits, n, a = 0, -1, i
            while a >= 0:
                bits |= 1 << a
                n += 1
                a = row[a]
            w.append(bits - (1 << 64) if bits >= 1 << 63 else bits)
            d.append(n)
        words.append(w)
        depths.append(d)
    return words, depths


def _random_parents(B, Sq, seed):
    g = torch.Generator().manual_seed(seed)
    return [[int(torch.randint(-1, i, (1,), generator=g)) for i in range(Sq)] for _ in range(B)]


@pytest.mark.parametrize("dtype", [torch.int64, torch.int32, torch.int16])
def test_tree_mask_from_parents_matches_an_ancestor_walk(dtype):
    chain = list(range(-1, 63))
    cases = {"random B 4 Sq 64": _random_parents(3, 64, 1) + [chain], "Sq 1": [[-1], [-1]], "chain": [chain[:7]],
             "star": [[-1] * 9], "random Sq 17": _random_parents(5, 17, 2)}
    for name, parents in cases.items():
        words, depths = ops.tree_mask_from_parents(torch.tensor(parents, dtype=dtype))
        assert words.dtype == torch.int64 and depths.dtype == torch.int32 and words.shape == depths.shape == (len(parents), len(parents[0]))
        want_w, want_d = _walk(parents)
        assert words.tolist() == want_w, name
        assert depths.tolist() == want_d, name
        pop = [[bin(w & (2 ** 64 - 1)).count("1") - 1 for w in row] for row in words.tolist()]
        assert pop == want_d, name                                               # depth = popcount - 1
    w, d = ops.tree_mask_from_parents(torch.tensor([chain]))
    assert int(w[0, 63]) == -1 and int(w[0, 62]) == 2 ** 63 - 1 and int(d[0, 63]) == 63        # bit 63 is the int64's sign bit
    w, d = ops.tree_mask_from_parents(torch.tensor([[-1] * 64]))
    assert int(w[0, 63]) == -2 ** 63 and int(w[0, 0]) == 1 and not bool(d.any())
    assert [int(x) for x in ops.tree_mask_from_parents(torch.tensor([[-1, 0, 1, 2]]))[0][0]] == [1, 3, 7, 15]


def test_tree_mask_from_parents_refusals():
    for bad in (torch.zeros(4, dtype=torch.int64), torch.zeros(2, 3, 4, dtype=torch.int64), torch.zeros(2, 4), [[-1, 0]],
                torch.zeros(2, 4, dtype=torch.bool)):
        with pytest.raises(ValueError, match=r"parents must be an integer \[B, Sq\] tensor"):
            ops.tree_mask_from_parents(bad)
    for sq in (65, 128, 0):
        with pytest.raises(ValueError, match="1 .. 64 nodes"):
            ops.tree_mask_from_parents(torch.full((2, sq), -1, dtype=torch.int64))
    for bad in ([[0, 0]], [[-1, 1]], [[-1, 0, 2]], [[-2, 0]], [[-1, -1, -1, 5]]):      # self, forward, out of range
        with pytest.raises(ValueError, match="-1 .. i - 1"):
            ops.tree_mask_from_parents(torch.tensor(bad))


# --- PagedKVCache.truncate and the accept flow ----------------------------------------------------------------------------------------

def _cache(**kw):
    from photonic_flash_attention_amd.integration.pytorch import PagedKVCache
    base = dict(num_pages=12, page_size=64, Hkv=2, D=64, dtype=torch.bfloat16, device="cpu", max_batch=3, max_pages_per_seq=8)
    base.update(kw)
    return PagedKVCache(**base)


def _tok(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(1, 2, n, 64, generator=g).to(torch.bfloat16), torch.randn(1, 2, n, 64, generator=g).to(torch.bfloat16)


@pytest.mark.parametrize("cow", [False, True])
@pytest.mark.parametrize("length, keep", [(200, 200), (200, 129), (200, 128), (200, 70), (200, 64), (200, 1), (200, 0), (64, 63), (0, 0)])
def test_truncate_bookkeeping(cow, length, keep):
    c = _cache(copy_on_write=cow)
    s, other = c.allocate(), c.allocate()
    ok, ov = _tok(100, 7)
    c.append(other, ok, ov)
    k, v = _tok(max(length, 1), 3)
    if length:
        c.append(s, k, v)
    c.reserve(s, length + 64)                                                    # one reserved page: truncate lets it go as well
    held = c.pages(s)
    assert len(held) == -(-(length + 64) // 64) and c.free_pages == 12 - 2 - len(held)
    row = c.block_table[s].clone()
    c.truncate(s, keep)
    want = -(-keep // 64)
    assert c.length(s) == keep and int(c.cache_seqlens[s]) == keep
    assert c.pages(s) == held[:want]
    assert c.free_pages == 12 - 2 - want
    assert all(c.page_refcount(p) == 1 for p in held[:want]) and all(c.page_refcount(p) == 0 for p in held[want:])
    assert torch.equal(c.block_table[s], row)                                    # stale entries stay, as after free
    gk, gv = c.gather(s)
    assert torch.equal(gk, k[0, :, :keep]) and torch.equal(gv, v[0, :, :keep])
    assert c.length(other) == 100 and torch.equal(c.gather(other)[0], ok[0])     # the neighbour is untouched
    # the pages that went back are handed out again, lowest id first, and an append continues at the new end
    nk, nv = _tok(130, 11)
    c.append(s, nk, nv)
    assert c.length(s) == keep + 130 and len(set(c.pages(s))) == len(c.pages(s)) == -(-(keep + 130) // 64)
    assert torch.equal(c.gather(s)[0], torch.cat([k[0, :, :keep], nk[0]], dim=1))
    c.free(s)
    c.free(other)
    assert c.free_pages == 12 and sorted(c._free_pages) == list(range(12))


def test_truncate_arguments():
    c = _cache()
    s = c.allocate()
    c.append(s, *_tok(100, 1))
    for bad in (-1, 101, 2.0, None, True, "3"):
        with pytest.raises(ValueError, match="n_tokens must be an integer in 0 .. 100"):
            c.truncate(s, bad)
    with pytest.raises(ValueError, match="not allocated"):
        c.truncate(1, 0)
    with pytest.raises(ValueError, match="not allocated"):
        c.truncate(7, 0)
    assert c.length(s) == 100 and len(c.pages(s)) == 2
    # behind a window: the page holding the new last key must still be there
    c.append(s, *_tok(100, 2))                                                   # 200 keys, 4 pages
    assert c.release_behind_window(s, 60) == 2                                   # pages 0 and 1 are gone
    for n in (1, 64, 128):
        with pytest.raises(ValueError, match="released behind the window"):
            c.truncate(s, n)
    assert c.length(s) == 200
    c.truncate(s, 129)
    assert c.pages(s)[:2] == (-1, -1) and len(c.pages(s)) == 3 and c.length(s) == 129
    c.truncate(s, 0)                                                             # nothing left to stand on a released page
    assert c.pages(s) == () and c.free_pages == 12


def test_truncate_with_shared_pages():
    c = _cache(copy_on_write=True)
    s = c.allocate()
    k, v = _tok(150, 5)
    c.append(s, k, v)
    child = c.fork(s)                                                            # shares pages 0, 1 and the partly filled tail page 2
    tail, mid = c.pages(s)[2], c.pages(s)[1]
    assert c.page_refcount(tail) == 2 and c.free_pages == 9
    # the parent lets go of the tail page: the child keeps it alive
    c.truncate(s, 100)
    assert c.pages(s) == c.pages(child)[:2] and c.page_refcount(tail) == 1 and c.page_refcount(mid) == 2 and c.free_pages == 9
    assert torch.equal(c.gather(child)[0], k[0]) and torch.equal(c.gather(child)[1], v[0])
    # page 1 is now the parent's partly filled tail (36 rows) and still shared: left shared, and the next append copies it
    nk, nv = _tok(10, 6)
    c.append(s, nk, nv)
    assert c.pages(s)[1] != mid and c.page_refcount(mid) == 1 and c.page_refcount(c.pages(s)[1]) == 1 and c.free_pages == 8
    assert torch.equal(c.gather(child)[0], k[0]) and torch.equal(c.gather(child)[1], v[0])           # the child reads what it read
    assert torch.equal(c.gather(s)[0], torch.cat([k[0, :, :100], nk[0]], dim=1))
    assert torch.equal(c.gather(s)[1], torch.cat([v[0, :, :100], nv[0]], dim=1))
    # the child truncates to a page boundary: nothing partly filled is left to copy
    c.truncate(child, 64)
    assert c.page_refcount(tail) == 0 and c.page_refcount(mid) == 0 and c.page_refcount(c.pages(child)[0]) == 2
    c.append(child, nk, nv)
    assert torch.equal(c.gather(child)[0], torch.cat([k[0, :, :64], nk[0]], dim=1))
    assert torch.equal(c.gather(s)[0][:, :64], k[0, :, :64])
    c.free(s)
    c.free(child)
    assert c.free_pages == 12 and sorted(c._free_pages) == list(range(12))


def test_truncate_resets_the_pending_copy_table():
    c = _cache(copy_on_write=True)
    s = c.allocate()
    c.append(s, *_tok(70, 1))
    child = c.fork(s)
    c.advance([child], [3])                                                      # a pending copy of the shared tail page
    assert c.cow_rows.tolist().count(-1) == 2 and c._pending
    c.truncate(s, 10)
    assert c.cow_rows.tolist() == [-1] * 3 and c.cow_pairs.tolist() == [[-1, -1]] * 3 and not c._pending


@pytest.mark.parametrize("cow", [False, True])
def test_the_accept_flow_equals_a_direct_append(cow):
    """A speculative step on the host: 70 cached tokens, a 5-node tree appended and verified, nodes [0, 2, 3] accepted."""
    c, direct = _cache(copy_on_write=cow), _cache(copy_on_write=cow)
    s, d = c.allocate(), direct.allocate()
    pk, pv = _tok(70, 1)
    tk, tv = _tok(5, 2)
    c.append(s, pk, pv)
    c.append(s, tk, tv)                                                          # the step's rows, as decode(tree_mask=) needs them
    assert c.length(s) == 75
    path = [0, 2, 3]
    c.truncate(s, 70)
    c.append_varlen([s], tk[0, :, path].transpose(0, 1).contiguous(), tv[0, :, path].transpose(0, 1).contiguous(), [3])
    direct.append(d, torch.cat([pk, tk[:, :, path]], dim=2), torch.cat([pv, tv[:, :, path]], dim=2))
    assert c.length(s) == direct.length(d) == 73 and int(c.cache_seqlens[s]) == 73
    assert torch.equal(c.gather(s)[0], direct.gather(d)[0]) and torch.equal(c.gather(s)[1], direct.gather(d)[1])
    assert c.pages(s) == direct.pages(d) and c.free_pages == direct.free_pages


def test_truncate_into_a_page_shared_with_a_fork_keeps_the_child():
    c = _cache(copy_on_write=True)
    s = c.allocate()
    k, v = _tok(140, 9)
    c.append(s, k, v)
    child = c.fork(s, 120)                                                       # pages 0 and 1 (partly: 56 rows)
    ck, cv = c.gather(child)
    c.truncate(s, 100)                                                           # into page 1, which the child shares
    assert c.page_refcount(c.pages(s)[1]) == 2
    nk, nv = _tok(30, 10)
    c.append(s, nk, nv)                                                          # would overwrite keys 100 .. 119 of the shared page
    assert torch.equal(c.gather(child)[0], ck) and torch.equal(c.gather(child)[1], cv)
    assert torch.equal(c.gather(s)[0], torch.cat([k[0, :, :100], nk[0]], dim=1))
    assert c.pages(s)[0] == c.pages(child)[0] and c.pages(s)[1] != c.pages(child)[1]


def test_paged_cache_passes_tree_mask_through(monkeypatch):
    from photonic_flash_attention_amd.integration.pytorch import paged_cache
    seen = []
    monkeypatch.setattr(paged_cache.ops, "fa3_decode", lambda q, k, v, **kw: seen.append(kw) or ("o", None))
    c = _cache()
    c.allocate()
    words = torch.ones(3, 4, dtype=torch.int64)
    c.decode(torch.zeros(3, 8, 4, 64, dtype=torch.bfloat16), tree_mask=words)
    assert seen[0]["tree_mask"] is words and seen[0]["block_table"] is c.block_table

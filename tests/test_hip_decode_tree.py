"""GPU tests of tree attention masks in the decode: ``ops.fa3_decode(tree_mask=)`` (``pfa_fa3_decode_tree`` with a ``pfa_fa3_tree_mask``),
``ops.tree_mask_from_parents`` and the accept step on a ``PagedKVCache`` (``truncate`` + ``append_varlen``).

The rule: with ``off_b = len_b - Sq``, row i of sequence b sees key j iff ``j < len_b`` and (``j < off_b`` or bit ``j - off_b`` of
``words[b, i]`` is set), and the key mask allows j.  The reference is ``reference`` of tests/kvcache_testlib.py with the rows folded into
the batch -- ``q [B * Sq, H, 1, D]``, the caches and lengths repeated Sq times, ``causal=False`` -- and that rule, written out below from
the words, as its key mask; the bounds are that module's ``check_out`` / ``check_lse``.  The kernels get caches with NaN at and past
every length (the reference reads clean copies) and, paged, NaN in every page no table entry names: outputs must be finite.

Two claims are pinned bit for bit: the chain (word i = bits 0 .. i) returns what ``causal=True`` without a tree returns, and a paged call
returns what the contiguous call returns.  Lengths 100 (D 128) and 68 (D 64) put new row 0 on the last key of a tile, which the causal
edge bound ``len - Sq + 1`` would leave unmasked: a build that keeps that bound fails the reference cases with zero and random words
(the chain itself sets bit 0 in every word, so it passes either way; it pins the masked tiles' arithmetic and a bound that is too low)."""

from __future__ import annotations

import functools

import pytest
import torch

from kvcache_testlib import (capture, check_lse, check_out, contiguous_of, device, folded_reference, guard, i32, reference, scatter,
                             tree_visible)  # noqa: F401  (tree_visible: kept importable from here)

pytestmark = pytest.mark.gpu

DT_D = [(torch.bfloat16, 128), (torch.float16, 64), (torch.bfloat16, 64), (torch.float16, 128)]
DT_IDS = ["bf16-d128", "fp16-d64", "bf16-d64", "fp16-d128"]
# off_b on a 32-key tile boundary (101); new row 0 the last key of its tile (100; D 64: 68); off_b on a 64-key boundary (69); the tree
# across the split boundary at 768 (770); no prefix (5); len < Sq (3); empty (0)
LENS1 = (101, 100, 69, 68, 770, 5, 3, 0)
SHAPE1 = dict(H=8, Hkv=2, Sq=5, Smax=1024, lens=LENS1)                      # 20 packed rows: a full and a partial row block; 4 splits
LENS4 = (64, 200, 127)
SHAPES4 = [dict(H=2, Hkv=2, Sq=64, Smax=256, lens=LENS4), dict(H=8, Hkv=2, Sq=64, Smax=256, lens=LENS4)]   # 4 and 16 row blocks


@functools.lru_cache(maxsize=None)
def _problem(H, Hkv, Sq, Smax, lens, D, dtype):
    """q, clean caches, their poisoned copies and the lengths; shared and never modified."""
    B = len(lens)
    g = torch.Generator(device=device()).manual_seed(1300 + 3 * D + Sq + H + (0 if dtype is torch.bfloat16 else 1))
    q = torch.randn(B, Sq, H, D, generator=g, device=device()).to(dtype).permute(0, 2, 1, 3)
    k = torch.randn(B, Hkv, Smax, D, generator=g, device=device()).to(dtype)
    v = torch.randn(B, Hkv, Smax, D, generator=g, device=device()).to(dtype)
    kn, vn = guard(k, v, lens)
    return dict(q=q, k=k, v=v, kn=kn, vn=vn, lens=i32(list(lens)), vmax=float(v.abs().max()), dtype=dtype, Sq=Sq, Smax=Smax, B=B)


@functools.lru_cache(maxsize=None)
def _pools(H, Hkv, Sq, Smax, lens, D, dtype, page):
    pr = _problem(H, Hkv, Sq, Smax, lens, D, dtype)
    return scatter(pr["kn"], pr["vn"], page, seed=page + D)


def _chain(B, Sq):
    w = torch.tensor([(1 << (i + 1)) - 1 if i < 63 else -1 for i in range(Sq)], dtype=torch.int64, device=device())
    return w[None].expand(B, Sq).contiguous()


def _tree_words(B, Sq, seed):
    from photonic_flash_attention_amd import ops
    g = torch.Generator().manual_seed(seed)
    parents = torch.stack([torch.randint(-1, i, (B,), generator=g) if i else torch.full((B,), -1) for i in range(Sq)], dim=1)
    return ops.tree_mask_from_parents(parents.to(device()))[0]


def _random_words(B, Sq, seed):
    """Arbitrary 64-bit words: bits above the diagonal, at and above Sq, the sign bit."""
    g = torch.Generator().manual_seed(seed)
    hi = torch.randint(-2 ** 31, 2 ** 31, (B, Sq), generator=g, dtype=torch.int64)
    lo = torch.randint(0, 2 ** 32, (B, Sq), generator=g, dtype=torch.int64)
    return ((hi << 32) | lo).to(device())


def _run(pr, words, paged=None, **kw):
    from photonic_flash_attention_amd import ops
    if paged is None:
        o, lse = ops.fa3_decode(pr["q"], pr["kn"], pr["vn"], cache_seqlens=pr["lens"], tree_mask=words, return_lse=True, **kw)
    else:
        kp, vp, table = paged
        o, lse = ops.fa3_decode(pr["q"], kp, vp, cache_seqlens=pr["lens"], block_table=table, tree_mask=words, return_lse=True, **kw)
    torch.cuda.synchronize()
    return o, lse


def _check(pr, words, o, lse, what, key_mask=None):
    ref, rlse, pn = folded_reference(pr, words, key_mask)
    check_out(o, ref, pn, pr["vmax"], pr["dtype"], what)
    check_lse(o, lse, rlse, what)


def _word_sets(B, Sq, seed):
    return {"random trees": _tree_words(B, Sq, seed), "random words": _random_words(B, Sq, seed + 1),
            "zero words": torch.zeros(B, Sq, dtype=torch.int64, device=device())}


# --- 1, 2, 3, 5: the edge tiles --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,D", DT_D, ids=DT_IDS)
def test_tree_edge_tiles_against_fp64(dtype, D):
    pr = _problem(D=D, dtype=dtype, **SHAPE1)
    for name, words in _word_sets(pr["B"], pr["Sq"], 10 + D).items():
        o, lse = _run(pr, words)
        assert o.dtype == dtype and o.shape == pr["q"].shape and lse.shape == pr["q"].shape[:3]
        _check(pr, words, o, lse, f"{name} D {D}")
        if name == "zero words":                                            # only the prefix is seen; without one, nothing
            assert bool((lse[5:] == float("-inf")).all()) and bool((o[5:] == 0).all()) and bool(torch.isfinite(lse[:5]).all())
        for page in (64, 128):                                              # 5: paged, bit-equal to the contiguous call
            op, lp = _run(pr, words, _pools(D=D, dtype=dtype, page=page, **SHAPE1))
            assert torch.equal(op, o) and torch.equal(lp, lse), (name, page)


def test_tree_edge_tiles_with_an_fp32_output():
    pr = _problem(D=128, dtype=torch.bfloat16, **SHAPE1)
    for name, words in _word_sets(pr["B"], pr["Sq"], 77).items():
        o, lse = _run(pr, words, out_dtype=torch.float32)
        assert o.dtype == torch.float32
        _check(pr, words, o, lse, f"{name} fp32 out")
    oc, lc = _run(pr, _chain(pr["B"], pr["Sq"]), out_dtype=torch.float32)
    o0, l0 = _run(pr, None, out_dtype=torch.float32)
    assert torch.equal(oc, o0) and torch.equal(lc, l0)


@pytest.mark.parametrize("dtype,D", DT_D, ids=DT_IDS)
def test_the_chain_is_bit_equal_to_causal(dtype, D):
    for shape in [SHAPE1] + SHAPES4:
        pr = _problem(D=D, dtype=dtype, **shape)
        chain = _chain(pr["B"], pr["Sq"])
        o, lse = _run(pr, chain)
        o0, l0 = _run(pr, None)                                             # causal=True, no tree
        assert torch.equal(o, o0) and torch.equal(lse, l0), shape
        _check(pr, chain, o, lse, f"chain D {D} Sq {pr['Sq']}")
        for page in (64, 128):
            op, lp = _run(pr, chain, _pools(D=D, dtype=dtype, page=page, **shape))
            assert torch.equal(op, o) and torch.equal(lp, lse), (shape, page)


@pytest.mark.parametrize("dtype,D", DT_D, ids=DT_IDS)
def test_all_ones_words_are_causal_false(dtype, D):
    pr = _problem(D=D, dtype=dtype, **SHAPE1)
    ones = torch.full((pr["B"], pr["Sq"]), -1, dtype=torch.int64, device=device())
    o, lse = _run(pr, ones)
    _check(pr, ones, o, lse, f"all-ones D {D}")
    o0, l0 = _run(pr, None, causal=False)
    same = torch.equal(o, o0) and torch.equal(lse, l0)
    print(f"all-ones words bit-equal to causal=False: {same}")
    assert same                                                              # a masked tile with every key visible computes what an unmasked one does


# --- 4: Sq 64 and Sq 1 -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES4, ids=["g1", "g4"])
@pytest.mark.parametrize("dtype,D", DT_D[:2], ids=DT_IDS[:2])
def test_sixty_four_nodes_use_bit_63(dtype, D, shape):
    # at D 128 the 64 new keys span three 32-key tiles of different waves (lengths 200 and 127); 64 has no prefix
    pr = _problem(D=D, dtype=dtype, **shape)
    sets = _word_sets(pr["B"], 64, 40 + D)
    assert bool((sets["random trees"][:, 63] < 0).all())                     # the last node's own bit is the sign bit
    sets["bit 63 only"] = torch.zeros(pr["B"], 64, dtype=torch.int64, device=device())
    sets["bit 63 only"][:, 63] = -2 ** 63                                    # the last row sees the prefix and itself, every other row the prefix
    for name, words in sets.items():
        o, lse = _run(pr, words)
        _check(pr, words, o, lse, f"Sq 64 {name} D {D}")
        for page in (64, 128):
            op, lp = _run(pr, words, _pools(D=D, dtype=dtype, page=page, **shape))
            assert torch.equal(op, o) and torch.equal(lp, lse), (name, page)
    o, lse = _run(pr, sets["bit 63 only"])
    assert bool(torch.isfinite(lse[0, :, 63]).all()) and bool((lse[0, :, :63] == float("-inf")).all())    # len 64: no prefix


@pytest.mark.parametrize("dtype,D", DT_D[:2], ids=DT_IDS[:2])
def test_one_node(dtype, D):
    pr = _problem(H=8, Hkv=2, Sq=1, Smax=256, lens=(50, 50, 1, 1, 0, 129), D=D, dtype=dtype)
    words = torch.tensor([[1], [0], [1], [0], [1], [-2]], dtype=torch.int64, device=device())
    o, lse = _run(pr, words)
    _check(pr, words, o, lse, f"Sq 1 D {D}")
    assert bool(torch.isfinite(lse[:3]).all()) and bool((lse[3:5] == float("-inf")).all()) and bool((o[3:5] == 0).all())
    op, lp = _run(pr, words, _pools(H=8, Hkv=2, Sq=1, Smax=256, lens=(50, 50, 1, 1, 0, 129), D=D, dtype=dtype, page=64))
    assert torch.equal(op, o) and torch.equal(lp, lse)


# --- 6: with a key mask ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,D", DT_D[:2], ids=DT_IDS[:2])
def test_tree_combined_with_a_key_mask(dtype, D):
    pr = _problem(D=D, dtype=dtype, **SHAPE1)
    km = torch.ones(pr["B"], pr["Smax"], dtype=torch.bool, device=device())
    km[:, :37] = False                                                       # left padding ...
    km[:, 64:70] = False                                                     # ... a hole across a tile boundary ...
    for b, n in enumerate(LENS1):
        if n >= 2:
            km[b, n - 2] = False                                             # ... and one key of the tree (new row Sq - 2)
    for name, words in list(_word_sets(pr["B"], pr["Sq"], 90 + D).items())[:2] + [("chain", _chain(pr["B"], pr["Sq"]))]:
        o, lse = _run(pr, words, key_mask=km)
        _check(pr, words, o, lse, f"key mask + {name} D {D}", key_mask=km)
        op, lp = _run(pr, words, _pools(D=D, dtype=dtype, page=64, **SHAPE1), key_mask=km)
        assert torch.equal(op, o) and torch.equal(lp, lse)


# --- 7: one capture, replays while words, lengths and table change ---------------------------------------------------------------------

def test_a_captured_tree_step_replays_while_its_inputs_change():
    from photonic_flash_attention_amd import ops
    pr = _problem(H=8, Hkv=2, Sq=5, Smax=1024, lens=(900, 333, 64), D=128, dtype=torch.bfloat16)
    kp, vp, table0 = scatter(pr["k"], pr["v"], 128, seed=3)                 # clean caches: the lengths below move up and down
    B, Sq = pr["B"], pr["Sq"]
    words, lens, table = _tree_words(B, Sq, 5).clone(), pr["lens"].clone(), table0.clone()

    def step():
        return ops.fa3_decode(pr["q"], kp, vp, cache_seqlens=lens, block_table=table, tree_mask=words, return_lse=True)

    graph, (o, lse) = capture(step)
    states = [(_tree_words(B, Sq, 5), [900, 333, 64], table0),
              (_random_words(B, Sq, 6), [100, 1024, 3], table0),
              (_chain(B, Sq), [770, 68, 0], table0.flip(0).contiguous()),
              (torch.zeros(B, Sq, dtype=torch.int64, device=device()), [5, 512, 101], table0.roll(1, 0).contiguous())]
    for n, (w, ln, tb) in enumerate(states):
        words.copy_(w)
        lens.copy_(i32(ln))
        table.copy_(tb)
        graph.replay()
        torch.cuda.synchronize()
        oe, le = step()
        torch.cuda.synchronize()
        assert torch.equal(o, oe) and torch.equal(lse, le), n
        assert bool(torch.isfinite(o).all())
    # the third state is the causal call
    words.copy_(states[2][0])
    lens.copy_(i32(states[2][1]))
    table.copy_(states[2][2])
    graph.replay()
    o0, l0 = ops.fa3_decode(pr["q"], kp, vp, cache_seqlens=lens, block_table=table, return_lse=True)
    torch.cuda.synchronize()
    assert torch.equal(o, o0) and torch.equal(lse, l0)


# --- 8: a speculative step on a PagedKVCache -------------------------------------------------------------------------------------------

def test_paged_cache_tree_step_then_accept():
    from photonic_flash_attention_amd import ops
    from photonic_flash_attention_amd.integration.pytorch import PagedKVCache
    dev, dtype, H, Hkv, D, Sq = device(), torch.bfloat16, 8, 2, 64, 5
    g = torch.Generator(device=dev).manual_seed(808)
    rnd = lambda *s: torch.randn(*s, generator=g, device=dev).to(dtype)
    prefix = [70, 130]
    mk = lambda: PagedKVCache(num_pages=10, page_size=64, Hkv=Hkv, D=D, dtype=dtype, device=dev, max_batch=2, max_pages_per_seq=4,
                              copy_on_write=True)
    cache, direct = mk(), mk()
    pk = [rnd(1, Hkv, n, D) for n in prefix]
    pv = [rnd(1, Hkv, n, D) for n in prefix]
    for c in (cache, direct):
        for s, (k, v) in enumerate(zip(pk, pv)):
            assert c.allocate() == s
            c.append(s, k, v)
    # the step: 5 drafted nodes per sequence
    parents = torch.tensor([[-1, -1, 0, 2, 1], [-1, 0, 0, 1, 3]], device=dev)
    words, depths = ops.tree_mask_from_parents(parents)
    assert depths.tolist() == [[0, 0, 1, 2, 1], [0, 1, 1, 2, 3]]
    k_new, v_new = rnd(2 * Sq, Hkv, D), rnd(2 * Sq, Hkv, D)                  # packed, sequence-major
    q = rnd(2, Sq, H, D).permute(0, 2, 1, 3)
    cache.advance([0, 1], [Sq, Sq])
    cache.write_step(k_new, v_new, [Sq, Sq])
    o, lse = cache.decode(q, tree_mask=words, return_lse=True)
    torch.cuda.synchronize()
    kc, vc = contiguous_of(cache, 256)
    pr = dict(q=q, k=kc, v=vc, lens=cache.cache_seqlens.clone(), B=2, Sq=Sq, Smax=256)
    ref, rlse, pn = folded_reference(pr, words)
    check_out(o, ref, pn, float(vc.abs().max()), dtype, "paged tree step")
    check_lse(o, lse, rlse, "paged tree step")
    # accept: sequence 0 the path 0 -> 2 -> 3, sequence 1 the path 0 -> 1
    paths = [[0, 2, 3], [0, 1]]
    for s, n in enumerate(prefix):
        cache.truncate(s, n)
    rows = torch.tensor([s * Sq + i for s, p in enumerate(paths) for i in p], device=dev)
    cache.append_varlen([0, 1], k_new[rows], v_new[rows], [len(p) for p in paths])
    direct.append_varlen([0, 1], k_new[rows], v_new[rows], [len(p) for p in paths])
    assert [cache.length(s) for s in (0, 1)] == [73, 132] == [direct.length(s) for s in (0, 1)]
    for s in (0, 1):
        assert torch.equal(cache.gather(s)[0], direct.gather(s)[0]) and torch.equal(cache.gather(s)[1], direct.gather(s)[1])
    # the next plain step reads the accepted tokens only
    q1 = rnd(2, 1, H, D).permute(0, 2, 1, 3)
    o1, l1 = cache.decode(q1, return_lse=True)
    o2, l2 = direct.decode(q1, return_lse=True)
    torch.cuda.synchronize()
    assert torch.equal(o1, o2) and torch.equal(l1, l2) and bool(torch.isfinite(l1).all())

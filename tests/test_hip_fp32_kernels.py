"""GPU tests of the exact-fp32 kernels (csrc/fa3_fwd_f32_kernel.h, csrc/fa3_bwd_f32_kernel.h: fp32 modules in both directions, and every
module's attention dropout) against the fp64 reference of tests/dense_testlib.py, whose docstring states the bounds and the exact
conditions once: masks of every form, rows that see no key, seqlens_k, grouped heads, block edges, layouts, stores and dropout.

The kernels' geometry fixes the shapes: a workgroup owns 128 rows, a wave 32, and walks the other side in tiles of 32 -- so Sq and Sk
come from {1, 31, 33, 97, 129, 130, 200, 257, 333}.  Masks are drawn from a seeded generator with key 0 kept in every row, then named
rows are cleared: the rows that see no key are known from the construction, and the reference must report exactly those.

Groups: (a) forward, (b) backward, (c) dropout in both directions, (d) fp32 modules."""

from __future__ import annotations

import functools
import types

import pytest
import torch

from dense_testlib import (DEV, GUARD, INF, NAN32, bwd_into, check_forward, check_grads, guarded, reference, seen, visible)
from photonic_flash_attention_amd import synth

pytestmark = pytest.mark.gpu

DEAD_ROWS = (5,) + tuple(range(100, 133))          # a single row, and a run that crosses the wave boundary at 128


def _case(name, B, H, Hkv, Sq, Sk, D, causal, **extra):
    return dict(name=name, B=B, H=H, Hkv=Hkv, Sq=Sq, Sk=Sk, D=D, causal=causal, **extra)


def _both(name, B, H, Hkv, Sq, Sk, D, **extra):
    """the case without and with the causal mask, at D and at the other head dim"""
    return [_case(name, B, H, Hkv, Sq, Sk, D, False, **extra), _case(name + "-causal", B, H, Hkv, Sq, Sk, 192 - D, True, **extra)]


CASES = (
    # ---- every mask form; 200 rows hold the dead run 100..132
    _both("mask-key", 2, 2, 2, 200, 333, 64, mask="key")
    + _both("mask-b1qk", 2, 2, 2, 200, 333, 128, mask="b1qk")
    + _both("mask-bhqk", 2, 3, 3, 200, 257, 64, mask="bhqk")                 # the heads' masks differ
    + _both("mask-11qk", 2, 2, 2, 200, 130, 128, mask="11qk")
    + _both("mask-3d", 2, 2, 2, 257, 129, 64, mask="3d")                     # Sq > Sk under the causal mask
    + _both("mask-leftpad", 2, 2, 2, 130, 97, 128, mask="leftpad")           # tile 0 fully masked, tile 1 not: rows come alive later
    + _both("mask-zero-batch", 2, 2, 2, 130, 129, 64, mask="zero_batch")
    # ---- seqlens_k: full, none, one key, one key past a tile; entries past Sk and below zero, as a tensor
    + _both("lens", 4, 2, 2, 130, 257, 64, lens=[257, 0, 1, 33])
    + _both("lens-clamped", 2, 2, 2, 130, 257, 128, lens=[257 + 5, -3], lens_tensor=True)
    + _both("lens-mid", 2, 2, 2, 130, 257, 64, lens=[140, 77])               # inside a wave's 32 keys and inside a 128-key block
    # ---- grouped heads: groups of 2, 3 and H
    + [_case("gqa2-causal", 2, 6, 3, 130, 200, 64, True),
       _case("gqa3-lens", 2, 6, 2, 97, 257, 128, False, lens=[257, 33]),
       _case("gqaH-bhqk", 2, 6, 1, 200, 129, 64, False, mask="bhqk"),
       _case("gqa2", 2, 4, 2, 129, 130, 128, False),
       _case("gqa3-b1qk-causal", 1, 6, 2, 200, 333, 128, True, mask="b1qk"),
       _case("gqa2-key", 2, 4, 2, 33, 97, 64, False, mask="key")]
    # ---- block edges
    + _both("edge-1x1", 2, 2, 2, 1, 1, 64)
    + _both("edge-1x333", 2, 2, 2, 1, 333, 128)
    + _both("edge-129x31", 2, 2, 2, 129, 31, 64)
    + _both("edge-33x129", 2, 2, 2, 33, 129, 128)
    + _both("edge-257x97", 2, 2, 2, 257, 97, 64)
    # ---- the caller's scale, the online-softmax rescale, zero-padded head dims
    + _both("scale", 1, 2, 2, 97, 130, 64, scale=0.2)
    + _both("rescale", 1, 2, 2, 130, 333, 128, rising=True)
    + [_case("d40-b1qk", 2, 2, 2, 200, 97, 40, False, mask="b1qk"), _case("d96-key-causal", 2, 2, 2, 130, 200, 96, True, mask="key")]
)
DROP_CASES = [
    _case("drop", 2, 2, 2, 130, 257, 128, False, drop="rand"),
    _case("drop-causal", 2, 2, 2, 97, 333, 64, True, drop="rand"),
    _case("drop-lens", 2, 2, 2, 130, 257, 64, False, drop="rand", lens=[257, 33]),
    _case("drop-key", 2, 2, 2, 130, 257, 128, False, drop="rand", mask="key"),
    _case("drop-bhqk", 2, 2, 2, 200, 333, 64, True, drop="rand", mask="bhqk"),
    _case("drop-gqa2", 2, 4, 2, 129, 130, 128, False, drop="rand"),
    _case("drop-d40", 2, 2, 2, 97, 129, 40, True, drop="rand"),
    _case("drop-whole-row", 2, 2, 2, 130, 200, 64, True, drop="row"),
]
BY_NAME = {c["name"]: c for c in CASES + DROP_CASES}
assert len(BY_NAME) == len(CASES) + len(DROP_CASES)
WHOLE_ROW = (0, 1, 37)                               # (b, h, row) of "drop-whole-row": every key it sees is dropped


def _ids(cases):
    return [c["name"] for c in cases]


def _masks(c, g):
    """-> (the kernels' mask keywords, what the reference keeps [broadcastable to B,H,Sq,Sk] or None, the rows built to see no key)"""
    B, H, Sq, Sk, causal, kind = c["B"], c["H"], c["Sq"], c["Sk"], c["causal"], c.get("mask")
    dead = torch.zeros(B, H, Sq, dtype=torch.bool)
    rows = [r for r in DEAD_ROWS if r < Sq]
    if kind is None:
        return {}, None, dead
    if kind == "key":
        m = torch.rand(B, Sk, generator=g) < 0.8
        m[:, 0] = True
        return dict(key_mask=m), m[:, None, None, :], dead
    if kind == "leftpad":                            # the first 40 (batch 1: 45) keys masked; under the causal mask the rows before them see nothing
        m = torch.ones(B, Sk, dtype=torch.bool)
        m[:, :40] = False
        m[1, 40:45] = False
        if causal:
            dead[0, :, :40] = True
            dead[1, :, :45] = True
        return dict(key_mask=m), m[:, None, None, :], dead
    if kind == "zero_batch":
        m = torch.rand(B, Sk, generator=g) < 0.8
        m[:, 0] = True
        m[1] = False
        dead[1] = True
        return dict(key_mask=m), m[:, None, None, :], dead
    shape = {"b1qk": (B, 1, Sq, Sk), "bhqk": (B, H, Sq, Sk), "11qk": (1, 1, Sq, Sk), "3d": (B, Sq, Sk)}[kind]
    m = torch.rand(shape, generator=g) < 0.7
    m[..., 0] = True                                 # every row sees key 0 (also under the causal mask), until it is cleared
    if kind == "bhqk":                               # other rows in every head: a kernel that reads head 0's mask for all heads fails
        m[:, 0, 5] = False
        m[:, 1, 100:133] = False
        m[1, H - 1, 64] = False
        dead[:, 0, 5] = dead[:, 1, 100:133] = dead[1, H - 1, 64] = True
    else:
        for r in rows:
            m[..., r, :] = False
            dead[:, :, r] = True
    return dict(mask=m), (m[:, None] if kind == "3d" else m), dead


@functools.lru_cache(maxsize=None)
def _problem(name):
    """Operands, kernel keywords and the fp64 reference (forward and gradients) of a case: built once, never modified."""
    c = BY_NAME[name]
    B, H, Hkv, Sq, Sk, D, causal = (c[n] for n in ("B", "H", "Hkv", "Sq", "Sk", "D", "causal"))
    idx = list(BY_NAME).index(name)
    shapes = ((B, Sq, H, D), (B, Sk, Hkv, D), (B, Sk, Hkv, D), (B, Sq, H, D))
    q, k, v, dout = (torch.from_numpy(synth.normal_f32(s, 8100 + 10 * idx + i)) for i, s in enumerate(shapes))        # [B,S,H,D]
    if c.get("rising"):
        # scores that rise tile after tile, for every row: q gets sqrt(D) along a unit vector u, key j gets 1.5 (j // 32) along it, so
        # scale q.k grows by 1.5 per tile of 32 keys on top of its N(0, ~2) spread -- every row's running maximum moves, and O is
        # rescaled, in most of the tiles (the forward test counts them); scores reach ~22
        u = torch.full((D,), D ** -0.5)
        q = q + D ** 0.5 * u
        k = k + 1.5 * (torch.arange(Sk) // 32).float()[None, :, None, None] * u
    g = torch.Generator().manual_seed(9100 + idx)
    kw, keep, dead = _masks(c, g)
    lens = c.get("lens")
    if lens is not None:
        kw["seqlens_k"] = torch.tensor(lens, dtype=torch.int32) if c.get("lens_tensor") else lens
        for b, n in enumerate(lens):
            if n <= 0:
                dead[b] = True
    if c.get("scale") is not None:
        kw["softmax_scale"] = c["scale"]
    drop, drop_scale = None, 1.0
    if c.get("drop"):
        drop, drop_scale = torch.rand(B, H, Sq, Sk, generator=g) >= 0.25, 1 / 0.75
        if c["drop"] == "row":
            drop[WHOLE_ROW] = False
    qh, kh, vh, gh = (t.permute(0, 2, 1, 3) for t in (q, k, v, dout))                                                 # [B,H,S,D] views
    ref = reference(qh, kh, vh, causal=causal, seqlens=lens, keep=keep, drop=drop, drop_scale=drop_scale, scale=c.get("scale"), dout=gh)
    vis = visible(B, H, Sq, Sk, causal=causal, seqlens=lens, keep=keep)
    row_seen, key_seen = seen(vis, Hkv)
    # the dead rows are the chosen ones: known from the construction, and the reference reports exactly those
    assert torch.equal(ref[1] == -INF, dead) and torch.equal(~row_seen, dead), name
    plain = reference(qh, kh, vh, causal=causal, seqlens=lens, keep=keep, scale=c.get("scale")) if drop is not None else ref
    return types.SimpleNamespace(c=c, q=qh, k=kh, v=vh, dout=gh, kw=kw, drop=drop, drop_scale=drop_scale, ref=ref, lse_plain=plain[1],
                                 row_seen=row_seen, key_seen=key_seen, dead=dead, vis=vis)


def _dev(t):
    """a [B,H,S,D] view of a [B,S,H,D] CPU array -> the same view of a device copy"""
    return t.permute(0, 2, 1, 3).contiguous().to(DEV).permute(0, 2, 1, 3)


def _kw_dev(P):
    kw = {n: (m.to(DEV) if isinstance(m, torch.Tensor) else m) for n, m in P.kw.items()}
    if P.drop is not None:
        kw.update(drop_mask=P.drop.to(DEV).contiguous(), drop_scale=P.drop_scale)
    return kw


def _run(P, backward=True):
    """the forward, and the backward on the forward's own ``out`` and ``lse`` -> (o, lse, grads or None)"""
    from photonic_flash_attention_amd import ops
    c = P.c
    q, k, v, g = (_dev(t) for t in (P.q, P.k, P.v, P.dout))
    kw = _kw_dev(P)
    o, lse = ops.fa3_forward(q, k, v, causal=c["causal"], return_lse=True, **kw)
    grads = ops.fa3_backward(q, k, v, o, g, lse, causal=c["causal"], **kw) if backward else None
    torch.cuda.synchronize()
    return o, lse, grads


# ---- (a) forward ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", _ids(CASES))
def test_forward_against_the_fp64_reference(name):
    P = _problem(name)
    o, lse, _ = _run(P, backward=False)
    check_forward(o, lse, P.ref[0], P.ref[1], f"(a) {name}")
    if P.c.get("rising") and not P.c["causal"]:        # the construction does what it says: every row's running maximum keeps moving
        s = (P.q.double() @ P.k.double().transpose(-1, -2))
        tile_max = torch.stack([s[..., t:t + 32].amax(-1) for t in range(0, P.c["Sk"], 32)], dim=-1)          # [B,H,Sq,tiles]
        moves = (tile_max[..., 1:] > tile_max.cummax(-1).values[..., :-1]).sum(-1)
        print(f"(a) {name}: the running maximum moves in {int(moves.min())}..{int(moves.max())} of {tile_max.shape[-1] - 1} tile steps")
        assert int(moves.min()) >= 5


@pytest.mark.parametrize("gqa", [False, True], ids=["qkv", "q+kv-grouped"])
def test_forward_reads_fused_projection_views_in_place(gqa):
    """q, k, v as slices of one [B,S,3,H,D] buffer -- what the module hands over --, and k, v as slices of a [B,Sk,2,Hkv,D] buffer under
    grouped heads: bit for bit the result of contiguous copies, in both directions."""
    from photonic_flash_attention_amd import ops
    B, H, Sq, D = 2, 4, 130, 64
    Hkv, Sk = (2, 257) if gqa else (H, Sq)
    if gqa:
        kv = torch.from_numpy(synth.normal_f32((B, Sk, 2, Hkv, D), 8801)).to(DEV)
        q = torch.from_numpy(synth.normal_f32((B, Sq, H, D), 8802)).to(DEV).permute(0, 2, 1, 3)
        k, v = (kv[:, :, i].permute(0, 2, 1, 3) for i in range(2))
    else:
        qkv = torch.from_numpy(synth.normal_f32((B, Sq, 3, H, D), 8800)).to(DEV)
        q, k, v = (qkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    g = torch.from_numpy(synth.normal_f32((B, Sq, H, D), 8803)).to(DEV).permute(0, 2, 1, 3)
    assert not k.is_contiguous() and k.stride(2) == (2 * Hkv * D if gqa else 3 * H * D) and v.data_ptr() - k.data_ptr() == 4 * Hkv * D
    for causal in (False, True):
        o, lse = ops.fa3_forward(q, k, v, causal=causal, return_lse=True)
        oc, lsec = ops.fa3_forward(q.contiguous(), k.contiguous(), v.contiguous(), causal=causal, return_lse=True)
        torch.cuda.synchronize()
        assert torch.equal(o, oc) and torch.equal(lse, lsec), f"causal={causal}: a strided view gives other bits than its contiguous copy"
        ref = reference(q, k, v, causal=causal, dout=g)
        check_forward(o, lse, ref[0], ref[1], f"(a) fused views gqa={gqa} causal={causal}")
        # the backward reads the same views (and, like autograd, a dout that is a view of a [B,Sq,H,D] buffer)
        grads = ops.fa3_backward(q, k, v, o, g, lse, causal=causal)
        gradsc = ops.fa3_backward(q.contiguous(), k.contiguous(), v.contiguous(), oc.contiguous(), g.contiguous(), lsec, causal=causal)
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(grads, gradsc)), f"causal={causal}: the backward reads a strided view differently"
        row_seen, key_seen = seen(visible(B, H, Sq, Sk, causal=causal), Hkv)
        check_grads(grads, ref[2:], row_seen, key_seen, f"(b) fused views gqa={gqa} causal={causal}")


@pytest.mark.parametrize("pad, D", [(1, 64), (1, 128), (4, 64), (4, 128)], ids=["scalar-d64", "scalar-d128", "vector-d64", "vector-d128"])
def test_forward_out_layouts_store_the_same_bits_and_nothing_else(pad, D):
    """``out=`` a [B,H,Sq,D] view of a NaN-patterned [B,Sq,H,D + pad] buffer.  pad 1: strides that are no multiple of 4 take the
    kernel's scalar store; pad 4: the vector store.  Either gives the plain call's bits and leaves every pad column alone."""
    from photonic_flash_attention_amd import ops
    B, H, Sq, Sk = 2, 2, 130, 97
    q, k, v = (torch.from_numpy(synth.normal_f32(s, 8810 + i)).to(DEV).permute(0, 2, 1, 3)
               for i, s in enumerate(((B, Sq, H, D), (B, Sk, H, D), (B, Sk, H, D))))
    plain, lse0 = ops.fa3_forward(q, k, v, causal=True, return_lse=True)
    ibuf = torch.full((B, Sq, H, D + pad), NAN32, dtype=torch.int32, device=DEV)
    out = ibuf.view(torch.float32)[..., :D].permute(0, 2, 1, 3)
    vector = out.data_ptr() % 16 == 0 and all(s % 4 == 0 for s in out.stride()[:3])
    assert vector == (pad == 4), out.stride()
    got, lse = ops.fa3_forward(q, k, v, causal=True, return_lse=True, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() and got.stride() == out.stride()
    assert bool((ibuf[..., D:] == NAN32).all()), "a pad column was written"
    assert not bool(torch.isnan(got).any()), "an element of the output was never written"
    assert torch.equal(got, plain) and torch.equal(lse, lse0)
    ref = reference(q, k, v, causal=True)
    check_forward(got, lse, ref[0], ref[1], f"(a) out= pad {pad} D {D}")


# ---- (b) backward --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", _ids(CASES))
def test_backward_against_the_fp64_reference(name):
    P = _problem(name)
    c = P.c
    o, lse, grads = _run(P)
    assert tuple(grads[0].shape) == (c["B"], c["H"], c["Sq"], c["D"])
    assert tuple(grads[1].shape) == tuple(grads[2].shape) == (c["B"], c["Hkv"], c["Sk"], c["D"])      # grouped heads: summed per group
    check_grads(grads, P.ref[2:], P.row_seen, P.key_seen, f"(b) {name}")


def test_fp32_backward_is_bitwise_reproducible():
    """fa3_bwd_f32_kernel.h: "no atomics, bitwise reproducible" -- with an element mask, dead rows and grouped heads"""
    P = _problem("gqa3-b1qk-causal")
    a, b = _run(P), _run(P)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert all(torch.equal(x, y) for x, y in zip(a[2], b[2]))


def test_backward_gives_a_row_the_forward_found_dead_no_gradient():
    """fa3_bwd_f32_kernel.h: "lse = -inf: a row the forward found fully masked" contributes nothing, whatever the masks of the backward
    call say.  (With the forward's own masks every key of such a row is masked in the backward too, and the rule cannot show.)  The LSE
    of chosen rows is set to -inf, their output to zero, and the backward runs WITHOUT a mask: the gradients are those of the problem
    with these rows masked, dq of the rows exactly zero."""
    from photonic_flash_attention_amd import ops
    B, H, Sq, Sk, D = 2, 2, 130, 97, 64
    q, k, v, g = (torch.from_numpy(synth.normal_f32(s, 8820 + i)).permute(0, 2, 1, 3)
                  for i, s in enumerate(((B, Sq, H, D), (B, Sk, H, D), (B, Sk, H, D), (B, Sq, H, D))))
    keep = torch.ones(B, H, Sq, 1, dtype=torch.bool)
    keep[0, 1, 3] = keep[1, 0, 31:34] = keep[1, 1, 129] = False
    ref = reference(q, k, v, keep=keep, dout=g)
    row_seen, key_seen = seen(visible(B, H, Sq, Sk, keep=keep), H)
    qd, kd, vd, gd = (_dev(t) for t in (q, k, v, g))
    o, lse = ops.fa3_forward(qd, kd, vd, return_lse=True)
    dead = ~row_seen.to(DEV)
    lse = lse.masked_fill(dead, -INF)
    o.masked_fill_(dead[..., None], 0.0)
    grads = ops.fa3_backward(qd, kd, vd, o, gd, lse)
    torch.cuda.synchronize()
    check_grads(grads, ref[2:], row_seen, key_seen, "(b) lse = -inf without a mask")


@pytest.mark.parametrize("case", [(2, 2, 33, 129, 128, True), (2, 2, 257, 100, 64, False)])
def test_fp32_backward_writes_every_gradient_element_and_nothing_else(case):
    """The fp32 kernels' own scalar gradient stores and their ``own < n_own`` guard, through the C ABI: dq, dk, dv into NaN-patterned
    [B, 32 + S + 32, H, D + 1] buffers, whose odd row strides the fp32 rules allow."""
    from photonic_flash_attention_amd import ops
    B, H, Sq, Sk, D, causal = case
    q, k, v, g = (torch.from_numpy(synth.normal_f32(s, 8830 + Sq + i)).permute(0, 2, 1, 3)
                  for i, s in enumerate(((B, Sq, H, D), (B, Sk, H, D), (B, Sk, H, D), (B, Sq, H, D))))
    ref = reference(q, k, v, causal=causal, dout=g)
    row_seen, key_seen = seen(visible(B, H, Sq, Sk, causal=causal), H)
    qd, kd, vd, gd = (_dev(t) for t in (q, k, v, g))
    out, lse = ops.fa3_forward(qd, kd, vd, causal=causal, return_lse=True)
    plain = ops.fa3_backward(qd, kd, vd, out, gd, lse, causal=causal)
    bufs, ibufs, pats = zip(*(guarded(B, S, H, D, torch.float32, pad=1) for S in (Sq, Sk, Sk)))
    assert all(b.stride(1) % 4 != 0 and b.stride(2) % 2 == 1 for b in bufs)              # no stride a 16-byte store could use
    bwd_into(qd, kd, vd, out, gd, lse, causal, torch.float32, bufs)
    what = f"(b) contained {case}"
    got_all = []
    for name, buf, ibuf, pat, S, p in zip(("dq", "dk", "dv"), bufs, ibufs, pats, (Sq, Sk, Sk), plain):
        inside = torch.zeros(ibuf.shape, dtype=torch.bool, device=DEV)
        inside[:, GUARD:GUARD + S, :, :D] = True
        stray = (ibuf != pat) & ~inside
        assert not bool(stray.any()), f"{name} {what}: written outside the tensor, first at [b, row, h, d] = " \
                                      f"{tuple(int(x) for x in stray.nonzero()[0])} (rows {GUARD}..{GUARD + S - 1} are the tensor)"
        got = buf[:, GUARD:GUARD + S, :, :D].permute(0, 2, 1, 3)       # [B,H,S,D]
        holes = torch.isnan(got)
        assert not bool(holes.any()), f"{name} {what}: {int(holes.sum())} elements never written, first at [b, h, row, d] = " \
                                      f"{tuple(int(x) for x in holes.nonzero()[0])}"
        assert torch.equal(got, p), f"{name} {what}: differs from ops.fa3_backward on the same operands"
        got_all.append(got)
    check_grads(got_all, ref[2:], row_seen, key_seen, what)


# ---- (c) dropout with a fixed keep-mask ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", _ids(DROP_CASES))
def test_dropout_both_directions_against_the_fp64_reference(name):
    """o against the reference, the LSE against the UN-dropped reference, the gradients against the reference"""
    P = _problem(name)
    o, lse, grads = _run(P)
    assert torch.equal(P.ref[1], P.lse_plain)              # (the reference keeps its own rule: dropout does not move the LSE)
    check_forward(o, lse, P.ref[0], P.lse_plain, f"(c) {name}")
    check_grads(grads, P.ref[2:], P.row_seen, P.key_seen, f"(c) {name}", dropout=True)
    if P.c["drop"] == "row":
        b, h, r = WHOLE_ROW
        assert bool(P.row_seen[b, h, r]) and not bool((P.drop[b, h, r] & P.vis[b, h, r]).any())
        assert bool((o[b, h, r] == 0).all()), "a row whose every visible key is dropped is not exactly zero"
        assert bool(torch.isfinite(lse[b, h, r])) and abs(float(lse[b, h, r]) - float(P.lse_plain[b, h, r])) <= 2e-5
        assert float((grads[0][b, h, r].cpu().double() - P.ref[2][b, h, r]).abs().max()) <= 3e-5 * max(1.0, float(P.ref[2].abs().max()))


@pytest.mark.parametrize("name", ["mask-b1qk-causal", "lens", "gqa3-lens"])
def test_keeping_every_weight_is_no_dropout_bit_for_bit(name):
    """an all-ones keep-mask with drop_scale 1 (p = 0): both directions give the bits of the call without ``drop_mask``"""
    from photonic_flash_attention_amd import ops
    P = _problem(name)
    c = P.c
    o0, lse0, g0 = _run(P)
    q, k, v, g = (_dev(t) for t in (P.q, P.k, P.v, P.dout))
    kw = _kw_dev(P)
    ones = torch.ones(c["B"], c["H"], c["Sq"], c["Sk"], dtype=torch.bool, device=DEV)
    o, lse = ops.fa3_forward(q, k, v, causal=c["causal"], return_lse=True, drop_mask=ones, drop_scale=1.0, **kw)
    grads = ops.fa3_backward(q, k, v, o, g, lse, causal=c["causal"], drop_mask=ones, drop_scale=1.0, **kw)
    torch.cuda.synchronize()
    assert torch.equal(o, o0) and torch.equal(lse, lse0)
    for n, x, y in zip(("dq", "dk", "dv"), grads, g0):
        assert torch.equal(x, y), n


def test_attention_dropout_function_replays_the_mask_it_drew(monkeypatch):
    """ops.fa3_attention_dropout with a key mask and grouped heads: the keep-mask the Function drew is taken from its backward call,
    and the output and the input gradients are the reference's under that mask."""
    from photonic_flash_attention_amd import ops
    B, H, Hkv, Sq, Sk, D, p = 2, 4, 2, 97, 130, 128, 0.3
    q, k, v, g = (torch.from_numpy(synth.normal_f32(s, 8840 + i)).permute(0, 2, 1, 3)
                  for i, s in enumerate(((B, Sq, H, D), (B, Sk, Hkv, D), (B, Sk, Hkv, D), (B, Sq, H, D))))
    km = torch.rand(B, Sk, generator=torch.Generator().manual_seed(8841)) < 0.8
    km[:, 0] = True
    qd, kd, vd = (_dev(t).requires_grad_(True) for t in (q, k, v))
    seen_calls = []
    real = ops.fa3_backward

    def spy(*a, **kw):
        seen_calls.append(kw)
        return real(*a, **kw)

    monkeypatch.setattr(ops, "fa3_backward", spy)
    torch.manual_seed(8842)
    out = ops.fa3_attention_dropout(qd, kd, vd, p, causal=True, key_mask=km.to(DEV))
    out.backward(_dev(g))
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert len(seen_calls) >= 1                            # (the fp32 grouped-head branch calls itself once more, on expanded heads)
    drop, drop_scale = seen_calls[0]["drop_mask"].cpu(), seen_calls[0]["drop_scale"]
    assert drop.dtype == torch.bool and tuple(drop.shape) == (B, H, Sq, Sk) and abs(drop_scale - 1 / (1 - p)) <= 1e-12
    assert 0.6 < float(drop.float().mean()) < 0.8          # a draw at p = 0.3, not all ones
    ref = reference(q, k, v, causal=True, keep=km[:, None, None, :], drop=drop, drop_scale=drop_scale, dout=g)
    row_seen, key_seen = seen(visible(B, H, Sq, Sk, causal=True, keep=km[:, None, None, :]), Hkv)
    err = float((out.detach().cpu().double() - ref[0]).abs().max())
    print(f"(c) fa3_attention_dropout: o max-abs {err:.3e}")
    assert out.dtype == torch.float32 and err <= 2e-5
    check_grads((qd.grad, kd.grad, vd.grad), ref[2:], row_seen, key_seen, "(c) fa3_attention_dropout", dropout=True)


def test_forward_refuses_a_wrong_drop_mask():
    from photonic_flash_attention_amd import ops
    q = torch.zeros(1, 2, 33, 64, device=DEV)
    good = torch.ones(1, 2, 33, 33, dtype=torch.bool, device=DEV)
    assert ops.fa3_forward(q, q, q, drop_mask=good)[0].shape == q.shape
    for bad in (torch.ones(1, 2, 33, 66, dtype=torch.bool, device=DEV)[..., ::2],       # not contiguous
                torch.ones(1, 2, 33, 34, dtype=torch.bool, device=DEV),                 # the wrong shape
                torch.ones(1, 1, 33, 33, dtype=torch.bool, device=DEV),
                good.cpu(),                                                             # the wrong device
                good.float()):
        with pytest.raises(ValueError):
            ops.fa3_forward(q, q, q, drop_mask=bad)
    with pytest.raises(ValueError):
        ops.fa3_forward(q.bfloat16(), q.bfloat16(), q.bfloat16(), drop_mask=good)       # dropout runs on the fp32 kernels only
    with pytest.raises(ValueError):
        ops.fa3_forward(q, q, q, drop_mask=good, drop_scale=0.5)                        # 1 / (1 - p) is never below 1


# ---- (d) fp32 modules ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [2, 3])
def test_fp32_module_with_a_mask_trains_on_the_oracle_numbers(dims):
    """An fp32 ``FlashAttention3`` in training mode with a 2-D / 3-D ``attention_mask``: output and ``x.grad`` against the oracle's module
    under autograd on the CPU.  Bound 1e-4 * max(1, max|ref|): the projections are fp32 GEMMs on both sides."""
    from oracle import fa3_oracle as orc
    from photonic_flash_attention_amd import FlashAttention3
    E, H, S, B = 128, 2, 96, 2
    torch.manual_seed(8850)
    m = FlashAttention3(E, H).to(DEV).train()
    x = torch.from_numpy(synth.normal_f32((B, S, E), 8851)).to(DEV).requires_grad_(True)
    dout = torch.from_numpy(synth.normal_f32((B, S, E), 8852))
    if dims == 2:
        am = torch.ones(B, S, dtype=torch.bool)
        am[0, 70:] = False
        am[1, 33:50] = False
        am4 = am[:, None, None, :]
    else:
        am = torch.rand(B, S, S, generator=torch.Generator().manual_seed(8853)) < 0.7
        am[..., 0] = True
        am4 = am[:, None]
    out, w = m(x, attention_mask=am.to(DEV))
    assert w is None and out.dtype == torch.float32
    out.backward(dout.to(DEV))
    torch.cuda.synchronize()
    sd = {k_: v_.detach().cpu().clone() for k_, v_ in m.state_dict().items()}
    xc = x.detach().cpu().requires_grad_(True)
    ref = orc.module_forward(sd, H, xc, mask=am4)
    ref.backward(dout)
    for name, got, r in (("out", out.detach().cpu(), ref.detach()), ("x.grad", x.grad.cpu(), xc.grad)):
        assert bool(torch.isfinite(got).all()), name
        err, scale = float((got - r).abs().max()), max(1.0, float(r.abs().max()))
        print(f"(d) fp32 module, {dims}-D mask: {name} max-abs {err:.3e} (bound {1e-4 * scale:.3e}, max |ref| {float(r.abs().max()):.3e})")
        assert err <= 1e-4 * scale, (name, err, scale)

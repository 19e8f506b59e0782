"""CPU tests of tests/far_testlib.py, what the far-address GPU tests rely on: the four truncation models; for every layout those tests use
(built here from their ``CASES``, without a GPU) that at least one index aliases under each model the placement claims and that every
alias lies inside the arena and outside every live region of every tensor placed in it; ``untouched`` on a small host arena; the data
path (``write`` / ``far_view`` / ``read``); and a NumPy stand-in kernel that truncates its addresses in one way each, which the
near-equals-far assertion and ``untouched`` must catch on a layout scaled down to a wrap width of 22 bits -- and pass when it is
honest.  ``pytest -s`` prints the placement table."""

from __future__ import annotations

import numpy as np
import pytest
import torch

import far_testlib as F
import test_hip_far_cache as cache_cases
import test_hip_far_dense as dense_cases
from far_testlib import MODELS, FarCase, Layout, aliases, claims, truncated
from photonic_flash_attention_amd import _capi

W = 22                                              # the scaled-down wrap width of the host arenas below
BYTES = MODELS[:2]
ALL_CASES = [pytest.param(mod, name, id=f"{tag}-{name}") for tag, mod in (("cache", cache_cases), ("dense", dense_cases)) for name in mod.CASES]


def test_truncation_models():
    s = 2 ** 31 + 2 ** 20                           # the wide stride, 16-bit elements
    assert truncated(None, 2 * s, 2) == 2 ** 33 + 2 ** 22
    assert truncated("int32 bytes", s, 2) == 2 ** 21 and truncated("uint32 bytes", s, 2) == 2 ** 21
    assert truncated("int32 elements", s, 2) == (2 ** 20 - 2 ** 31) * 2 and truncated("uint32 elements", s, 2) == 2 * s
    assert truncated("uint32 elements", 2 * s, 2) == 2 ** 22
    n = 2 ** 30 - 8                                 # the narrow stride: only the product overflows
    assert truncated("int32 bytes", n, 2) == 2 * n and truncated("int32 bytes", 2 * n, 2) == -32
    assert truncated("uint32 bytes", 4 * n, 2) == 2 ** 32 - 64 and truncated("int32 elements", 3 * n, 2) == (3 * n - 2 ** 32) * 2
    assert truncated("int32 bytes", 2 ** 21, 2, wrap=W) == -(2 ** 22) + 2 ** 22 and truncated("uint32 bytes", 2 ** 21 + 3, 2, wrap=W) == 6


def _expected_claims(p):
    """From the thresholds, not from ``aliases``: a model is caught when some live index's offset, or one far axis' own product, does
    not fit the model's type."""
    half, full = 1 << (p.wrap - 1), 1 << p.wrap
    got = set()
    for _, idx, off in p.live():
        for x in [off] + [i * p.strides[ax] for ax, i in zip(p.far_axes, idx)]:
            for model, v, lim in (("int32 bytes", x * p.esize, half), ("uint32 bytes", x * p.esize, full), ("int32 elements", x, half),
                                  ("uint32 elements", x, full)):
                if v >= lim:
                    got.add(model)
    return tuple(m for m in MODELS if m in got)


def test_the_placement_table():
    """The table the far-address tests are built on: which models each kind of placement catches, with a 4 GiB lead."""
    lay = Layout()
    bf = lambda *shape: torch.empty(shape, dtype=torch.bfloat16)
    assert claims(lay.like("wide16", bf(3, 2, 64, 128), "wide")) == MODELS
    assert claims(lay.like("narrow16", bf(5, 2, 64, 128), "narrow")) == MODELS[:3]
    assert claims(lay.like("u32max16", bf(3, 2, 64, 128), "u32max")) == MODELS[:3]
    assert claims(lay.like("wide8", torch.empty(2, 2, 64, 128, dtype=torch.uint8), "wide")) == MODELS
    assert claims(lay.like("wide32", torch.empty(2, 2, 64, 128), "wide")) == BYTES          # fp32: the element models are not claimed
    assert claims(lay.pages("pages", cache_cases.NUM_PAGES, (2, 64, 128), 2, cache_cases.page_ids(9))) == MODELS
    assert claims(lay.rows("rows", 1064, (4, 128), (128, 1), 2, 2 ** 22 + 8, range(1064))) == MODELS
    assert lay.problems() == []
    with pytest.raises(AssertionError):             # an fp32 tensor 8 GiB out: its int32-elements alias falls in front of the arena
        lay.place("wide32x3", (3, 64), (2 ** 30 + 2 ** 19, 1), 4, [(0, range(3))])
    print("\n" + "\n".join(lay.table()))


@pytest.mark.parametrize("mod,name", ALL_CASES)
def test_every_gpu_layout_is_sound(mod, name):
    lay = mod.CASES[name]().case.layout
    print("\n" + "\n".join(lay.table()))
    assert lay.placements and lay.problems() == []
    regions = np.concatenate([p.regions() for p in lay.placements])
    caught = set()
    for p in lay.placements:
        assert p.base >= F.LEAD and p.base % 16 == 0
        got = claims(p)
        assert got == _expected_claims(p), (p.name, got)
        if p.kind == "near":                        # packed rows H * D apart: in the arena, among NaN, but not far
            assert got == ()
            continue
        assert "int32 bytes" in got, (p.name, got)                                         # every far tensor crosses 2^31 bytes
        assert set(got) >= (set(MODELS) if p.esize <= 2 and p.kind in ("pages", "rows") else set()), (p.name, got)
        caught |= set(got)
        addr = np.array([a.address for a in aliases(p)], dtype=np.int64)                   # the rule, spelt out alias by region
        assert addr.min() >= 0 and addr.max() + p.slab_bytes <= F.ARENA_BYTES, p.name
        inside = (addr[:, None] >= regions[None, :, 0]) & (addr[:, None] < regions[None, :, 1])
        assert not inside.any(), (p.name, int(addr[inside.any(axis=1)][0]))
    r = regions[np.argsort(regions[:, 0])]
    assert (r[1:, 0] >= r[:-1, 1]).all() and r[0, 0] >= F.LEAD and r[:, 1].max() <= F.ARENA_BYTES
    # a case catches both byte models, and the signed element model where a 1- or 2-byte tensor is far.  One exception: two K/V heads
    # under the persistent kernel, whose largest admitted stride stays below 2^32 bytes
    assert set(BYTES) <= caught or name == "fwd-45-narrow-head", caught
    if any(p.esize <= 2 and p.kind != "near" for p in lay.placements):
        assert "int32 elements" in caught, caught


def test_a_layout_with_a_tensor_on_anothers_alias_is_refused():
    lay = Layout(wrap=W)
    a = lay.place("a", (3, 64), (F.stride_bytes("wide", W) // 2, 1), 2, [(0, range(3))])
    bad = F.Placement("b", a.base + (1 << (W - 11)) - 16, 2, (1, 64), (64, 1), ((0, (0,)),), "", W)   # across a's uint32-bytes alias
    assert any("alias of a" in s for s in lay.problems(bad))
    assert any("overlap" in s for s in lay.problems(a.moved(a.base + 64)))
    assert lay.problems(bad.moved(a.base + 1024)) == []


def test_untouched_on_a_host_arena():
    arena = F.make_arena("cpu", 1 << 16)
    regions = [(1001, 1100), (5000, 5003), (1100, 1200)]
    arena[1001:1200] = 7
    arena[5000:5003] = 0
    F.untouched(arena, regions, chunk=4096)
    for at in (0, 7, 1000, 1200, 4095, 4096, 4999, 5003, 40001, (1 << 16) - 1):
        arena[at] = 0xFE
        with pytest.raises(AssertionError, match=f"byte {at} of the arena"):
            F.untouched(arena, regions, chunk=4096)
        arena[at] = F.FILL
    arena[300], arena[9000] = 1, 2
    with pytest.raises(AssertionError, match="byte 300 of the arena"):          # the first offender
        F.untouched(arena, regions, chunk=4096)


def test_data_goes_through_the_far_view_and_comes_back():
    arena = F.make_arena("cpu", F.arena_bytes(W))
    case = FarCase(wrap=W)
    x = torch.randn(3, 4, 2, 8).to(torch.bfloat16).permute(0, 2, 1, 3)          # a [B,H,S,D] view of a [B,S,H,D] array
    ids = cache_cases.page_ids(4)
    pool = torch.randn(4, 2, 2, 4).to(torch.float16)
    case.put("x", x, "wide")
    case.put_at("pool", pool, case.layout.pages("pool", 2 ** 18 + 64, (2, 2, 4), 2, ids))
    case.put("y", x, "narrow", role="out")
    views = case.upload(arena)
    assert views["x"].stride(0) == F.stride_bytes("wide", W) // 2 and torch.equal(F.bits(views["x"]), F.bits(x))
    assert all(torch.equal(F.bits(views["pool"][pid]), F.bits(pool[n])) for n, pid in enumerate(ids))
    assert bool(torch.isnan(views["pool"][5]).all()) and bool(torch.isnan(views["y"]).all())      # the fill reads as NaN
    assert bool((arena.view(torch.int32)[:8] == -1).all()) and bool(torch.isnan(arena.view(torch.float32)[:8]).all())
    assert bool(torch.isnan(arena.view(torch.float8_e4m3fn)[:8].float()).all())
    views["y"].copy_(x)
    got = case.finish(arena)
    assert torch.equal(F.bits(got["y"]), F.bits(x)) and bool((arena == F.FILL).all())
    near = case.near_inputs("cpu")
    assert near["x"].stride() == x.stride() and torch.equal(near["x"], x) and bool(torch.isnan(near["y"]).all())


def _standin(kind, B, read_model=None, write_model=None, esize=2):
    """One far run of the stand-in copy kernel x -> y on a host arena -> the AssertionError that caught it, or None."""
    arena = F.make_arena("cpu", F.arena_bytes(W))
    case = FarCase(wrap=W)
    dtype = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[esize]
    x = torch.randint(0, 100, (B, 2, 4, 8), generator=torch.Generator().manual_seed(B)).to(dtype)
    if kind == "pages":
        ids = cache_cases.page_ids(B)
        x = x[:, :, 0].contiguous()                  # 32-byte pages: 2^18 of them are 2 x 2^W bytes, as 32 KiB pages are at W = 32
        for name, role in (("x", "in"), ("y", "out")):
            case.put_at(name, x, case.layout.pages(name, cache_cases.NUM_PAGES, (2, 8), esize, ids), role)
    else:
        case.put("x", x, kind)
        case.put("y", x, kind, role="out")
    case.upload(arena)
    assert all(set(claims(p)) >= {m for m in (read_model, write_model) if m} for p in case.place.values()), "the placement does not claim the model"
    F.standin_copy(arena.numpy(), case.place["x"], case.place["y"], read_model, write_model)
    try:
        got = case.finish(arena)                     # (e): nothing written elsewhere, no input changed
        assert torch.equal(F.bits(got["y"]), F.bits(x)), "y: the far run's bits differ from the near run's"          # (c)
    except AssertionError as e:
        return e
    return None


PLACED = [("wide", 3, 2), ("narrow", 5, 2), ("u32max", 3, 2), ("pages", 9, 2), ("wide", 2, 1), ("wide", 2, 4)]


@pytest.mark.parametrize("kind,B,esize", PLACED)
def test_the_honest_standin_passes(kind, B, esize):
    assert _standin(kind, B, esize=esize) is None


@pytest.mark.parametrize("side", ["read", "write"])
@pytest.mark.parametrize("model", MODELS)
def test_each_truncating_standin_is_caught(model, side):
    """On every placement that claims the model; the wide 16-bit placement claims all four."""
    hit = 0
    for kind, B, esize in PLACED:
        lay = Layout(wrap=W)
        probe = lay.like("p", torch.empty((B, 2, 4, 8), dtype={1: torch.uint8, 2: torch.int16, 4: torch.int32}[esize]), kind) if kind != "pages" else \
            lay.pages("p", cache_cases.NUM_PAGES, (2, 8), esize, cache_cases.page_ids(B))
        if model not in claims(probe):
            assert (kind, esize) != ("wide", 2) and (kind, esize) != ("pages", 2)
            continue
        err = _standin(kind, B, esize=esize, **{f"{side}_model": model})
        assert err is not None, f"{kind} x {B}, {esize}-byte: the {side} side truncated as {model} went unnoticed"
        assert ("differ" in str(err)) if side == "read" else ("holds" in str(err) or "differ" in str(err)), str(err)
        hit += 1
    assert hit >= 3


def test_blocks_records_what_capi_makes():
    made = _capi.make_cache_ext(window=3)
    with F.Blocks() as b:
        a = _capi.make_decode_args(B=2, q=0x1000, q_stride_b=2 ** 40)
        e = _capi.make_cache_ext(window=5)
    assert b.of("PfaFa3DecodeArgs") is a and b.of("PfaFa3CacheExt") is e and b.of("PfaFa3Sinks") is None and made not in b.made
    assert _capi._make is b._make                   # the spy is gone
    view = torch.as_strided(torch.empty(4096, dtype=torch.bfloat16), (2, 4, 3, 8), (2048, 8, 32, 1))
    a.q, a.q_stride_b, a.q_stride_h, a.q_stride_s = view.data_ptr(), 2048, 8, 32
    F.saw_view(a, "q", view)
    a.q_stride_b = 1024
    with pytest.raises(AssertionError):
        F.saw_view(a, "q", view)

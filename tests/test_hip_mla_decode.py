"""GPU tests of the MLA decode over a latent KV cache (``ops.mla_decode`` -> ``pfa_mla_decode``; csrc/fa3_mla_decode_kernel.h).

The fp64 reference and the bounds -- per element for a 16-bit output, 1e-3 for an fp32 output, 2e-3 on the LSE with exact -inf rows --
are tests/kvcache_testlib.py's, on K = the latent rows at width 576 and V = their first 512 columns as the one K/V head.  The shapes are
the smallest that reach every edge of this kernel: a wave tile is 16 keys, a round of the four waves 64, a split boundary a multiple of
64; H 8 is a padded row block, H 24 with Sq 2 a block that spans two query positions, H 128 eight and sixteen row blocks, siblings 8
workgroup ids apart; with B 10 the plan cuts Smax 1024 into four splits (partials + combine) and leaves Smax 128 one split (the direct
epilogue).  The scale is DeepSeek's (128 + 64)^-0.5.  Every case fails on a library without the kernel, where ``ops.mla_decode`` does not
exist."""

from __future__ import annotations

import pytest
import torch

from kvcache_testlib import capture, check_lse, check_out, device, gen, guard, i32, reference, scatter
from photonic_flash_attention_amd import _capi_mla, ops

pytestmark = pytest.mark.gpu

BF, FP, F32 = torch.bfloat16, torch.float16, torch.float32
SCALE = 192 ** -0.5
LENS = (0, 1, 15, 16, 17, 64, 65, 257, 1000, 1024)          # one ragged batch: empty, below / at / past a tile, a wave round, a split


def _problem(B, H, Sq, Smax, dtype, seed):
    """q as a [B,H,Sq,576] view of a [B,Sq,H,576] buffer and a contiguous latent cache [B,Smax,576], drawn on the device."""
    g = gen(seed)
    q = torch.randn(B, Sq, H, 576, generator=g, device=device()).to(dtype).permute(0, 2, 1, 3)
    return q, torch.randn(B, Smax, 576, generator=g, device=device()).to(dtype)


def _guarded(kv, lens):
    return guard(kv[:, None], kv[:, None], lens)[0][:, 0]


def _name(q, kv, lens, table=None):
    a, _, _, keep = ops._mla_call_args(q, kv, i32(lens), SCALE, True, table, None, None)
    a.workspace, a.workspace_bytes = 0x1000, 1 << 40
    return _capi_mla.describe_mla_decode(a)[0]


def _check(o, lse, q, kv, lens, what, causal=True):
    ro, rlse, pn = reference(q, kv[:, None], kv[:, None, :, :512], seqlens=i32(lens), causal=causal, scale=SCALE)
    check_out(o, ro, pn, float(kv.abs().max()), q.dtype, what)
    check_lse(o, lse, rlse, what)


def _run_and_check(q, kv, lens, what, **kw):
    o, lse = ops.mla_decode(q, _guarded(kv, lens), cache_seqlens=i32(lens), softmax_scale=SCALE, return_lse=True, **kw)
    torch.cuda.synchronize()
    assert o.shape == q.shape[:3] + (512,) and o.dtype == kw.get("out_dtype", q.dtype)
    _check(o, lse, q, kv, lens, what, kw.get("causal", True))


@pytest.mark.parametrize("Smax", [1024, 128])
@pytest.mark.parametrize("Sq", [1, 2])
@pytest.mark.parametrize("H", [8, 16, 24, 128])
@pytest.mark.parametrize("dtype", [BF, FP], ids=["bf16", "fp16"])
def test_against_fp64_on_a_ragged_batch(dtype, H, Sq, Smax):
    lens = [min(n, Smax) for n in LENS]
    q, kv = _problem(len(lens), H, Sq, Smax, dtype, seed=H + Sq + Smax)
    assert _name(q, kv, lens) == f"mla_decode_{'bf16' if dtype == BF else 'fp16'}_o16" + ("+combine" if Smax == 1024 else "")
    _run_and_check(q, kv, lens, f"mla H {H} Sq {Sq} Smax {Smax}")


@pytest.mark.parametrize("kw", [dict(out_dtype=F32), dict(causal=False)], ids=["o32", "not-causal"])
@pytest.mark.parametrize("Smax", [1024, 128])
def test_fp32_output_and_no_causal_cut(Smax, kw):
    lens = [min(n, Smax) for n in LENS]
    q, kv = _problem(len(lens), 16, 2, Smax, BF, seed=Smax + 1)
    _run_and_check(q, kv, lens, f"mla {kw}", **kw)


@pytest.mark.parametrize("page", [64, 256])
def test_paged_equals_contiguous_bit_for_bit(page):
    """Pages in a random order with page 0 unnamed (a clamped -1 would land there) and NaN in every page no table entry names."""
    lens = list(LENS)
    q, kv = _problem(len(lens), 24, 2, 1024, BF, seed=page)
    kn = _guarded(kv, lens)
    kp, _, table = scatter(kn[:, None], kn[:, None], page, seed=page + 1, first=1)
    kw = dict(cache_seqlens=i32(lens), softmax_scale=SCALE, return_lse=True)
    assert _name(q, kp[:, 0], lens, table) == "mla_decode_bf16_o16+combine_paged"
    oc, lc = ops.mla_decode(q, kn, **kw)
    op, lp = ops.mla_decode(q, kp[:, 0], block_table=table, **kw)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(op).all()) and bool(torch.isfinite(oc).all()), "a key or a page the call must never read was read"
    assert torch.equal(op, oc) and torch.equal(lp, lc)
    _check(op, lp, q, kv, lens, f"mla paged {page}")


def test_two_runs_are_bit_equal():
    q, kv = _problem(2, 128, 1, 4096, BF, seed=3)
    kw = dict(cache_seqlens=i32([4096, 2500]), softmax_scale=SCALE, return_lse=True)
    o1, l1 = ops.mla_decode(q, kv, **kw)
    o2, l2 = ops.mla_decode(q, kv, **kw)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(o1).all()) and torch.equal(o1, o2) and torch.equal(l1, l2)


def test_a_captured_paged_step_replays_after_lengths_table_and_cache_changed():
    q, kv = _problem(3, 24, 2, 1024, BF, seed=6)
    kp, _, table = scatter(kv[:, None], kv[:, None], 64, seed=7)
    sl = i32([1024, 300, 65])
    step = lambda: ops.mla_decode(q, kp[:, 0], cache_seqlens=sl, block_table=table, softmax_scale=SCALE, return_lse=True)     # noqa: E731
    graph, (o, lse) = capture(step)
    for n, new_lens in enumerate(([17, 1000, 640], [1024, 16, 257])):
        sl.copy_(i32(new_lens))
        kv2 = torch.randn(kv.shape, generator=gen(60 + n), device=q.device).to(kv.dtype)
        kp2, _, table2 = scatter(kv2[:, None], kv2[:, None], 64, seed=70 + n)
        kp.copy_(kp2), table.copy_(table2)
        graph.replay()
        torch.cuda.synchronize()
        oe, le = step()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(o).all()) and torch.equal(o, oe) and torch.equal(lse, le), f"replay {n}"
        _check(o, lse, q, kv2, new_lens, f"mla replay {n}")

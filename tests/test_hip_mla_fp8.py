"""GPU tests of the latent cache of a serving step: ``ops.mla_decode`` over an FP8 (e4m3fn) cache (``pfa_mla_decode_q8``;
csrc/fa3_mla_decode_fp8_kernel.h) and ``ops.mla_append`` (``pfa_mla_append``; csrc/mla_append_kernel.h).

The shapes are tests/test_hip_mla_decode.py's, the smallest that reach every edge of the tile, the wave round, the split and the row
block.  Against fp64 the reference runs on the exactly dequantised cache with tests/kvcache_testlib.py's bounds: the quantisation is in
the reference's input, not in the error.  With descales that are powers of two the FP8 call must return the bits of the 16-bit call on
the dequantised cache.  The append must leave the bytes the CPU model leaves.  Every case fails on a library without the feature,
where ``ops.mla_append`` does not exist and ``ops.mla_decode`` refuses a ``float8_e4m3fn`` cache."""

from __future__ import annotations

import pytest
import torch

from kvcache_testlib import FP8, NANB, b8, capture, check_lse, check_out, dequant, device, gen, i32, poisoned, quant, reference, scatter_fp8
from photonic_flash_attention_amd import _capi_mla_cache, ops

pytestmark = pytest.mark.gpu

BF, FP, F32 = torch.bfloat16, torch.float16, torch.float32
SCALE = 192 ** -0.5
LENS = (0, 1, 15, 16, 17, 64, 65, 257, 1000, 1024)          # one ragged batch: empty, below / at / past a tile, a wave round, a split


def _q(B, H, Sq, dtype, seed, mul=1.0):
    return (torch.randn(B, Sq, H, 576, generator=gen(seed), device=device()) * mul).to(dtype).permute(0, 2, 1, 3)


def _absmax_cache(B, Smax, seed):
    """A latent cache whose sequences differ in magnitude, quantised with per-sequence absmax descales -> (FP8 [B,Smax,576], descale [B])."""
    kv = torch.randn(B, Smax, 576, generator=gen(seed), device=device()) * torch.linspace(0.3, 5.0, B, device=device())[:, None, None]
    d = kv.abs().amax(dim=(1, 2)) / 448
    return quant(kv[:, None], d[:, None])[:, 0], d


@pytest.mark.parametrize("Smax", [1024, 128])
@pytest.mark.parametrize("Sq", [1, 2])
@pytest.mark.parametrize("H", [16, 24])
@pytest.mark.parametrize("dtype", [BF, FP], ids=["bf16", "fp16"])
def test_against_fp64_on_the_dequantised_cache(dtype, H, Sq, Smax):
    lens = [min(n, Smax) for n in LENS]
    q = _q(len(lens), H, Sq, dtype, seed=H + Sq + Smax)
    kv8, d = _absmax_cache(len(lens), Smax, seed=Smax + H)
    a = ops._mla_call_args(q, kv8, i32(lens), SCALE, True, None, None, None, True)[0]
    a.workspace, a.workspace_bytes = 0x1000, 1 << 40
    name = _capi_mla_cache.describe_mla_decode_q8(a, ops._mla_kv_quant_arg("t", kv8, d, len(lens), q.device))[0]
    assert name == f"mla_decode_q8_{'bf16' if dtype == BF else 'fp16'}_o16" + ("+combine" if Smax == 1024 else "")
    o, lse = ops.mla_decode(q, poisoned(kv8[:, None], lens)[:, 0], cache_seqlens=i32(lens), softmax_scale=SCALE, return_lse=True, kv_descale=d)
    torch.cuda.synchronize()
    kv64 = dequant(kv8[:, None], d[:, None], torch.float64)
    ro, rlse, pn = reference(q, kv64, kv64[..., :512], seqlens=i32(lens), scale=SCALE)
    assert o.shape == q.shape[:3] + (512,) and o.dtype == dtype
    check_out(o, ro, pn, float(kv64.abs().max()), dtype, f"mla fp8 H {H} Sq {Sq} Smax {Smax}")
    check_lse(o, lse, rlse, "mla fp8")


def _code_cache(B, Smax, seed):
    """FP8 bytes [B,Smax,576]: random finite codes of moderate size, and in sequence B - 1 rows that enumerate all 254 finite e4m3fn
    codes in the first 512 columns and, over 254 rows, in the last 64."""
    kv8 = quant(torch.randn(B, 1, Smax, 576, generator=gen(seed), device=device()), torch.full((B, 1), 1 / 16, device=device()))[:, 0]
    codes = torch.tensor([c for c in range(256) if c & 0x7f != 0x7f], dtype=torch.uint8, device=device())
    b8(kv8)[B - 1] = codes[(torch.arange(Smax, device=device())[:, None] + torch.arange(576, device=device())[None]) % 254]
    return kv8


@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
@pytest.mark.parametrize("out_dtype", [None, F32], ids=["o16", "o32"])
@pytest.mark.parametrize("dtype", [BF, FP], ids=["bf16", "fp16"])
def test_power_of_two_descales_return_the_16_bit_kernels_bits(dtype, out_dtype, paged):
    lens = list(LENS)
    q = _q(len(lens), 24, 2, dtype, seed=21, mul=1 / 16)
    kv8 = poisoned(_code_cache(len(lens), 1024, seed=22)[:, None], lens)[:, 0]
    d = torch.tensor([1.0, 0.5, 4.0], device=q.device)[torch.arange(len(lens), device=q.device) % 3]
    kw = dict(cache_seqlens=i32(lens), softmax_scale=SCALE, return_lse=True, out_dtype=out_dtype)
    o16, l16 = ops.mla_decode(q, dequant(kv8[:, None], d[:, None], dtype)[:, 0], **kw)
    if paged:                                    # pages of 64 in a random order; page 0, where a clamped id lands, is NaN bytes
        kp, _, table = scatter_fp8(kv8[:, None], kv8[:, None], 64, 23, lens)
        o8, l8 = ops.mla_decode(q, kp[:, 0], block_table=table, kv_descale=d, **kw)
    else:
        o8, l8 = ops.mla_decode(q, kv8, kv_descale=d, **kw)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(o8).all()) and float(o8.abs().max()) > 0, "a key the call must never read was read"
    assert torch.equal(o8, o16) and torch.equal(l8, l16)


def test_paged_equals_contiguous_and_two_runs_are_bit_equal():
    lens = list(LENS)
    q = _q(len(lens), 24, 2, BF, seed=31)
    kv8, d = _absmax_cache(len(lens), 1024, seed=32)
    kn = poisoned(kv8[:, None], lens)
    kp, _, table = scatter_fp8(kn, kn, 64, 33, lens)
    kw = dict(cache_seqlens=i32(lens), softmax_scale=SCALE, return_lse=True, kv_descale=d)
    oc, lc = ops.mla_decode(q, kn[:, 0], **kw)
    oc2, lc2 = ops.mla_decode(q, kn[:, 0], **kw)
    op, lp = ops.mla_decode(q, kp[:, 0], block_table=table, **kw)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(op).all()) and bool(torch.isfinite(oc).all()), "a key or a page the call must never read was read"
    assert torch.equal(oc, oc2) and torch.equal(lc, lc2) and torch.equal(op, oc) and torch.equal(lp, lc)


@pytest.mark.parametrize("ragged", [False, True], ids=["uniform", "ragged"])
@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
@pytest.mark.parametrize("fp8", [False, True], ids=["16-bit", "fp8"])
def test_append_leaves_the_bytes_of_the_cpu_model(fp8, paged, ragged):
    """kv_c and k_pe are column slices of one [.., 576] buffer (strided sources); sequence 1 has len_b < Sq_b (rows dropped in front);
    paged, sequence 0's last page id lies outside the pool (rows dropped); the cache starts as a canary that every other row keeps."""
    B, Smax, page, dev = 4, 256, 64, device()
    if ragged:
        cu, lens, msq = [0, 40, 45, 45, 70], [200, 2, 9, 65], 40      # sequence 0: keys 160 .. 199, of which 192 .. 199 lie in the last page
        rows = torch.randn(70, 576, generator=gen(41), device=dev).to(BF)
    else:
        cu, lens, msq = None, [194, 2, 0, 65], 3                      # sequence 0: keys 191 .. 193
        rows = torch.randn(B, 3, 576, generator=gen(42), device=dev).to(BF)
    rows[..., 7] = float("nan")                                   # NaN stays NaN through the quantising store
    d = torch.tensor([0.5, 0.013, 1.7, 0.3], device=dev) if fp8 else None
    shape = (B * 4 + 1, page, 576) if paged else (B, Smax, 576)
    cache = torch.full(shape, 0x55, dtype=torch.uint8, device=dev).view(FP8) if fp8 else torch.full(shape, -7.0, dtype=BF, device=dev)
    table = None
    if paged:
        table = (torch.randperm(B * 4, generator=torch.Generator().manual_seed(43)).to(torch.int32) + 1).reshape(B, 4).to(dev)
        table[0, 3] = B * 4 + 1
    kw = dict(cache_seqlens=i32(lens), cu_seqlens_q=None if cu is None else i32(cu), max_seqlen_q=msq if ragged else None)
    cpu = lambda t: None if t is None else t.cpu()                # noqa: E731
    bits = torch.uint8 if fp8 else torch.int16
    canary = cache.cpu().view(bits)
    want = canary.clone().view(cache.dtype)
    ops.mla_append(rows[..., :512].cpu(), rows[..., 512:].cpu(), want, block_table=cpu(table), kv_descale=cpu(d),
                   **{k: cpu(v) if torch.is_tensor(v) else v for k, v in kw.items()})
    ops.mla_append(rows[..., :512], rows[..., 512:], cache, block_table=table, kv_descale=d, **kw)
    torch.cuda.synchronize()
    assert not torch.equal(want.view(bits), canary) and torch.equal(cache.cpu().view(bits), want.view(bits))


def test_a_captured_append_and_decode_step_replays_after_everything_changed():
    B, H, Sq, page, dev = 3, 16, 2, 64, device()
    q = _q(B, H, Sq, BF, seed=51)
    kv8, d0 = _absmax_cache(B, 1024, seed=52)
    pool, _, table = scatter_fp8(kv8[:, None], kv8[:, None], page, 53, [1024] * B)
    pool, d, sl = pool[:, 0], d0.clone(), i32([1024, 300, 65])
    new = torch.randn(B, Sq, 576, generator=gen(54), device=dev).to(BF)

    def step():
        ops.mla_append(new[..., :512], new[..., 512:], pool, cache_seqlens=sl, block_table=table, kv_descale=d)
        return ops.mla_decode(q, pool, cache_seqlens=sl, block_table=table, softmax_scale=SCALE, return_lse=True, kv_descale=d)
    graph, (o, lse) = capture(step)
    for n, new_lens in enumerate(([17, 1000, 640], [1024, 2, 257])):
        kv2, d2 = _absmax_cache(B, 1024, seed=60 + n)
        pool2, _, table2 = scatter_fp8(kv2[:, None], kv2[:, None], page, 70 + n, [1024] * B)
        sl.copy_(i32(new_lens)), d.copy_(d2 * (1.5 + n)), table.copy_(table2)
        new.copy_(torch.randn(new.shape, generator=gen(80 + n), device=dev).to(BF))
        b8(pool).copy_(b8(pool2[:, 0]))
        graph.replay()
        torch.cuda.synchronize()
        got = (o.clone(), lse.clone(), b8(pool).clone())
        b8(pool).copy_(b8(pool2[:, 0]))
        oe, le = step()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(got[0]).all()) and torch.equal(got[0], oe) and torch.equal(got[1], le), f"replay {n}"
        assert torch.equal(got[2], b8(pool)) and not torch.equal(got[2], b8(pool2[:, 0])), f"replay {n}: the appended rows"

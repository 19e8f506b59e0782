"""GPU tests of the FP8 (e4m3fn) KV cache: ``ops.fa3_decode`` over ``torch.float8_e4m3fn`` caches (``pfa_fa3_decode_q8``) and the quantising
``ops.kv_append`` (``pfa_kv_append_q8``).

1. The code-to-value decode itself, exactly: sequences of one key, so that softmax is 1 and O is the V row -- all 254 finite codes
   times the descale -- and one-hot query rows whose LSE is the K code they are aimed at times ``k_descale * softmax_scale``.
2. Against the fp64 reference on the DEQUANTISED cache (``kvcache_testlib``'s reference and bounds; quantisation error is not in them).
3. Paged = contiguous, and run = run, bit for bit, with NaN bytes wherever the call must not read.
4. With all descales 1, the bits of the 16-bit kernel on the converted cache (the 8-byte K load keeps its element-to-k-step mapping).
5. The quantising append against its plain-torch model, byte for byte.
6. Append + decode captured once and replayed after lengths, table, rows and descale contents changed.
7. ``PagedKVCache`` in FP8.

Quantised tensors are made on the CPU (``ops.quantize_kv``) and moved as bytes, so the tests do not lean on device-side casts."""

from __future__ import annotations

import pytest
import torch

from kvcache_testlib import (FP8, NANB, b8, both, capture, check_lse, check_out, dequant, device, i32, poisoned, problem, quant, reference,
                             scatter, scatter_fp8)
from photonic_flash_attention_amd import ops

pytestmark = pytest.mark.gpu

LENS = [1000, 37, 0, 513]


# --- 1. the decode table, exactly ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("paged", [False, True])
@pytest.mark.parametrize("D, Hkv", [(128, 2), (64, 4)])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_every_code_decodes_to_its_value(dtype, D, Hkv, paged):
    """One key per sequence, causal=False, fp32 output: P is exactly 1 (hi = 1, lo = 0).  The key's K and V rows hold, over the Hkv
    heads, all 256 codes (the two NaN codes replaced by 0).  O must be the V row times v_descale; row (i, h) is one-hot at a
    dimension of its own, so its LSE is that K code times k_descale * softmax_scale."""
    dev = device()
    H, Sq, G = 4, 64, 4 // Hkv
    codes = torch.arange(Hkv * D, dtype=torch.uint8)
    codes[(codes & 0x7f) == 0x7f] = 0
    assert Hkv * D == 256 and len(set(codes.tolist())) == 254
    row = codes.reshape(Hkv, D)
    vals = row.view(FP8).double()                                                # the CPU cast: the table a decode is checked against
    assert float(vals.max()) == 448.0 and float(vals.min()) == -448.0
    k8 = torch.full((1, Hkv, 64, D), NANB, dtype=torch.uint8)
    k8[0, :, 0] = row
    k8 = k8.to(dev).view(FP8)
    v8 = k8.clone()
    # row (i, h): with g = h % G its dimension is (i * G + g) % D -- the Sq * G rows of a K/V head cover its D dimensions
    q = torch.zeros(1, H, Sq, D)
    aim = torch.empty(H, Sq, dtype=torch.int64)
    for h in range(H):
        for i in range(Sq):
            aim[h, i] = (i * G + h % G) % D
            q[0, h, i, aim[h, i]] = 1.0
    assert all(len(set(aim[kv * G:(kv + 1) * G].flatten().tolist())) == D for kv in range(Hkv))
    q = q.to(dev, dtype)
    lens = i32([1])
    kw = {}
    if paged:
        pool = torch.full((3, Hkv, 64, D), NANB, dtype=torch.uint8, device=dev)
        pool[2] = b8(k8)[0]
        k8 = pool.view(FP8)
        v8 = k8.clone()
        kw["block_table"] = i32([[2]])
    scale = D ** -0.5
    for kd, vd in ((torch.tensor([0.5, 2.0, 1.0, 0.125][:Hkv]), torch.tensor([2.0, 0.25, 1.0, 8.0][:Hkv])),
                   (torch.tensor([0.3, 1.7, 0.011, 0.9][:Hkv]), torch.tensor([1.3, 0.7, 0.37, 0.0021][:Hkv]))):
        o, lse = ops.fa3_decode(q, k8, v8, cache_seqlens=lens, causal=False, out_dtype=torch.float32, return_lse=True,
                                k_descale=kd.to(dev), v_descale=vd.to(dev), **kw)
        torch.cuda.synchronize()
        o, lse = o.cpu(), lse.cpu()
        pow2 = bool((torch.frexp(vd)[0] == 0.5).all())
        for h in range(H):
            kv = h // G
            want = vals[kv] * vd[kv].double()                                    # exact in fp64
            got = o[0, h].double()                                               # [Sq, D]: every row is the V row
            if pow2:
                assert torch.equal(got, want[None].expand(Sq, D)), (h, "O is not code * v_descale")
            else:
                err = (got - want[None]).abs()
                assert bool((err <= want.abs()[None] * 2.0 ** -24).all()), (h, float(err.max()))              # one fp32 rounding
            code = vals[kv][aim[h]]                                              # the K code each row is aimed at
            want_lse = code * kd[kv].double() * scale
            zero = code == 0
            if bool(zero.any()):                                                 # rows aimed at code 0: compared absolutely
                assert float(lse[0, h][zero].abs().max()) <= 1e-6, h
            rel = ((lse[0, h].double() - want_lse)[~zero] / want_lse[~zero]).abs()
            assert float(rel.max()) <= 1e-3, (h, float(rel.max()))


# --- 2. against fp64 on the dequantised cache ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_against_fp64_on_the_dequantised_cache(dtype, D):
    dev = device()
    B, H, Hkv, Smax = 4, 8, 2, 1024                                              # 4 splits
    q5, k, v = problem(B, H, Hkv, 5, Smax, D, dtype, 11 + D)
    kd_h, vd_h = torch.tensor([0.011, 0.0173], device=dev), torch.tensor([0.013, 0.0091], device=dev)
    per_b = torch.tensor([[1.0], [0.37], [2.9], [1.21]], device=dev)
    k8, v8 = quant(k, kd_h), quant(v, vd_h)
    k8n, v8n = poisoned(k8, LENS), poisoned(v8, LENS)
    lens = i32(LENS)
    km = torch.rand(B, Smax, generator=torch.Generator().manual_seed(5)).to(dev) < 0.7
    km[0, :3] = False
    for kd, vd in ((kd_h, vd_h), ((kd_h[None] * per_b).contiguous(), (vd_h[None] / per_b).contiguous())):
        kf, vf = dequant(k8, kd, torch.float64), dequant(v8, vd, torch.float64)
        vmax = float(vf.abs().max())
        for Sq in (1, 5):
            q = q5[:, :, :Sq]
            for causal in (True, False):
                for mask in (None, km):
                    ref_o, ref_lse, pnorm = reference(q, kf, vf, seqlens=lens, key_mask=mask, causal=causal)
                    for odt in (dtype, torch.float32):
                        what = f"{dtype} D{D} Sq{Sq} causal={causal} mask={mask is not None} descale{tuple(kd.shape)} out={odt}"
                        o, lse = ops.fa3_decode(q, k8n, v8n, cache_seqlens=lens, key_mask=mask, causal=causal, out_dtype=odt, return_lse=True,
                                                k_descale=kd, v_descale=vd)
                        torch.cuda.synchronize()
                        assert o.dtype == odt and o.shape == q.shape
                        check_out(o, ref_o, pnorm, vmax, dtype, what)
                        check_lse(o, lse, ref_lse, what)


# --- 3. paged = contiguous, run = run, bit for bit -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("page", [64, 256])
@pytest.mark.parametrize("dtype, D", [(torch.bfloat16, 128), (torch.float16, 64)])
def test_paged_equals_contiguous_bit_for_bit(dtype, D, page):
    dev = device()
    B, H, Hkv, Smax = 4, 8, 2, 1024
    q, k, v = problem(B, H, Hkv, 5, Smax, D, dtype, 21 + D)
    kd, vd = torch.tensor([0.011, 0.0173], device=dev), torch.tensor([0.013, 0.0091], device=dev)
    k8n, v8n = poisoned(quant(k, kd), LENS), poisoned(quant(v, vd), LENS)
    kp, vp, table = scatter_fp8(k8n, v8n, page, 7 + page, LENS)
    assert bool((b8(kp)[0] == NANB).all()) and kp.stride(1) != kp.shape[2] * D    # page 0 is NaN; the flash-attn pool layout
    lens = i32(LENS)
    for odt in (dtype, torch.float32):
        for causal in (True, False):
            kw = dict(cache_seqlens=lens, causal=causal, out_dtype=odt, return_lse=True, k_descale=kd, v_descale=vd)
            op, lp = both(ops.fa3_decode, q, k8n, v8n, kp, vp, table, **kw)
            op2, lp2 = ops.fa3_decode(q, kp, vp, block_table=table, **kw)
            torch.cuda.synchronize()
            assert torch.equal(op, op2) and torch.equal(lp, lp2), (odt, causal)


# --- 4. the bits of the 16-bit kernel ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("paged", [False, True])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_descales_of_one_give_the_bits_of_the_16_bit_kernel(dtype, D, paged):
    dev = device()
    B, H, Hkv, Smax = 4, 8, 2, 1024
    q, k, v = problem(B, H, Hkv, 5, Smax, D, dtype, 31 + D)
    one = torch.ones(Hkv, device=dev)
    k8, v8 = quant(k * 40, one), quant(v * 40, one)                              # codes over the whole range, saturated ones among them
    k16, v16 = dequant(k8, one, dtype), dequant(v8, one, dtype)                  # = k8.to(dtype): every e4m3 value is a value of dtype
    assert torch.equal(k16.double(), dequant(k8, one, torch.float64))
    lens = i32(LENS)
    km = torch.rand(B, Smax, generator=torch.Generator().manual_seed(6)).to(dev) < 0.8
    kw8, kw16 = {}, {}
    if paged:
        k8, v8, table = scatter_fp8(k8, v8, 128, 3, [Smax] * B)
        k16, v16, table16 = scatter(k16, v16, 128, 3)
        kw8["block_table"], kw16["block_table"] = table, table16
    for odt in (dtype, torch.float32):
        for causal, mask, Sq in ((True, None, 5), (False, None, 1), (True, km, 5)):
            kw = dict(cache_seqlens=lens, causal=causal, key_mask=mask, out_dtype=odt, return_lse=True)
            o8, l8 = ops.fa3_decode(q[:, :, :Sq], k8, v8, k_descale=one, v_descale=one, **kw, **kw8)
            o16, l16 = ops.fa3_decode(q[:, :, :Sq], k16, v16, **kw, **kw16)
            torch.cuda.synchronize()
            assert torch.equal(o8, o16) and torch.equal(l8, l16), (odt, causal, mask is not None)


# --- 5. the quantising append ------------------------------------------------------------------------------------------------------------

def _rows(shape, seed, dt):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g) * 3.0
    x.view(-1)[::7] *= 200.0                                                     # far beyond +-448 * descale: saturates
    x.view(-1)[5::31] = float("nan")
    x.view(-1)[11::53] = 0.0
    return x.to(dt)


@pytest.mark.parametrize("D", [32, 128, 256])
@pytest.mark.parametrize("paged", [False, True])
@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_quantising_append_equals_its_model(dt, ragged, paged, D):
    dev = device()
    B, Hkv, Smax, page = 4, 2, 256, 64
    lens = torch.tensor([66, 2, 256, 0], dtype=torch.int32)                     # sequence 1: rows in front of key 0; sequence 3: none at all
    kw = {}
    if ragged:
        kw = dict(cu_seqlens_q=torch.tensor([0, 5, 9, 12, 12], dtype=torch.int32), max_seqlen_q=5)
        kn, vn = _rows((14, Hkv, D), 1, dt), _rows((14, Hkv, D), 2, dt)
    else:
        kn, vn = _rows((B, Hkv, 5, D), 1, dt), _rows((B, Hkv, 5, D), 2, dt)
    if paged:                                                                    # rows 61 .. 65 of sequence 0 straddle pages; 99 and -1: outside the pool
        kw["block_table"] = torch.tensor([[3, 99, 1, 0], [2, 9, 9, 9], [4, 5, -1, 6], [8, 8, 8, 8]], dtype=torch.int32)
        shape = (10, page, Hkv, D)
    else:
        shape = (B, Smax, Hkv, D)
    for kd in (torch.tensor([0.37, 2.5]), torch.tensor([[0.37, 1.0], [2.5, 0.011], [1.0, 1.0], [0.6, 0.7]])):
        vd = (kd * 1.3).contiguous()
        # where rows land: the 16-bit model with marker rows
        mk, mv = torch.zeros(shape, dtype=dt).transpose(1, 2), torch.zeros(shape, dtype=dt).transpose(1, 2)
        ops.kv_append(torch.ones_like(kn), torch.ones_like(vn), mk, mv, cache_seqlens=lens, **kw)
        written = mk == 1
        assert 0 < int(written.sum()) < written.numel()
        # the model on the CPU, the kernel on the device, from NaN-patterned destinations in the flash-attn layout
        want_k = torch.full(shape, NANB, dtype=torch.uint8).view(FP8).transpose(1, 2)
        want_v = torch.full(shape, NANB, dtype=torch.uint8).view(FP8).transpose(1, 2)
        ops.kv_append(kn, vn, want_k, want_v, cache_seqlens=lens, k_descale=kd, v_descale=vd, **kw)
        got_k = torch.full(shape, NANB, dtype=torch.uint8, device=dev).view(FP8).transpose(1, 2)
        got_v = torch.full(shape, NANB, dtype=torch.uint8, device=dev).view(FP8).transpose(1, 2)
        ops.kv_append(kn.to(dev), vn.to(dev), got_k, got_v, cache_seqlens=lens.to(dev), k_descale=kd.to(dev), v_descale=vd.to(dev),
                      **{n: (t.to(dev) if isinstance(t, torch.Tensor) else t) for n, t in kw.items()})
        torch.cuda.synchronize()
        for got, want in ((got_k.cpu(), want_k), (got_v.cpu(), want_v)):
            g, w = b8(got), b8(want)
            assert bool((g[~written] == NANB).all()), "a byte outside the written rows changed"
            gnan, wnan = (g & 0x7f) == 0x7f, (w & 0x7f) == 0x7f
            assert torch.equal(gnan, wnan), "NaN positions differ"
            assert bool(wnan[written].any()) and torch.equal(g[~wnan], w[~wnan])
            fin = want.float()[written & ~wnan]
            assert float(fin.max()) == 448.0 and float(fin.min()) == -448.0      # values beyond the range saturate


# --- 6. graph replay ---------------------------------------------------------------------------------------------------------------------

def test_a_captured_append_and_decode_replays_while_everything_changes():
    dev = device()
    B, H, Hkv, D, page, pages, Sq = 3, 8, 2, 128, 64, 8, 2
    dtype = torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(77)
    NP = B * pages + 2
    pool_k = b8(quant(torch.randn(NP, Hkv, page, D, generator=g, device=dev), torch.tensor([0.02, 0.03]))).clone()
    pool_v = b8(quant(torch.randn(NP, Hkv, page, D, generator=g, device=dev), torch.tensor([0.02, 0.03]))).clone()
    state = dict(q=torch.randn(B, Sq, H, D, generator=g, device=dev).to(dtype).permute(0, 2, 1, 3),
                 kn=torch.randn(B, Sq, Hkv, D, generator=g, device=dev).to(dtype).permute(0, 2, 1, 3),
                 vn=torch.randn(B, Sq, Hkv, D, generator=g, device=dev).to(dtype).permute(0, 2, 1, 3),
                 lens=i32([300, 64, 17]), table=torch.arange(B * pages, dtype=torch.int32, device=dev).reshape(B, pages),
                 kd=torch.tensor([0.02, 0.03], device=dev), vd=torch.tensor([0.025, 0.015], device=dev))

    def step(kp, vp):
        return ops.fa3_decode(state["q"], kp.view(FP8), vp.view(FP8), cache_seqlens=state["lens"], block_table=state["table"],
                              k_new=state["kn"], v_new=state["vn"], return_lse=True, k_descale=state["kd"], v_descale=state["vd"])

    kp, vp = pool_k.clone(), pool_v.clone()
    graph, (o_g, lse_g) = capture(lambda: step(kp, vp))
    for lens, seed in (([300, 64, 17], 1), ([512, 2, 129], 2), ([1, 500, 65], 3)):
        gg = torch.Generator(device=dev).manual_seed(seed)
        kp.copy_(pool_k)
        vp.copy_(pool_v)
        state["lens"].copy_(i32(lens))
        state["table"].copy_(torch.randperm(NP, generator=torch.Generator().manual_seed(seed))[:B * pages].to(torch.int32).reshape(B, pages).to(dev))
        for name in ("q", "kn", "vn"):
            state[name].copy_(torch.randn(state[name].shape, generator=gg, device=dev))
        state["kd"].copy_(torch.tensor([0.02, 0.03], device=dev) * (1 + 0.3 * seed))
        state["vd"].copy_(torch.tensor([0.025, 0.015], device=dev) / (1 + 0.2 * seed))
        graph.replay()
        ke, ve = pool_k.clone(), pool_v.clone()
        o_e, lse_e = step(ke, ve)
        torch.cuda.synchronize()
        assert torch.equal(kp, ke) and torch.equal(vp, ve) and not torch.equal(kp, pool_k), lens
        assert bool(torch.isfinite(o_e).all()) and torch.equal(o_g, o_e) and torch.equal(lse_g, lse_e), lens


# --- 7. PagedKVCache in FP8 ---------------------------------------------------------------------------------------------------------------

def test_paged_cache_in_fp8():
    from photonic_flash_attention_amd.integration.pytorch import PagedKVCache
    dev = device()
    H, Hkv, D, dtype = 8, 2, 128, torch.bfloat16
    kd, vd = torch.tensor([0.021, 0.017], device=dev), torch.tensor([0.013, 0.019], device=dev)
    c = PagedKVCache(num_pages=12, page_size=64, Hkv=Hkv, D=D, dtype=FP8, device=dev, max_batch=3, max_pages_per_seq=4, copy_on_write=True,
                     k_descale=kd, v_descale=vd)
    g = torch.Generator(device=dev).manual_seed(9)

    def tok(n):
        return tuple(torch.randn(1, Hkv, n, D, generator=g, device=dev).to(dtype) for _ in range(2))

    def check(slots, what):
        """decode over the slots == ops.fa3_decode on the gathered pages, and within the bounds of the dequantised reference."""
        q = torch.randn(len(slots), 1, H, D, generator=g, device=dev).to(dtype).permute(0, 2, 1, 3)
        o, lse = c.decode(q, slots, return_lse=True)
        kc = torch.full((len(slots), Hkv, 256, D), NANB, dtype=torch.uint8, device=dev)
        vc = kc.clone()
        for i, s in enumerate(slots):
            gk, gv = c.gather(s)
            assert gk.dtype == FP8
            kc[i, :, :gk.shape[1]], vc[i, :, :gv.shape[1]] = b8(gk), b8(gv)
        lens = i32([c.length(s) for s in slots])
        o2, lse2 = ops.fa3_decode(q, kc.view(FP8), vc.view(FP8), cache_seqlens=lens, return_lse=True, k_descale=kd, v_descale=vd)
        torch.cuda.synchronize()
        assert torch.equal(o, o2) and torch.equal(lse, lse2), what
        clean_k, clean_v = kc.clone(), vc.clone()
        for i, s in enumerate(slots):
            clean_k[i, :, c.length(s):] = 0
            clean_v[i, :, c.length(s):] = 0
        vf = dequant(clean_v.view(FP8), vd, torch.float64)
        ref_o, ref_lse, pnorm = reference(q, dequant(clean_k.view(FP8), kd, torch.float64), vf, seqlens=lens)
        check_out(o, ref_o, pnorm, float(vf.abs().max()), dtype, what)
        check_lse(o, lse, ref_lse, what)

    s = c.allocate()
    k, v = tok(100)
    c.append(s, k, v)
    assert torch.equal(b8(c.gather(s)[0]).cpu(), b8(ops.quantize_kv(k.cpu().float(), kd.cpu())[0]))        # the append quantises by the rule
    check([s], "append -> decode")
    # fork, then append into the shared, partly filled tail page: it is copied through the 2-byte view
    child = c.fork(s)
    tail = c.pages(s)[1]
    before = b8(c.gather(s)[0]).clone()
    c.append(child, *tok(3))
    assert c.pages(child)[1] != tail and c.page_refcount(tail) == 1
    assert torch.equal(b8(c.gather(child)[0])[:, :100], before) and torch.equal(b8(c.gather(s)[0]), before)
    check([s, child], "fork + append")
    # advance + write_step: the quantising HIP append, behind the pending copy of another fork
    c2 = c.fork(s)
    pk, pv = tok(3)
    c.advance([s, c2], [2, 1])
    rows_k = torch.cat([pk[0, :, :2], pk[0, :, 2:]], dim=1).transpose(0, 1).contiguous()
    rows_v = torch.cat([pv[0, :, :2], pv[0, :, 2:]], dim=1).transpose(0, 1).contiguous()
    c.write_step(rows_k, rows_v, [2, 1], [s, c2])
    want = ops.quantize_kv(pk.cpu().float(), kd.cpu())[0]
    assert torch.equal(b8(c.gather(s)[0])[:, 100:].cpu(), b8(want)[:, :2]) and torch.equal(b8(c.gather(c2)[0])[:, 100:].cpu(), b8(want)[:, 2:])
    assert torch.equal(b8(c.gather(c2)[0])[:, :100], before)
    check([s, child, c2], "advance + write_step")
    # what is not built for an FP8 cache raises
    q = torch.zeros(3, H, 1, D, dtype=dtype, device=dev)
    with pytest.raises(ValueError, match="prefill over an FP8 cache is not built"):
        c.prefill(q)
    with pytest.raises(ValueError, match="prefill_varlen over an FP8 cache is not built"):
        c.prefill_varlen(q[:, :, 0], [1, 0, 0])
    with pytest.raises(ValueError, match="rotary is not fused"):
        c.write_step(rows_k, rows_v, [2, 1], [s, c2], rotary_cos=torch.zeros(8, 64, device=dev), rotary_sin=torch.zeros(8, 64, device=dev))
    for kw in (dict(window=8), dict(tree_mask=torch.ones(3, 1, dtype=torch.int64, device=dev)), dict(shared_prefix=64)):
        with pytest.raises(ValueError, match="is not supported with an FP8"):
            c.decode(q, **kw)

"""GPU tests of the forward over an FP8 (e4m3fn) KV cache: ``ops.fa3_prefill_cache`` and ``ops.fa3_prefill_varlen`` over
``torch.float8_e4m3fn`` caches (``pfa_fa3_prefill_q8``, ``pfa_fa3_prefill_varlen_q8``).

1. The code-to-value decode itself: sequences of one key, all 254 finite codes, one-hot query rows.
2. With all descales 1, the bits of the 16-bit kernel on the converted cache (the LDS images are the same images).
3. Against the fp64 reference on the DEQUANTISED cache (``kvcache_testlib``'s reference and bounds; quantisation error is not in them).
4. Paged = contiguous and run = run, bit for bit, with NaN bytes wherever the call must not read.
5. Ragged = per-sequence uniform calls, bit for bit; rows no sequence covers keep a sentinel.
6. ``k_new=, v_new=``: the quantising append in front of the attention.
7. Append + ragged prefill over ``PagedKVCache.operands`` captured once and replayed while everything changes.
8. Chunked prefill through the class.
9. The refusals, on device tensors: nothing is launched.

Every cache tail and every page no table entry names is filled with the NaN byte 0x7f, and every output is asserted finite.  Quantised
tensors are made on the CPU (``ops.quantize_kv``) and moved as bytes, so the tests do not lean on device-side casts."""

from __future__ import annotations

import pytest
import torch

from kvcache_testlib import (FP8, NANB, b8, both, capture, check_lse, check_out, dequant, device, i32, poisoned, problem, quant, reference,
                             scatter_fp8, to16)
from photonic_flash_attention_amd import ops

pytestmark = pytest.mark.gpu

BOTH = [torch.bfloat16, torch.float16]


# --- 1. the decode table ----------------------------------------------------------------------------------------------------------------

def exact_scale():
    """A softmax_scale whose fp32 product with fp32 log2(e) -- the kernel's scale_log2 -- is exactly 2^-11."""
    import numpy as np
    log2e, x = np.float32(1.4426950408889634), np.float32(2.0 ** -11 / 1.4426950408889634)
    for cand in (x, np.nextafter(x, np.float32(1)), np.nextafter(x, np.float32(0))):
        if np.float32(cand * log2e) == np.float32(2.0 ** -11):
            return float(cand)
    raise AssertionError("no fp32 softmax_scale gives scale_log2 = 2^-11")


def _codes_problem(dtype, D, Hkv, paged):
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
    q = torch.zeros(1, H, Sq, D)
    aim = torch.empty(H, Sq, dtype=torch.int64)
    for h in range(H):
        for i in range(Sq):
            aim[h, i] = (i * G + h % G) % D                                      # the Sq * G rows of a K/V head cover its D dimensions
            q[0, h, i, aim[h, i]] = 1.0
    assert all(len(set(aim[kv * G:(kv + 1) * G].flatten().tolist())) == D for kv in range(Hkv))
    kw = {}
    if paged:
        pool = torch.full((3, Hkv, 64, D), NANB, dtype=torch.uint8, device=dev)
        pool[2] = b8(k8)[0]
        k8 = pool.view(FP8)
        kw["block_table"] = i32([[2]])
    return q.to(dev, dtype), k8, k8.clone(), vals, aim, kw


@pytest.mark.parametrize("paged", [False, True])
@pytest.mark.parametrize("D, Hkv", [(128, 2), (64, 4)])
@pytest.mark.parametrize("dtype", BOTH)
def test_every_code_decodes_to_its_value(dtype, D, Hkv, paged):
    """The construction of test_hip_decode_fp8's test of the same name, through the uniform call at Sq 64 and through the ragged call:
    one key per sequence, causal=False, fp32 output, so that P is exactly 1 (hi = 1, lo = 0).  The key's K and V rows hold, over the
    Hkv heads, all 256 codes (the two NaN codes replaced by 0).  O must be the V row times v_descale -- exactly for power-of-two
    descales, within one fp32 rounding otherwise; row (i, h) is one-hot at a dimension of its own, so its LSE is that K code times
    k_descale * softmax_scale.

    The softmax scale is what makes the premise "P is exactly 1" true in THIS kernel.  Its softmax (the 16-bit kernel's, shared code)
    computes P = exp2(fma(s, c, -fl(m * c))) with c = scale_log2 * k_descale: for the one visible key m = s, and the argument is the
    rounding residual of s * c, not 0.  The scale is chosen so that scale_log2 = 2^-11: with power-of-two descales s * c is exact, and
    with the others |s * c| < 0.5, the residual is below 2^-26 and exp2 of it rounds to 1.  At the default scale 1 / sqrt(D) the
    residual is up to 2^-18, P = 1 + 2e-6, its hi + lo pair carries 16 bits of it and O = V * (hi + lo) / P is off by one ulp:
    measured 1.06e-7 relative, the same bits as the 16-bit kernel gives (the test below pins that instead)."""
    dev = device()
    q, k8, v8, vals, aim, kw = _codes_problem(dtype, D, Hkv, paged)
    H, Sq, G = 4, 64, 4 // Hkv
    lens = i32([1])
    scale = exact_scale()
    for kd, vd in ((torch.tensor([0.5, 2.0, 1.0, 0.125][:Hkv]), torch.tensor([2.0, 0.25, 1.0, 8.0][:Hkv])),
                   (torch.tensor([0.3, 1.7, 0.011, 0.9][:Hkv]), torch.tensor([1.3, 0.7, 0.37, 0.0021][:Hkv]))):
        kw2 = dict(cache_seqlens=lens, causal=False, out_dtype=torch.float32, return_lse=True, softmax_scale=scale, k_descale=kd.to(dev),
                   v_descale=vd.to(dev), **kw)
        o_u, lse_u = ops.fa3_prefill_cache(q, k8, v8, **kw2)
        o_r, lse_r = ops.fa3_prefill_varlen(q[0].transpose(0, 1), k8, v8, cu_seqlens_q=i32([0, Sq]), max_seqlen_q=Sq, **kw2)
        torch.cuda.synchronize()
        pow2 = bool((torch.frexp(vd)[0] == 0.5).all())
        for name, o, lse in (("uniform", o_u[0].cpu(), lse_u[0].cpu()), ("ragged", o_r.transpose(0, 1).cpu(), lse_r.cpu())):
            assert bool(torch.isfinite(o).all()) and bool(torch.isfinite(lse).all()), name
            for h in range(H):
                kv = h // G
                want = vals[kv] * vd[kv].double()                                # exact in fp64
                got = o[h].double()                                              # [Sq, D]: every row is the V row
                err = (got - want[None]).abs()
                rel = float((err / want.abs()[None].clamp_min(1e-300)).max())
                print(f"{name} {dtype} D{D} paged={paged} pow2={pow2} head {h}: max relative error of O {rel:.3e}")
                if pow2:
                    assert torch.equal(got, want[None].expand(Sq, D)), (name, h, "O is not code * v_descale", rel)
                else:
                    assert bool((err <= want.abs()[None] * 2.0 ** -24).all()), (name, h, float(err.max()))     # one fp32 rounding
                code = vals[kv][aim[h]]                                          # the K code each row is aimed at
                want_lse = code * kd[kv].double() * scale
                zero = code == 0
                if bool(zero.any()):                                             # rows aimed at code 0: compared absolutely
                    assert float(lse[h][zero].abs().max()) <= 1e-6, (name, h)
                rel = ((lse[h].double() - want_lse)[~zero] / want_lse[~zero]).abs()
                assert float(rel.max()) <= 1e-3, (name, h, float(rel.max()))


@pytest.mark.parametrize("paged", [False, True])
@pytest.mark.parametrize("D, Hkv", [(128, 2), (64, 4)])
@pytest.mark.parametrize("dtype", BOTH)
def test_every_code_at_the_default_scale_has_the_bits_of_the_16_bit_kernel(dtype, D, Hkv, paged):
    """The same cache at the default scale 1 / sqrt(D) and power-of-two descales, which fold exactly into the 16-bit call:
    softmax_scale * k_descale[hk] going in, v_descale[hk] times the output coming out.  Head by K/V head, O and LSE of the FP8 call are
    those bits -- what is left of code * v_descale (one ulp, see above) is the shared softmax's rounding, none of it the conversion's.
    O stays within 2^-22 relative of code * v_descale and the LSE within 1e-3."""
    dev = device()
    q, k8, v8, vals, aim, kw = _codes_problem(dtype, D, Hkv, paged)
    H, G = 4, 4 // Hkv
    lens = i32([1])
    kd, vd = torch.tensor([0.5, 2.0, 1.0, 0.125][:Hkv]), torch.tensor([2.0, 0.25, 1.0, 8.0][:Hkv])
    base = dict(cache_seqlens=lens, causal=False, out_dtype=torch.float32, return_lse=True, **kw)
    o8, l8 = ops.fa3_prefill_cache(q, k8, v8, k_descale=kd.to(dev), v_descale=vd.to(dev), **base)
    k16, v16 = to16(k8, dtype), to16(v8, dtype)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(o8).all()) and bool(torch.isfinite(l8).all())
    for kv in range(Hkv):
        heads = slice(kv * G, (kv + 1) * G)
        o16, l16 = ops.fa3_prefill_cache(q[:, heads], k16[:, kv:kv + 1], v16[:, kv:kv + 1], softmax_scale=D ** -0.5 * float(kd[kv]), **base)
        torch.cuda.synchronize()
        assert torch.equal(o8[:, heads], o16 * float(vd[kv])) and torch.equal(l8[:, heads], l16), kv
        want = (vals[kv] * vd[kv].double()).to(dev)
        rel = float(((o8[0, heads].double() - want).abs() / want.abs().clamp_min(1e-300)).max())
        print(f"{dtype} D{D} paged={paged} K/V head {kv}: max relative error of O at the default scale {rel:.3e}")
        assert rel <= 2.0 ** -22


# --- 2. the bits of the 16-bit kernel at descales 1 ---------------------------------------------------------------------------------------

LENS2 = [384, 70, 130]


@pytest.mark.parametrize("paged", [False, True])
@pytest.mark.parametrize("dtype, D, sqs", [(torch.bfloat16, 128, (1, 33, 65, 257)), (torch.float16, 128, (1, 33, 65, 257)),
                                           (torch.bfloat16, 64, (33, 257)), (torch.float16, 64, (33, 257))])
def test_descales_of_one_give_the_bits_of_the_16_bit_kernel(dtype, D, sqs, paged):
    dev = device()
    B, H, Hkv, Smax = 3, 8, 2, 384
    q, k, v = problem(B, H, Hkv, max(sqs), Smax, D, dtype, 31 + D)
    one = torch.ones(Hkv, device=dev)
    k, v = k * 40, v * 40                                                        # codes over the whole range ...
    k.view(-1)[::97] *= 20                                                       # ... and, every 97th element, far past it: saturated codes
    v.view(-1)[::89] *= 20
    k8, v8 = quant(k, one), quant(v, one)
    assert float(k8.cpu().float().abs().max()) == 448.0 and float(v8.cpu().float().abs().max()) == 448.0
    k8, v8 = poisoned(k8, LENS2), poisoned(v8, LENS2)
    lens = i32(LENS2)
    kw = {}
    if paged:
        k8, v8, table = scatter_fp8(k8, v8, 128, 3, LENS2)
        kw["block_table"] = table
    k16, v16 = to16(k8, dtype), to16(v8, dtype)                                  # NaN bytes become NaN: the same keys must stay unread
    for odt in (dtype, torch.float32):
        for causal in (True, False):
            kw2 = dict(cache_seqlens=lens, causal=causal, out_dtype=odt, return_lse=True, **kw)
            for Sq in sqs:
                o8, l8 = ops.fa3_prefill_cache(q[:, :, :Sq], k8, v8, k_descale=one, v_descale=one, **kw2)
                o16, l16 = ops.fa3_prefill_cache(q[:, :, :Sq], k16, v16, **kw2)
                torch.cuda.synchronize()
                assert bool(torch.isfinite(o8).all()) and not bool(torch.isnan(l8).any())
                assert torch.equal(o8, o16) and torch.equal(l8, l16), (odt, causal, Sq)
            # one ragged batch
            q_lens = [max(sqs), 33, 1]
            cu = i32([0, q_lens[0], q_lens[0] + 33, q_lens[0] + 34])
            qp = torch.cat([q[b, :, :n].transpose(0, 1) for b, n in enumerate(q_lens)])
            o8, l8 = ops.fa3_prefill_varlen(qp, k8, v8, cu_seqlens_q=cu, max_seqlen_q=q_lens[0], k_descale=one, v_descale=one, **kw2)
            o16, l16 = ops.fa3_prefill_varlen(qp, k16, v16, cu_seqlens_q=cu, max_seqlen_q=q_lens[0], **kw2)
            torch.cuda.synchronize()
            assert bool(torch.isfinite(o8).all()) and not bool(torch.isnan(l8).any())
            assert torch.equal(o8, o16) and torch.equal(l8, l16), (odt, causal, "ragged")


# --- 3. against fp64 on the dequantised cache -------------------------------------------------------------------------------------------

LENS3 = [63, 64, 65, 127, 128, 129, 0, 192]            # next to tile and page edges; tile counts 1, 2, 3; an empty sequence
SQS3 = (1, 33, 65, 200, 257, 300)                       # 200, 257, 300: len_b < Sq for every sequence


@pytest.mark.parametrize("H, Hkv", [(4, 4), (16, 1)])
@pytest.mark.parametrize("dtype, D", [(torch.bfloat16, 128), (torch.float16, 128), (torch.bfloat16, 64), (torch.float16, 64)])
def test_against_fp64_on_the_dequantised_cache(dtype, D, H, Hkv):
    dev = device()
    B, Smax = len(LENS3), 256
    q300, k, v = problem(B, H, Hkv, max(SQS3), Smax, D, dtype, 11 + D + H)
    kd_h = torch.tensor([0.011, 0.0173, 0.009, 0.021][:Hkv], device=dev)
    vd_h = torch.tensor([0.013, 0.0091, 0.017, 0.008][:Hkv], device=dev)
    per_b = torch.tensor([[1.0], [0.37], [2.9], [1.21], [0.8], [1.7], [1.0], [0.55]], device=dev)
    k8, v8 = quant(k, kd_h), quant(v, vd_h)
    k8n, v8n = poisoned(k8, LENS3), poisoned(v8, LENS3)
    lens = i32(LENS3)
    caches = [("contiguous", k8n, v8n, {})]
    for page in (64, 128):
        kp, vp, table = scatter_fp8(k8n, v8n, page, 5 + page, LENS3)
        caches.append((f"page {page}", kp, vp, dict(block_table=table)))
    for kd, vd in ((kd_h, vd_h), ((kd_h[None] * per_b).contiguous(), (vd_h[None] / per_b).contiguous())):
        kf, vf = dequant(k8, kd, torch.float64), dequant(v8, vd, torch.float64)
        vmax = float(vf.abs().max())
        for Sq in SQS3:
            q = q300[:, :, :Sq]
            for causal in (True, False):
                ref_o, ref_lse, pnorm = reference(q, kf, vf, seqlens=lens, causal=causal)
                for odt in (dtype, torch.float32):
                    for name, kc, vc, kw in caches:
                        what = f"{dtype} D{D} H{H}/{Hkv} Sq{Sq} causal={causal} descale{tuple(kd.shape)} out={odt} {name}"
                        o, lse = ops.fa3_prefill_cache(q, kc, vc, cache_seqlens=lens, causal=causal, out_dtype=odt, return_lse=True,
                                                       k_descale=kd, v_descale=vd, **kw)
                        torch.cuda.synchronize()
                        assert o.dtype == odt and o.shape == q.shape
                        check_out(o, ref_o, pnorm, vmax, dtype, what)
                        check_lse(o, lse, ref_lse, what)


# --- 4. paged = contiguous, run = run, bit for bit -------------------------------------------------------------------------------------

LENS4 = [500, 37, 0, 257]


@pytest.mark.parametrize("layout", ["phsd", "hpsd"])
@pytest.mark.parametrize("page", [64, 256])
@pytest.mark.parametrize("dtype, D", [(torch.bfloat16, 128), (torch.float16, 64)])
def test_paged_equals_contiguous_bit_for_bit(dtype, D, page, layout):
    dev = device()
    B, H, Hkv, Smax, Sq = 4, 8, 2, 512, 70
    q, k, v = problem(B, H, Hkv, Sq, Smax, D, dtype, 21 + D)
    kd, vd = torch.tensor([0.011, 0.0173], device=dev), torch.tensor([0.013, 0.0091], device=dev)
    k8n, v8n = poisoned(quant(k, kd), LENS4), poisoned(quant(v, vd), LENS4)
    kp, vp, table = scatter_fp8(k8n, v8n, page, 7 + page, LENS4, layout)
    assert (kp.stride(1) == page * D) == (layout == "hpsd")                      # head-major, or the token-major flash-attn pool
    lens = i32(LENS4)
    for odt in (dtype, torch.float32):
        for causal in (True, False):
            kw = dict(cache_seqlens=lens, causal=causal, out_dtype=odt, return_lse=True, k_descale=kd, v_descale=vd)
            op, lp = both(ops.fa3_prefill_cache, q, k8n, v8n, kp, vp, table, **kw)
            op2, lp2 = ops.fa3_prefill_cache(q, kp, vp, block_table=table, **kw)
            torch.cuda.synchronize()
            assert not bool(torch.isnan(lp).any())
            assert torch.equal(op, op2) and torch.equal(lp, lp2), (odt, causal)


@pytest.mark.parametrize("dtype, D", [(torch.bfloat16, 128), (torch.float16, 64)])
def test_two_sequences_sharing_prefix_pages(dtype, D):
    """Sequences 0 and 1 name the same two prefix pages and own their tails; one [Hkv] descale serves the shared pages."""
    dev = device()
    H, Hkv, page, Sq = 8, 2, 64, 40
    q, k, v = problem(2, H, Hkv, Sq, 256, D, dtype, 41 + D)
    k[1, :, :128], v[1, :, :128] = k[0, :, :128], v[0, :, :128]
    kd, vd = torch.tensor([0.012, 0.02], device=dev), torch.tensor([0.015, 0.01], device=dev)
    lens_l = [200, 131]
    k8, v8 = poisoned(quant(k, kd), lens_l), poisoned(quant(v, vd), lens_l)
    pool_k = torch.full((9, Hkv, page, D), NANB, dtype=torch.uint8, device=dev)
    pool_v = pool_k.clone()
    table = i32([[5, 2, 7, 1], [5, 2, 3, 0]])                                    # pages 5, 2 shared; page 0 (NaN) behind sequence 1's length
    for b, row in enumerate(table.tolist()):
        for j, pg in enumerate(row):
            if j * page < lens_l[b]:
                pool_k[pg], pool_v[pg] = b8(k8)[b, :, j * page:(j + 1) * page], b8(v8)[b, :, j * page:(j + 1) * page]
    lens = i32(lens_l)
    kf, vf = dequant(quant(k, kd), kd, torch.float64), dequant(quant(v, vd), vd, torch.float64)
    for causal in (True, False):
        kw = dict(cache_seqlens=lens, causal=causal, return_lse=True, k_descale=kd, v_descale=vd)
        op, lp = both(ops.fa3_prefill_cache, q, k8, v8, pool_k.view(FP8), pool_v.view(FP8), table, **kw)
        ref_o, ref_lse, pnorm = reference(q, kf, vf, seqlens=lens, causal=causal)
        check_out(op, ref_o, pnorm, float(vf.abs().max()), dtype, f"shared prefix pages causal={causal}")
        check_lse(op, lp, ref_lse, "shared prefix pages")


# --- 5. ragged = per-sequence uniform calls ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("dtype, D", [(torch.bfloat16, 128), (torch.float16, 64)])
def test_ragged_equals_per_sequence_uniform_calls(dtype, D, causal):
    dev = device()
    H, Hkv, Smax = 8, 2, 512
    q_lens, lens_l = [300, 1, 0, 33, 64], [500, 1, 40, 33, 164]                  # a prefix for sequences 0 and 4, none for 1 and 3; 2 brings no row
    B, total = len(q_lens), sum(q_lens) + 10                                     # 10 packed rows behind cu[B]
    qs, k, v = problem(B, H, Hkv, 300, Smax, D, dtype, 51 + D)
    kd = torch.tensor([[0.011, 0.0173]], device=dev) * torch.tensor([[1.0], [0.5], [2.0], [1.3], [0.7]], device=dev)
    vd = (kd * 0.9).contiguous()
    k8, v8 = poisoned(quant(k, kd), lens_l), poisoned(quant(v, vd), lens_l)
    kp, vp, table = scatter_fp8(k8, v8, 128, 9, lens_l)
    cu_l = [0]
    for n in q_lens:
        cu_l.append(cu_l[-1] + n)
    qp = torch.zeros(total, H, D, dtype=dtype, device=dev)
    for b, n in enumerate(q_lens):
        qp[cu_l[b]:cu_l[b + 1]] = qs[b, :, :n].transpose(0, 1)
    lens, cu = i32(lens_l), i32(cu_l)
    for msq in (300, 256):                                                       # 256: sequence 0's rows 256 .. 299 lie past max_seqlen_q
        for name, kc, vc, kw in (("contiguous", k8, v8, {}), ("paged", kp, vp, dict(block_table=table))):
            out = torch.full((total, H, D), -7.0, dtype=torch.float32, device=dev)
            o, lse = ops.fa3_prefill_varlen(qp, kc, vc, cu_seqlens_q=cu, max_seqlen_q=msq, cache_seqlens=lens, causal=causal,
                                            out_dtype=torch.float32, return_lse=True, out=out, k_descale=kd, v_descale=vd, **kw)
            torch.cuda.synchronize()
            covered = torch.zeros(total, dtype=torch.bool, device=dev)
            for b, n in enumerate(q_lens):
                n = min(n, msq)
                if n == 0:
                    continue
                rows = slice(cu_l[b], cu_l[b] + n)
                covered[rows] = True
                kwb = {} if not kw else dict(block_table=table[b:b + 1])
                ou, lu = ops.fa3_prefill_cache(qs[b:b + 1, :, :n], kc if kw else kc[b:b + 1], vc if kw else vc[b:b + 1], cache_seqlens=lens[b:b + 1],
                                               causal=causal, out_dtype=torch.float32, return_lse=True, k_descale=kd[b:b + 1].contiguous(),
                                               v_descale=vd[b:b + 1].contiguous(), **kwb)
                torch.cuda.synchronize()
                assert bool(torch.isfinite(ou).all())
                assert torch.equal(o[rows], ou[0].transpose(0, 1)) and torch.equal(lse[:, rows], lu[0]), (name, msq, b)
            assert bool(covered.any()) and bool((o[~covered] == -7.0).all()), (name, msq, "a row no sequence covers was written")
            assert bool(torch.isfinite(o).all())


# --- 6. k_new=, v_new= -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype, D", [(torch.bfloat16, 128), (torch.float16, 64)])
def test_new_rows_are_quantised_in_front_of_the_attention(dtype, D):
    dev = device()
    B, H, Hkv, Smax, Sq = 3, 8, 2, 256, 70
    lens_l = [200, 70, 131]                                                      # the lengths after the step
    q, k, v = problem(B, H, Hkv, Sq, Smax, D, dtype, 61 + D)
    g = torch.Generator(device=dev).manual_seed(5)
    kn, vn = (torch.randn(B, Hkv, Sq, D, generator=g, device=dev).to(dtype) for _ in range(2))
    kd, vd = torch.tensor([0.02, 0.031], device=dev), torch.tensor([0.025, 0.017], device=dev)
    old = [n - Sq for n in lens_l]
    k0, v0 = poisoned(quant(k, kd), old), poisoned(quant(v, vd), old)
    lens = i32(lens_l)
    kw = dict(cache_seqlens=lens, return_lse=True, k_descale=kd, v_descale=vd)
    # uniform
    ka, va = k0.clone(), v0.clone()
    o1, l1 = ops.fa3_prefill_cache(q, ka, va, k_new=kn, v_new=vn, **kw)
    kb, vb = k0.clone(), v0.clone()
    ops.kv_append(kn, vn, kb, vb, cache_seqlens=lens, k_descale=kd, v_descale=vd)
    o2, l2 = ops.fa3_prefill_cache(q, kb, vb, **kw)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(o1).all()) and torch.equal(o1, o2) and torch.equal(l1, l2)
    assert torch.equal(b8(ka), b8(kb)) and torch.equal(b8(va), b8(vb))
    kn8, vn8 = quant(kn, kd), quant(vn, vd)
    for b, n in enumerate(lens_l):
        assert torch.equal(b8(ka)[b, :, n - Sq:n], b8(kn8)[b]) and torch.equal(b8(va)[b, :, n - Sq:n], b8(vn8)[b]), b
        assert torch.equal(b8(ka)[b, :, :n - Sq], b8(k0)[b, :, :n - Sq]) and bool((b8(ka)[b, :, n:] == NANB).all())
    # ragged: sequence b brings q_lens[b] rows
    q_lens = [70, 1, 33]
    cu_l = [0, 70, 71, 104]
    cu = i32(cu_l)
    qp = torch.cat([q[b, :, :n].transpose(0, 1) for b, n in enumerate(q_lens)])
    knp = torch.cat([kn[b, :, :n].transpose(0, 1) for b, n in enumerate(q_lens)])
    vnp = torch.cat([vn[b, :, :n].transpose(0, 1) for b, n in enumerate(q_lens)])
    old = [n - m for n, m in zip(lens_l, q_lens)]
    k0, v0 = poisoned(quant(k, kd), old), poisoned(quant(v, vd), old)
    ka, va = k0.clone(), v0.clone()
    o1, l1 = ops.fa3_prefill_varlen(qp, ka, va, cu_seqlens_q=cu, max_seqlen_q=70, k_new=knp, v_new=vnp, **kw)
    kb, vb = k0.clone(), v0.clone()
    ops.kv_append(knp, vnp, kb, vb, cache_seqlens=lens, cu_seqlens_q=cu, max_seqlen_q=70, k_descale=kd, v_descale=vd)
    o2, l2 = ops.fa3_prefill_varlen(qp, kb, vb, cu_seqlens_q=cu, max_seqlen_q=70, **kw)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(o1).all()) and torch.equal(o1, o2) and torch.equal(l1, l2)
    assert torch.equal(b8(ka), b8(kb)) and torch.equal(b8(va), b8(vb))
    for b, (n, m) in enumerate(zip(lens_l, q_lens)):
        assert torch.equal(b8(ka)[b, :, n - m:n], b8(kn8)[b, :, :m]), b


# --- 7. graph capture ----------------------------------------------------------------------------------------------------------------------

def test_a_captured_append_and_ragged_prefill_replays_while_everything_changes():
    from photonic_flash_attention_amd.integration.pytorch import PagedKVCache
    dev = device()
    B, H, Hkv, D, page, M, total = 3, 8, 2, 128, 64, 130, 300
    dtype = torch.bfloat16
    kd, vd = torch.tensor([0.02, 0.03], device=dev), torch.tensor([0.025, 0.015], device=dev)
    c = PagedKVCache(num_pages=40, page_size=page, Hkv=Hkv, D=D, dtype=FP8, device=dev, max_batch=B, max_pages_per_seq=12,
                     k_descale=kd, v_descale=vd)
    b8(c.k_pool).fill_(NANB)
    b8(c.v_pool).fill_(NANB)
    g = torch.Generator(device=dev).manual_seed(77)
    slots = [c.allocate() for _ in range(B)]
    assert slots == [0, 1, 2]
    state = dict(q=torch.zeros(total, H, D, dtype=dtype, device=dev), kn=torch.zeros(total, Hkv, D, dtype=dtype, device=dev),
                 vn=torch.zeros(total, Hkv, D, dtype=dtype, device=dev), cu=i32([0, 0, 0, 0]))
    k, v, kw = c.operands(None)
    assert k.dtype == FP8 and kw["k_descale"] is kd

    def step():
        ops.kv_append(state["kn"], state["vn"], k, v, cu_seqlens_q=state["cu"], max_seqlen_q=M, **kw)
        return ops.fa3_prefill_varlen(state["q"], k, v, cu_seqlens_q=state["cu"], max_seqlen_q=M, return_lse=True, **kw)

    def advance(q_lens, seed):
        gg = torch.Generator(device=dev).manual_seed(seed)
        c.advance(slots, q_lens)
        cu = [0]
        for n in q_lens:
            cu.append(cu[-1] + n)
        state["cu"].copy_(i32(cu))
        for name in ("q", "kn", "vn"):
            state[name].copy_(torch.randn(state[name].shape, generator=gg, device=dev))
        return cu

    advance([130, 1, 64], 1)
    graph, (o_g, lse_g) = capture(step)
    for q_lens, seed in (([130, 1, 64], 2), ([5, 129, 0], 3), ([64, 70, 130], 4)):
        cu = advance(q_lens, seed)                                               # lengths grow, new pages enter the table, cu changes in place
        if seed == 3:
            c.swap_pages(0, 0, 2)                                                # pages move
        kd.mul_(1.25)                                                            # the descales' contents change in place
        vd.mul_(0.8)
        graph.replay()
        torch.cuda.synchronize()
        o_r, lse_r, pool_r = o_g.clone(), lse_g.clone(), b8(c.k_pool).clone()
        o_e, lse_e = step()                                                      # the same append again (the same bytes), then the attention
        torch.cuda.synchronize()
        rows = slice(0, cu[-1])
        assert torch.equal(pool_r, b8(c.k_pool))
        assert bool(torch.isfinite(o_e[rows]).all()) and bool(torch.isfinite(lse_e[:, rows]).all()), q_lens
        assert torch.equal(o_r[rows], o_e[rows]) and torch.equal(lse_r[:, rows], lse_e[:, rows]), q_lens
        assert [c.length(s) for s in slots] == c.cache_seqlens.tolist()


# --- 8. through the class ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype, D", [(torch.bfloat16, 128), (torch.float16, 64)])
def test_chunked_prefill_through_the_class(dtype, D):
    from photonic_flash_attention_amd.integration.pytorch import PagedKVCache
    dev = device()
    H, Hkv, page = 8, 2, 64
    kd, vd = torch.tensor([0.021, 0.017], device=dev), torch.tensor([0.013, 0.019], device=dev)
    c = PagedKVCache(num_pages=16, page_size=page, Hkv=Hkv, D=D, dtype=FP8, device=dev, max_batch=2, max_pages_per_seq=8,
                     k_descale=kd, v_descale=vd)
    b8(c.k_pool).fill_(NANB)
    b8(c.v_pool).fill_(NANB)
    g = torch.Generator(device=dev).manual_seed(9)
    prompt = [300, 170]                                                          # two prompts; the second chunk is the last 100 rows of each
    chunk = 100
    slots = [c.allocate(), c.allocate()]
    kn, vn = (torch.randn(sum(prompt), Hkv, D, generator=g, device=dev).to(dtype) for _ in range(2))
    c.append_varlen(slots, kn, vn, prompt)
    q = torch.randn(2, chunk, H, D, generator=g, device=dev).to(dtype).permute(0, 2, 1, 3)
    k, v, kw = c.operands(slots)
    o, lse = ops.fa3_prefill_cache(q, k, v, return_lse=True, **kw)
    torch.cuda.synchronize()
    kf = torch.zeros(2, Hkv, 320, D, dtype=torch.float64, device=dev)
    vf = torch.zeros_like(kf)
    for i, s in enumerate(slots):
        gk, gv = c.gather(s)
        assert gk.dtype == FP8 and gk.shape[1] == prompt[i]
        kf[i, :, :prompt[i]] = dequant(gk[None], kd, torch.float64)[0]
        vf[i, :, :prompt[i]] = dequant(gv[None], vd, torch.float64)[0]
    ref_o, ref_lse, pnorm = reference(q, kf, vf, seqlens=i32(prompt))
    check_out(o, ref_o, pnorm, float(vf.abs().max()), dtype, f"{dtype} D{D} second chunk over the class's pages")
    check_lse(o, lse, ref_lse, "second chunk")
    assert bool(torch.isfinite(lse).all())


# --- 9. refusals on device tensors -----------------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing():
    dev = device()
    B, H, Hkv, Smax, Sq, D = 2, 8, 2, 256, 70, 128
    dtype = torch.bfloat16
    q, k, v = problem(B, H, Hkv, Sq, Smax, D, dtype, 3)
    one = torch.ones(Hkv, device=dev)
    k8, v8 = quant(k, one), quant(v, one)
    before_k, before_v = b8(k8).clone(), b8(v8).clone()
    lens = i32([200, 131])
    kn = torch.ones(B, Hkv, Sq, D, dtype=dtype, device=dev)
    out = torch.full((B, Sq, H, D), -7.0, dtype=dtype, device=dev).permute(0, 2, 1, 3)
    rot = dict(rotary_cos=torch.zeros(512, 64, device=dev), rotary_sin=torch.zeros(512, 64, device=dev))
    base = dict(cache_seqlens=lens, k_descale=one, v_descale=one, out=out, k_new=kn, v_new=kn)
    for kw, name in ((dict(window=16), "window"), (dict(shared_prefix=64), "shared_prefix"), (dict(key_splits=2), "key_splits"),
                     (dict(key_splits="auto"), "key_splits"), (dict(shared_prefix=64, prefix_key_splits=2), "shared_prefix"),
                     (dict(prefix_key_splits=2), "prefix_key_splits"), (rot, "rotary_cos / rotary_sin")):
        with pytest.raises(ValueError, match=f"{name} is not supported with an FP8"):
            ops.fa3_prefill_cache(q, k8, v8, **base, **kw)
    qp = q.transpose(1, 2).reshape(B * Sq, H, D)
    outp = torch.full((B * Sq, H, D), -7.0, dtype=dtype, device=dev)
    knp = torch.ones(B * Sq, Hkv, D, dtype=dtype, device=dev)
    basep = dict(cu_seqlens_q=i32([0, Sq, 2 * Sq]), max_seqlen_q=Sq, cache_seqlens=lens, k_descale=one, v_descale=one, out=outp, k_new=knp, v_new=knp)
    for kw, name in ((dict(window=16), "window"), (rot, "rotary_cos / rotary_sin")):
        with pytest.raises(ValueError, match=f"{name} is not supported with an FP8"):
            ops.fa3_prefill_varlen(qp, k8, v8, **basep, **kw)
    # descales without an FP8 cache, an FP8 cache without descales
    k16 = torch.zeros(B, Hkv, Smax, D, dtype=dtype, device=dev)
    with pytest.raises(ValueError, match="go with torch.float8_e4m3fn caches only"):
        ops.fa3_prefill_cache(q, k16, k16, cache_seqlens=lens, k_descale=one, v_descale=one, out=out)
    with pytest.raises(ValueError, match="caches need k_descale and v_descale"):
        ops.fa3_prefill_cache(q, k8, v8, cache_seqlens=lens, out=out)
    with pytest.raises(ValueError, match="caches need k_descale and v_descale"):
        ops.fa3_prefill_varlen(qp, k8, v8, cu_seqlens_q=i32([0, Sq, 2 * Sq]), max_seqlen_q=Sq, cache_seqlens=lens, out=outp)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((outp == -7.0).all())              # no attention launch
    assert torch.equal(b8(k8), before_k) and torch.equal(b8(v8), before_v)       # no append

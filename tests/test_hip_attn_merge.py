"""GPU tests of the merge of partial attention results (``ops.attn_merge`` / ``pfa_attn_merge``) and of ``shared_prefix=`` on
``ops.fa3_decode`` / ``ops.fa3_prefill_cache``.

The merge is checked against the rule in fp64 on the same inputs.  Bounds: fp32 output ``|err| <= 1e-5 * max_n |O_n[d]|`` (ten times
the N + 3 fp32 roundings plus the hardware exp's argument error, whose weighted effect is at most 0.37 * 88 * 2^-24); 16-bit output that
plus ``2^-8 |ref|`` (bf16) or ``2^-11 |ref|`` (fp16), twice one round-to-nearest-even; LSE ``|err| <= 4e-6 * max(1, |ref|)``.

A shared-prefix step is checked against fp64 attention over the whole logical cache, within the bounds of that reference
(tests/kvcache_testlib.py, which also builds the step: ``prefix_problem``).  NaN fills every cache tail, every page no table names,
every table entry past a sequence's last page and -- in the contiguous cache -- the prefix region of every sequence but the first:
the prefix is read from sequence 0 alone."""

from __future__ import annotations

import ctypes as C

import pytest
import torch

from capi_testlib import decode_args
from kvcache_testlib import INF, NAN, PREFIX_PAGE, both_prefix_caches, capture, check_step, device, merge_ref64, prefix_problem, reference

pytestmark = pytest.mark.gpu

RNE2 = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
OUT_DTYPES = {torch.float32: (torch.float32, torch.bfloat16, torch.float16), torch.bfloat16: (torch.bfloat16, torch.float32),
              torch.float16: (torch.float16, torch.float32)}
B, SQ, H = 3, 5, 4                      # 3 * 5 * 4 * (128 / 8) = 960 items: four workgroups at D = 128, the last partly empty
OFFSETS = [0.0, 5.0, -5.0, 120.0, -120.0, 0.0, 5.0, -5.0]


# ---- the merge --------------------------------------------------------------------------------------------------------------------

def _parts(N, D, dtype, seed):
    """N parts as slices of larger [B, Sq + 1, H + 1, D] buffers; LSEs 3 * normal + a per-part offset, so that some weights underflow to
    zero; part 1's LSE in the layout of one call over all B * Sq rows as one sequence, [1, H, B * Sq]."""
    g = torch.Generator().manual_seed(seed)
    dev = device()
    outs = [torch.randn(B, SQ + 1, H + 1, D, generator=g).to(dev, dtype)[:, :SQ, :H].permute(0, 2, 1, 3) for _ in range(N)]
    lses = [(3 * torch.randn(B, H, SQ, generator=g) + OFFSETS[n]).to(dev) for n in range(N)]
    lses[1] = lses[1].permute(1, 0, 2).contiguous().view(1, H, B * SQ).view(H, B, SQ).transpose(0, 1)
    assert lses[1].stride() == (SQ, B * SQ, 1)
    return outs, lses


def _check_merge(o, lse, outs, lses):
    ref_o, ref_lse = merge_ref64(outs, lses)
    err = (o.double() - ref_o).abs()
    bound = 1e-5 * torch.stack([t.double().abs() for t in outs]).max(dim=0).values
    if o.dtype != torch.float32:
        bound = bound + RNE2[o.dtype] * ref_o.abs()
    lerr = (lse.double() - ref_lse).abs()
    lbound = 4e-6 * ref_lse.abs().clamp_min(1.0)
    print(f"merge {outs[0].dtype}->{o.dtype} N={len(outs)} D={o.shape[-1]}: O max err {float(err.max()):.3e} "
          f"(worst err - bound {float((err - bound).max()):.3e}), LSE max err {float(lerr.max()):.3e} "
          f"(worst err - bound {float((lerr - lbound).max()):.3e})")
    assert bool((err <= bound).all()), float((err - bound).max())
    assert bool((lerr <= lbound).all()), float((lerr - lbound).max())


@pytest.mark.parametrize("D", [8, 64, 128, 256])
@pytest.mark.parametrize("N", [2, 3, 8])
def test_merge_matches_fp64_for_every_dtype_pair(N, D):
    from photonic_flash_attention_amd import ops
    for dtype, odts in OUT_DTYPES.items():
        outs, lses = _parts(N, D, dtype, 1000 * N + D)
        for odt in odts:
            o, lse = ops.attn_merge(outs, lses, out_dtype=odt, return_lse=True)
            again = ops.attn_merge(outs, lses, out_dtype=odt, return_lse=True)
            torch.cuda.synchronize()
            assert o.dtype == odt and o.shape == (B, H, SQ, D) and lse.shape == (B, H, SQ)
            _check_merge(o, lse, outs, lses)
            assert torch.equal(o, again[0]) and torch.equal(lse, again[1])              # two launches: the same bits


def test_merge_skips_inf_parts_zeroes_empty_rows_and_keeps_nan_rows_to_themselves():
    from photonic_flash_attention_amd import ops
    for dtype in (torch.float32, torch.bfloat16):
        outs, lses = _parts(3, 64, dtype, 5)
        clean_o, clean_lse = ops.attn_merge(outs, lses, return_lse=True, out_dtype=torch.float32)
        lses = [l.clone() for l in lses]
        lses[0][0, 0, 1] = -INF
        outs[0][0, 0, 1] = NAN                                  # a skipped part's O, NaN: it must not reach the result
        lses[2][2, 3, 4] = -INF
        outs[2][2, 3, 4] = INF
        for l in lses:
            l[0, 1, 2] = -INF                                   # no visible key in any part
        outs[1][0, 1, 2] = NAN
        lses[1][1, 0, 3] = NAN                                  # a NaN LSE
        o, lse = ops.attn_merge(outs, lses, return_lse=True, out_dtype=torch.float32)
        torch.cuda.synchronize()
        touched = torch.zeros(B, H, SQ, dtype=torch.bool, device=o.device)
        touched[0, 0, 1] = touched[2, 3, 4] = touched[0, 1, 2] = touched[1, 0, 3] = True
        assert bool((o[0, 1, 2] == 0).all()) and float(lse[0, 1, 2]) == -INF
        assert bool(torch.isnan(o[1, 0, 3]).all()) and bool(torch.isnan(lse[1, 0, 3]))
        for row, rest in (((0, 0, 1), (1, 2)), ((2, 3, 4), (0, 1))):
            assert bool(torch.isfinite(o[row]).all()) and bool(torch.isfinite(lse[row]))
            _check_merge(o[row][None, None, None], lse[row][None, None, None], [outs[n][row][None, None, None] for n in rest],
                         [lses[n][row][None, None, None] for n in rest])
        # every other row is what it was without them, bit for bit
        assert torch.equal(o[~touched], clean_o[~touched]) and torch.equal(lse[~touched], clean_lse[~touched])


@pytest.mark.parametrize("N", [2, 8])
def test_merge_of_one_finite_part_is_exact(N):
    from photonic_flash_attention_amd import ops
    dev = device()
    g = torch.Generator().manual_seed(N)
    for dtype, odts in OUT_DTYPES.items():
        part = (torch.randn(B, SQ, H, 128, generator=g) * 3).to(dev, dtype).permute(0, 2, 1, 3)
        finite = (30 * torch.randn(B, H, SQ, generator=g)).to(dev)
        for where in (0, N - 1):
            outs = [torch.full_like(part, NAN) for _ in range(N)]
            lses = [torch.full_like(finite, -INF) for _ in range(N)]
            outs[where], lses[where] = part, finite
            for odt in odts:
                o, lse = ops.attn_merge(outs, lses, out_dtype=odt, return_lse=True)
                torch.cuda.synchronize()
                assert torch.equal(lse, finite)
                assert torch.equal(o, part.to(odt))             # fp32 -> 16 bits: one round-to-nearest-even; otherwise the same bits


def test_merge_writes_nothing_but_its_rows():
    from photonic_flash_attention_amd import ops
    outs, lses = _parts(2, 64, torch.bfloat16, 9)
    for odt in (torch.bfloat16, torch.float32):
        big = torch.full((B + 2, SQ + 2, H + 2, 64 + 16), 77.0, dtype=odt, device=device())
        out = big[1:B + 1, 1:SQ + 1, 1:H + 1, 8:72].permute(0, 2, 1, 3)
        o, _ = ops.attn_merge(outs, lses, out=out)
        want, _ = ops.attn_merge(outs, lses, out_dtype=odt)
        torch.cuda.synchronize()
        assert o is out and torch.equal(out, want)
        poison = torch.ones_like(big, dtype=torch.bool)
        poison[1:B + 1, 1:SQ + 1, 1:H + 1, 8:72] = False
        assert bool((big[poison] == 77.0).all())


# ---- shared_prefix ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("Sq", [1, 3])
@pytest.mark.parametrize("D", [128, 64])
def test_shared_prefix_decode(D, Sq, dtype):
    from photonic_flash_attention_amd import ops
    private = (1, 64, 65, 130) if Sq == 1 else (3, 64, 65, 130)
    pr = prefix_problem(4, Sq, D, private, 320, dtype)
    both_prefix_caches(ops.fa3_decode, pr, f"decode D{D} Sq{Sq}")


@pytest.mark.parametrize("Bc,Sq,private,Smax", [(3, 40, (40, 64, 130), 320), (2, 300, (300, 330), 512)])
def test_shared_prefix_prefill(Bc, Sq, private, Smax):
    from photonic_flash_attention_amd import ops
    for D in (128, 64):
        pr = prefix_problem(Bc, Sq, D, private, Smax, torch.bfloat16)
        both_prefix_caches(ops.fa3_prefill_cache, pr, f"prefill B{Bc} Sq{Sq} D{D}")
    # fp32 output: the merge writes the caller's dtype
    o32, _ = ops.fa3_prefill_cache(pr["q"], pr["kc"], pr["vc"], cache_seqlens=pr["lens"], shared_prefix=pr["P"], out_dtype=torch.float32)
    torch.cuda.synchronize()
    assert o32.dtype == torch.float32 and float((o32.double() - pr["ref"][0]).abs().max()) <= 1e-3


@pytest.fixture
def pass_spy(monkeypatch):
    """Every call of ``ops.fa3_decode`` / ``ops.fa3_prefill_cache`` made through the module, by name and q shape."""
    from photonic_flash_attention_amd import ops
    calls = []
    for name in ("fa3_decode", "fa3_prefill_cache"):
        def spy(*a, _real=getattr(ops, name), _name=name, **kw):
            calls.append((_name, tuple(a[0].shape), kw.get("causal"), kw.get("shared_prefix")))
            return _real(*a, **kw)
        monkeypatch.setattr(ops, name, spy)
    return calls


@pytest.mark.parametrize("Bc,Sq,prefix_pass", [(4, 16, "fa3_decode"), (5, 13, "fa3_prefill_cache")])
def test_the_prefix_pass_changes_kernel_past_64_rows(pass_spy, Bc, Sq, prefix_pass):
    """B * Sq = 64 rows: the prefix pass is the split-KV decode kernel over one sequence of 64 rows; 65 rows: the MFMA forward."""
    from photonic_flash_attention_amd import _capi, ops
    pr = prefix_problem(Bc, Sq, 64, tuple([Sq, 64, 65, 130, 100][:Bc]), 320, torch.bfloat16)
    o, lse = ops.fa3_decode(pr["q"], pr["kc"], pr["vc"], cache_seqlens=pr["lens"], shared_prefix=128, return_lse=True)
    torch.cuda.synchronize()
    check_step(o, lse, pr["ref"], pr["dtype"], pr["vmax"], f"threshold B{Bc} Sq{Sq}")
    rows = Bc * Sq
    inner = [c for c in pass_spy if c[3] is None]                                       # the two passes, in the order they are enqueued
    assert inner == [(prefix_pass, (1, 8, rows, 64), False, None), ("fa3_decode", (Bc, 8, Sq, 64), True, None)], pass_spy
    # and the kernels behind those two calls, on an equivalent argument block
    a = decode_args(dict(B=1, D=64, dtype_out=2, causal=0), Sq=rows, Smax=128)
    if prefix_pass == "fa3_decode":
        assert _capi.describe_decode(a)[0].startswith("fa3_decode")
    else:
        assert _capi.load().pfa_fa3_decode_check(C.byref(a)) == -3 and _capi.describe_prefill(a)[0].startswith("fa3_prefill")


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("rotary", [False, True])
@pytest.mark.parametrize("paged", [False, True])
def test_shared_prefix_with_new_rows_and_rotary(paged, rotary):
    """The append runs once, first: the cache ends up as the plain call leaves it, and both passes read the rotated q."""
    from photonic_flash_attention_amd import ops
    Sq, D = 3, 64
    pr = prefix_problem(4, Sq, D, (3, 64, 65, 130), 320, torch.bfloat16)
    dev, lens = device(), pr["lens"]
    g = torch.Generator().manual_seed(31)
    kn, vn = (torch.randn(4, 2, Sq, D, generator=g).to(dev, torch.bfloat16) for _ in range(2))
    kw = {}
    if rotary:
        cos, sin = ops.rotary_tables(512, D, device=dev)
        kw = dict(rotary_cos=cos, rotary_sin=sin)
    # the reference: the CPU model of the append on the logical cache, and the q it rotates
    kl, vl = pr["kl"].cpu().clone(), pr["vl"].cpu().clone()
    if rotary:
        q_ref = ops.rope_append(kn.cpu(), vn.cpu(), kl, vl, cache_seqlens=lens.cpu(), q=pr["q"].cpu(),
                                rotary_cos=cos.cpu(), rotary_sin=sin.cpu())
    else:
        ops.kv_append(kn.cpu(), vn.cpu(), kl, vl, cache_seqlens=lens.cpu())
        q_ref = pr["q"].cpu()
    ref = reference(q_ref.to(dev), kl.to(dev), vl.to(dev), seqlens=lens)
    caches = (pr["kp"], pr["vp"]) if paged else (pr["kc"], pr["vc"])
    table = dict(block_table=pr["table"]) if paged else {}
    k1, v1, k2, v2 = caches[0].clone(), caches[1].clone(), caches[0].clone(), caches[1].clone()
    ops.fa3_decode(pr["q"], k1, v1, cache_seqlens=lens, k_new=kn, v_new=vn, **table, **kw)
    o, lse = ops.fa3_decode(pr["q"], k2, v2, cache_seqlens=lens, k_new=kn, v_new=vn, shared_prefix=128, return_lse=True, **table, **kw)
    torch.cuda.synchronize()
    assert torch.equal(_bits(k1), _bits(k2)) and torch.equal(_bits(v1), _bits(v2))
    assert not torch.equal(_bits(k2), _bits(caches[0]))         # ... and something was appended
    check_step(o, lse, ref, torch.bfloat16, float(vl.abs().max()), f"new rows paged={paged} rotary={rotary}")


def test_shared_prefix_step_replays_in_a_graph():
    """Append + prefix pass + own-keys pass + merge captured once; replayed after lengths, table, cache contents, new rows and q
    changed: each replay equals the eager call bit for bit."""
    from photonic_flash_attention_amd import ops
    dev, dtype, Bc, Hq, Hkv, D, n_pages = device(), torch.bfloat16, 4, 8, 2, 64, 24
    g = torch.Generator().manual_seed(88)

    def rnd(*shape):
        return torch.randn(*shape, generator=g).to(dev, dtype)

    q_s, kn_s, vn_s = rnd(Bc, 1, Hq, D).permute(0, 2, 1, 3), rnd(Bc, Hkv, 1, D), rnd(Bc, Hkv, 1, D)
    kp, vp = rnd(n_pages, Hkv, PREFIX_PAGE, D), rnd(n_pages, Hkv, PREFIX_PAGE, D)
    o_s = torch.empty(Bc, 1, Hq, D, dtype=dtype, device=dev).permute(0, 2, 1, 3)

    def table_of(seed):
        perm = torch.randperm(n_pages, generator=torch.Generator().manual_seed(seed))
        t = perm[2:2 + Bc * 3].reshape(Bc, 3)
        return torch.cat([perm[:2].expand(Bc, 2), t], dim=1).to(torch.int32)      # two shared prefix pages, three of their own

    lens_s = torch.tensor([129, 200, 257, 320], dtype=torch.int32, device=dev)
    table_s = table_of(0).to(dev)

    def step(q, kn, vn, k, v, lens, table, out):
        return ops.fa3_decode(q, k, v, cache_seqlens=lens, block_table=table, k_new=kn, v_new=vn, shared_prefix=128, out=out,
                              return_lse=True)

    graph, (o_g, lse_g) = capture(lambda: step(q_s, kn_s, vn_s, kp, vp, lens_s, table_s, o_s))
    assert o_g is o_s

    for n, lens in enumerate(([129, 200, 257, 320], [192, 130, 300, 193], [320, 129, 129, 256])):
        if n:                                                   # everything the graph reads from the device changes
            q_s.copy_(rnd(Bc, 1, Hq, D).permute(0, 2, 1, 3))
            kn_s.copy_(rnd(Bc, Hkv, 1, D))
            vn_s.copy_(rnd(Bc, Hkv, 1, D))
            kp.copy_(rnd(n_pages, Hkv, PREFIX_PAGE, D))
            vp.copy_(rnd(n_pages, Hkv, PREFIX_PAGE, D))
            lens_s.copy_(torch.tensor(lens, dtype=torch.int32))
            table_s.copy_(table_of(n))
        ke, ve = kp.clone(), vp.clone()
        o_e, lse_e = step(q_s.clone(), kn_s.clone(), vn_s.clone(), ke, ve, lens_s.clone(), table_s.clone(), None)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(o_g, o_e) and torch.equal(lse_g, lse_e), n
        assert torch.equal(kp, ke) and torch.equal(vp, ve), n
        assert bool(torch.isfinite(o_g.float()).all())


def test_shared_prefix_none_is_the_plain_call():
    from photonic_flash_attention_amd import ops
    pr = prefix_problem(4, 3, 64, (3, 64, 65, 130), 320, torch.bfloat16)
    for fn in (ops.fa3_decode, ops.fa3_prefill_cache):
        kw = dict(cache_seqlens=pr["lens"], block_table=pr["table"], return_lse=True)
        plain = fn(pr["q"], pr["kp"], pr["vp"], **kw)
        none = fn(pr["q"], pr["kp"], pr["vp"], shared_prefix=None, **kw)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(plain[0].float()).all())
        assert torch.equal(plain[0], none[0]) and torch.equal(plain[1], none[1])
        check_step(*plain, pr["ref"], pr["dtype"], pr["vmax"], "plain paged call")

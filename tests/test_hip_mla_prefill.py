"""GPU tests of the non-absorbed MLA prefill over packed sequences (``ops.mla_prefill`` -> ``pfa_mla_prefill``;
csrc/fa3_mla_prefill_kernel.h).

The fp64 reference and the bounds -- per element for a 16-bit output, 1e-3 for an fp32 output, 2e-3 on the LSE with exact -inf rows --
are tests/kvcache_testlib.py's, called per sequence on K = cat(k_nope, k_rope expanded) at width 192 and V at width 128; the exact
counts are tests/probe_testlib.py's.  One ragged batch serves every test.  Its sequences (Lq, Lk) sit at the kernel's own edges: one
below, at and one past a wave's 32 rows, a workgroup's 256 rows and the 64-key tile; a chunk over a longer context; Lk < Lq (rows that
see nothing under the causal flag); no key; no row.  The last sequence ends in the middle of a key tile with NaN behind it.  The scale
is DeepSeek's (128 + 64)^-0.5.  Every case fails on a library without the kernel, where ``ops.mla_prefill`` does not exist."""

from __future__ import annotations

import pytest
import torch

import probe_testlib as pt
from kvcache_testlib import NAN, capture, check_lse, check_out, device, gen, i32, reference
from photonic_flash_attention_amd import _capi_mla_prefill, ops

pytestmark = pytest.mark.gpu

BF, FP, F32 = torch.bfloat16, torch.float16, torch.float32
SCALE = 192 ** -0.5
H = 3
SEQS = [(31, 63), (32, 64), (33, 65), (5, 0), (255, 300), (256, 256), (0, 17), (257, 40), (128, 700)]      # 997 rows, 1505 keys


def _problem(dtype, rope_heads, seed, seqs=SEQS):
    """The packed operands of ``seqs`` as strided views -- q the first 192 of 200 columns, k_nope and v the halves of one 256-wide buffer
    -- with 70 rows of NaN behind cu[B] in every buffer -> dict(q, kn, kr, v, cu_q, cu_k, kw) with kw the call's keyword arguments."""
    g, dev = gen(seed), device()
    cu = torch.tensor([[0, 0]] + list(seqs)).cumsum(0)
    tq, tk = int(cu[-1, 0]), int(cu[-1, 1])
    q = torch.randn(tq + 70, H, 200, generator=g, device=dev).to(dtype)
    kv = torch.randn(tk + 70, H, 256, generator=g, device=dev).to(dtype)
    kr = torch.randn(tk + 70, rope_heads, 64, generator=g, device=dev).to(dtype)
    q[tq:], kv[tk:], kr[tk:] = NAN, NAN, NAN
    cu_q, cu_k = i32(cu[:, 0].tolist()), i32(cu[:, 1].tolist())
    kw = dict(cu_seqlens_q=cu_q, cu_seqlens_k=cu_k, max_seqlen_q=max(s[0] for s in seqs), max_seqlen_k=max(max(s[1] for s in seqs), 1),
              softmax_scale=SCALE, return_lse=True)
    return dict(q=q[..., :192], kn=kv[..., :128], kr=kr, v=kv[..., 128:], cu=cu.tolist(), seqs=list(seqs), kw=kw)


def _per_sequence(pr):
    """(b, rows, keys) of every sequence with a row; ``keys`` holds one key row where the sequence has none (neither the reference nor a
    call takes an empty tensor; the length says 0)."""
    for b, (nq, nk) in enumerate(pr["seqs"]):
        if nq:
            yield b, slice(pr["cu"][b][0], pr["cu"][b][0] + nq), slice(pr["cu"][b][1], pr["cu"][b][1] + max(nk, 1))


def _check(pr, o, lse, causal, what):
    for b, rq, rk in _per_sequence(pr):
        k = torch.cat([pr["kn"][rk], pr["kr"][rk].expand(-1, H, 64)], dim=-1)
        ro, rlse, pn = reference(pr["q"][rq].transpose(0, 1)[None], k.transpose(0, 1)[None], pr["v"][rk].transpose(0, 1)[None],
                                 seqlens=i32([pr["seqs"][b][1]]), causal=causal, scale=SCALE)
        ob = o[rq].transpose(0, 1)[None]
        check_out(ob, ro, pn, float(pr["v"][rk].abs().max()), pr["q"].dtype, f"{what} seq {b}")
        check_lse(ob, lse[:, rq][None], rlse, f"{what} seq {b}")


def _call(pr, **kw):
    return ops.mla_prefill(pr["q"], pr["kn"], pr["kr"], pr["v"], **{**pr["kw"], **kw})


@pytest.mark.parametrize("dtype,causal,rope_heads,odt", [(d, c, r, None) for d in (BF, FP) for c in (True, False) for r in (1, H)]
                         + [(BF, True, 1, F32)], ids=lambda x: str(x).replace("torch.", ""))
def test_a_ragged_batch_against_fp64(dtype, causal, rope_heads, odt):
    pr = _problem(dtype, rope_heads, seed=10 * rope_heads + causal)
    a = ops._mla_prefill_call_args(pr["q"], pr["kn"], pr["kr"], pr["v"], None, pr["kw"]["cu_seqlens_q"], pr["kw"]["cu_seqlens_k"], 257, 700,
                                   SCALE, causal, None, odt)[0]
    assert _capi_mla_prefill.describe_mla_prefill(a) == (
        f"mla_prefill_{'bf16' if dtype == BF else 'fp16'}_{'o32' if odt else 'o16'}_{'causal' if causal else 'full'}_rope{rope_heads if rope_heads == 1 else 'H'}",
        2 * len(SEQS) * H)
    out = torch.full((pr["q"].shape[0], H, 128), 7.0, dtype=odt or dtype, device=device())
    o, lse = _call(pr, causal=causal, out=out, out_dtype=odt)
    torch.cuda.synchronize()
    assert o is out and lse.shape == (H, o.shape[0]) and bool((o[pr["cu"][-1][0]:] == 7).all()), "a row behind cu_seqlens_q[B] was written"
    _check(pr, o, lse, causal, f"mla prefill {dtype} causal {causal} rope {rope_heads}")


@pytest.mark.parametrize("causal", [True, False])
def test_bit_equalities(causal):
    pr = _problem(BF, 1, seed=3)
    o, lse = _call(pr, causal=causal)
    o2, lse2 = _call(pr, causal=causal)
    for b, rq, rk in _per_sequence(pr):                                  # the packed call equals the per-sequence calls
        nq, nk = pr["seqs"][b]
        ob, lb = ops.mla_prefill(pr["q"][rq], pr["kn"][rk], pr["kr"][rk], pr["v"][rk], cu_seqlens_q=i32([0, nq]), cu_seqlens_k=i32([0, nk]),
                                 max_seqlen_q=nq, max_seqlen_k=max(nk, 1), softmax_scale=SCALE, causal=causal, return_lse=True)
        assert torch.equal(ob, o[rq]) and torch.equal(lb, lse[:, rq]), f"sequence {b} alone"
    k192 = torch.cat([pr["kn"], pr["kr"].expand(-1, H, 64)], dim=-1)
    ok, lk = ops.mla_prefill(pr["q"], v=pr["v"], k=k192, **pr["kw"], causal=causal)
    oh, lh = ops.mla_prefill(pr["q"], pr["kn"], k192[..., 128:].contiguous(), pr["v"], **pr["kw"], causal=causal)
    torch.cuda.synchronize()
    live = slice(0, pr["cu"][-1][0])
    assert bool(torch.isfinite(o[live]).all())
    assert torch.equal(o2[live], o[live]) and torch.equal(lse2[:, live], lse[:, live]), "two runs"
    assert torch.equal(ok[live], o[live]) and torch.equal(lk[:, live], lse[:, live]), "k= of width 192"
    assert torch.equal(oh[live], o[live]) and torch.equal(lh[:, live], lse[:, live]), "the rope expanded to H heads"


@pytest.mark.parametrize("causal", [True, False])
def test_every_row_counts_exactly_its_keys(causal):
    """q = 0 and the 0 / 1 probe V: a key of a neighbouring sequence, one behind a length or one past a diagonal shows by name."""
    pr = _problem(BF, 1, seed=4)
    B, S = len(SEQS), max(nk for _, nk in SEQS)
    vis = [pt.cache_visible(1, H, max(nq, 1), S, [nk], causal=causal) for nq, nk in SEQS]
    unseen = torch.cat([pt.unseen_keys(x, H) if nq else torch.ones(1, H, S, dtype=torch.bool) for x, (nq, _) in zip(vis, SEQS)])
    pv = pt.probe_v(B, H, S, 128, BF, unseen=unseen)
    for b, (_, nk) in enumerate(SEQS):
        pr["v"][pr["cu"][b][1]:pr["cu"][b][1] + nk] = pv[b, :, :nk].transpose(0, 1).to(device())
    pr["q"].zero_()
    o, lse = _call(pr, causal=causal, out_dtype=F32)
    torch.cuda.synchronize()
    for b, rq, _ in _per_sequence(pr):
        pt.check_probe(o[rq].transpose(0, 1)[None], lse[:, rq][None], pt.expected(vis[b], pv[b:b + 1]), F32, f"seq {b} {SEQS[b]}", count_mode=True)


def test_a_context_chunk_and_the_new_tokens_merge_into_attention_over_both():
    """What serving stacks build chunked and prefix-cached MLA prefill from: full attention over 200 context keys and causal attention
    over the 70 new tokens, joined by ``attn_merge``, against fp64 over all 270 keys."""
    pr = _problem(BF, 1, seed=5, seqs=[(70, 270)])
    ctx, new = slice(0, 200), slice(200, 270)
    kw = dict(cu_seqlens_q=i32([0, 70]), max_seqlen_q=70, softmax_scale=SCALE, return_lse=True)
    q = pr["q"][:70]
    oc, lc = ops.mla_prefill(q, pr["kn"][ctx], pr["kr"][ctx], pr["v"][ctx], cu_seqlens_k=i32([0, 200]), max_seqlen_k=200, causal=False, **kw)
    on, ln = ops.mla_prefill(q, pr["kn"][new], pr["kr"][new], pr["v"][new], cu_seqlens_k=i32([0, 70]), max_seqlen_k=70, causal=True, **kw)
    o, lse = ops.attn_merge([oc.transpose(0, 1)[None], on.transpose(0, 1)[None]], [lc[None], ln[None]], return_lse=True)
    torch.cuda.synchronize()
    _check(pr, o[0].transpose(0, 1), lse[0], True, "merged")


def test_a_captured_call_replays_after_both_cu_seqlens_and_the_operands_changed():
    pr = _problem(BF, 1, seed=6)
    step = lambda: _call(pr, causal=True)     # noqa: E731
    graph, (o, lse) = capture(step)
    for n in range(2):
        seqs = [SEQS[(b + 2 * n + 1) % len(SEQS)][:1] + SEQS[(b + 5 * n + 3) % len(SEQS)][1:] for b in range(len(SEQS))]      # same totals
        new = _problem(BF, 1, seed=60 + n, seqs=seqs)
        for name in ("q", "kn", "kr", "v"):
            pr[name].copy_(new[name])
        pr["kw"]["cu_seqlens_q"].copy_(new["kw"]["cu_seqlens_q"]), pr["kw"]["cu_seqlens_k"].copy_(new["kw"]["cu_seqlens_k"])
        pr["cu"], pr["seqs"] = new["cu"], seqs
        o.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        oe, le = step()
        torch.cuda.synchronize()
        live = slice(0, pr["cu"][-1][0])
        assert torch.equal(o[live], oe[live]) and torch.equal(lse[:, live], le[:, live]), f"replay {n}"
        _check(pr, o, lse, True, f"replay {n}")

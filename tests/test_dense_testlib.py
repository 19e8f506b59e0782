"""CPU tests of tests/dense_testlib.py, the reference and the checks every fp32-kernel GPU test relies on: the fp64 reference against the
oracle (outputs, LSE and autograd gradients) where the two overlap -- no mask, causal, seqlens_k --, against a direct eager
``dropout(softmax) @ v`` with a fixed keep-mask, its conventions for rows that see no key, its grouped-head gradient, and the two checks
against outputs they must reject.  The same for the attention-weights pass: ``weights_reference`` against a per-row loop, ``weights_bound``
against an fp32 emulation of the kernel's expression, ``check_weights`` and ``check_guards`` against what they must reject.  And for the
16-bit backward (the last section): ``backward_given`` against the reference's gradients, ``backward_bound`` against an emulation of the
kernels' rounding points -- the honest one inside it, five wrong ones outside -- and against the whole-tensor tolerance it replaces."""

from __future__ import annotations

import pytest
import torch

import math

from dense_testlib import (BWD16_CASES, INF, LOG2E, MUTANTS, NAN16, NAN32, TOL16, backward_bound, backward_given, backward_model,
                           bwd16_isolated, check_forward, check_grads, check_grads16, check_guards, check_weights, guarded_weights,
                           reference, seen, visible, weights_bound, weights_reference)
from oracle import fa3_oracle as orc
from photonic_flash_attention_amd import synth

B, H, SQ, SK, D = 2, 4, 7, 11, 8


def _inputs(Hkv=H, seed=0):
    """q [B,H,SQ,D], k, v [B,Hkv,SK,D], dout like q: fp32 values, as views of [B,S,H,D] arrays"""
    shapes = ((B, SQ, H, D), (B, SK, Hkv, D), (B, SK, Hkv, D), (B, SQ, H, D))
    return tuple(torch.from_numpy(synth.normal_f32(s, 40 + seed + i)).permute(0, 2, 1, 3) for i, s in enumerate(shapes))


@pytest.mark.parametrize("causal, lens", [(False, None), (True, None), (False, [SK, 3]), (True, [5, SK])])
def test_reference_matches_the_oracle_where_they_overlap(causal, lens):
    q, k, v, dout = _inputs()
    o, lse, dq, dk, dv = reference(q, k, v, causal=causal, seqlens=lens, dout=dout)
    qb, kb, vb = (t.permute(0, 2, 1, 3).clone().requires_grad_(True) for t in (q, k, v))             # the oracle's [B,S,H,D], fp32
    want = orc.attention_bshd(qb, kb, vb, causal=causal, seqlens_k=lens)
    want.backward(dout.permute(0, 2, 1, 3))
    assert o.dtype == torch.float64 and lse.dtype == torch.float64
    assert float((o.permute(0, 2, 1, 3) - want.detach()).abs().max()) <= 2e-6
    assert float((lse - orc.lse_bshd(q.permute(0, 2, 1, 3), k.permute(0, 2, 1, 3), causal=causal, seqlens_k=lens)).abs().max()) <= 2e-6
    for got, leaf in ((dq, qb), (dk, kb), (dv, vb)):
        assert float((got.permute(0, 2, 1, 3) - leaf.grad).abs().max()) <= 5e-6 * max(1.0, float(leaf.grad.abs().max()))
    assert reference(q, k, v, causal=causal, seqlens=lens)[0].equal(o)                               # without dout: the same forward


def test_reference_is_eager_dropout_of_the_softmax_under_autograd():
    q, k, v, dout = _inputs(seed=10)
    g = torch.Generator().manual_seed(3)
    drop = torch.rand(B, H, SQ, SK, generator=g) >= 0.25
    keep = torch.rand(B, 1, SQ, SK, generator=g) < 0.7
    keep[..., 0] = True
    o, lse, dq, dk, dv = reference(q, k, v, causal=True, keep=keep, drop=drop, drop_scale=4 / 3, scale=0.3, dout=dout)
    qd, kd, vd = (t.double().clone().requires_grad_(True) for t in (q, k, v))
    s = (qd @ kd.transpose(-1, -2)) * 0.3
    s = s.masked_fill(~(keep & torch.tril(torch.ones(SQ, SK, dtype=torch.bool))), -INF)
    want = (torch.softmax(s, dim=-1) * drop * (4 / 3)) @ vd
    want.backward(dout.double())
    assert float((o - want.detach()).abs().max()) <= 1e-13
    assert float((lse - torch.logsumexp(s.detach(), dim=-1)).abs().max()) <= 1e-13                   # the UN-dropped normaliser
    for got, leaf in ((dq, qd), (dk, kd), (dv, vd)):
        assert float((got - leaf.grad).abs().max()) <= 1e-12
    # an all-ones keep-mask with scale 1 is no dropout
    a = reference(q, k, v, causal=True, keep=keep, dout=dout)
    b = reference(q, k, v, causal=True, keep=keep, drop=torch.ones_like(drop), drop_scale=1.0, dout=dout)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_rows_that_see_no_key():
    q, k, v, dout = _inputs(seed=20)
    keep = torch.ones(B, H, SQ, SK, dtype=torch.bool)
    keep[0, 1, 2] = False                                 # one row of one head
    keep[1, :, :, 4:] = False                             # batch 1 sees keys 0..3 only ...
    lens = [SK + 5, -3]                                   # ... and none at all: the lengths are clamped to 0 .. SK
    o, lse, dq, dk, dv = reference(q, k, v, seqlens=lens, keep=keep, dout=dout)
    dead = torch.zeros(B, H, SQ, dtype=torch.bool)
    dead[0, 1, 2] = True
    dead[1] = True
    assert torch.equal(lse == -INF, dead) and bool(torch.isfinite(lse[~dead]).all())
    assert bool((o[dead] == 0).all()) and bool((dq[dead] == 0).all())
    assert bool((dk[1] == 0).all()) and bool((dv[1] == 0).all())                                     # keys no row sees
    assert all(bool(torch.isfinite(t).all()) for t in (o, dq, dk, dv))
    assert torch.equal(reference(q, k, v, seqlens=[SK, 0], keep=keep)[1], lse)                       # the clamped lengths
    row_seen, key_seen = seen(visible(B, H, SQ, SK, seqlens=lens, keep=keep), H)
    assert torch.equal(row_seen, ~dead) and bool(key_seen[0].all()) and not bool(key_seen[1].any())
    # the dense causal rule is top-left: with Sq < Sk row i sees keys 0 .. i, and the keys past Sq are seen by no row
    vis = visible(1, 1, SQ, SK, causal=True)[0, 0]
    assert all(int(vis[i].sum()) == i + 1 and bool(vis[i, :i + 1].all()) for i in range(SQ))
    assert not bool(seen(visible(B, H, SQ, SK, causal=True), H)[1][..., SQ:].any())


@pytest.mark.parametrize("Hkv", [1, 2])
def test_grouped_gradient_is_the_expanded_gradient_summed_per_group(Hkv):
    q, k, v, dout = _inputs(Hkv=Hkv, seed=30)
    g = H // Hkv
    o, lse, dq, dk, dv = reference(q, k, v, causal=True, dout=dout)
    ke, ve = k.repeat_interleave(g, dim=1), v.repeat_interleave(g, dim=1)
    oe, lsee, dqe, dke, dve = reference(q, ke, ve, causal=True, dout=dout)
    assert tuple(dk.shape) == (B, Hkv, SK, D) and tuple(dv.shape) == (B, Hkv, SK, D)
    assert torch.equal(o, oe) and torch.equal(lse, lsee) and torch.equal(dq, dqe)
    assert float((dk - dke.reshape(B, Hkv, g, SK, D).sum(2)).abs().max()) <= 1e-13
    assert float((dv - dve.reshape(B, Hkv, g, SK, D).sum(2)).abs().max()) <= 1e-13
    # query head h reads K/V head h // g, not h % Hkv: head 1 of a group of two reads K/V head 0
    if Hkv == 2:
        one = reference(q[:, 1:2], k[:, 0:1], v[:, 0:1], causal=True)[0]
        assert float((o[:, 1:2] - one).abs().max()) <= 1e-13


def test_the_checks_reject_what_they_must():
    q, k, v, dout = _inputs(seed=50)
    keep = torch.ones(B, 1, SQ, SK, dtype=torch.bool)
    keep[:, :, 3] = False
    keep[:, :, :, SK - 1] = False                         # a key nobody sees
    o, lse, dq, dk, dv = reference(q, k, v, keep=keep, dout=dout)
    row_seen, key_seen = seen(visible(B, H, SQ, SK, keep=keep), H)
    good = (o.float(), lse.float(), dq.float(), dk.float(), dv.float())
    check_forward(good[0], good[1], o, lse, "good")
    check_grads(good[2:], (dq, dk, dv), row_seen, key_seen, "good")

    def fwd_fails(o_, lse_):
        with pytest.raises(AssertionError):
            check_forward(o_, lse_, o, lse)

    def grads_fail(i, t, **kw):
        gs = list(good[2:])
        gs[i] = t
        with pytest.raises(AssertionError):
            check_grads(gs, (dq, dk, dv), row_seen, key_seen, **kw)

    bad = good[0].clone(); bad[0, 0, 0, 0] += 3e-5
    fwd_fails(bad, good[1])                               # over the bound
    bad = good[0].clone(); bad[0, 0, 3, 0] = 1e-30
    fwd_fails(bad, good[1])                               # a dead row that is not exactly zero
    bad = good[0].clone(); bad[1, 1, 1, 1] = float("nan")
    fwd_fails(bad, good[1])
    bad = good[1].clone(); bad[0, 0, 3] = -1e30
    fwd_fails(good[0], bad)                               # a dead row with a finite LSE
    bad = good[1].clone(); bad[0, 0, 2] = -INF
    fwd_fails(good[0], bad)                               # -inf on a row that sees keys
    bad = good[1].clone(); bad[0, 0, 2] += 3e-5
    fwd_fails(good[0], bad)
    bad = good[2].clone(); bad[0, 0, 3, 0] = 1e-30
    grads_fail(0, bad)                                    # dq of a dead row
    bad = good[3].clone(); bad[0, 0, SK - 1, 0] = 1e-30
    grads_fail(1, bad)                                    # dk of a key nobody sees
    bad = good[4].clone(); bad[0, 0, 0, 0] += 2.5e-5 * max(1.0, float(dv.abs().max()))
    grads_fail(2, bad)                                    # over the bound without dropout ...
    gs = list(good[2:]); gs[2] = bad
    check_grads(gs, (dq, dk, dv), row_seen, key_seen, "dropout bound", dropout=True)      # ... inside the one with
    grads_fail(2, good[4][:, :1])                         # a wrong shape


# --- the attention-weights pass ------------------------------------------------------------------------------------------------------

def _weights_case(g):
    """q [B,6,SQ,D], k [B,6/g,SK,D] in bf16 values, a keep-mask with dead rows, lengths that include 0 and one above SK"""
    Hq = 6
    q = torch.from_numpy(synth.normal_f32((B, SQ, Hq, D), 70 + g)).permute(0, 2, 1, 3).bfloat16()
    k = torch.from_numpy(synth.normal_f32((B, SK, Hq // g, D), 80 + g)).permute(0, 2, 1, 3).bfloat16()
    gen = torch.Generator().manual_seed(g)
    keep = torch.rand(B, Hq, SQ, SK, generator=gen) < 0.7
    keep[:, 1, 2] = False                                 # a row that sees nothing
    keep[:, :, :, 0] = True
    keep[:, 1, 2] = False
    return q, k, keep


@pytest.mark.parametrize("g", [1, 2, 3])
@pytest.mark.parametrize("causal, lens, masked", [(False, None, False), (True, None, False), (False, [0, SK + 4], False),
                                                  (True, [5, -2], True), (False, None, True), (True, [SK, 3], True)])
def test_weights_reference_against_a_per_row_loop(g, causal, lens, masked):
    q, k, keep = _weights_case(g)
    keep = keep if masked else None
    Hq, scale = q.shape[1], 0.3
    w, lse32 = weights_reference(q, k, causal=causal, seqlens=lens, keep=keep, scale=scale)
    assert w.dtype == torch.float64 and lse32.dtype == torch.float32 and tuple(w.shape) == (B, Hq, SQ, SK) and tuple(lse32.shape) == (B, Hq, SQ)
    vis = visible(B, Hq, SQ, SK, causal=causal, seqlens=lens, keep=keep)
    want = torch.zeros(B, Hq, SQ, SK, dtype=torch.float64)
    for b in range(B):
        n = SK if lens is None else min(max(lens[b], 0), SK)
        for h in range(Hq):
            for i in range(SQ):
                js = [j for j in range(n) if (not causal or j <= i) and (keep is None or bool(keep[b, h, i, j]))]
                assert js == [j for j in range(SK) if bool(vis[b, h, i, j])]
                sc = {j: scale * sum(float(q[b, h, i, d]) * float(k[b, h // g, j, d]) for d in range(D)) for j in js}
                if not js:
                    assert float(lse32[b, h, i]) == -INF
                    continue
                m = max(sc.values())
                lse = m + math.log(sum(math.exp(x - m) for x in sc.values()))
                assert float(lse32[b, h, i]) == float(torch.tensor(lse, dtype=torch.float64).float())
                for j in js:
                    want[b, h, i, j] = math.exp(sc[j] - float(lse32[b, h, i]))
    assert float((w - want).abs().max()) <= 1e-12
    assert bool((w[~vis] == 0).all())
    # a row sums to 1 up to the fp32 rounding of its LSE (|lse| 2^-24 <= 1e-6 here), a row that sees no key to exactly 0
    live = vis.any(-1)
    assert float((w.sum(-1)[live] - 1).abs().max()) <= 1e-6 and bool((w.sum(-1)[~live] == 0).all())
    # a given LSE is used as it is, and -inf in it zeroes the row
    given = lse32.clone() + 0.25
    given[0, 0, 0] = -INF
    w2, back = weights_reference(q, k, causal=causal, seqlens=lens, keep=keep, scale=scale, lse32=given)
    assert back.equal(given) and bool((w2[0, 0, 0] == 0).all())
    rest = torch.ones(B, Hq, SQ, dtype=torch.bool)
    rest[0, 0, 0] = False
    shift = torch.exp(torch.nan_to_num(lse32.double() - given.double(), nan=0.0, neginf=0.0))[..., None]       # (fp32 sum: not exactly 0.25)
    assert float((w2 - w * shift)[rest].abs().max()) <= 1e-12


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("Dh", [64, 128])
@pytest.mark.parametrize("qscale", [1.0, 2.5])
def test_fp32_emulation_of_the_kernel_stays_inside_the_weights_bound(dt, Dh, qscale):
    """torch's fp32 matmul, the fp32 product ``lse * log2e`` and an fp32 ``exp2`` are the kernel's arithmetic up to the order of the sums
    and one more rounding (no fma): well inside ``weights_bound`` for an fp32 W, and inside it for the 16-bit stores."""
    Bq, Hq, Sq, Sk = 1, 2, 96, 160
    name = "bf16" if dt == torch.bfloat16 else "fp16"
    q, k, _ = (t.permute(0, 2, 1, 3) for t in synth.qkv(Bq, Hq, Sq, Sk, Dh, 90 + Dh, name))
    q = (q.float() * qscale).to(dt)
    lens = [Sk - 9]
    ref, lse32 = weights_reference(q, k, causal=True, seqlens=lens)
    vis = visible(Bq, Hq, Sq, Sk, causal=True, seqlens=lens)
    c = torch.tensor(Dh ** -0.5 * LOG2E, dtype=torch.float32)
    e = (q.float() @ k.float().transpose(-1, -2)) * c - (lse32 * torch.tensor(LOG2E, dtype=torch.float32))[..., None]
    w32 = torch.where(vis, torch.exp2(e), torch.zeros((), dtype=torch.float32))
    assert w32.dtype == torch.float32
    r32 = check_weights(w32, ref, weights_bound(q, k, ref, lse32, wdt=torch.float32), vis, "emulation, fp32 W", wdt=torch.float32)
    r16 = check_weights(w32.to(dt), ref, weights_bound(q, k, ref, lse32, wdt=dt), vis, f"emulation, {name} W", wdt=dt)
    assert r32 <= 0.25 and r16 <= 1.0, (r32, r16)
    if qscale > 1 and dt == torch.float16:
        assert bool(((w32.to(dt) > 0) & (w32.to(dt) < 2.0 ** -14)).any())        # fp16 subnormals do occur at this scale


def test_check_weights_rejects_what_it_must():
    Bq, Hq, Sq, Sk, Dh = 2, 3, 40, 72, 64
    q, k, _ = (t.permute(0, 2, 1, 3) for t in synth.qkv(Bq, Hq, Sq, Sk, Dh, 95, "bf16"))
    ref, lse32 = weights_reference(q, k, causal=True)
    vis = visible(Bq, Hq, Sq, Sk, causal=True)
    bound = weights_bound(q, k, ref, lse32)
    good = ref.float()
    assert check_weights(good, ref, bound, vis, "good", wdt=torch.float32) <= 1.0

    def fails(w, **kw):
        with pytest.raises(AssertionError):
            check_weights(w, ref, bound, vis, **kw)

    bad = good.clone(); bad[1, 2, 30, 7], bad[1, 2, 30, 8] = good[1, 2, 30, 8], good[1, 2, 30, 7]
    fails(bad)                                            # two neighbouring keys swapped in one row
    bad = good.clone(); bad[0, 1, 17] *= 1.001
    fails(bad)                                            # one row scaled
    bad = good.clone(); bad[0, 0, 3, 4] = 1e-30
    fails(bad)                                            # a non-zero above the diagonal
    bad = good.clone(); bad[1, 0, 5, 2] = float("nan")
    fails(bad)
    bad = good.clone(); bad[0, 1], bad[0, 2] = good[0, 2], good[0, 1]
    fails(bad)                                            # one head's rows exchanged with another's
    fails(good, wdt=torch.bfloat16)                       # not the dtype asked for
    fails(good[:, :2])                                    # a wrong shape
    b16 = weights_bound(q, k, ref, lse32, wdt=torch.bfloat16)
    assert check_weights(good.bfloat16(), ref, b16, vis, "good bf16", wdt=torch.bfloat16) <= 1.0
    with pytest.raises(AssertionError):
        check_weights((good * (1 + 2.0 ** -6)).bfloat16(), ref, b16, vis)         # beyond the bf16 rounding


@pytest.mark.parametrize("wdt, pat", [(torch.float32, NAN32), (torch.bfloat16, NAN16), (torch.float16, NAN16)])
def test_check_guards_rejects_a_stray_store_and_a_missing_one(wdt, pat):
    Bq, Hq, Sq, Sk, pad, off = 2, 2, 5, 9, 3, 1
    inner, ibuf = guarded_weights(wdt, Bq, Hq, Sq, Sk, pad=pad, col_off=off, device="cpu")
    assert tuple(inner.shape) == (Bq, Hq, Sq, Sk) and tuple(ibuf.shape) == (Bq, Hq + 1, 32 + Sq + 32, off + Sk + pad)
    assert bool(torch.isnan(inner.float()).all()) and bool((ibuf == pat).all())
    with pytest.raises(AssertionError):
        check_guards(ibuf, Hq, Sq, Sk, off)               # nothing written yet
    inner.copy_(torch.rand(Bq, Hq, Sq, Sk).to(wdt))
    check_guards(ibuf, Hq, Sq, Sk, off)
    for at in [(0, 0, 31, off), (0, 0, 32, off - 1), (1, 1, 32 + Sq, off + Sk - 1), (0, 1, 33, off + Sk), (1, Hq, 32, off)]:
        stray = ibuf.clone()
        stray[at] = 0                                     # the row in front, the column in front, the row behind, the column behind, the next head
        with pytest.raises(AssertionError):
            check_guards(stray, Hq, Sq, Sk, off)
    missing = ibuf.clone()
    missing[1, 1, 32 + Sq - 1, off + Sk - 1] = pat
    with pytest.raises(AssertionError):
        check_guards(missing, Hq, Sq, Sk, off)


# --- the 16-bit backward -------------------------------------------------------------------------------------------------------------

DT16 = [torch.bfloat16, torch.float16]
DT16_IDS = ["bf16", "fp16"]
CASE_IDS = [f"case{min(i + 1, 12)}{'b' if i == 12 else ''}" for i in range(len(BWD16_CASES))]


@pytest.mark.parametrize("idx", [0, 2, 3, 4, 6, 9, 10], ids=lambda i: CASE_IDS[i])
def test_backward_given_with_exact_forward_operands_is_the_gradient(idx):
    """With the exact fp64 ``o`` and ``lse`` the formula the kernels evaluate is the gradient: ``reference``'s autograd, to 1e-12 relative."""
    p = bwd16_isolated(idx, torch.bfloat16)
    kw = p["kw"]
    keep = kw["mask"] if "mask" in kw else (kw["key_mask"][:, None, None, :] if "key_mask" in kw else None)
    o, lse, *true = reference(p["q"], p["k"], p["v"], causal=p["causal"], seqlens=kw.get("seqlens_k"), keep=keep, scale=p["scale"], dout=p["dout"])
    dq, dk, dv, parts = backward_given(p["q"], p["k"], p["v"], o, p["dout"], lse, vis=p["vis"], scale=p["scale"])
    for name, got, want in zip(("dq", "dk", "dv"), (dq, dk, dv), true):
        assert got.dtype == torch.float64 and tuple(got.shape) == tuple(want.shape), name
        assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), name
    assert bool((parts["P"][~p["vis"]] == 0).all()) and float((parts["P"].sum(-1)[p["row_seen"]] - 1).abs().max()) <= 1e-12
    assert bool((dq[~p["row_seen"]] == 0).all()) and bool((dk[~p["key_seen"]] == 0).all()) and bool((dv[~p["key_seen"]] == 0).all())


@pytest.mark.parametrize("dt", DT16, ids=DT16_IDS)
@pytest.mark.parametrize("idx", range(len(BWD16_CASES)), ids=CASE_IDS)
def test_honest_model_of_the_backward_stays_inside_its_bound(idx, dt):
    """The emulation of the kernels' rounding points is within ``backward_bound`` at every element of every GPU case (the worst ratio is
    printed: 0.63 bf16 / 0.50 fp16 over the cases), the bound is exactly zero where nothing is seen, and the new check implies the one it
    stands beside: no element's bound exceeds ``TOL16 * max|ref|`` of its gradient (at most 1.48e-2 bf16, 2.1e-3 fp16 over the cases)."""
    p = bwd16_isolated(idx, dt)
    model = backward_model(p["q"], p["k"], p["v"], p["o16"], p["dout"], p["lse32"], vis=p["vis"], scale=p["scale"], dtype=dt)
    worst = check_grads16(model, p["given"], p["bounds"], p["row_seen"], p["key_seen"], f"{CASE_IDS[idx]} model")
    assert max(worst) <= 1.0
    for name, b, live, true in zip(("dq", "dk", "dv"), p["bounds"], (p["row_seen"], p["key_seen"], p["key_seen"]), p["true"]):
        assert bool((b[~live] == 0).all()) and bool((b[live] > 0).all()) and bool(torch.isfinite(b).all()), name
        top = float(true.abs().max())
        if top > 0:                                        # (case 1: one key, dq and dk are exactly zero)
            print(f"{CASE_IDS[idx]} {name}: max bound / max|ref| {float(b.max()) / top:.3e} (whole-tensor tolerance {TOL16[dt]:.1e})")
            assert float(b.max()) <= TOL16[dt] * top, name
    assert idx != 0 or (float(p["true"][0].abs().max()) == 0 and float(p["true"][1].abs().max()) == 0)


# where a mutant changes nothing that a check could see
NOT_APPLICABLE = {(0, "dq_dk_scaled"), (0, "last_key_dropped"),                     # one key: dq = dk = 0, dS = 0
                  (5, "last_key_dropped"), (7, "last_key_dropped"),                  # causal with Sk > Sq: no row sees the last key
                  (4, "diagonal_dropped")}                                           # Sq > Sk: the last 32 rows have no diagonal key
NOT_APPLICABLE |= {(i, "diagonal_dropped") for i, c in enumerate(BWD16_CASES) if not c[6]}
# cases 3 and 4: the worst err / bound of a CPU prototype of this bound, halved for ROUND16's u
REQUIRED = {"delta0_last_rows": 28.0, "p_scaled_last_block": 5.8, "dq_dk_scaled": 2.6, "last_key_dropped": 10.0, "diagonal_dropped": 24.0}


@pytest.mark.parametrize("dt", DT16, ids=DT16_IDS)
@pytest.mark.parametrize("idx, mutant", [(i, m) for i in range(len(BWD16_CASES)) for m in MUTANTS if (i, m) not in NOT_APPLICABLE],
                         ids=lambda x: CASE_IDS[x] if isinstance(x, int) else x)
def test_wrong_backward_models_are_over_the_bound(idx, mutant, dt):
    """Each wrong kernel that the whole-tensor tolerance lets through puts at least one element over its bound wherever it changes anything,
    and by the prototype's margin at case 3 (causal, 300 x 300, D 128) and case 4 (full, grouped heads)."""
    p = bwd16_isolated(idx, dt)
    model = backward_model(p["q"], p["k"], p["v"], p["o16"], p["dout"], p["lse32"], vis=p["vis"], scale=p["scale"], dtype=dt, mutant=mutant)
    worst = 0.0
    for got, ref, b in zip(model, p["given"], p["bounds"]):
        err = (got.double() - ref).abs()
        worst = max(worst, float(torch.where(err > 0, err / b, torch.zeros((), dtype=torch.float64)).max()))
    print(f"{CASE_IDS[idx]} {mutant}: worst err / bound {worst:.2f}")
    assert worst > (REQUIRED[mutant] if idx in (2, 3) else 1.0)
    with pytest.raises(AssertionError):
        check_grads16(model, p["given"], p["bounds"], p["row_seen"], p["key_seen"])


def test_check_grads16_rejects_what_it_must():
    p = bwd16_isolated(9, torch.float16)                   # rows 5 and 100..132 see nothing
    good = tuple(g.float() for g in p["given"])
    args = (p["given"], p["bounds"], p["row_seen"], p["key_seen"])
    assert max(check_grads16(good, *args, "good")) <= 1.0

    def fails(i, t):
        gs = list(good)
        gs[i] = t
        with pytest.raises(AssertionError):
            check_grads16(gs, *args)

    bad = good[0].clone(); bad[0, 1, 5, 3] = 1e-30
    fails(0, bad)                                          # dq of a row that sees nothing
    bad = good[0].clone(); bad[0, 0, 7, 1] = float("nan")
    fails(0, bad)
    b1 = torch.where(p["bounds"][1] > 0, p["bounds"][1], torch.full((), INF, dtype=torch.float64))
    at = tuple(int(x) for x in torch.nonzero(b1 == b1.min())[0])                    # the seen key element with the tightest bound
    bad = good[1].clone(); bad[at] += 1.5 * float(p["bounds"][1][at])
    fails(1, bad)                                          # one element over its own bound, far below the tensor's largest
    assert 1.5 * float(p["bounds"][1][at]) < 0.1 * TOL16[torch.float16] * float(p["given"][1].abs().max())
    fails(2, good[2].double())                             # not an fp32 store
    fails(2, good[2][:, :1])                               # a wrong shape
    # a key nobody sees: case 6's keys past Sq
    p = bwd16_isolated(5, torch.bfloat16)
    good = [g.float() for g in p["given"]]
    good[2][0, 0, 400, 0] = 1e-30
    with pytest.raises(AssertionError):
        check_grads16(good, p["given"], p["bounds"], p["row_seen"], p["key_seen"])

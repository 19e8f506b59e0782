"""CPU tests of tests/dense_testlib.py, the reference and the checks every fp32-kernel GPU test relies on: the fp64 reference against the
oracle (outputs, LSE and autograd gradients) where the two overlap -- no mask, causal, seqlens_k --, against a direct eager
``dropout(softmax) @ v`` with a fixed keep-mask, its conventions for rows that see no key, its grouped-head gradient, and the two checks
against outputs they must reject."""

from __future__ import annotations

import pytest
import torch

from dense_testlib import INF, check_forward, check_grads, reference, seen, visible
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

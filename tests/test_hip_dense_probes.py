"""GPU tests of WHICH KEYS A ROW SEES in the dense forward -- ``ops.fa3_forward`` on every kernel family (selector 44: the 8-wave HIP
kernel, 43: the 4-wave HIP kernel, 45: the persistent assembly kernel, and the default choice), the exact fp32 kernel, and the packed
``ops.fa3_varlen_forward`` -- with the exact probes of tests/probe_testlib.py (``count`` and ``stair``; see
tests/test_hip_cache_probes.py).  The rules: top-left causal, ``seqlens_k``, a ``[B,Sk]`` key mask, 3-D and 4-D element masks.  Every
case asserts through ``_capi.describe`` which kernel family ran; ``family`` below spells the library's choice out."""

from __future__ import annotations

import pytest
import torch

from photonic_flash_attention_amd import _capi, ops
from probe_testlib import check_probe, count, dense_visible, expected, probe_v, stair, unseen_keys

pytestmark = pytest.mark.gpu

BF, FP, F32 = torch.bfloat16, torch.float16, torch.float32
DEV = "cuda:0"
PROBES = ("count", "stair")


def family(selector, *, D, Sq, Sk, causal, o32, key_mask=False, mask=False):
    """The family ``pfa_fa3_fwd`` picks (csrc/pfa_capi.hip ``pick``): the persistent kernel takes selector 45 and the default where it is
    eligible (no element mask, Sq >= 128, Sk >= 193, causal only square); the 4-wave kernel D 128 with a 16-bit store and no mask, on
    selector 43 or from 16 key tiles a workgroup on; the 8-wave kernel everything else."""
    if selector in (0, 45) and not mask and Sq >= 128 and Sk >= 193 and (not causal or Sq == Sk):
        return "fa3_fwd_p4_"
    if D == 128 and not o32 and not key_mask and not mask and (selector == 43 or (selector in (0, 45) and (Sk // 2 if causal else Sk) // 64 >= 16)):
        return "fa3_fwd_w4_"
    return "fa3_fwd_bf16_", "fa3_fwd_fp16_"


def _steps(Sk, b=0):
    """The kernels move a row's running maximum only on a jump above 8 (in log2 units) and otherwise keep the stale one.  Even b: a
    jump of 9 a third in (the rescale branch), then 12 behind the middle (3 more: deferred, weights up to 2^3), 6 on the last key, 2
    at the head of the second 256-row block's diagonal tile.  Odd b: a jump of exactly 8 (deferred), then 11 (above 8 from the stale
    maximum: the rescale), and 3 on the last key."""
    marks = ((Sk // 3, 9), (Sk // 2 + 5, 12), (Sk - 1, 6), (min(256, Sk - 2), 2)) if b % 2 == 0 else ((Sk // 3, 8), (Sk // 2 + 5, 11), (Sk - 1, 3))
    return {j: h for j, h in marks if 0 <= j < Sk}


def run_dense(what, *, B, H, Hkv, Sq, Sk, D, dtype, selectors, causal=False, seqlens=None, key_mask=None, mask=None, probes=PROBES):
    vis = dense_visible(B, H, Sq, Sk, causal=causal, seqlens=seqlens, key_mask=key_mask, mask=mask)
    kw = dict(causal=causal)
    if seqlens is not None:
        kw["seqlens_k"] = seqlens
    if key_mask is not None:
        kw["key_mask"] = key_mask.to(DEV)
    if mask is not None:
        kw["mask"] = mask.to(DEV)
    for kind in probes:
        pr = count(B, H, Hkv, Sq, Sk, D, dtype) if kind == "count" else stair(B, H, Hkv, Sq, Sk, D, dtype, [_steps(Sk, b) for b in range(B)])
        v = probe_v(B, Hkv, Sk, D, dtype, unseen_keys(vis, Hkv))
        exp = expected(vis, v, pr["steps"])
        q, k, vd = pr["q"].to(DEV), pr["k"].to(DEV), v.to(DEV)
        for n, sel in enumerate(selectors):
            # fp32 and 16-bit stores alternate over the selectors and the probes; the 4-wave kernel has the 16-bit store only (an
            # fp32 store means split P, which selector 43 hands to the 8-wave kernel), so at D 128 it gets both probes with it
            w4 = sel == 43 and D == 128 and key_mask is None and mask is None
            o32 = dtype != F32 and not w4 and (n + (kind == "stair")) % 2 == 0
            odt = F32 if o32 or dtype == F32 else dtype
            out = torch.empty(B, Sq, H, D, dtype=odt, device=DEV).permute(0, 2, 1, 3)
            name = _capi.describe(ops.build_args(q, k, vd, out, split_p=o32, variant=sel, **kw)[0])[0]
            if dtype == F32:
                assert name.startswith("fa3_fwd_f32_"), name
            else:
                assert name.startswith(family(sel, D=D, Sq=Sq, Sk=Sk, causal=causal, o32=o32, key_mask=key_mask is not None, mask=mask is not None)), name
                assert not w4 or name.startswith("fa3_fwd_w4_"), name
            o, lse = ops.fa3_forward(q, k, vd, softmax_scale=pr["scale"], out_dtype=odt, return_lse=True, _variant=sel or None, **kw)
            torch.cuda.synchronize()
            check_probe(o, lse, exp, odt, f"dense {what} {kind} selector {sel} {name}", kind == "count")


# --- 1. the shapes, on every family ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D,dtype", [(128, BF), (64, FP)], ids=["d128-bf16", "d64-fp16"])
def test_causal_769_three_blocks_and_one_row(D, dtype):
    """Three 256-row blocks and one row; the default choice is the persistent kernel's ragged (``kl``) flavour."""
    q = torch.zeros(2, 4, 769, D, dtype=dtype, device=DEV)
    name = _capi.describe(ops.build_args(q, q[:, :2], q[:, :2], torch.empty_like(q), causal=True)[0])[0]
    assert name.startswith("fa3_fwd_p4_") and "_kl_" in name, name
    run_dense("769 causal", B=2, H=4, Hkv=2, Sq=769, Sk=769, D=D, dtype=dtype, selectors=(44, 43, 45, 0), causal=True)


@pytest.mark.parametrize("D,dtype", [(128, FP), (64, BF)], ids=["d128-fp16", "d64-bf16"])
def test_full_300_by_1000(D, dtype):
    run_dense("300x1000", B=2, H=4, Hkv=2, Sq=300, Sk=1000, D=D, dtype=dtype, selectors=(44, 43, 45, 0))


def test_full_257_by_193_on_the_hip_kernels():
    """Four key tiles, the last of one key.  193 keys are the fewest the persistent kernel takes (``p4_eligible``), 192 -- the shape of
    tests/test_hip_parity.py -- it does not: the default choice there is a HIP kernel."""
    q = torch.zeros(2, 4, 257, 128, dtype=BF, device=DEV)
    k = torch.zeros(2, 2, 193, 128, dtype=BF, device=DEV)
    assert "p4" not in _capi.describe(ops.build_args(q, k[:, :, :192], k[:, :, :192], torch.empty_like(q))[0])[0]
    assert "p4" in _capi.describe(ops.build_args(q, k, k, torch.empty_like(q))[0])[0]
    run_dense("257x193", B=2, H=4, Hkv=2, Sq=257, Sk=193, D=128, dtype=BF, selectors=(44, 43))
    run_dense("257x193", B=2, H=4, Hkv=2, Sq=257, Sk=193, D=64, dtype=FP, selectors=(44,))


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("D,dtype", [(128, BF), (64, FP)], ids=["d128-bf16", "d64-fp16"])
def test_aligned_1024(D, dtype, causal):
    run_dense("1024 aligned", B=2, H=4, Hkv=2, Sq=1024, Sk=1024, D=D, dtype=dtype, selectors=(44, 43, 45, 0), causal=causal)


# --- 2. the visibility rules ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
def test_seqlens_k(causal):
    """0, 1, 517 and all keys; causal on the square shape the persistent kernel takes."""
    Sq = 1000 if causal else 300
    run_dense("seqlens_k", B=4, H=4, Hkv=2, Sq=Sq, Sk=1000, D=128, dtype=BF, selectors=(44, 45, 0), causal=causal, seqlens=[0, 1, 517, 1000])


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
def test_key_mask_with_a_hidden_batch(causal):
    B, Sk = 3, 1000
    km = torch.rand(B, Sk, generator=torch.Generator().manual_seed(21)) > 0.35
    km[1] = False
    km[2, :300] = False                                              # left padding
    Sq = Sk if causal else 300
    run_dense("key mask", B=B, H=4, Hkv=2, Sq=Sq, Sk=Sk, D=64, dtype=FP, selectors=(44, 45, 0), causal=causal, key_mask=km)


@pytest.mark.parametrize("dims", [3, 4])
def test_element_masks_with_fully_masked_rows(dims):
    B, H, Sq, Sk = 2, 4, 300, 1000
    g = torch.Generator().manual_seed(22 + dims)
    m = torch.rand((B, Sq, Sk) if dims == 3 else (B, H, Sq, Sk), generator=g) > 0.5
    m[0, ..., 7, :] = False                                          # fully masked rows
    m[1, ..., 256:260, :] = False
    m[1, ..., 299, :999] = False                                     # a row that sees the last key alone
    run_dense(f"{dims}-D mask", B=B, H=H, Hkv=2, Sq=Sq, Sk=Sk, D=128 if dims == 3 else 64, dtype=BF if dims == 3 else FP, selectors=(44, 0),
              causal=dims == 4, mask=m.to(torch.uint8) if dims == 4 else m)


def test_exact_fp32_kernel_counts():
    """fp32 operands run the exact kernel: ``count`` only (its scores are not in log2 units), Sq 130 over 257 keys."""
    km = torch.rand(2, 257, generator=torch.Generator().manual_seed(23)) > 0.3
    for kw in (dict(), dict(causal=True), dict(seqlens=[257, 65]), dict(key_mask=km, causal=True)):
        run_dense(f"fp32 {sorted(kw)}", B=2, H=4, Hkv=2, Sq=130, Sk=257, D=64, dtype=F32, selectors=(0,), probes=("count",), **kw)


# --- 3. the packed forward --------------------------------------------------------------------------------------------------------------

SELF = ([1, 31, 33, 64, 255, 256, 257, 300, 0, 128],) * 2            # the lengths of tests/test_hip_varlen.py
CROSS = ([5, 0, 257, 64], [129, 7, 0, 300])


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("layout,D,dtype", [("self", 128, BF), ("cross", 64, FP), ("cross", 128, FP), ("self", 64, BF)])
def test_varlen_forward(layout, D, dtype, causal):
    lq, lk = SELF if layout == "self" else CROSS
    H, Hkv, B = 4, 2, len(lq)
    cq, ck = [0], [0]
    for a, b in zip(lq, lk):
        cq.append(cq[-1] + a)
        ck.append(ck[-1] + b)
    cu_q, cu_k = (torch.tensor(c, dtype=torch.int32, device=DEV) for c in (cq, ck))
    vis = [dense_visible(1, H, max(lq[b], 1), max(lk[b], 1), causal=causal, seqlens=[lk[b]]) for b in range(B)]
    for kind in PROBES:
        prs = [count(1, H, Hkv, max(lq[b], 1), max(lk[b], 1), D, dtype, seed=b) if kind == "count" else
               stair(1, H, Hkv, max(lq[b], 1), max(lk[b], 1), D, dtype, _steps(max(lk[b], 1), b), seed=b) for b in range(B)]
        vs = [probe_v(1, Hkv, max(lk[b], 1), D, dtype, unseen_keys(vis[b], Hkv)) for b in range(B)]
        q = torch.cat([prs[b]["q"][0, :, :lq[b]].permute(1, 0, 2) for b in range(B)]).to(DEV)
        k = torch.cat([prs[b]["k"][0, :, :lk[b]].permute(1, 0, 2) for b in range(B)]).to(DEV)
        v = torch.cat([vs[b][0, :, :lk[b]].permute(1, 0, 2) for b in range(B)]).to(DEV)
        for o32 in (False, True):
            odt = F32 if o32 else dtype
            a = _capi.make_varlen_args(q=q.data_ptr(), k=k.data_ptr(), v=v.data_ptr(), o=0x1000, cu_seqlens_q=cu_q.data_ptr(), cu_seqlens_k=cu_k.data_ptr(),
                                       q_stride_s=H * D, q_stride_h=D, k_stride_s=Hkv * D, k_stride_h=D, v_stride_s=Hkv * D, v_stride_h=D,
                                       o_stride_s=H * D, o_stride_h=D, B=B, H=H, Hkv=Hkv, total_q=cq[-1], total_k=ck[-1], max_seqlen_q=max(lq),
                                       max_seqlen_k=max(lk), D=D, dtype_in=0 if dtype == BF else 1, dtype_out=2 if o32 else (0 if dtype == BF else 1),
                                       causal=1 if causal else 0, softmax_scale=1.0)
            name = _capi.describe_varlen(a)[0]
            assert name == (f"fa3_fwd_varlen_{'bf16' if dtype == BF else 'fp16'}_d{D}_{'causal' if causal else 'full'}"
                            f"{'_splitp_o32' if o32 else '_o16'}"), name
            o, lse = ops.fa3_varlen_forward(q, k, v, cu_seqlens_q=cu_q, cu_seqlens_k=cu_k, max_seqlen_q=max(lq), max_seqlen_k=max(lk), causal=causal,
                                            softmax_scale=prs[0]["scale"], out_dtype=odt, return_lse=True)
            torch.cuda.synchronize()
            for b in range(B):
                if lq[b] == 0:
                    continue
                vb, stb = (vs[b], prs[b]["steps"]) if lk[b] else (torch.zeros_like(vs[b]), None)
                exp = expected(vis[b] if lk[b] else torch.zeros_like(vis[b]), vb, stb)
                check_probe(o[cq[b]:cq[b + 1]].permute(1, 0, 2)[None], lse[None, :, cq[b]:cq[b + 1]], exp, odt,
                            f"dense varlen {layout} {kind} {'o32' if o32 else 'o16'} sequence {b}", kind == "count")

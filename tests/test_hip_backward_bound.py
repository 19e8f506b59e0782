"""GPU tests of the 16-bit dense backward (``fa3_bwd_dq_kernel`` / ``fa3_bwd_dkdv_kernel``, the training hot path) against a per-element
a-priori bound, where tests/test_hip_backward.py and its neighbours compare every element with the largest one of its tensor.

Reference: ``dense_testlib.backward_given`` -- fp64 on the CPU of what the kernels compute from the operands they are handed.  Bound:
``dense_testlib.backward_bound`` -- C_P = 3 times the root of the summed squares of the 16-bit roundings of P and dS, plus the worst case of
everything that stays in fp32; fixed by the derivation in its docstring, by ``ROUND16`` and by ``C_P``, never by a measurement.
tests/test_dense_testlib.py shows on the CPU that an honest model of the kernels is inside it and that five wrong ones are outside.

Every case of ``dense_testlib.BWD16_CASES`` (shapes on the kernels' block, wave and tile edges) runs with fp32-stored gradients in two modes:

  isolated   ``o`` is the fp64 reference output rounded to 16 bits and ``lse`` the fp64 LSE rounded to fp32, both made on the CPU: the
             backward depends on no forward kernel
  chained    ``o`` and ``lse`` come from ``ops.fa3_forward`` as in training; the whole-tensor criterion of tests/test_hip_backward.py against
             the TRUE gradients and the 16-bit store's one rounding (tests/test_hip_backward_store.py) are asserted beside the bound

The measured worst ``err / bound`` per case are in profiles/backward_bound.md."""

from __future__ import annotations

import pytest
import torch

from dense_testlib import (BWD16_CASES, DEV, TOL16, backward_bound, backward_given, bwd16_isolated, check_grads16)

pytestmark = pytest.mark.gpu

DT16 = [torch.bfloat16, torch.float16]
DT16_IDS = ["bf16", "fp16"]
CASE_IDS = [f"case{min(i + 1, 12)}{'b' if i == 12 else ''}" for i in range(len(BWD16_CASES))]


def _on_device(p):
    """the problem's operands and keywords on the GPU, laid out as on the CPU ([B,H,S,D] views of [B,S,H,D] arrays)"""
    q, k, v, dout = (p[n].permute(0, 2, 1, 3).contiguous().to(DEV).permute(0, 2, 1, 3) for n in ("q", "k", "v", "dout"))
    kw = {n: (m.to(DEV) if isinstance(m, torch.Tensor) else m) for n, m in p["kw"].items()}
    return q, k, v, dout, kw


@pytest.mark.parametrize("dt", DT16, ids=DT16_IDS)
@pytest.mark.parametrize("idx", range(len(BWD16_CASES)), ids=CASE_IDS)
def test_isolated_backward_within_its_bound(idx, dt):
    from photonic_flash_attention_amd import ops
    p = bwd16_isolated(idx, dt)
    q, k, v, dout, kw = _on_device(p)
    o = p["o16"].permute(0, 2, 1, 3).contiguous().to(DEV).permute(0, 2, 1, 3)
    grads = ops.fa3_backward(q, k, v, o, dout, p["lse32"].contiguous().to(DEV), causal=p["causal"], grad_dtype=torch.float32, **kw)
    torch.cuda.synchronize()
    check_grads16(grads, p["given"], p["bounds"], p["row_seen"], p["key_seen"], f"{CASE_IDS[idx]} {DT16_IDS[DT16.index(dt)]} isolated")


@pytest.mark.parametrize("dt", DT16, ids=DT16_IDS)
@pytest.mark.parametrize("idx", range(len(BWD16_CASES)), ids=CASE_IDS)
def test_chained_backward_within_its_bound(idx, dt):
    from photonic_flash_attention_amd import ops
    p = bwd16_isolated(idx, dt)
    q, k, v, dout, kw = _on_device(p)
    what = f"{CASE_IDS[idx]} {DT16_IDS[DT16.index(dt)]} chained"
    out, lse = ops.fa3_forward(q, k, v, causal=p["causal"], return_lse=True, **kw)
    g32 = ops.fa3_backward(q, k, v, out, dout, lse, causal=p["causal"], grad_dtype=torch.float32, **kw)
    g16 = ops.fa3_backward(q, k, v, out, dout, lse, causal=p["causal"], **kw)                         # the training path
    torch.cuda.synchronize()
    assert out.dtype == dt and lse.dtype == torch.float32
    assert torch.equal(torch.isfinite(lse).cpu(), p["row_seen"]), f"{what}: the forward's finite LSEs are not the rows that see a key"
    # the bound, for the operands actually handed over
    *given, parts = backward_given(p["q"], p["k"], p["v"], out.cpu(), p["dout"], lse.cpu(), vis=p["vis"], scale=p["scale"])
    bounds = backward_bound(p["q"], p["k"], p["v"], out.cpu(), p["dout"], lse.cpu(), parts, scale=p["scale"], dtype=dt)
    check_grads16(g32, given, bounds, p["row_seen"], p["key_seen"], what)
    for name, got, narrow, true in zip(("dq", "dk", "dv"), g32, g16, p["true"]):
        # the whole-tensor criterion of tests/test_hip_backward.py, against the true gradients
        wide = got.cpu().double()
        err, top = float((wide - true).abs().max()), float(true.abs().max())
        cos = float(torch.nn.functional.cosine_similarity(wide.flatten(), true.flatten(), dim=0)) if top > 0 else 1.0
        print(f"{what} {name}: against the true gradient max-abs {err:.3e} (bound {TOL16[dt] * top + 1e-6:.3e}), cosine {cos:.6f}")
        assert err <= TOL16[dt] * top + 1e-6, f"{what} {name}: err {err:.3e} vs max {top:.3e}"
        assert cos >= 0.9995, f"{what} {name}: cosine {cos}"
        # the 16-bit store: the same arithmetic up to the epilogue, rounded once
        assert narrow.dtype == dt and tuple(narrow.shape) == tuple(true.shape), (name, narrow.dtype, tuple(narrow.shape))
        assert torch.equal(got.to(dt), narrow), f"{what} {name}: the 16-bit store is not the rounded fp32 store"


@pytest.mark.parametrize("dt", DT16, ids=DT16_IDS)
def test_the_two_kernels_agree_on_delta(dt):
    """The dQ kernel publishes ``delta`` per row and the dK/dV kernel reads it back.  Rows with ``dout = 0`` have ``delta = 0`` and
    ``dP = 0``, so they add exactly nothing to dk and dv -- unless the dK/dV kernel pairs a row with another row's delta.  Case 2's shape
    (not causal: every row sees every key), ``dout = 0`` on rows 20..32, bit for bit against the call on rows 0..19 alone.  The zeroed rows
    are the LAST ones so that the remaining rows keep their places in the 64-row tiles and both calls sum in the same order; they share a
    16-row MFMA step (rows 16..31) and a 32-row half (row 32 opens the second) with live rows."""
    from photonic_flash_attention_amd import ops
    p = bwd16_isolated(1, dt)
    assert not p["causal"] and not p["kw"] and p["q"].shape[2] == 33
    q, k, v, dout, _ = _on_device(p)
    n = 20
    o = p["o16"].permute(0, 2, 1, 3).contiguous().to(DEV).permute(0, 2, 1, 3)
    lse = p["lse32"].contiguous().to(DEV)
    dz = dout.clone()
    dz[:, :, n:] = 0
    _, dk_all, dv_all = ops.fa3_backward(q, k, v, o, dz, lse, grad_dtype=torch.float32)
    _, dk_few, dv_few = ops.fa3_backward(q[:, :, :n], k, v, o[:, :, :n], dout[:, :, :n], lse[:, :, :n].contiguous(), grad_dtype=torch.float32)
    torch.cuda.synchronize()
    assert float(dk_few.abs().max()) > 0 and float(dv_few.abs().max()) > 0
    assert torch.equal(dk_all, dk_few), f"dk: rows with dout = 0 add {float((dk_all - dk_few).abs().max()):.3e}"
    assert torch.equal(dv_all, dv_few), f"dv: rows with dout = 0 add {float((dv_all - dv_few).abs().max()):.3e}"

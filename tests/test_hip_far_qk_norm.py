"""GPU tests of ``ops.qk_norm`` -- one forward and one backward call -- on tensors spread past 4 and 8 GiB, built with
tests/far_testlib.py as tests/test_hip_far_rotary.py builds its case: packed Q and K with their outputs (the backward: x, dy and dx of
both) in one 12.5 GiB arena, the packed rows 2^22 + 8 elements apart -- the 32-bit product of row and stride wraps from row 256 on, the
last row lies 8.3 GiB from its tensor's first -- and the fp32 tables 4 GiB deep.  ``far_testlib.two_runs`` asserts that the library saw
the far views, that both runs name one kernel, that the far run's outputs (the weight gradients among them) are the near run's bit for
bit, that the near run is the CPU model's (dw: inside the bound of tests/qk_norm_testlib.py), and that nothing in the arena outside the
declared outputs changed.  The layouts are checked on the host without a GPU."""

from __future__ import annotations

import pytest
import torch

import far_testlib as F
import qk_norm_testlib as Q
from far_testlib import FarCase, Spec
from photonic_flash_attention_amd import _capi_qk_norm, ops

H, HKV, D = 4, 2, 128
ROW_STRIDE = 2 ** 22 + 8
CU = [0, 255, 510, 765, 1020, 1024, 1064]                                # sequences of 255, 255, 255, 255, 4 and 40 rows
OFFSETS = [0, 40, -7, 44, 295, 259]                                      # into tables of 300 positions: one sequence clamps at 0, two end at position 298
MAX_SEQLEN, EPS = 255, 1e-6


def _case(names, seed, dtype=torch.bfloat16):
    """``names``: (name, heads, role) of every 16-bit tensor.  -> (case, weights, cu, offsets)."""
    total = CU[-1]
    g = torch.Generator().manual_seed(seed)
    case = FarCase()
    for name, h, role in names:
        t = torch.randn(total, h, D, generator=g).to(dtype)
        case.put_at(name, t, case.layout.rows(name, total, (h, D), (D, 1), 2, ROW_STRIDE, range(total)), role)
    cos, sin = ops.rotary_tables(300, 64)                                # fp32, 300 positions 2^22 + 8 elements apart: position 255 lies 4 GiB out
    for name, t in (("cos", cos), ("sin", sin)):
        case.put_at(name, t, case.layout.rows(name, 300, (32,), (1,), 4, ROW_STRIDE, range(300)))
    ws = [1.0 + 0.5 * torch.randn(D, generator=g) for _ in range(2)]
    return case, ws, torch.tensor(CU, dtype=torch.int32), torch.tensor(OFFSETS, dtype=torch.int32)


def _seen(a, t, fields):
    for field, pre, name in fields:
        assert getattr(a, field) == t[name].data_ptr(), f"{field}: the block holds another pointer -- the library saw a copy"
        assert (getattr(a, pre + "_stride_s"), getattr(a, pre + "_stride_h")) == t[name].stride()[:2]
    assert a.cos == t["cos"].data_ptr() and a.sin == t["sin"].data_ptr() and a.cs_stride == t["cos"].stride(0) == ROW_STRIDE


def forward_case():
    case, ws, cu, off = _case([("q", H, "in"), ("q_out", H, "out"), ("k", HKV, "in"), ("k_out", HKV, "out")], 41)

    def run(t, dev):
        w = [x.to(dev) for x in ws]
        geo = ops._qk_norm_geometry(t["q"], t["k"], w[0], w[1], EPS, t["cos"], t["sin"], cu.to(dev), MAX_SEQLEN, off.to(dev), None)
        ops._qk_norm_call([t["q"], t["k"]], w, geo, EPS, False, t["cos"], t["sin"], False, cu.to(dev), off.to(dev), None, False,
                          outs=[t["q_out"], t["k_out"]])

    def call(t):
        run(t, t["q"].device)
        return {}

    def seen(blocks, t):
        _seen(blocks.of("PfaQkNormArgs"), t, (("x0", "x0", "q"), ("x0_out", "x0o", "q_out"), ("x1", "x1", "k"), ("x1_out", "x1o", "k_out")))

    def check(near, ex):
        """the near run against ``ops``' CPU model of the same call, bit for bit"""
        cpu = case.near_inputs(torch.device("cpu"))
        run(cpu, torch.device("cpu"))
        for n in ("q_out", "k_out"):
            assert torch.equal(F.bits(near[n].cpu()), F.bits(cpu[n])), f"{n}: the near run is not the CPU model's"
            assert not torch.equal(F.bits(cpu[n]), F.bits(cpu[n[0]])), "nothing was computed"

    return Spec(case, call, seen, lambda blocks: _capi_qk_norm.describe_qk_norm(blocks.of("PfaQkNormArgs")), check, "qk_norm_bf16_d128_packed_rot")


def backward_case():
    names = [("q", H, "in"), ("dyq", H, "in"), ("dq", H, "out"), ("k", HKV, "in"), ("dyk", HKV, "in"), ("dk", HKV, "out")]
    case, ws, cu, off = _case(names, 43)

    def run(t, dev):
        w = [x.to(dev) for x in ws]
        geo = ops._qk_norm_geometry(t["q"], t["k"], w[0], w[1], EPS, t["cos"], t["sin"], cu.to(dev), MAX_SEQLEN, off.to(dev), None)
        _, dws = ops._qk_norm_bwd_call([t["q"], t["k"]], [t["dyq"], t["dyk"]], w, geo, EPS, False, t["cos"], t["sin"], False, cu.to(dev),
                                       off.to(dev), None, dxs=[t["dq"], t["dk"]])
        return dict(dw_q=dws[0], dw_k=dws[1])

    def call(t):
        return run(t, t["q"].device)

    def seen(blocks, t):
        _seen(blocks.of("PfaQkNormBwdArgs"), t, (("x0", "x0", "q"), ("dy0", "dy0", "dyq"), ("dx0", "dx0", "dq"), ("x1", "x1", "k"),
                                                 ("dy1", "dy1", "dyk"), ("dx1", "dx1", "dk")))

    def check(near, ex):
        """the near run against ``ops``' CPU model (dx bit for bit) and fp64 (dw inside its bound)"""
        cpu = case.near_inputs(torch.device("cpu"))
        run(cpu, torch.device("cpu"))
        for n in ("dq", "dk"):
            assert torch.equal(F.bits(near[n].cpu()), F.bits(cpu[n])), f"{n}: the near run is not the CPU model's"
        for x, dy, w, name in (("q", "dyq", ws[0], "dw_q"), ("k", "dyk", ws[1], "dw_k")):
            want, bound = Q.dw_reference(cpu[x], cpu[dy], w, EPS, False, cpu["cos"], cpu["sin"], False, CU, MAX_SEQLEN, OFFSETS)
            assert float(((ex[name].cpu().double() - want).abs() / bound).max()) <= 1.0, name

    return Spec(case, call, seen, lambda blocks: _capi_qk_norm.describe_qk_norm_bwd(blocks.of("PfaQkNormBwdArgs")), check,
                "qk_norm_bwd_bf16_d128_packed_rot")


@pytest.mark.parametrize("make", [forward_case, backward_case], ids=["forward", "backward"])
def test_the_layout_is_sound_and_far_on_the_host(make):
    case = make().case
    assert not case.layout.problems(), case.layout.problems()
    q, k = case.place["q"], case.place["k"]
    assert (CU[-1] - 1) * ROW_STRIDE * 2 > 2 ** 33 and 256 * ROW_STRIDE * 2 >= 2 ** 31 and 512 * ROW_STRIDE >= 2 ** 31     # bytes and elements wrap
    for name, p in case.place.items():
        if name not in ("cos", "sin"):
            assert set(F.claims(p)) == set(F.MODELS), name
    assert abs((q.base + (CU[-1] - 1) * ROW_STRIDE * 2) - k.base) > 2 ** 33


@pytest.fixture(scope="module")
def arena():
    """The module's one arena.  Less than the arena plus 2 GiB free: the module skips, and says how much there was."""
    free = torch.cuda.mem_get_info()[0]
    if free < F.ARENA_BYTES + 2 * 2 ** 30:
        pytest.skip(f"{free / 2 ** 30:.1f} GiB of device memory free: the far-address test needs {F.ARENA_BYTES / 2 ** 30 + 2:.1f} GiB")
    a = F.make_arena(torch.device("cuda:0"))
    yield a
    del a
    torch.cuda.empty_cache()


@pytest.mark.gpu
def test_far_qk_norm_forward(arena):
    F.two_runs(arena, forward_case())


@pytest.mark.gpu
def test_far_qk_norm_backward(arena):
    F.two_runs(arena, backward_case())

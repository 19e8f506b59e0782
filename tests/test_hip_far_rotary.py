"""GPU test of ``ops.apply_rotary`` on tensors spread past 4 and 8 GiB, built with tests/far_testlib.py as tests/test_hip_far_cache.py
builds the far case of the rotary append: packed Q and K with their outputs in one 12.5 GiB arena, the packed rows 2^22 + 8 elements
apart -- the 32-bit product of row and stride wraps from row 256 on, the last row lies 8.3 GiB from its tensor's first -- and the fp32
tables 4 GiB deep.  ``far_testlib.two_runs`` asserts that the library saw the far views (pointers and strides of the argument block),
that both runs name one kernel, that the far run's outputs are the near run's bit for bit, that the near run is the CPU model's, and that
nothing in the arena outside the declared outputs changed.  The layout is checked on the host without a GPU."""

from __future__ import annotations

import pytest
import torch

import far_testlib as F
from far_testlib import FarCase, Spec
from photonic_flash_attention_amd import _capi_rotary, ops

H, HKV, D = 4, 2, 128
ROW_STRIDE, ROW_LENS = 2 ** 22 + 8, [255, 255, 255, 255, 4, 40]         # sequences start at rows 0, 255, 510, 765, 1020, 1024
CU = [0, 255, 510, 765, 1020, 1024, 1064]
OFFSETS = [0, 40, -7, 44, 295, 259]                                      # into tables of 300 positions: one sequence clamps at 0, two end at position 298


def rotary_case(seed=31, dtype=torch.bfloat16):
    total = CU[-1]
    g = torch.Generator().manual_seed(seed)
    case = FarCase()
    rows = {"q": torch.randn(total, H, D, generator=g).to(dtype), "k": torch.randn(total, HKV, D, generator=g).to(dtype)}
    for name, t in rows.items():
        for n, role in ((name, "in"), (name + "_out", "out")):
            case.put_at(n, t, case.layout.rows(n, total, tuple(t.shape[1:]), (D, 1), 2, ROW_STRIDE, range(total)), role)
    cos, sin = ops.rotary_tables(300, 64)                                # fp32, 300 positions 2^22 + 8 elements apart: position 255 lies 4 GiB out
    for name, t in (("cos", cos), ("sin", sin)):
        case.put_at(name, t, case.layout.rows(name, 300, (32,), (1,), 4, ROW_STRIDE, range(300)))
    cu, off = torch.tensor(CU, dtype=torch.int32), torch.tensor(OFFSETS, dtype=torch.int32)

    def run(t, dev):
        geo = ops._rotary_geometry(t["q"], t["k"], t["cos"], t["sin"], cu.to(dev), max(ROW_LENS), off.to(dev), None)
        ops._rotary_call([t["q"], t["k"]], geo, t["cos"], t["sin"], False, cu.to(dev), off.to(dev), None, False, False,
                         outs=[t["q_out"], t["k_out"]])

    def call(t):
        run(t, t["q"].device)
        return {}

    def seen(blocks, t):
        a = blocks.of("PfaRotaryArgs")
        for field, pre, name in (("x0", "x0", "q"), ("x0_out", "x0o", "q_out"), ("x1", "x1", "k"), ("x1_out", "x1o", "k_out")):
            assert getattr(a, field) == t[name].data_ptr(), f"{field}: the block holds another pointer -- the library saw a copy"
            assert (getattr(a, pre + "_stride_s"), getattr(a, pre + "_stride_h")) == t[name].stride()[:2]
        assert a.cos == t["cos"].data_ptr() and a.sin == t["sin"].data_ptr() and a.cs_stride == t["cos"].stride(0) == ROW_STRIDE

    def check(near, ex):
        """the near run against ``ops``' CPU model of the same call, bit for bit"""
        cpu = case.near_inputs(torch.device("cpu"))
        run(cpu, torch.device("cpu"))
        for n in ("q_out", "k_out"):
            assert torch.equal(F.bits(near[n].cpu()), F.bits(cpu[n])), f"{n}: the near run is not the CPU model's"
            assert not torch.equal(F.bits(cpu[n]), F.bits(cpu[n[0]])), "nothing was rotated"

    return Spec(case, call, seen, lambda blocks: _capi_rotary.describe_rotary(blocks.of("PfaRotaryArgs")), check, "rotary_bf16_packed")


def test_the_layout_is_sound_and_far_on_the_host():
    case = rotary_case().case
    assert not case.layout.problems(), case.layout.problems()
    q, k = case.place["q"], case.place["k"]
    assert (CU[-1] - 1) * ROW_STRIDE * 2 > 2 ** 33 and 256 * ROW_STRIDE * 2 >= 2 ** 31 and 512 * ROW_STRIDE >= 2 ** 31     # bytes and elements wrap
    assert set(F.claims(q)) == set(F.MODELS) and set(F.claims(k)) == set(F.MODELS)
    # Q's and K's rows interleave through the arena: from K's first row to Q's last it is more than 8 GiB, and 4 GiB before row 512
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
def test_far_rotary(arena):
    F.two_runs(arena, rotary_case())

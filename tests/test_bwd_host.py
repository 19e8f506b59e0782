"""CPU-side tests (no GPU) of the backward's C ABI: the rules ``pfa_fa3_bwd`` checks and the order it reports them in, and the two
workspace sizes.  Every block sent to ``pfa_fa3_bwd`` here is refused by the validation, which runs before the first HIP call: an
accepted block would be launched on the made-up pointers wherever a GPU is present, so none is ever sent."""

from __future__ import annotations

import ctypes as C

from capi_testlib import lib  # noqa: F401
from photonic_flash_attention_amd import _capi

TENSORS = ("q", "k", "v", "o", "do", "dq", "dk", "dv")          # stride prefixes; the pointer of "do" is dout


def _bwd_args(**over):
    """A 16-bit block ``check_bwd`` accepts (B 1, H 2, Sq 64, Sk 64, D 64, [B,S,H,D] buffers), then the given fields."""
    base = dict(q=0x1000, k=0x2000, v=0x3000, o=0x4000, dout=0x5000, lse=0x6000, dq=0x7000, dk=0x8000, dv=0x9000, delta=0xa000,
                B=1, H=2, Sq=64, Sk=64, D=64, dtype=0, dtype_grad=0, softmax_scale=0.125)
    for t in TENSORS:
        base.update({f"{t}_stride_b": 8192, f"{t}_stride_h": 64, f"{t}_stride_s": 128})
    base.update(over)
    return _capi._make(_capi.PfaFa3BwdArgs, base)


def _f32_args(**over):
    return _bwd_args(**dict(dict(dtype=2, dtype_grad=2), **over))


def _refused(lib, a) -> int:
    st = lib.pfa_fa3_bwd(None if a is None else C.byref(a), None)
    assert st < 0             # (0 would mean the block went on to the device switch)
    return st


def test_backward_validation_without_a_gpu(lib):
    nan = float("nan")
    cases = [
        (dict(flags=1), -10), (dict(kv_group=-1), -10), (dict(kv_group=3), -10), (dict(drop_mask=0xb000), -10),
        (dict(delta=0), -1), (dict(dq=0), -1), (dict(B=0), -3), (dict(Sk=0), -3), (dict(D=80), -4),
        (dict(dtype=3), -5), (dict(dtype_grad=1), -5), (dict(softmax_scale=0.0), -3), (dict(softmax_scale=nan), -3),
        (dict(do_stride_s=129), -6), (dict(dq_stride_s=132), -6), (dict(dq_stride_s=130, dtype_grad=2), -6),
        (dict(dout=0x5008), -7), (dict(k_stride_s=-128), -3), (dict(k_stride_s=1 << 25), -3),
    ]
    for over, want in cases:
        assert _refused(lib, _bwd_args(**over)) == want, over
    assert _refused(lib, None) == -1
    assert _refused(lib, _bwd_args(size=8)) == -2


def test_backward_validation_reports_in_a_fixed_order(lib):
    pairs = [
        (dict(drop_mask=0xb000, q=0), -10),          # flags before pointers
        (dict(flags=1, size=8), -2),                 # the struct size before everything
        (dict(B=0, D=80), -3),                       # shape before head dim
        (dict(D=80, dtype=3), -4),                   # head dim before dtype
        (dict(q_stride_h=65, k=0x2004), -6),         # strides before alignment
    ]
    for over, want in pairs:
        assert _refused(lib, _bwd_args(**over)) == want, over


def test_fp32_backward_validation_without_a_gpu(lib):
    cases = [
        (dict(dtype_grad=0), -5), (dict(kv_group=2), -10), (dict(drop_mask=0xb000, drop_scale=0.5), -10),
        (dict(q_stride_s=32), -6), (dict(dq_stride_s=0), -6), (dict(do_stride_b=8190), -6),
        (dict(lse=0x6002), -7), (dict(o=0x4002), -7), (dict(q=0x1004), -7), (dict(Sq=1 << 23), -3),
    ]
    for over, want in cases:
        assert _refused(lib, _f32_args(**over)) == want, over


def test_backward_workspace_sizes(lib):
    """B 2, H 3, Sq 300, Sk 200: 4 key tiles of 64 (nt), 5 row tiles of 64 (ntq), 2 granules of 256 rows, 2 key blocks of 128; a tile
    range is 16 parts x 2 int32 = 128 bytes per granule / key block.  One (batch, head) of the mask then takes
    300 * 4 * 8 (row words) + 2 * 128 (row ranges) + 200 * 5 * 8 (column words) + 2 * 128 (column ranges) = 18112 bytes."""
    dims = dict(B=2, H=3, Sq=300, Sk=200)
    assert lib.pfa_fa3_bwd_workspace_bytes(C.byref(_bwd_args(**dims))) == 2 * 3 * 300 * 4          # delta: fp32 [B, H, Sq]
    assert lib.pfa_fa3_bwd_workspace_bytes(None) == 0
    assert lib.pfa_fa3_bwd_workspace_bytes(C.byref(_bwd_args(B=0))) == 0
    mws = lib.pfa_fa3_bwd_mask_workspace_bytes
    assert mws(None) == 0 and mws(C.byref(_bwd_args(**dims))) == 0                                 # no mask
    key_only = dict(dims, mask=0xc000, mask_stride_b=200, mask_stride_k=1)                         # [B, 1, 1, Sk]
    assert mws(C.byref(_bwd_args(**key_only))) == 0
    broadcast = dict(dims, mask=0xc000, mask_stride_q=200, mask_stride_k=1)                        # [1, 1, Sq, Sk]
    assert mws(C.byref(_bwd_args(**broadcast))) == 18112
    full = dict(dims, mask=0xc000, mask_stride_b=180000, mask_stride_h=60000, mask_stride_q=200, mask_stride_k=1)
    assert mws(C.byref(_bwd_args(**full))) == 6 * 18112
    assert mws(C.byref(_f32_args(**full))) == 0                                                    # the fp32 kernels read the bytes

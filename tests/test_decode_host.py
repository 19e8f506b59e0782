"""CPU-side tests (no GPU) of the split-KV decode path: argument validation, workspace contract, host-tensor refusal and
the Hugging Face routing decision."""

from __future__ import annotations

import ctypes as C

import pytest
import torch

from capi_testlib import decode_args, lib  # noqa: F401
from photonic_flash_attention_amd import _capi, ops


def _dargs(**over):
    """B 2, H 8, Hkv 2, Sq 1, Smax 4096, D 128, [B, S, H, D] q and cache, with the workspace the library asks for; the strides are
    those of this shape whatever is overridden."""
    return decode_args({**dict(k_cache=0x100000, v_cache=0x200000, o=0x3000), **over}, Sq=1, ws="asked", follow="")


def test_decode_argument_validation(lib):
    assert lib.pfa_fa3_decode_check(C.byref(_dargs())) == 0
    assert lib.pfa_fa3_decode_check(None) == -1
    bad = _dargs()
    bad.size = 16
    assert lib.pfa_fa3_decode_check(C.byref(bad)) == -2
    cases = [
        (dict(q=0), -1), (dict(k_cache=0), -1), (dict(o=0), -1),
        (dict(D=96), -4), (dict(Sq=0), -3), (dict(Sq=65), -3), (dict(H=8, Hkv=3), -3), (dict(B=0), -3), (dict(Smax=0), -3),
        (dict(softmax_scale=0.0), -3), (dict(k_cache=0x100008), -7), (dict(q=0x1004), -7), (dict(k_stride_s=2 * 128 + 1), -6),
        (dict(q_stride_h=129), -6), (dict(o_stride_s=6), -6), (dict(flags=1), -10), (dict(flags=0x100), -10),
        (dict(dtype_in=2, dtype_out=2), -5), (dict(dtype_out=1), -5),
        (dict(workspace=0), -1),
    ]
    for over, want in cases:
        assert lib.pfa_fa3_decode_check(C.byref(_dargs(**over))) == want, over
    for ok in (dict(D=64), dict(Sq=64), dict(H=64, Hkv=1), dict(dtype_in=1, dtype_out=1), dict(dtype_out=2), dict(Smax=1)):
        assert lib.pfa_fa3_decode_check(C.byref(_dargs(**ok))) == 0, ok


def test_decode_workspace_depends_on_shapes_only(lib):
    plain = lib.pfa_fa3_decode_workspace_bytes(C.byref(_dargs()))
    with_ptrs = lib.pfa_fa3_decode_workspace_bytes(C.byref(_dargs(cache_seqlens=0x5000, key_mask=0x6000, key_mask_stride_b=4096)))
    assert plain == with_ptrs > 0
    small = lib.pfa_fa3_decode_workspace_bytes(C.byref(_dargs(Smax=512)))
    big = lib.pfa_fa3_decode_workspace_bytes(C.byref(_dargs(Smax=32768)))
    assert small < plain < big
    name, wgs, nsplit = _capi.describe_decode(_dargs())
    assert name.startswith("fa3_decode_bf16_d128") and nsplit > 1 and wgs == 2 * 2 * nsplit
    assert plain == nsplit * 2 * 8 * 1 * (128 + 2) * 4
    # one split: no workspace, and none is asked for
    one = _dargs(Smax=64)
    assert lib.pfa_fa3_decode_workspace_bytes(C.byref(one)) == 0
    assert _capi.describe_decode(one)[2] == 1


def test_fa3_decode_refuses_host_tensors():
    q = torch.zeros(1, 8, 1, 128, dtype=torch.bfloat16)
    k = torch.zeros(1, 2, 256, 128, dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        ops.fa3_decode(q, k, k.clone())


# --- Hugging Face routing ------------------------------------------------------------------------------------------------------------

class _Spy:
    def __init__(self):
        self.calls = []

    def decode(self, q, k, v, **kw):
        self.calls.append(("decode", kw))
        B, H, Sq, D = q.shape
        return torch.zeros(B, Sq, H, D, dtype=kw.get("out_dtype") or q.dtype).permute(0, 2, 1, 3), None

    def attention(self, q, k, v, **kw):
        self.calls.append(("attention", kw))
        B, H, Sq, D = q.shape
        return torch.zeros(B, Sq, H, D, dtype=kw.get("out_dtype") or q.dtype).permute(0, 2, 1, 3)


@pytest.fixture
def spy(monkeypatch):
    from photonic_flash_attention_amd.integration.pytorch import hf
    s = _Spy()
    monkeypatch.setattr(hf.ops, "fa3_decode", s.decode)
    monkeypatch.setattr(hf.ops, "fa3_attention", s.attention)
    return s


def _qkv(q_len, k_len, B=2, H=8, Hkv=2, D=64, requires_grad=False):
    q = torch.randn(B, H, q_len, D, dtype=torch.bfloat16, requires_grad=requires_grad)
    k = torch.randn(B, Hkv, k_len, D, dtype=torch.bfloat16, requires_grad=requires_grad)
    v = torch.randn(B, Hkv, k_len, D, dtype=torch.bfloat16, requires_grad=requires_grad)
    return q, k, v


class _Mod(torch.nn.Module):
    is_causal = True


def test_hf_decode_step_with_a_key_row_mask_goes_to_fa3_decode(spy):
    from photonic_flash_attention_amd.integration.pytorch.hf import pfa_attention_forward
    q, k, v = _qkv(1, 40)
    mask = torch.ones(2, 1, 1, 40, dtype=torch.bool)
    mask[1, ..., :7] = False
    with torch.no_grad():
        out, _ = pfa_attention_forward(_Mod(), q, k, v, mask, scaling=0.125)
    assert [c[0] for c in spy.calls] == ["decode"]
    km = spy.calls[0][1]["key_mask"]
    assert km.shape == (2, 40) and torch.equal(km, mask[:, 0, 0, :])
    assert out.shape == (2, 1, 8, 64)
    # no mask at all: still the decode kernel
    spy.calls.clear()
    with torch.no_grad():
        pfa_attention_forward(_Mod(), q, k, v, None, scaling=0.125)
    assert spy.calls[0][0] == "decode" and spy.calls[0][1]["key_mask"] is None


def test_hf_decode_step_wanting_gradients_keeps_the_autograd_path(spy):
    from photonic_flash_attention_amd.integration.pytorch.hf import pfa_attention_forward
    q, k, v = _qkv(1, 40, requires_grad=True)
    with torch.enable_grad():
        pfa_attention_forward(_Mod(), q, k, v, None, scaling=0.125)
    assert [c[0] for c in spy.calls] == ["attention"]


def test_hf_per_head_mask_and_multi_row_steps_keep_the_general_path(spy):
    from photonic_flash_attention_amd.integration.pytorch.hf import pfa_attention_forward
    q, k, v = _qkv(1, 40)
    with torch.no_grad():
        pfa_attention_forward(_Mod(), q, k, v, torch.ones(2, 8, 1, 40, dtype=torch.bool), scaling=0.125)
        q4, k4, v4 = _qkv(4, 40)
        pfa_attention_forward(_Mod(), q4, k4, v4, torch.ones(2, 1, 4, 40, dtype=torch.bool), scaling=0.125)
        q96, k96, v96 = _qkv(1, 40, D=96)
        pfa_attention_forward(_Mod(), q96, k96, v96, None, scaling=0.125)
    assert [c[0] for c in spy.calls] == ["attention"] * 3

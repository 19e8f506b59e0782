"""CPU-side tests (no GPU): C-ABI surface, argument validation, and the reference-shaped
host modules (constructor contract, routing pinned to 'gpu', plumbing around the core seam)."""

from __future__ import annotations

import ctypes as C
import os
import threading

import pytest
import torch

from capi_testlib import fa3_args as _args, lib  # noqa: F401
from conftest import REPO, load_golden
from photonic_flash_attention_amd import _capi, synth


def test_argument_validation_without_a_gpu(lib):
    assert lib.pfa_fa3_check(C.byref(_args())) == 0
    cases = [
        (dict(D=80), -4), (dict(D=256), -4), (dict(dtype_in=2), -5), (dict(dtype_out=1), -5),
        (dict(q=0), -1), (dict(o=0), -1), (dict(B=0), -3), (dict(Sk=0), -3), (dict(softmax_scale=0.0), -3),
        (dict(softmax_scale=float("nan")), -3), (dict(q_stride_s=129), -6), (dict(o_stride_s=6), -6),
        (dict(k=0x2008), -7), (dict(flags=0x80), -10),
    ]
    for over, want in cases:
        assert lib.pfa_fa3_check(C.byref(_args(**over))) == want, over
    f32 = dict(dtype_in=2, dtype_out=2)           # the exact fp32 kernel's branch: no split P, 16-byte rows at least D apart, 32-bit slabs
    assert lib.pfa_fa3_check(C.byref(_args(**f32))) == 0
    for over, want in [(dict(flags=1), -10), (dict(q_stride_b=8190), -6), (dict(k_stride_s=32), -6), (dict(o=0x4002), -7),
                       (dict(Sq=1 << 23), -3)]:
        assert lib.pfa_fa3_check(C.byref(_args(**f32, **over))) == want, over
    # ... a misaligned q, output rows closer than D, a kernel selector; the dropout keep-mask: fp32 operands only, kept weights scaled up
    for over, want in [(dict(q=0x1004), -7), (dict(v_stride_h=66), -6), (dict(o_stride_s=32), -6), (dict(flags=43 << 8), -10),
                       (dict(flags=1 | 45 << 8), -10), (dict(drop_mask=0xb000, drop_scale=0.5), -10),
                       (dict(drop_mask=0xb000, drop_scale=float("nan")), -10), (dict(drop_mask=0xb000, drop_scale=float("inf")), -10)]:
        assert lib.pfa_fa3_check(C.byref(_args(**f32, **over))) == want, over
    assert lib.pfa_fa3_check(C.byref(_args(**f32, drop_mask=0xb000, drop_scale=1.25))) == 0
    assert lib.pfa_fa3_check(C.byref(_args(**f32, o_stride_s=65, o_stride_h=4225))) == 0          # the output alone may have any stride >= D
    for dt in (0, 1):
        assert lib.pfa_fa3_check(C.byref(_args(dtype_in=dt, dtype_out=dt, drop_mask=0xb000, drop_scale=1.25))) == -10, dt
    bad = _args()
    bad.size = 8
    assert lib.pfa_fa3_check(C.byref(bad)) == -2
    assert lib.pfa_fa3_check(None) == -1
    assert lib.pfa_fa3_workspace_bytes(C.byref(_args())) == 0
    for st in range(0, -11, -1):
        assert _capi.status_string(st) != "unknown pfa_status"
    assert _capi.status_string(-99) == "unknown pfa_status"


def test_weights_pass_argument_validation_without_a_gpu(lib):
    """pfa_fa3_weights' refusals, none of which reaches a device; what it accepts is shown by PFA_ERR_DEVICE (-8) for a device ordinal no
    machine has -- the one rule behind the argument rules -- so that nothing is launched on a machine with a GPU either."""
    no_dev = 9999

    def call(w=0x8000, w_dtype=0, strides=(64 * 64 * 2, 64 * 64, 64), a=True, **over):
        args = _args(**{**dict(lse=0x5000, device_id=no_dev), **over})
        return lib.pfa_fa3_weights(C.byref(args) if a else None, C.c_void_p(w), w_dtype, *strides, None)

    assert call() == -8                                                   # valid: only the device is missing
    assert call(a=False) == -1 and call(w=0) == -1                        # a or w NULL
    assert call(dtype_in=2, dtype_out=2, w_dtype=2) == -5                 # fp32 operands: the pass is MFMA only
    assert call(lse=0) == -1                                              # the LSE is required
    assert call(w_dtype=1) == -5 and call(w_dtype=3) == -5                # W in the operands' type or fp32, nothing else
    assert call(dtype_in=1, dtype_out=1, w_dtype=1) == -8 and call(dtype_in=1, dtype_out=1, w_dtype=2) == -8
    # the forward's errors pass through: a misaligned q, a bad head dim, a stride, both masks
    assert call(q=0x1004) == -7 and call(D=80) == -4 and call(k_stride_s=129) == -6 and call(key_mask=0x6000, mask=0x7000) == -10
    # v and o are not read: NULL is fine, and W is never judged by the output's 16-byte rule -- an fp32 W aligned to 4 bytes, a 16-bit
    # W aligned to 2, both with odd row strides (the kernel then stores element by element)
    assert call(v=0, o=0) == -8
    assert call(o=0, w=0x8004, w_dtype=2, strides=(2 * 64 * 65, 64 * 65, 65)) == -8
    assert call(o=0, w=0x8002, strides=(2 * 64 * 67, 64 * 67, 67)) == -8
    assert call(o=0, dtype_in=1, w=0x8002, w_dtype=1) == -8               # (o NULL: dtype_out is not looked at either)
    assert call(w=0x8004, w_dtype=2) == -8 and call(w=0x8002) == -8       # ... the same with o set
    # W's own rules, with o set or not: aligned to its element, rows forward and at least Sk apart
    for o in (0, 0x4000):
        assert call(o=o, w=0x8002, w_dtype=2) == -7 and call(o=o, w=0x8001) == -7
        assert call(o=o, strides=(8192, 4096, 63)) == -6 and call(o=o, strides=(8192, 4096, -64)) == -6
        assert call(o=o, strides=(-8192, 4096, 64)) == -6 and call(o=o, strides=(8192, -4096, 64)) == -6
        assert call(o=o, strides=(0, 0, 64)) == -8                        # (a broadcast W is the caller's business)
    assert call(o=0x4008) == -7                                           # an o that is given is still the forward's o


def test_drop_mask_rules_of_the_tensor_layer():
    """ops.fa3_forward / fa3_backward hand ``drop_mask`` to the library through ``ops._drop_mask_ptr``: a contiguous u8 / bool
    [B, H, Sq, Sk] tensor on the operands' device, fp32 operands -- anything else is a ValueError before any pointer is taken."""
    from photonic_flash_attention_amd import ops
    B, H, Sq, Sk = 1, 2, 5, 7
    like = torch.zeros(B, H, Sq, 64)
    good = torch.ones(B, H, Sq, Sk, dtype=torch.bool)
    assert ops._drop_mask_ptr(good, B, H, Sq, Sk, like) == good.data_ptr()
    assert ops._drop_mask_ptr(good.view(torch.uint8), B, H, Sq, Sk, like) == good.data_ptr()
    bad = [torch.ones(B, H, Sq, 2 * Sk, dtype=torch.bool)[..., ::2],          # not contiguous
           torch.ones(B, H, Sk, Sq, dtype=torch.bool).transpose(2, 3),
           torch.ones(B, H, Sq, Sk + 1, dtype=torch.bool),                    # the wrong shape
           torch.ones(B, 1, Sq, Sk, dtype=torch.bool),
           torch.ones(B * H, Sq, Sk, dtype=torch.bool),
           torch.ones(B, H, Sq, Sk, dtype=torch.bool, device="meta"),         # the wrong device
           torch.ones(B, H, Sq, Sk)]                                          # the wrong dtype
    for m in bad:
        with pytest.raises(ValueError):
            ops._drop_mask_ptr(m, B, H, Sq, Sk, like)
    with pytest.raises(ValueError):
        ops._drop_mask_ptr(good, B, H, Sq, Sk, like.bfloat16())               # dropout runs on the fp32 kernels only


def test_stride_filler_puts_every_axis_in_its_field():
    """``ops._set_view`` (and ``ops._set_strides`` on the dense blocks) write a tensor's pointer and, per letter of the block's axis order,
    the stride of the axis that letter names -- on views whose strides all differ, so that a slip in the order shows.  Nothing else in
    the block is touched, and a head dim that is not contiguous is refused with the one message every path has."""
    from photonic_flash_attention_amd import ops
    t4 = torch.zeros(2, 5, 3, 8).permute(0, 2, 1, 3)               # [B,H,S,D] = [2,3,5,8] with strides 120, 8, 24, 1
    t3 = torch.zeros(3, 5, 8).permute(1, 0, 2)                     # packed [S,H,D] = [5,3,8] with strides 8, 40, 1
    assert len(set(t4.stride())) == 4 and len(set(t3.stride())) == 3
    dim4, dim3 = dict(b=0, h=1, s=2), dict(s=0, h=1)
    cases = [(_capi.PfaFa3DecodeArgs, "bhs", t4, dim4, dict(q="q", k_cache="k", v_cache="v", o="o")),
             (_capi.PfaFa3PrefillVarlenArgs, "sh", t3, dim3, dict(q="q", o="o")),
             (_capi.PfaFa3PrefillVarlenArgs, "bhs", t4, dim4, dict(k_cache="k", v_cache="v")),
             (_capi.PfaKvAppendArgs, "bsh", t4, dim4, dict(k_new="kn", v_new="vn")),
             (_capi.PfaKvAppendArgs, "sh", t3, dim3, dict(k_new="kn", v_new="vn")),      # the packed rows: no batch stride is written
             (_capi.PfaKvAppendArgs, "bhs", t4, dim4, dict(k_cache="k", v_cache="v"))]
    for cls, axes, t, dim, fields in cases:
        for name, pre in fields.items():
            a = cls()
            ops._set_view(a, name, t, axes)
            want = {name: t.data_ptr()}
            want.update({f"{pre}_stride_{x}": t.stride(dim[x]) for x in axes})
            got = {f: getattr(a, f) for f, _ in cls._fields_ if getattr(a, f)}
            assert got == want, (cls.__name__, name, axes)
    for cls, names in ((_capi.PfaFa3Args, ("q", "k", "v", "o")), (_capi.PfaFa3BwdArgs, ("q", "k", "v", "o", "dout", "dq", "dk", "dv"))):
        for name in names:
            a = cls()
            ops._set_strides(a, ((name, t4),))
            pre = "do" if name == "dout" else name
            want = {name: t4.data_ptr(), f"{pre}_stride_b": 120, f"{pre}_stride_h": 8, f"{pre}_stride_s": 24}
            assert {f: getattr(a, f) for f, _ in cls._fields_ if getattr(a, f)} == want, (cls.__name__, name)
    for bad, axes in ((t4[..., ::2], "bhs"), (t4[..., ::2], "bsh"), (t3[..., ::2], "sh")):
        with pytest.raises(ValueError, match=r"last \(head_dim\) stride must be 1"):
            ops._set_view(_capi.PfaKvAppendArgs(), "k_new", bad, axes)
    with pytest.raises(ValueError, match=r"last \(head_dim\) stride must be 1"):
        ops._set_strides(_capi.PfaFa3Args(), (("q", t4[..., ::2]),))


def test_production_library_refuses_development_variants(lib):
    """flags bits 8..15: 0 or one of the three production kernel selectors; every other value is refused.  The round-1 schedule
    experiments and timing-only ablations that once lived behind these bits are in git history and in the profile logs, not in the tree."""
    for sel in (0, 43, 44, 45):
        assert lib.pfa_fa3_check(C.byref(_args(flags=sel << 8))) == 0, sel
    for var in (1, 9, 0x14, 19, 28, 30, 41, 42, 46, 49, 255):          # 0x14 << 8 = 0x1400
        assert lib.pfa_fa3_check(C.byref(_args(flags=var << 8))) == -10, var
    assert lib.pfa_fa3_check(C.byref(_args(flags=0x1400))) == -10


def test_no_environment_variable_selects_a_kernel(monkeypatch):
    """ops.fa3_forward must not read a kernel variant from the environment (only the explicit `_variant=` of tools / tests)."""
    import inspect
    from photonic_flash_attention_amd import ops
    src = inspect.getsource(ops)
    assert "os.environ" not in src and "PFA_VARIANT" not in src


def test_describe_picks_kernel_variant(lib):
    """Selector 44 names the 8-wave kernel whatever the machine: 16 row blocks x 64 (batch, head) pairs.  Selector 0 lets the library
    choose, and this shape may go to the persistent kernel, whose grid is the device's CU count rounded down to a multiple of 8 -- with
    no device there is none and the 8-wave kernel takes the call.  So selector 0 asserts what holds on both machines."""
    shape = dict(D=128, causal=1, Sq=4096, Sk=4096, B=4, H=16, dtype_out=2)
    name, nwg = _capi.describe(_args(**shape, flags=1 | 44 << 8))
    assert "d128" in name and "o32" in name and nwg == 16 * 64
    chosen, n = _capi.describe(_args(**shape, flags=1))
    assert "d128" in chosen and "o32" in chosen
    if chosen.startswith("fa3_fwd_p4_"):
        assert n >= 8 and n % 8 == 0
    else:
        assert chosen == name and n == 16 * 64


# ---------------------------------------------------------------- reference-shaped modules
def test_constructor_contract():
    from photonic_flash_attention_amd import (FlashAttention3, HybridFlashAttention, PhotonicFlashAttention,
                                              PhotonicMultiHeadAttention)
    m = FlashAttention3(512, 8)
    # tests/unit/test_flash_attention_3.py:25-39 of the reference
    assert (m.embed_dim, m.num_heads, m.head_dim) == (512, 8, 64) and m.scaling == 64 ** -0.5
    assert m.qkv_proj.weight.shape == (1536, 512) and m.out_proj.weight.shape == (512, 512)
    assert sorted(m.state_dict()) == ["out_proj.bias", "out_proj.weight", "qkv_proj.bias", "qkv_proj.weight"]
    with pytest.raises(AssertionError):
        FlashAttention3(100, 8)
    assert set(m.get_performance_stats()) == {"latency_ms", "memory_mb", "device", "implementation"}
    p = PhotonicFlashAttention(256, 4)
    assert sorted(p.state_dict())[0].startswith("gpu_attention.") and p.photonic_attention is None
    assert p.last_device_used == "gpu" and p.photonic_threshold == 512
    p.set_photonic_threshold(64)
    assert not p._should_use_photonic(8, 100000)
    with pytest.raises(NotImplementedError):
        PhotonicMultiHeadAttention(256, 4, add_bias_kv=True)
    with pytest.raises(NotImplementedError):
        PhotonicMultiHeadAttention(256, 4, kdim=64)
    h = HybridFlashAttention(256, 4, enable_scaling=False)
    assert h.photonic_attention is None and h.executor is None
    assert "gpu_stats" in h.get_performance_stats()


def test_router_is_pinned_to_gpu_for_every_baseline_shape():
    from photonic_flash_attention_amd.core.hybrid_router import (AdaptiveRouter, PerformanceMetrics,
                                                                 WorkloadCharacteristics)
    r = AdaptiveRouter()
    for B, S, E, H in [(2, 128, 256, 4), (4, 1024, 768, 12), (4, 4096, 2048, 16), (1, 16384, 4096, 32)]:
        w = WorkloadCharacteristics(B, S, E, H, dtype=torch.bfloat16)
        for _ in range(120):   # far past the reference's 50-sample learned/exploring regime
            assert r.select_device(w) == "gpu"
            r.update_performance("gpu", w, PerformanceMetrics(latency_ms=1.0))
    st = r.get_stats()
    assert st["photonic_samples"] == 0 and st["gpu_samples"] == 480 and st["cache_hit_rate"] > 0.9


def test_no_cpu_or_eager_path_in_the_product():
    """Host tensors must fail loudly: the product has no CPU implementation of the core."""
    from photonic_flash_attention_amd import FlashAttention3, ops
    m = FlashAttention3(128, 2).eval()
    with torch.no_grad(), pytest.raises(RuntimeError, match="MI355X"):
        m(torch.zeros(1, 8, 128))
    z = torch.zeros(1, 2, 8, 64, dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        ops.fa3_forward(z, z, z)
    import photonic_flash_attention_amd as pkg
    src_dir = os.path.dirname(pkg.__file__)
    for root, _, files in os.walk(src_dir):
        for f in files:
            if f.endswith(".py"):
                text = open(os.path.join(root, f)).read()
                assert "import oracle" not in text and "from oracle" not in text, f


def _oracle_core(self, q, k, v, attention_mask=None, need_weights=False, is_causal=False):
    """Test double for the core seam (tests may use the oracle as the checker)."""
    from oracle import fa3_oracle as orc
    mask = orc.causal_mask(q.shape[2], k.shape[2]) if is_causal else attention_mask
    return orc.flash_attention_forward(q, k, v, mask, self.scaling), None


def test_module_plumbing_matches_reference_module(monkeypatch):
    """Projection plumbing around the seam (chunk order, head split/merge, out_proj) against the
    real reference's FlashAttention3.forward output (golden g1_c1_module), core replaced by the oracle."""
    from photonic_flash_attention_amd import FlashAttention3, PhotonicFlashAttention
    meta, arr = load_golden("g1_c1_module")
    E, H, seed = meta["E"], meta["H"], meta["seed"]
    sd = {
        "qkv_proj.weight": torch.from_numpy(synth.normal_f32((3 * E, E), seed + 10)) * E ** -0.5,
        "qkv_proj.bias": torch.from_numpy(synth.normal_f32((3 * E,), seed + 11)) * 0.1,
        "out_proj.weight": torch.from_numpy(synth.normal_f32((E, E), seed + 12)) * E ** -0.5,
        "out_proj.bias": torch.from_numpy(synth.normal_f32((E,), seed + 13)) * 0.1,
    }
    monkeypatch.setattr(FlashAttention3, "_flash_attention_forward", _oracle_core)
    x = torch.from_numpy(synth.normal_f32((meta["B"], meta["S"], E), seed))
    ref = torch.from_numpy(arr["out"])
    m = FlashAttention3(E, H).eval()
    m.load_state_dict(sd)
    with torch.no_grad():
        y, w = m(x)
        y2, _ = m(x, x.clone(), x.clone())       # cross-attention branch computes the same numbers
    assert w is None and float((y - ref).abs().max()) <= 5e-6 and float((y2 - ref).abs().max()) <= 5e-6
    p = PhotonicFlashAttention(E, H).eval()
    p.gpu_attention.load_state_dict(sd)
    with torch.no_grad():
        z = p(x)
    assert isinstance(z, torch.Tensor) and float((z - ref).abs().max()) <= 5e-6
    assert p.get_performance_stats()["gpu_calls"] == 1


def test_mha_facade_layouts(monkeypatch):
    from photonic_flash_attention_amd import FlashAttention3, PhotonicMultiHeadAttention
    monkeypatch.setattr(FlashAttention3, "_flash_attention_forward", _oracle_core)
    mb = PhotonicMultiHeadAttention(128, 2, batch_first=True).eval()
    ms = PhotonicMultiHeadAttention(128, 2, batch_first=False).eval()
    ms.load_state_dict(mb.state_dict())
    x = torch.from_numpy(synth.normal_f32((2, 40, 128), 3))
    with torch.no_grad():
        yb, wb = mb(x, x, x, need_weights=False)
        xs = x.transpose(0, 1)
        ys, _ = ms(xs, xs, xs, need_weights=False)
    assert wb is None and yb.shape == (2, 40, 128) and ys.shape == (40, 2, 128)
    assert float((ys.transpose(0, 1) - yb).abs().max()) <= 1e-6


def test_hybrid_overload_path_and_concurrency(monkeypatch):
    """tests/performance/test_benchmarks.py:298-376 of the reference: 8 caller threads."""
    from photonic_flash_attention_amd import FlashAttention3, HybridFlashAttention
    monkeypatch.setattr(FlashAttention3, "_flash_attention_forward", _oracle_core)
    h = HybridFlashAttention(128, 2, max_concurrent_requests=2).eval()
    x = torch.from_numpy(synth.normal_f32((2, 64, 128), 5))
    with torch.no_grad():
        want = h(x)[0]
    outs, errs = [None] * 8, []

    def work(i):
        try:
            with torch.no_grad():
                outs[i] = h(x)
        except Exception as e:  # pragma: no cover
            errs.append(e)

    ts = [threading.Thread(target=work, args=(i,)) for i in range(8)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not errs
    for o in outs:
        assert isinstance(o, tuple) and o[1] is None and torch.equal(o[0], want)
    st = h.get_performance_stats()
    assert st["total_requests"] == 9 and st["peak_concurrent"] >= 1 and st["photonic_samples"] == 0


def test_global_config_env_and_update(monkeypatch):
    from photonic_flash_attention_amd import set_global_config
    from photonic_flash_attention_amd.config import GlobalConfig, get_config
    GlobalConfig.reset()
    monkeypatch.setenv("PHOTONIC_THRESHOLD", "2048")
    monkeypatch.setenv("AUTO_DEVICE_SELECTION", "off")
    c = get_config()
    assert c.photonic_threshold == 2048 and c.auto_device_selection is False and c.max_memory_usage == 0.8
    set_global_config(max_memory_usage=0.5)
    assert get_config().max_memory_usage == 0.5
    with pytest.raises(ValueError):
        set_global_config(no_such_key=1)
    GlobalConfig.reset()


def test_convert_to_photonic_replaces_torch_mha(monkeypatch):
    """model conversion for local nn.Module objects (reference convert.py:441-452
    weight rule).  Core replaced by the oracle double; checks weight mapping + PyTorch mask dialect translation
    against the ORIGINAL torch layer."""
    import torch.nn as nn
    from photonic_flash_attention_amd import FlashAttention3
    from photonic_flash_attention_amd.integration.pytorch.convert import TorchMHAReplacement, convert_to_photonic
    monkeypatch.setattr(FlashAttention3, "_flash_attention_forward", _oracle_core)
    torch.manual_seed(0)
    layer = nn.TransformerEncoderLayer(d_model=256, nhead=4, dim_feedforward=512, dropout=0.0, batch_first=True).eval()
    conv, rep = convert_to_photonic(layer)
    assert rep.converted_layers == ["self_attn"] and not rep.skipped_layers and not rep.conversion_errors
    assert isinstance(conv.self_attn, TorchMHAReplacement) and isinstance(layer.self_attn, nn.MultiheadAttention)
    x = torch.from_numpy(synth.normal_f32((2, 50, 256), 8))
    pad = torch.zeros(2, 50, dtype=torch.bool)
    pad[0, 40:] = True                                               # PyTorch convention: True = ignore
    causal = nn.Transformer.generate_square_subsequent_mask(50)
    with torch.no_grad():
        for kw in (dict(), dict(src_key_padding_mask=pad), dict(src_mask=causal, is_causal=True),
                   dict(src_mask=causal), dict(src_mask=causal, src_key_padding_mask=pad)):
            want = layer(x, **kw)
            got = conv(x, **kw)
            keep = ~pad if "src_key_padding_mask" in kw else torch.ones(2, 50, dtype=torch.bool)
            assert float((got - want)[keep].abs().max()) <= 2e-5, kw
    # float masks: binary in effect (0 / -inf / finfo.min / -1e4) are translated, finite biases are refused -- never dropped silently
    big = torch.zeros(50, 50)
    big[:, 30:] = torch.finfo(torch.float32).min
    soft = torch.zeros(50, 50)
    soft[:, 30:] = -1e4
    with torch.no_grad():
        a = conv(x, src_mask=big)
        b = conv(x, src_mask=soft)
        assert float((a - layer(x, src_mask=big)).abs().max()) <= 2e-5 and torch.equal(a, b)
        alibi = -0.5 * torch.arange(50.0)[None, :].expand(50, 50).contiguous()
        with pytest.raises(ValueError, match="finite biases"):
            conv(x, src_mask=alibi)
    keep = TorchMHAReplacement._to_keep_mask(torch.tensor([[0.0, -1e4, float("-inf"), torch.finfo(torch.float32).min]]))
    from photonic_flash_attention_amd.integration.pytorch import hf
    assert keep.tolist() == [[True, False, False, False]] == hf._keep_mask(torch.tensor([[0.0, -1e4, float("-inf"), -3e38]])).tolist()
    # skipped layers are reported, strings are refused
    odd = nn.MultiheadAttention(768, 4)                              # head_dim 192 > 128: no kernel
    _, rep2 = convert_to_photonic(nn.Sequential(odd))
    assert rep2.skipped_layers == ["0"] and "head_dim" in rep2.compatibility_warnings[0]
    with pytest.raises(ValueError):
        convert_to_photonic("bert-base-uncased")


def test_integration_md_binding_matches_the_abi():
    """The ctypes struct INTEGRATION.md tells a maintainer to paste must be the library's struct (same fields, same size)."""
    import ctypes as C
    import os
    from photonic_flash_attention_amd import _capi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "INTEGRATION.md")).read()
    code = src[src.index("class PfaFa3Args(C.Structure):"):src.index("_lib = C.CDLL")]
    ns = {}
    exec("import ctypes as C\n" + code, ns)
    doc = ns["PfaFa3Args"]
    assert [f[0] for f in doc._fields_] == [f[0] for f in _capi.PfaFa3Args._fields_]
    assert C.sizeof(doc) == C.sizeof(_capi.PfaFa3Args)


def test_hf_attention_registration_and_mask_dialect():
    """transformers models take the kernel through AttentionInterface; on a CPU tensor the call fails loudly (no fallback)."""
    transformers = pytest.importorskip("transformers")
    import torch
    from photonic_flash_attention_amd.integration.pytorch import hf
    from photonic_flash_attention_amd.integration.pytorch.convert import convert_to_photonic
    name = hf.register_hf_attention()
    assert name in transformers.AttentionInterface().valid_keys()
    assert hf._keep_mask(None) is None
    b = torch.tensor([[True, False]])
    assert hf._keep_mask(b) is b
    add = torch.tensor([[0.0, -1e4, float("-inf"), torch.finfo(torch.float32).min]])
    assert hf._keep_mask(add).tolist() == [[True, False, False, False]]
    cfg = transformers.BertConfig(hidden_size=256, num_attention_heads=4, num_hidden_layers=1, intermediate_size=256, vocab_size=50)
    model = transformers.BertModel(cfg).eval()
    conv, report = convert_to_photonic(model)
    assert conv is not model and conv.config._attn_implementation == hf.IMPLEMENTATION_NAME
    assert model.config._attn_implementation != hf.IMPLEMENTATION_NAME and report.converted_layers
    with torch.no_grad(), pytest.raises((ValueError, RuntimeError)):
        conv(input_ids=torch.tensor([[1, 2, 3, 4]]))


def test_hf_mask_interface_hands_on_the_compact_form():
    """pfa_attention_mask: a plain causal / bidirectional prefill keeps the caller's 2-D padding mask (the triangle is a flag of the
    kernels); cached decoding, offsets and user mask functions get sdpa's 4-D mask."""
    pytest.importorskip("transformers")
    import torch
    from transformers import masking_utils as mu
    from photonic_flash_attention_amd.integration.pytorch import hf
    am = torch.ones(2, 16, dtype=torch.bool)
    am[1, 10:] = False
    kw = dict(batch_size=2, q_length=16, kv_length=16)
    for fn in (mu.causal_mask_function, mu.bidirectional_mask_function):
        got = hf.pfa_attention_mask(mask_function=fn, attention_mask=am, **kw)
        assert got.dim() == 2 and torch.equal(got, am)
        assert hf.pfa_attention_mask(mask_function=fn, attention_mask=None, **kw) is None
    dec = hf.pfa_attention_mask(batch_size=2, q_length=1, kv_length=16, mask_function=mu.causal_mask_function, attention_mask=am, q_offset=15)
    assert dec is None or dec.dim() == 4                                       # a decode step: sdpa's form (here nothing, or [B,1,1,Sk])
    win = mu.and_masks(mu.causal_mask_function, mu.sliding_window_causal_mask_function(4)) if hasattr(mu, "and_masks") else None
    if win is not None:
        m4 = hf.pfa_attention_mask(mask_function=win, attention_mask=am, **kw)
        assert m4 is not None and m4.dim() == 4 and m4.shape[-2:] == (16, 16)


def test_generator_takes_no_knobs_in_the_product_build_and_is_deterministic(tmp_path):
    """csrc/gen_fa3_fwd_p4.py: a P4_* knob left in the environment stops the product build (they are honoured only with P4_DEV=1,
    which tools/p4_variants.py sets); two runs give byte-identical assembly, 48 kernels."""
    import subprocess
    import sys
    gen = os.path.join(REPO, "photonic_flash_attention_amd", "csrc", "gen_fa3_fwd_p4.py")
    env = {k: v for k, v in os.environ.items() if not k.startswith("P4_")}
    a = subprocess.run([sys.executable, gen], env=env, capture_output=True, text=True, timeout=300)
    b = subprocess.run([sys.executable, gen], env=env, capture_output=True, text=True, timeout=300)
    assert a.returncode == 0 and a.stdout == b.stdout and a.stdout.count(".amdhsa_kernel ") == 48
    bad = subprocess.run([sys.executable, gen], env=dict(env, P4_STAMP="1"), capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0 and "P4_DEV" in bad.stderr and not bad.stdout


def _run_p4_generator(**knobs):
    import subprocess
    import sys
    gen = os.path.join(REPO, "photonic_flash_attention_amd", "csrc", "gen_fa3_fwd_p4.py")
    env = {k: v for k, v in os.environ.items() if not k.startswith("P4_")}
    return subprocess.run([sys.executable, gen], env=dict(env, **knobs), capture_output=True, text=True, timeout=300)


def test_generator_stamped_build_is_the_fast_and_parity_kernels_only_and_deterministic():
    """P4_DEV=1 P4_STAMP=3 (the one diagnostic: kernel totals): 16 kernels -- no key-mask (_km_) or ragged (_kl_) flavour, their mask
    words live where the stamps keep their clock -- that differ from the product build's; two runs give byte-identical assembly."""
    import re
    a, b = _run_p4_generator(P4_DEV="1", P4_STAMP="3"), _run_p4_generator(P4_DEV="1", P4_STAMP="3")
    assert a.returncode == 0 and b.returncode == 0 and a.stdout == b.stdout
    names = re.findall(r"\.amdhsa_kernel (\S+)", a.stdout)
    assert len(names) == 16 and len(set(names)) == 16
    assert not [n for n in names if "_km_" in n or "_kl_" in n]
    prod = _run_p4_generator()
    assert prod.returncode == 0 and prod.stdout != a.stdout


def test_generator_refuses_a_knob_it_does_not_know():
    """P4_DEV=1 with a P4_* name other than P4_STAMP (here a knob that once existed) stops the generator and names it: a mistyped or
    retired knob must not build the base schedule under another name."""
    r = _run_p4_generator(P4_DEV="1", P4_LEAN="0")
    assert r.returncode != 0 and "P4_LEAN" in r.stderr and not r.stdout


def test_generator_knows_one_stamp_mode():
    """P4_STAMP accepts 0 / unset and 3; the per-phase modes 1 and 2 are gone."""
    r = _run_p4_generator(P4_DEV="1", P4_STAMP="1")
    assert r.returncode != 0 and not r.stdout


def test_bench_reads_the_traffic_figure_from_the_newest_profile():
    """bench.py roofline.traffic: parsed from profiles/r*_<workload>_rocprof_summary.md (FETCH_SIZE x 2 + WRITE_SIZE, KiB), not pasted."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("pfa_bench", os.path.join(REPO, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    b, src = bench.pmc_traffic("C3")
    assert b is not None and "r03_C3_rocprof_summary" in src and 2.5e8 < b < 5e8
    assert bench.pmc_traffic("nope") == (None, "no profiles/r*_nope_rocprof_summary.md")

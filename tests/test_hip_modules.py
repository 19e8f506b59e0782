"""GPU tests of the reference-shaped modules and of the rank-2 "next" rows of SURVEY.md section 8(f):
general 4-D masks and need_weights, all through the C ABI.  The assertions re-express what the
reference's own unit tests pin (tests/unit/test_flash_attention_3.py of the reference: shapes/dtype :51-53,
weights shape / row-sum 1 +- 1e-3 / non-negative :71-79, mask changes output :104-115, Sq != Skv :117-135,
eval determinism :186-191, batch sizes :232-247, (E,H) grid :264-285, stats keys :221-229)."""

from __future__ import annotations

import pytest
import torch

from conftest import load_golden
from photonic_flash_attention_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _oracle():
    from oracle import fa3_oracle as orc
    return orc


def _state(E, seed):
    return {
        "qkv_proj.weight": torch.from_numpy(synth.normal_f32((3 * E, E), seed + 10)) * E ** -0.5,
        "qkv_proj.bias": torch.from_numpy(synth.normal_f32((3 * E,), seed + 11)) * 0.1,
        "out_proj.weight": torch.from_numpy(synth.normal_f32((E, E), seed + 12)) * E ** -0.5,
        "out_proj.bias": torch.from_numpy(synth.normal_f32((E,), seed + 13)) * 0.1,
    }


def test_general_4d_mask_matches_reference_golden():
    """g4 fixtures were produced by the reference with a 4-D mask; feed the same 4-D mask through `mask=`."""
    from photonic_flash_attention_amd import ops
    for name in ("g4_s640_d64_kvtail", "g4_s640_d128_kvtail_causal"):
        meta, arr = load_golden(name)
        q, k, v = synth.qkv(meta["B"], meta["H"], meta["Sq"], meta["Sk"], meta["D"], meta["seed"], "bf16")
        Sq, Sk = meta["Sq"], meta["Sk"]
        m = (torch.arange(Sk) < meta["kv_valid"]).view(1, 1, 1, Sk).expand(meta["B"], 1, Sq, Sk)
        if meta["causal"]:
            m = m & torch.tril(torch.ones(Sq, Sk, dtype=torch.bool)).view(1, 1, Sq, Sk)
        o, _ = ops.fa3_forward_bshd(q.to(DEV), k.to(DEV), v.to(DEV), mask=m.to(DEV), out_dtype=torch.float32)
        err = float((o.cpu() - torch.from_numpy(arr["out"])).abs().max())
        assert err <= 1e-3, (name, err)


def test_random_4d_mask_and_broadcast_forms():
    from photonic_flash_attention_amd import ops
    orc = _oracle()
    B, H, Sq, Sk, D = 2, 3, 200, 333, 64
    q, k, v = synth.qkv(B, H, Sq, Sk, D, 77, "bf16")
    g = torch.Generator().manual_seed(5)
    for shape in [(B, H, Sq, Sk), (1, 1, Sq, Sk), (B, 1, 1, Sk), (1, H, Sq, Sk)]:
        m = torch.rand(shape, generator=g) > 0.4
        m[..., 0] = True                       # keep every row alive (parity domain)
        ref = orc.flash_attention_forward(q.float().permute(0, 2, 1, 3), k.float().permute(0, 2, 1, 3),
                                          v.float().permute(0, 2, 1, 3), m.expand(B, H, Sq, Sk)).permute(0, 2, 1, 3)
        o, _ = ops.fa3_forward_bshd(q.to(DEV), k.to(DEV), v.to(DEV), mask=m.to(DEV), out_dtype=torch.float32)
        assert float((o.cpu() - ref).abs().max()) <= 1e-3, shape


@pytest.mark.parametrize("case", [(2, 2, 128, 128, 64, False), (1, 3, 300, 517, 128, False), (1, 2, 384, 384, 64, True)])
def test_attention_weights_are_the_true_softmax(case):
    from photonic_flash_attention_amd import ops
    B, H, Sq, Sk, D, causal = case
    q, k, v = synth.qkv(B, H, Sq, Sk, D, 31, "bf16")
    o, _, w = ops.fa3_forward_bshd(q.to(DEV), k.to(DEV), v.to(DEV), causal=causal, return_weights=True,
                                   weights_dtype=torch.float32, out_dtype=torch.float32)
    s = torch.matmul(q.double().permute(0, 2, 1, 3), k.double().permute(0, 2, 3, 1)) * D ** -0.5
    if causal:
        s = s.masked_fill(~torch.tril(torch.ones(Sq, Sk, dtype=torch.bool)), float("-inf"))
    ref = torch.softmax(s, dim=-1).float()
    w = w.cpu()
    assert w.shape == (B, H, Sq, Sk)
    assert float((w - ref).abs().max()) <= 1e-4
    assert bool((w >= 0).all()) and float((w.sum(-1) - 1).abs().max()) <= 1e-3      # reference test :75-79
    # and P V reproduces the kernel's own output
    pv = torch.matmul(w.double(), v.double().permute(0, 2, 1, 3)).permute(0, 2, 1, 3).float()
    assert float((pv - o.cpu()).abs().max()) <= 1e-3


def test_module_forward_matches_reference_module_golden():
    """Whole PhotonicFlashAttention forward on the GPU (projections by hipBLASLt through nn.Linear + our
    kernel) against the real reference module's fp32 CPU output (g1_c1_module, BASELINE config C1).
    An fp32 module (the reference's default dtype) runs the EXACT fp32 core by default: the north-star tolerance holds at the
    module output.  fp32_attention="bf16" is the explicit opt-in to bf16 attention operands (tolerance = bf16 input rounding)."""
    from photonic_flash_attention_amd import PhotonicFlashAttention, _capi, ops
    meta, arr = load_golden("g1_c1_module")
    E, H, seed = meta["E"], meta["H"], meta["seed"]
    m = PhotonicFlashAttention(E, H).eval()
    m.gpu_attention.load_state_dict(_state(E, seed))
    m = m.to(DEV)
    x = torch.from_numpy(synth.normal_f32((meta["B"], meta["S"], E), seed)).to(DEV)
    with torch.no_grad():
        y = m(x)
    assert isinstance(y, torch.Tensor) and y.shape == x.shape and y.dtype == x.dtype and y.device == x.device
    err = float((y.cpu() - torch.from_numpy(arr["out"])).abs().max())
    print(f"fp32 module (exact core) vs reference module: max-abs {err:.3e}")
    assert err <= 1e-3                                  # measured ~1e-6: fp32 GEMMs + fp32 core
    assert m.last_device_used == "gpu" and m.get_performance_stats()["gpu_calls"] == 1
    m.gpu_attention.fp32_attention = "bf16"
    with torch.no_grad():
        yb = m(x)
    errb = float((yb.cpu() - torch.from_numpy(arr["out"])).abs().max())
    print(f"fp32 module, bf16 attention operands (opt-in): max-abs {errb:.3e}")
    assert err < errb <= 3e-2
    q = torch.zeros(1, 2, 64, 64, device=DEV)
    assert _capi.describe(ops.build_args(q, q, q, torch.empty_like(q))[0])[0] == "fa3_fwd_f32_mfma_d64_exact"


@pytest.mark.parametrize("case", [(2, 3, 130, 257, 64, True, None), (1, 2, 300, 300, 128, True, [211]), (2, 2, 64, 1000, 128, False, [1000, 3]),
                                  (1, 4, 200, 200, 40, False, None), (1, 8, 96, 96, 128, False, None)])
def test_exact_fp32_kernel_against_the_oracle(case):
    """fp32 operands at the C ABI (the exact kernel of fp32 modules): the oracle's numbers to fp32 rounding, masks included, LSE too;
    grouped-query heads read in place."""
    from photonic_flash_attention_amd import ops
    orc = _oracle()
    B, H, Sq, Sk, D, causal, lens = case
    q = torch.from_numpy(synth.normal_f32((B, Sq, H, D), 1 + Sq))
    k = torch.from_numpy(synth.normal_f32((B, Sk, H, D), 2 + Sk))
    v = torch.from_numpy(synth.normal_f32((B, Sk, H, D), 3 + D))
    ref = orc.attention_bshd(q, k, v, causal=causal, seqlens_k=lens)
    out, lse = ops.fa3_forward_bshd(q.to(DEV), k.to(DEV), v.to(DEV), causal=causal, seqlens_k=lens, return_lse=True)
    assert out.dtype == torch.float32
    assert float((out.cpu() - ref).abs().max()) <= 2e-5, case
    ref_lse = orc.lse_bshd(q, k, causal=causal, seqlens_k=lens)
    fin = torch.isfinite(ref_lse)
    assert float((lse.cpu() - ref_lse)[fin].abs().max()) <= 2e-5 and torch.equal(torch.isfinite(lse.cpu()), fin)
    if lens is None and not causal:                      # a general [B,1,Sq,Sk] mask and a [B,Sk] key mask
        m4 = torch.from_numpy(synth.normal_f32((B, 1, Sq, Sk), 9)) > -0.7
        m4[..., 0] = True
        got = ops.fa3_forward_bshd(q.to(DEV), k.to(DEV), v.to(DEV), mask=m4.to(DEV))[0]
        want = orc.flash_attention_forward(q.permute(0, 2, 1, 3), k.permute(0, 2, 1, 3), v.permute(0, 2, 1, 3), m4, D ** -0.5).permute(0, 2, 1, 3)
        assert float((got.cpu() - want).abs().max()) <= 2e-5
        if H % 2 == 0:
            kg, vg = k[:, :, ::2].contiguous(), v[:, :, ::2].contiguous()      # two query heads per K/V head
            got = ops.fa3_forward_bshd(q.to(DEV), kg.to(DEV), vg.to(DEV))[0]
            want = orc.attention_bshd(q, kg.repeat_interleave(2, dim=2), vg.repeat_interleave(2, dim=2))
            assert float((got.cpu() - want).abs().max()) <= 2e-5


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("cfg", [(2, 128, 512, 8), (4, 256, 768, 12), (1, 512, 1024, 16), (2, 96, 384, 6),
                                 (2, 160, 256, 8), (1, 640, 384, 4)])      # head dims 32 and 96: zero-padded kernels
def test_module_contract_like_reference_unit_tests(cfg, dtype):
    from photonic_flash_attention_amd import FlashAttention3
    orc = _oracle()
    B, S, E, H = cfg
    m = FlashAttention3(E, H, dtype=dtype).to(DEV).eval()
    x = torch.from_numpy(synth.normal_f32((B, S, E), 3)).to(DEV, dtype)
    mask = torch.ones(B, S, dtype=torch.bool, device=DEV)
    mask[:, S - S // 10:] = False                                    # conftest.py:41-59 of the reference
    with torch.no_grad():
        out, w0 = m(x)
        out2, _ = m(x)
        outm, _ = m(x, attention_mask=mask)
        outw, w = m(x, need_weights=True)
    assert w0 is None and out.shape == (B, S, E) and out.dtype == dtype and out.device == x.device
    assert bool(torch.isfinite(out.float()).all()) and float(out.float().abs().max()) > 0
    assert torch.equal(out, out2)                                    # eval-mode determinism
    assert not torch.allclose(out.float(), outm.float())            # mask changes the output
    assert w.shape == (B, H, S, S) and bool((w >= 0).all())
    assert float((w.float().sum(-1) - 1).abs().max()) <= (1e-3 if dtype == torch.float16 else 8e-3)
    assert torch.equal(out, outw)
    # numbers: same weights in the oracle's module restatement, fp32
    sd = {k_: v_.float().cpu() for k_, v_ in m.state_dict().items()}
    ref = orc.module_forward(sd, H, x.float().cpu())
    tol = 3e-2 if dtype == torch.bfloat16 else 6e-3
    assert float((out.float().cpu() - ref).abs().max()) <= tol
    assert set(m.get_performance_stats()) == {"latency_ms", "memory_mb", "device", "implementation"}


def test_cross_attention_and_mha_facade():
    from photonic_flash_attention_amd import FlashAttention3, PhotonicMultiHeadAttention
    orc = _oracle()
    E, H = 256, 4
    m = FlashAttention3(E, H, dtype=torch.bfloat16).to(DEV).eval()
    xq = torch.from_numpy(synth.normal_f32((2, 100, E), 1)).to(DEV, torch.bfloat16)
    xkv = torch.from_numpy(synth.normal_f32((2, 333, E), 2)).to(DEV, torch.bfloat16)
    with torch.no_grad():
        y, _ = m(xq, xkv, xkv)                                     # Sq != Skv (reference test :117-135)
    sd = {k_: v_.float().cpu() for k_, v_ in m.state_dict().items()}
    ref = orc.module_forward(sd, H, xq.float().cpu(), xkv.float().cpu(), xkv.float().cpu())
    assert y.shape == (2, 100, E) and float((y.float().cpu() - ref).abs().max()) <= 3e-2

    mha = PhotonicMultiHeadAttention(E, H, batch_first=False, dtype=torch.bfloat16).to(DEV).eval()
    x = xq.transpose(0, 1).contiguous()                              # (L, N, E)
    kpm = torch.ones(2, 100, dtype=torch.bool, device=DEV)
    kpm[:, 90:] = False                                              # reference semantics: 0 = masked
    with torch.no_grad():
        out, w = mha(x, x, x, key_padding_mask=kpm)                  # need_weights defaults to True
        out_c, w_none = mha(x, x, x, need_weights=False, is_causal=True)
    assert out.shape == (100, 2, E) and w.shape == (2, 100, 100) and w_none is None and out_c.shape == out.shape
    assert float(w[:, :, 90:].abs().max()) == 0.0
    assert float((w.float().sum(-1) - 1).abs().max()) <= 8e-3


def test_hybrid_returns_raw_tuple_and_counts_gpu_samples():
    from photonic_flash_attention_amd import HybridFlashAttention
    h = HybridFlashAttention(512, 8, dtype=torch.bfloat16, max_concurrent_requests=2).to(DEV).eval()
    x = torch.from_numpy(synth.normal_f32((8, 1024, 512), 4)).to(DEV, torch.bfloat16)   # B*S*S >> 1e6
    with torch.no_grad():
        for _ in range(12):
            r = h(x, is_causal=True)
    assert isinstance(r, tuple) and r[1] is None and r[0].shape == x.shape
    st = h.get_performance_stats()
    assert st["gpu_samples"] == 12 and st["photonic_samples"] == 0 and st["total_requests"] == 12


def test_grad_mode_and_dropout_rules():
    from photonic_flash_attention_amd import FlashAttention3
    m = FlashAttention3(128, 2, dropout=0.1, dtype=torch.bfloat16).to(DEV)
    x = torch.zeros(1, 16, 128, device=DEV, dtype=torch.bfloat16)
    m.train()
    assert m(x)[0].shape == x.shape                     # training-mode attention dropout of the dense branch: the fp32 kernels
    with torch.no_grad():
        assert m(x)[0].shape == x.shape
    with pytest.raises(NotImplementedError):            # ... only the dropped weights themselves are not returned
        m(x, need_weights=True)
    m.eval()
    assert m(x)[0].requires_grad                        # eval + autograd: differentiable through pfa_fa3_bwd
    assert m(x, attention_mask=torch.ones(1, 16, device=DEV))[0].requires_grad    # ... masks included
    out, w = m(x, need_weights=True)                   # ... and the weights come back detached (second pass on the saved LSE)
    assert out.requires_grad and w is not None and not w.requires_grad and w.shape == (1, 2, 16, 16)
    with torch.no_grad():
        assert m(x)[0].shape == x.shape                 # dropout is a no-op in eval (:174-175)


def test_forward_is_capturable_in_a_hip_graph():
    """Launch-bound shapes (BASELINE config C1) replay from a captured graph: the C ABI launches on the caller's
    stream with no hidden synchronisation or allocation, so stream capture sees one kernel node per call."""
    from photonic_flash_attention_amd import ops
    q, k, v = (t.to(DEV).permute(0, 2, 1, 3) for t in synth.qkv(2, 4, 128, 128, 64, 1001, "bf16"))
    out = torch.empty(2, 128, 4, 64, device=DEV, dtype=torch.bfloat16).permute(0, 2, 1, 3)
    eager = ops.fa3_forward(q, k, v, causal=True)[0].clone()
    g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(s):
        ops.fa3_forward(q, k, v, causal=True, out=out)         # warm-up outside the capture (library load, attributes)
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            ops.fa3_forward(q, k, v, causal=True, out=out)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


def test_hugging_face_models_run_on_the_kernel():
    """transformers model OBJECTS (random weights built offline from a config) switched to the HIP attention function:
    BERT (bidirectional, padding mask) and GPT-2 (causal) reproduce their own sdpa outputs within the bf16-operand
    tolerance, and train (gradients reach the embeddings)."""
    transformers = pytest.importorskip("transformers")
    from photonic_flash_attention_amd import convert_to_photonic
    torch.manual_seed(0)
    cfg = transformers.BertConfig(hidden_size=256, num_attention_heads=4, num_hidden_layers=2, intermediate_size=512,
                                  vocab_size=500, max_position_embeddings=256)
    bert = transformers.BertModel(cfg).to(DEV).eval()
    ids = torch.randint(0, 500, (2, 200), device=DEV)
    am = torch.ones(2, 200, dtype=torch.long, device=DEV)
    am[1, 150:] = 0
    with torch.no_grad():
        ref = bert(input_ids=ids, attention_mask=am).last_hidden_state
    conv, report = convert_to_photonic(bert)
    assert report.converted_layers and conv.config._attn_implementation == "pfa_hip"
    with torch.no_grad():
        got = conv(input_ids=ids, attention_mask=am).last_hidden_state
    valid = am.bool()
    err = float((got - ref)[valid].abs().max())
    print(f"BERT (2 layers) vs its sdpa path: max-abs {err:.3e}")
    assert err <= 5e-2 and bool(torch.isfinite(got).all())
    conv.train()
    for m_ in conv.modules():
        if isinstance(m_, torch.nn.Dropout):
            m_.p = 0.0
    out = conv(input_ids=ids, attention_mask=am).last_hidden_state
    out[valid].square().mean().backward()
    g = conv.embeddings.word_embeddings.weight.grad
    assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().sum()) > 0

    gcfg = transformers.GPT2Config(n_embd=256, n_head=4, n_layer=2, vocab_size=500, n_positions=512, bos_token_id=0, eos_token_id=1)
    gpt = transformers.GPT2Model(gcfg).to(DEV).eval()
    ids2 = torch.randint(0, 500, (2, 300), device=DEV)
    with torch.no_grad():
        ref2 = gpt(input_ids=ids2).last_hidden_state
        conv2, _ = convert_to_photonic(gpt)
        got2 = conv2(input_ids=ids2).last_hidden_state
    err2 = float((got2 - ref2).abs().max())
    print(f"GPT-2 (2 layers) vs its sdpa path: max-abs {err2:.3e}")
    assert err2 <= 5e-2
    # padded decoder batches (round 3): the mask interface hands the kernels the 2-D padding mask + the causal flag instead of a
    # [B,1,Sq,Sk] tensor -> the persistent key-mask kernels, tile counts cut to each batch's keys; right and left padding
    from photonic_flash_attention_amd.integration.pytorch import hf
    seen = []
    orig = hf.ops.fa3_attention

    def spy(q, k, v, **kw):
        seen.append((kw.get("causal"), None if kw.get("key_mask") is None else tuple(kw["key_mask"].shape), kw.get("mask") is not None))
        return orig(q, k, v, **kw)
    hf.ops.fa3_attention = spy
    try:
        for side in ("right", "left"):
            am2 = torch.ones(2, 300, dtype=torch.long, device=DEV)
            if side == "right":
                am2[1, 210:] = 0
            else:
                am2[1, :90] = 0
            pos = (am2.cumsum(-1) - 1).clamp(min=0)
            with torch.no_grad():
                conv2.config._attn_implementation = "sdpa"
                want = conv2(input_ids=ids2, attention_mask=am2, position_ids=pos).last_hidden_state
                conv2.config._attn_implementation = "pfa_hip"
                seen.clear()
                got3 = conv2(input_ids=ids2, attention_mask=am2, position_ids=pos).last_hidden_state
            err3 = float((got3 - want)[am2.bool()].abs().max())
            print(f"GPT-2, {side}-padded batch vs its sdpa path (valid positions): max-abs {err3:.3e}; kernel calls {seen[:1]}")
            assert err3 <= 5e-2 and bool(torch.isfinite(got3[am2.bool()]).all())
            assert seen and all(c is True and km == (2, 300) and not m4 for c, km, m4 in seen)      # flag + 2-D mask, no 4-D tensor
    finally:
        hf.ops.fa3_attention = orig


def test_hugging_face_llama_style_gqa_model():
    """A Llama-style decoder (rotary embeddings, grouped-query attention: 4 query heads on 2 K/V heads, head_dim 64)."""
    transformers = pytest.importorskip("transformers")
    from photonic_flash_attention_amd import convert_to_photonic
    torch.manual_seed(1)
    cfg = transformers.LlamaConfig(hidden_size=256, num_attention_heads=4, num_key_value_heads=2, num_hidden_layers=2,
                                   intermediate_size=512, vocab_size=500, max_position_embeddings=1024)
    model = transformers.LlamaModel(cfg).to(DEV).eval()
    ids = torch.randint(0, 500, (2, 384), device=DEV)
    with torch.no_grad():
        ref = model(input_ids=ids).last_hidden_state
        conv, _ = convert_to_photonic(model)
        got = conv(input_ids=ids).last_hidden_state
    err = float((got - ref).abs().max())
    print(f"Llama-style (2 layers, GQA) vs its sdpa path: max-abs {err:.3e}")
    assert err <= 5e-2 and bool(torch.isfinite(got).all())


def test_hugging_face_llama_style_gqa_model_trains_without_expanding_kv():
    """Same decoder in bf16 under autograd: the HIP path hands the backward K/V with 2 heads for 4 query heads (ABI v7, summed over the
    group inside the dK/dV kernel); parameter gradients against the model's own sdpa path."""
    transformers = pytest.importorskip("transformers")
    from photonic_flash_attention_amd import convert_to_photonic, ops
    torch.manual_seed(2)
    cfg = transformers.LlamaConfig(hidden_size=256, num_attention_heads=4, num_key_value_heads=2, num_hidden_layers=2,
                                   intermediate_size=512, vocab_size=500, max_position_embeddings=1024)
    import copy
    model32 = transformers.LlamaModel(cfg).to(DEV).train()
    model = copy.deepcopy(model32).to(torch.bfloat16)
    ids = torch.randint(0, 500, (2, 320), device=DEV)

    def grads(m):
        m.zero_grad(set_to_none=True)
        (m(input_ids=ids).last_hidden_state.float().square().mean() * 1024.0).backward()
        return {n: p.grad.float().clone() for n, p in m.named_parameters() if ("k_proj" in n or "v_proj" in n or "q_proj" in n) and p.grad is not None}
    ref32 = grads(model32)           # the fp32 model on its own sdpa path: the yardstick
    ref16 = grads(model)             # the bf16 model on its own sdpa path: what bf16 costs
    conv, _ = convert_to_photonic(model)
    seen = []
    orig = ops.fa3_backward

    def spy(q, k, v, *a, **kw):
        seen.append((q.shape[1], k.shape[1]))
        return orig(q, k, v, *a, **kw)
    ops.fa3_backward = spy
    try:
        got = grads(conv)
    finally:
        ops.fa3_backward = orig
    assert seen and all(hq == 4 and hk == 2 for hq, hk in seen), seen          # K/V were NOT expanded for the backward
    assert set(got) == set(ref32) and len(got) >= 6
    for n in ref32:
        nrm = float(ref32[n].norm())
        e_sdpa, e_pfa = float((ref16[n] - ref32[n]).norm()) / nrm, float((got[n] - ref32[n]).norm()) / nrm
        assert e_pfa <= 1.5 * e_sdpa + 0.02, (n, e_pfa, e_sdpa)


def test_training_dropout_follows_the_reference_branch_rule():
    """The reference drops attention weights only in its dense branch (S <= 512, `:174-175`); its tiled branch has no
    dropout.  A dropout > 0 module therefore trains at S = 640 with no dropout applied (two passes agree bit for bit), as in the
    reference, and drops weights at S = 128 (two passes differ)."""
    from photonic_flash_attention_amd import FlashAttention3
    m = FlashAttention3(128, 2, dropout=0.1, dtype=torch.bfloat16).to(DEV).train()
    x = torch.randn(1, 640, 128, device=DEV, dtype=torch.bfloat16, requires_grad=True)
    y = m(x)[0]
    y.float().square().mean().backward()
    assert x.grad is not None and bool(torch.isfinite(x.grad.float()).all())
    with torch.no_grad():
        assert torch.equal(m(x)[0], m(x)[0])
        xs = torch.randn(1, 128, 128, device=DEV, dtype=torch.bfloat16)
        assert not torch.equal(m(xs)[0], m(xs)[0])


@pytest.mark.parametrize("case", [(2, 3, 200, 333, 64, True), (1, 2, 300, 1024, 128, True), (2, 2, 257, 640, 128, False),
                                  (1, 4, 1024, 1024, 64, True)])
def test_weights_pass_writes_every_element(case):
    """`pfa_fa3_weights` takes an UNINITIALISED buffer: blocks above the causal diagonal / past a batch's key length are written as
    zeros by the kernel itself (no caller zero-fill).  The allocator is poisoned with NaN first so that an element the kernel
    skipped cannot pass by luck; Sk = 333 also takes the unaligned per-lane path."""
    from photonic_flash_attention_amd import ops
    orc = _oracle()
    B, H, Sq, Sk, D, causal = case
    q, k, v = synth.qkv(B, H, Sq, Sk, D, 7100 + Sq, "bf16")
    lens = [Sk - 37 * b_ for b_ in range(B)]
    qd, kd, vd = (t.to(DEV).permute(0, 2, 1, 3) for t in (q, k, v))
    for wdt in (torch.float32, torch.bfloat16):
        poison = torch.full((B, H, Sq, Sk), float("nan"), dtype=wdt, device=DEV)
        del poison                       # the caching allocator hands the same block to the weights tensor below
        w = ops.fa3_forward(qd, kd, vd, causal=causal, seqlens_k=lens, return_weights=True, weights_dtype=wdt)[2]
        torch.cuda.synchronize()
        assert bool(torch.isfinite(w.float()).all()), (case, wdt)
        s = (q.float().permute(0, 2, 1, 3) @ k.float().permute(0, 2, 3, 1)) * D ** -0.5
        keep = torch.ones(Sq, Sk, dtype=torch.bool)
        if causal:
            keep &= torch.ones(Sq, Sk, dtype=torch.bool).tril()
        keep = keep[None, None].expand(B, H, Sq, Sk).clone()
        for b_, n_ in enumerate(lens):
            keep[b_, :, :, n_:] = False
        ref = torch.nan_to_num(torch.softmax(s.masked_fill(~keep, float("-inf")), dim=-1), nan=0.0)
        got = w.float().cpu()
        assert float((got - ref).abs().max()) <= (2e-3 if wdt == torch.float32 else 6e-3), (case, wdt)
        assert float(got[~keep].abs().max()) == 0.0


def test_cli_benchmark_schema(tmp_path):
    """Counterpart of the reference's `photonic-benchmark` (cli.py:20-145): same flags, same result keys (cli.py:91-141)."""
    import json
    from photonic_flash_attention_amd import cli
    out = tmp_path / "bench.json"
    args = cli._parser().parse_args(["--seq-lengths", "128", "640", "--batch-sizes", "2", "--embed-dim", "256",
                                     "--num-heads", "4", "--num-iterations", "3", "--output", str(out)])
    res = cli.benchmark(args)
    ref_keys = {"batch_size", "seq_length", "embed_dim", "num_heads", "avg_latency_ms", "std_latency_ms",
                "min_latency_ms", "max_latency_ms", "tokens_per_sec", "last_device_used", "gpu_calls",
                "photonic_calls", "photonic_usage_ratio"}
    assert len(res) == 2 and all(ref_keys <= set(r) for r in res)
    assert all(r["last_device_used"] == "gpu" and r["attn_tflops"] > 0 for r in res)
    data = json.loads(out.read_text())
    assert set(data) == {"benchmark_info", "results"} and {"version", "timestamp", "device_info", "config"} <= set(data["benchmark_info"])


def test_bench_plain_run_times_its_steps_and_dumps_the_output(tmp_path):
    """bench.py without --full: one JSON line over exactly --steps timed launches and none of the secondary legs; --dump-outputs
    writes what the last step computed (a fixed sample of C3's output rows), the forward of the same seeded inputs."""
    import json
    import os
    import subprocess
    import sys

    import numpy as np
    from conftest import REPO
    from photonic_flash_attention_amd import ops
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["metric"] == "attention_fwd_tflops" and line["steps"] == 3 and line["ms_per_step"] > 0 and line["dtype"] == "bf16"
    assert line["timing"]["reps"] == 1 and len(line["timing"]["reps_ms_per_step"]) == 1
    assert not {"parity", "cpu_baseline", "other_workloads", "backward", "parity_variant"} & set(line)
    assert sorted(os.listdir(tmp_path)) == ["out_rows.npy", "out_rows_index.npy"]
    rows, idx = np.load(tmp_path / "out_rows.npy"), np.load(tmp_path / "out_rows_index.npy").astype(np.int64)
    assert rows.dtype == np.float32 and rows.shape == (len(idx), 128) and rows.nbytes + idx.nbytes <= 64e6
    gen = torch.Generator(device=DEV).manual_seed(1234)                   # bench.py's make(4, 16, 4096, 128, 1234)
    q, k, v = (torch.randn(4, 4096, 16, 128, device=DEV, dtype=torch.float32, generator=gen).to(torch.bfloat16) for _ in range(3))
    o, _ = ops.fa3_forward_bshd(q, k, v, causal=True)
    ref = o[tuple(torch.from_numpy(idx[:, i]).to(DEV) for i in range(3))].float().cpu().numpy()
    assert float(np.abs(rows - ref).max()) <= 1e-2


def test_convert_to_photonic_transformer_layer_on_gpu():
    """Converted nn.TransformerEncoderLayer (bf16, our kernel; weight rule of the reference's convert.py:441-452) vs the
    ORIGINAL torch layer in fp32 on the CPU."""
    import torch.nn as nn
    from photonic_flash_attention_amd import convert_to_photonic
    torch.manual_seed(1)
    layer = nn.TransformerEncoderLayer(d_model=512, nhead=4, dim_feedforward=1024, dropout=0.0, batch_first=True).eval()
    x = torch.from_numpy(synth.normal_f32((2, 300, 512), 21))
    pad = torch.zeros(2, 300, dtype=torch.bool)
    pad[1, 250:] = True
    causal = nn.Transformer.generate_square_subsequent_mask(300)
    conv, rep = convert_to_photonic(layer, dtype=torch.bfloat16)
    assert rep.converted_layers == ["self_attn"]
    conv = conv.to(DEV).to(torch.bfloat16)
    with torch.no_grad():
        for kw in (dict(), dict(src_key_padding_mask=pad), dict(src_mask=causal, is_causal=True), dict(src_mask=causal)):
            want = layer(x, **kw)
            kw_dev = {k_: (v_.to(DEV) if torch.is_tensor(v_) else v_) for k_, v_ in kw.items()}
            got = conv(x.to(DEV, torch.bfloat16), **kw_dev).float().cpu()
            keep = ~pad if "src_key_padding_mask" in kw else torch.ones(2, 300, dtype=torch.bool)
            err = float((got - want)[keep].abs().max())
            assert err <= 0.12, (list(kw), err)            # bf16 end-to-end layer (LayerNorm + FFN in bf16)
            assert float((got - want)[keep].abs().mean()) <= 0.012
        alibi = (-0.25 * torch.arange(300.0))[None, :].expand(300, 300).contiguous().to(DEV)
        with pytest.raises(ValueError, match="finite biases"):
            conv(x.to(DEV, torch.bfloat16), src_mask=alibi)


@pytest.mark.parametrize("batch_first", [False, True])
def test_mha_facade_numbers_against_the_oracle(batch_first):
    """PhotonicMultiHeadAttention (reference modules.py:235-336): both layouts, key_padding_mask, attn_mask + key_padding_mask
    merged by `+` (:310-315: a score is masked only where BOTH masks are 0), head-averaged weights (:324-325) -- OUTPUT and
    WEIGHTS compared with the oracle's module restatement; the default call (need_weights=True) also with autograd on."""
    from photonic_flash_attention_amd import PhotonicMultiHeadAttention
    orc = _oracle()
    E, H, L, N = 256, 4, 136, 2
    mha = PhotonicMultiHeadAttention(E, H, batch_first=batch_first, dtype=torch.bfloat16).to(DEV).eval()
    mha.gpu_attention.load_state_dict({k_: v_.to(DEV) for k_, v_ in _state(E, 40).items()})
    sd = {k_: v_.float().cpu() for k_, v_ in mha.gpu_attention.state_dict().items()}
    xb = torch.from_numpy(synth.normal_f32((N, L, E), 3)).to(torch.bfloat16)                 # (N, L, E)
    x = (xb if batch_first else xb.transpose(0, 1).contiguous()).to(DEV)
    kpm = torch.ones(N, L)
    kpm[0, 100:] = 0
    kpm[1, 64:] = 0
    am = torch.tril(torch.ones(L, L))                                                        # 0 = masked
    cases = {
        "none": (None, None, None),
        "kpm": (kpm, None, kpm[:, None, None, :]),
        "am+kpm": (kpm, am, ((am[None] + kpm[:, None, :]) != 0).float()[:, None]),           # the reference's `+` merge
    }
    for name, (kp, a_m, ref_mask) in cases.items():
        ref = orc.module_forward(sd, H, xb.float(), mask=ref_mask)
        kw = dict(key_padding_mask=None if kp is None else kp.to(DEV), attn_mask=None if a_m is None else a_m.to(DEV))
        with torch.no_grad():
            out, w = mha(x, x, x, **kw)                                                     # need_weights defaults to True
        outb = out if batch_first else out.transpose(0, 1)
        assert outb.shape == (N, L, E) and w.shape == (N, L, L)
        err = float((outb.float().cpu() - ref).abs().max())
        assert err <= 3e-2, (name, err)                                                     # bf16 projections + bf16 core
        # weights: head average of the true softmax of the oracle's scores
        q, k_, _v = torch.nn.functional.linear(xb.float(), sd["qkv_proj.weight"], sd["qkv_proj.bias"]).chunk(3, dim=-1)
        sc = torch.einsum("nlhd,nshd->nhls", q.view(N, L, H, -1), k_.view(N, L, H, -1)) * (E // H) ** -0.5
        if ref_mask is not None:
            sc = sc.masked_fill(ref_mask.expand(N, H, L, L) == 0 if ref_mask.dim() == 4 else ref_mask == 0, float("-inf"))
        wref = torch.softmax(sc, dim=-1).mean(dim=1)
        assert float((w.float().cpu() - wref).abs().max()) <= 2e-2, name
        assert float((w.float().sum(-1) - 1).abs().max()) <= 8e-3
    # the plain default-argument call under autograd (training or eval): output differentiable, weights returned detached
    xg = x.clone().requires_grad_(True)
    out, w = mha(xg, xg, xg)
    assert w is not None and not w.requires_grad and out.requires_grad
    out.float().square().mean().backward()
    assert xg.grad is not None and bool(torch.isfinite(xg.grad.float()).all()) and float(xg.grad.float().abs().max()) > 0
    ref = orc.module_forward(sd, H, xb.float())
    outb = out if batch_first else out.transpose(0, 1)
    assert float((outb.detach().float().cpu() - ref).abs().max()) <= 3e-2

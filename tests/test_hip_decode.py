"""GPU tests of the split-KV decode path (``ops.fa3_decode`` / ``pfa_fa3_decode``) against fp64 attention with the bottom-right causal
cut, ragged cache lengths and key masks; and the Hugging Face generation loop through it.

The reference and the bounds on O and on the LSE are those of tests/kvcache_testlib.py."""

from __future__ import annotations

import copy

import pytest
import torch

from kvcache_testlib import EPS, capture, check_lse, check_out, device, reference, run_and_check

pytestmark = pytest.mark.gpu


def _problem(B, H, Hkv, Sq, Smax, D, dtype, seed, layout="bhsd"):
    g = torch.Generator(device="cpu").manual_seed(seed)
    dev = device()
    q = torch.randn(B, Sq, H, D, generator=g).to(dev, dtype).permute(0, 2, 1, 3)
    if layout == "bshd":        # flash-attn style [B, Smax, Hkv, D] buffer, passed as a [B, Hkv, Smax, D] view
        k = torch.randn(B, Smax, Hkv, D, generator=g).to(dev, dtype).transpose(1, 2)
        v = torch.randn(B, Smax, Hkv, D, generator=g).to(dev, dtype).transpose(1, 2)
    elif layout == "slice":     # the first Smax positions of a larger preallocated [B, Hkv, Smax + 96, D] cache
        k = torch.randn(B, Hkv, Smax + 96, D, generator=g).to(dev, dtype)[:, :, :Smax]
        v = torch.randn(B, Hkv, Smax + 96, D, generator=g).to(dev, dtype)[:, :, :Smax]
    else:
        k = torch.randn(B, Hkv, Smax, D, generator=g).to(dev, dtype)
        v = torch.randn(B, Hkv, Smax, D, generator=g).to(dev, dtype)
    return q, k, v


def _run_and_check(q, k, v, *, seqlens=None, **kw):
    """The decode on the clean caches it is given (every key of them is finite) against fp64."""
    from photonic_flash_attention_amd import ops
    what = f"decode Sq {q.shape[2]} Smax {k.shape[2]} D {q.shape[-1]}"
    return run_and_check(ops.fa3_decode, q, k, v, seqlens, guarded=False, what=what, **kw)


@pytest.mark.parametrize("H,Hkv", [(32, 8), (8, 8), (28, 4), (64, 1)])
@pytest.mark.parametrize("D", [64, 128])
def test_single_token_head_groups(H, Hkv, D):
    for dtype, Smax in ((torch.bfloat16, 4097), (torch.float16, 65)):
        q, k, v = _problem(2, H, Hkv, 1, Smax, D, dtype, seed=H * 7 + Hkv + D)
        sl = torch.tensor([Smax, Smax // 2 + 1], dtype=torch.int32, device=q.device)
        _run_and_check(q, k, v, seqlens=sl)


@pytest.mark.parametrize("Smax", [1, 63, 64, 65, 4097, 32768])
def test_cache_lengths_and_ragged_batches(Smax):
    q, k, v = _problem(4, 32, 8, 1, Smax, 128, torch.bfloat16, seed=Smax)
    _run_and_check(q, k, v)
    sl = torch.tensor([0, Smax, max(Smax // 3, 1), max(Smax - 1, 0)], dtype=torch.int32, device=q.device)
    _run_and_check(q, k, v, seqlens=sl)
    _run_and_check(q, k, v, seqlens=sl, out_dtype=torch.float32)
    if Smax >= 64:
        q64, k64, v64 = _problem(3, 16, 16, 1, Smax, 64, torch.float16, seed=Smax + 1)
        _run_and_check(q64, k64, v64, seqlens=torch.tensor([Smax, 5, Smax // 2], dtype=torch.int32, device=q.device))


@pytest.mark.parametrize("Sq", [2, 4, 8])
@pytest.mark.parametrize("D", [64, 128])
def test_bottom_right_causal_multi_row(Sq, D):
    q, k, v = _problem(3, 16, 4, Sq, 3000, D, torch.bfloat16, seed=Sq * 11 + D)
    sl = torch.tensor([3000, 1234, Sq - 1], dtype=torch.int32, device=q.device)     # the last batch has rows that see nothing
    _run_and_check(q, k, v, seqlens=sl, causal=True)
    _run_and_check(q, k, v, seqlens=sl, causal=False)
    _run_and_check(q, k, v, seqlens=sl, causal=True, out_dtype=torch.float32)


def test_left_padding_key_mask_with_lengths():
    B, Smax = 3, 2100
    q, k, v = _problem(B, 32, 8, 1, Smax, 128, torch.bfloat16, seed=5)
    dev = q.device
    sl = torch.tensor([2100, 1500, 700], dtype=torch.int32, device=dev)
    km = torch.ones(B, Smax, dtype=torch.bool, device=dev)
    km[1, :300] = False           # left padding
    km[2, :650] = False
    km[0, 1000:1100] = False      # a hole
    _run_and_check(q, k, v, seqlens=sl, key_mask=km)
    # a key mask alone: each batch's length comes from its last visible key (the masked tail is never read)
    km2 = km.clone()
    km2[0, 1800:] = False
    _run_and_check(q, k, v, key_mask=km2)
    # a batch whose mask hides everything
    km2[2] = False
    _run_and_check(q, k, v, key_mask=km2)


@pytest.mark.parametrize("layout", ["bshd", "slice"])
def test_cache_layouts(layout):
    q, k, v = _problem(2, 32, 8, 4, 5000, 128, torch.bfloat16, seed=9, layout=layout)
    sl = torch.tensor([5000, 2222], dtype=torch.int32, device=q.device)
    _run_and_check(q, k, v, seqlens=sl)


def test_outputs_are_bitwise_reproducible():
    from photonic_flash_attention_amd import ops
    q, k, v = _problem(2, 32, 8, 1, 32768, 128, torch.bfloat16, seed=3)
    sl = torch.tensor([32768, 20000], dtype=torch.int32, device=q.device)
    o1, l1 = ops.fa3_decode(q, k, v, cache_seqlens=sl, return_lse=True)
    o2, l2 = ops.fa3_decode(q, k, v, cache_seqlens=sl, return_lse=True)
    torch.cuda.synchronize()
    assert torch.equal(o1, o2) and torch.equal(l1, l2)


def test_agrees_with_the_forward_on_a_single_token():
    from photonic_flash_attention_amd import ops
    q, k, v = _problem(2, 32, 8, 1, 3000, 128, torch.bfloat16, seed=4)
    km = torch.ones(2, 3000, dtype=torch.bool, device=q.device)
    km[1, :100] = False
    km[1, 2500:] = False
    od, _ = ops.fa3_decode(q, k, v, key_mask=km, causal=False)
    of, _ = ops.fa3_forward(q, k, v, key_mask=km)
    torch.cuda.synchronize()
    ref, _, pn = reference(q, k, v, key_mask=km, causal=False)
    eps = EPS[torch.bfloat16]
    bound = 2 * (eps * ref.abs() + 3 * eps * float(v.abs().max()) * pn + 2e-6)
    assert float(((od.double() - of.double()).abs() - bound).max()) <= 0


def test_graph_capture_replays_with_new_lengths_and_cache():
    from photonic_flash_attention_amd import ops
    q, k, v = _problem(2, 32, 8, 1, 4096, 128, torch.bfloat16, seed=6)
    dev = q.device
    sl = torch.tensor([4096, 1000], dtype=torch.int32, device=dev)
    graph, (o, lse) = capture(lambda: ops.fa3_decode(q, k, v, cache_seqlens=sl, return_lse=True))
    graph.replay()
    torch.cuda.synchronize()
    ref, rlse, pn = reference(q, k, v, seqlens=sl)
    check_out(o, ref, pn, float(v.abs().max()), q.dtype, "graph, first replay")
    check_lse(o, lse, rlse, "graph, first replay")
    # new lengths and new cache contents, written in place
    sl.copy_(torch.tensor([77, 3333], dtype=torch.int32))
    g = torch.Generator(device="cpu").manual_seed(60)
    k.copy_(torch.randn(k.shape, generator=g).to(dev, k.dtype))
    v.copy_(torch.randn(v.shape, generator=g).to(dev, v.dtype))
    graph.replay()
    torch.cuda.synchronize()
    ref, rlse, pn = reference(q, k, v, seqlens=sl)
    check_out(o, ref, pn, float(v.abs().max()), q.dtype, "graph, new lengths and cache")
    check_lse(o, lse, rlse, "graph, new lengths and cache")


# --- Hugging Face generation ---------------------------------------------------------------------------------------------------------

def _llama(transformers):
    torch.manual_seed(1)
    cfg = transformers.LlamaConfig(hidden_size=256, num_attention_heads=4, num_key_value_heads=2, num_hidden_layers=2,
                                   intermediate_size=512, vocab_size=500, max_position_embeddings=1024)
    ref = transformers.LlamaForCausalLM(cfg).to(device()).eval()
    ref.config._attn_implementation = "sdpa"
    from photonic_flash_attention_amd.integration.pytorch.hf import convert_hf_model
    return cfg, ref, convert_hf_model(copy.deepcopy(ref))


@pytest.fixture
def decode_spy(monkeypatch):
    from photonic_flash_attention_amd import ops
    calls = []
    real = ops.fa3_decode

    def spy(*a, **kw):
        calls.append(a[0].shape)
        return real(*a, **kw)
    monkeypatch.setattr(ops, "fa3_decode", spy)
    return calls


def _teacher_forced(transformers, ref, conv, ids, attention_mask, make_cache, prefill, steps):
    caches = [make_cache(), make_cache()]
    worst = 0.0
    with torch.no_grad():
        am = attention_mask[:, :prefill] if attention_mask is not None else None
        outs = [m(input_ids=ids[:, :prefill], attention_mask=am, past_key_values=c, use_cache=True) for m, c in zip((ref, conv), caches)]
        worst = max(worst, float((outs[1].logits - outs[0].logits).abs().max()))
        for t in range(prefill, prefill + steps):
            am = attention_mask[:, :t + 1] if attention_mask is not None else None
            outs = [m(input_ids=ids[:, t:t + 1], attention_mask=am, past_key_values=c, use_cache=True) for m, c in zip((ref, conv), caches)]
            assert bool(torch.isfinite(outs[1].logits).all())
            worst = max(worst, float((outs[1].logits - outs[0].logits).abs().max()))
    return worst


def test_hf_cached_decode_steps_reach_the_decode_kernel(decode_spy):
    transformers = pytest.importorskip("transformers")
    cfg, ref, conv = _llama(transformers)
    ids = torch.randint(0, 500, (2, 300), device=device())
    err = _teacher_forced(transformers, ref, conv, ids, None, lambda: transformers.DynamicCache(config=cfg), 284, 16)
    print(f"DynamicCache, 16 steps: logits max-abs vs sdpa {err:.3e}")
    assert err <= 5e-2
    assert len(decode_spy) == 16 * cfg.num_hidden_layers


def test_hf_left_padded_batch_decode(decode_spy):
    transformers = pytest.importorskip("transformers")
    cfg, ref, conv = _llama(transformers)
    ids = torch.randint(0, 500, (2, 200), device=device())
    am = torch.ones(2, 200, dtype=torch.long, device=ids.device)
    am[1, :37] = 0
    err = _teacher_forced(transformers, ref, conv, ids, am, lambda: transformers.DynamicCache(config=cfg), 184, 16)
    print(f"left-padded DynamicCache, 16 steps: logits max-abs vs sdpa {err:.3e}")
    assert err <= 5e-2
    assert len(decode_spy) == 16 * cfg.num_hidden_layers


def test_hf_static_cache_decode(decode_spy):
    transformers = pytest.importorskip("transformers")
    if not hasattr(transformers, "StaticCache"):
        pytest.skip("this transformers has no StaticCache")
    cfg, ref, conv = _llama(transformers)
    ids = torch.randint(0, 500, (2, 150), device=device())
    am = torch.ones(2, 150, dtype=torch.long, device=ids.device)
    am[0, :11] = 0
    err = _teacher_forced(transformers, ref, conv, ids, am,
                          lambda: transformers.StaticCache(config=cfg, max_cache_len=256), 134, 16)
    print(f"StaticCache, 16 steps: logits max-abs vs sdpa {err:.3e}")
    assert err <= 5e-2
    assert len(decode_spy) == 16 * cfg.num_hidden_layers


def test_hf_greedy_generate(decode_spy):
    transformers = pytest.importorskip("transformers")
    cfg, ref, conv = _llama(transformers)
    ids = torch.randint(0, 500, (2, 40), device=device())
    with torch.no_grad():
        out = conv.generate(input_ids=ids, attention_mask=torch.ones_like(ids), max_new_tokens=8, do_sample=False)
    assert out.shape == (2, 48)
    assert len(decode_spy) > 0

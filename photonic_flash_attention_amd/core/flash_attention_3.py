"""``FlashAttention3``: the reference's electronic attention module on the MI355X kernel.

Mirror of ``core/flash_attention_3.py:11-302`` of the reference: same constructor, same
parameter names/shapes (``qkv_proj.weight [3E,E]``, ``out_proj.weight [E,E]`` so existing
state dicts load), same ``forward`` signature and always-a-2-tuple return (:118).  What
changes is everything between the two projections:

* the core seam ``_flash_attention_forward`` (:120-150) is ONE call into ``libpfa_hip.so``
  (``ops.fa3_forward``) instead of the eager dense / 512-tile loops (:152-262);
* q/k/v are consumed as the strided views of the fused projection (:97-99) and the output is
  written ``[B,S,H,D]``, so the ``q * scaling`` pass (:138) and the ``.contiguous()`` copy
  (:107) disappear;
* self-attention is recognised by identity (``key is None or key is query``), not by two
  full-tensor ``torch.equal`` compares that force a host sync (:86); both branches compute
  the same numbers, only the GEMM count differs;
* the per-call ``torch.cuda.synchronize()`` (:114) is opt-in (``GlobalConfig.enable_profiling``).

There is no eager/CPU implementation in this class: host tensors, missing library or an
unsupported argument raise.
"""

from __future__ import annotations

from typing import Optional, Tuple

import torch
import torch.nn as nn

from .. import ops
from ..config import get_config


class _HeadNormWeight(nn.Module):
    """The learned scale of a per-head RMSNorm: ``weight [head_dim]``, ones.  The norm itself runs inside ``ops.qk_norm``."""

    def __init__(self, head_dim: int, device=None, dtype=None):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(head_dim, device=device, dtype=dtype))


class FlashAttention3(nn.Module):
    """Electronic ("gpu") attention branch: QKV projection -> HIP flash forward -> out projection."""

    def __init__(
        self,
        embed_dim: int,
        num_heads: int,
        dropout: float = 0.0,
        bias: bool = True,
        device: Optional[torch.device] = None,
        dtype: Optional[torch.dtype] = None,
        fp32_attention: str = "exact",
        attention_sinks: bool = False,
        rotary: bool = False,
        rotary_base: float = 10000.0,
        rotary_max_position: int = 4096,
        qk_norm: bool = False,
        qk_norm_eps: float = 1e-6,
    ):
        """``fp32_attention`` (not in the reference; only matters for fp32 modules, the reference's default dtype): "exact" runs the
        attention core of an fp32 module in fp32 on the vector ALUs -- the reference's numbers to ~1e-6, at a few TFLOP/s -- and is
        the default, so that nothing is rounded behind the caller's back; "bf16" rounds q, k, v to bf16 and takes the MFMA kernels
        (about 1e-2 from the fp32 reference at the module output, two orders of magnitude faster).  "exact" covers autograd too: the
        fp32 forward and the fp32 backward kernels.

        ``attention_sinks`` (not in the reference): the module holds ``sinks``, one learned fp32 value per head (initially 0: an extra
        key of weight 1 and a zero value row), in every row's softmax denominator -- the GPT-OSS-style layer (``ops.fa3_attention(...,
        sinks=)``).  The attention then runs on the 16-bit kernels; no attention dropout, no ``need_weights``.  False
        (the default): parameters, state dict and launches are the module's without the option.

        ``rotary`` (not in the reference): q and k are rotated between the projection and the attention by the position of their row --
        the Llama / Qwen / GPT-OSS layer (``ops.fa3_attention(..., rotary_cos=, rotary_sin=)``) -- over the whole head dim,
        in the ``rotate_half`` pairing, with the tables of ``ops.rotary_tables(rotary_max_position, head_dim, rotary_base)`` held as
        non-persistent buffers: the state dict is the module's without the option.  Rows at and past ``rotary_max_position`` rotate as
        the last table row.  The attention then runs on the 16-bit kernels; no attention dropout, no ``need_weights``.  False (the
        default): constructor, state dict and launches are what they were.

        ``qk_norm`` (not in the reference): every head of q and k is RMS-normalised over the head dim between the projection and the
        rotation -- the Qwen3 / OLMo-2-style layer (``ops.fa3_attention(..., q_norm_weight=, k_norm_weight=)``) -- with the
        learned ``q_norm.weight`` and ``k_norm.weight`` (``[head_dim]``, initially ones) and ``qk_norm_eps``; with ``rotary`` the norm
        and the rotation are one launch.  The head dim must be 64 or 128.  It refuses where ``rotary`` refuses: attention dropout,
        ``need_weights``, an exact-fp32 module.  False (the default): parameters, state dict and launches are what they were."""
        super().__init__()
        if qk_norm and dropout > 0:
            raise ValueError("qk_norm does not combine with attention dropout")
        if rotary and dropout > 0:
            raise ValueError("rotary does not combine with attention dropout")
        if attention_sinks and dropout > 0:
            raise ValueError("attention_sinks does not combine with attention dropout")
        if fp32_attention not in ("exact", "bf16"):
            raise ValueError('fp32_attention must be "exact" or "bf16"')
        self.fp32_attention = fp32_attention
        self.embed_dim = embed_dim
        self.num_heads = num_heads
        self.dropout = dropout
        self.head_dim = embed_dim // num_heads
        assert self.head_dim * num_heads == embed_dim, "embed_dim must be divisible by num_heads"
        self.scaling = self.head_dim ** -0.5

        self.qkv_proj = nn.Linear(embed_dim, 3 * embed_dim, bias=bias, device=device, dtype=dtype)
        self.out_proj = nn.Linear(embed_dim, embed_dim, bias=bias, device=device, dtype=dtype)
        self.dropout_module = nn.Dropout(dropout) if dropout > 0 else None
        self.sinks = nn.Parameter(torch.zeros(num_heads, dtype=torch.float32, device=device)) if attention_sinks else None

        self.rotary, self.rotary_base, self.rotary_max_position = bool(rotary), float(rotary_base), int(rotary_max_position)
        if self.rotary:
            if self.head_dim % 16 or not 16 <= self.head_dim <= 256:
                raise ValueError(f"rotary needs a head dim that is a multiple of 16 in 16 .. 256, got {self.head_dim}")
            cos, sin = ops.rotary_tables(self.rotary_max_position, self.head_dim, self.rotary_base, device=device)
            self.register_buffer("rotary_cos", cos, persistent=False)
            self.register_buffer("rotary_sin", sin, persistent=False)

        self.qk_norm, self.qk_norm_eps = bool(qk_norm), float(qk_norm_eps)
        if self.qk_norm:
            if self.head_dim not in (64, 128):
                raise ValueError(f"qk_norm needs a head dim of 64 or 128, got {self.head_dim}")
            self.q_norm = _HeadNormWeight(self.head_dim, device, dtype)
            self.k_norm = _HeadNormWeight(self.head_dim, device, dtype)

        # fp32 modules with fp32_attention="bf16", and every fp32 module under autograd, compute attention in this dtype
        self.compute_dtype = torch.bfloat16
        self.last_latency_ms = 0.0
        self.last_memory_mb = 0.0

    # ------------------------------------------------------------------ forward
    def forward(
        self,
        query: torch.Tensor,
        key: Optional[torch.Tensor] = None,
        value: Optional[torch.Tensor] = None,
        attention_mask: Optional[torch.Tensor] = None,
        need_weights: bool = False,
        is_causal: bool = False,
    ) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """query/key/value: ``[B, S, E]``.  Returns ``(output [B,S,E], weights or None)``.

        ``attention_mask``: ``None``, a 2-D ``[B, Sk]`` key mask, or a 3-D/4-D mask broadcastable to
        ``[B, H, Sq, Sk]`` (0 = masked, as in the reference).  Causality, which the reference can only
        express as a dense 4-D mask, is also available as the ``is_causal`` flag (an addition to the
        reference signature; it costs no mask traffic and skips the masked half of the work).
        ``need_weights=True`` returns the true softmax matrix ``[B,H,Sq,Sk]`` from a second kernel pass."""
        profile = get_config().enable_profiling and query.is_cuda
        if profile:
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()

        batch_size, seq_len, embed_dim = query.shape
        self_attn = (key is None or key is query) and (value is None or value is query)
        if self_attn:
            q, k, v = self.qkv_proj(query).chunk(3, dim=-1)
        else:
            key = query if key is None else key
            value = query if value is None else value
            w, b = self.qkv_proj.weight, self.qkv_proj.bias
            e = embed_dim
            lin = nn.functional.linear
            q = lin(query, w[:e], None if b is None else b[:e])
            if key is value:
                k, v = lin(key, w[e:], None if b is None else b[e:]).chunk(2, dim=-1)
            else:
                k = lin(key, w[e:2 * e], None if b is None else b[e:2 * e])
                v = lin(value, w[2 * e:], None if b is None else b[2 * e:])

        q = q.view(batch_size, seq_len, self.num_heads, self.head_dim).transpose(1, 2)
        k = k.view(batch_size, -1, self.num_heads, self.head_dim).transpose(1, 2)
        v = v.view(batch_size, -1, self.num_heads, self.head_dim).transpose(1, 2)

        attn_output, attn_weights = self._flash_attention_forward(
            q, k, v, attention_mask, need_weights, is_causal=is_causal)

        # [B,H,S,D] view of a [B,S,H,D] buffer: this transpose+contiguous is free
        attn_output = attn_output.transpose(1, 2).contiguous().view(batch_size, seq_len, embed_dim)
        output = self.out_proj(attn_output.to(self.out_proj.weight.dtype))

        if profile:
            end.record()
            torch.cuda.synchronize()
            self.last_latency_ms = start.elapsed_time(end)
            self.last_memory_mb = torch.cuda.max_memory_allocated() / 1024 / 1024
        return output, attn_weights if need_weights else None

    # ------------------------------------------------------------------ core seam
    def _flash_attention_forward(
        self,
        q: torch.Tensor,
        k: torch.Tensor,
        v: torch.Tensor,
        attention_mask: Optional[torch.Tensor] = None,
        need_weights: bool = False,
        is_causal: bool = False,
    ) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """q,k,v: ``[B,H,S,D]`` (strided views are fine).  The replaced seam (:120-150)."""
        if not q.is_cuda:
            raise RuntimeError(
                "FlashAttention3 runs on MI355X only: move the module and its inputs to a GPU "
                "(this package ships no CPU or eager implementation of the core)")
        needs_grad = torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or v.requires_grad)
        # 2-D [B,Sk] masks take the cheap key-mask path (:166-167); 3-D / 4-D masks the general one (:168,:235)
        key_mask = attention_mask if (attention_mask is not None and attention_mask.dim() == 2) else None
        mask = attention_mask if (attention_mask is not None and attention_mask.dim() != 2) else None
        if self.rotary or self.qk_norm:
            what = "rotary" if self.rotary else "qk_norm"
            if need_weights:
                raise NotImplementedError(f"need_weights together with {what} is not supported")
            if q.dtype == torch.float32 and self.fp32_attention == "exact":
                raise ValueError(f'{what} runs on the 16-bit kernels: build an fp32 module with fp32_attention="bf16"')
            if self.rotary and self.rotary_cos.dtype != torch.float32:      # module.to(bfloat16) narrowed the buffers with the weights: the tables stay fp32
                self.rotary_cos, self.rotary_sin = ops.rotary_tables(self.rotary_max_position, self.head_dim, self.rotary_base,
                                                                     device=self.rotary_cos.device)
            cd = self.compute_dtype if q.dtype == torch.float32 else q.dtype
            extra = dict(rotary_cos=self.rotary_cos, rotary_sin=self.rotary_sin) if self.rotary else {}
            if self.qk_norm:      # fp32 weights or the compute dtype's: what the kernel takes
                wq, wk = (w if w.dtype in (torch.float32, cd) else w.to(cd) for w in (self.q_norm.weight, self.k_norm.weight))
                extra.update(q_norm_weight=wq, k_norm_weight=wk, qk_norm_eps=self.qk_norm_eps)
            out = ops.fa3_attention(q.to(cd), k.to(cd), v.to(cd), causal=is_causal, key_mask=key_mask, mask=mask, softmax_scale=self.scaling,
                                    out_dtype=q.dtype, sinks=None if self.sinks is None else self.sinks.float(), **extra)
            return out, None
        if self.sinks is not None:
            if need_weights:
                raise NotImplementedError("need_weights together with attention_sinks is not supported")
            if q.dtype == torch.float32 and self.fp32_attention == "exact":
                raise ValueError('attention_sinks runs on the 16-bit kernels: build an fp32 module with fp32_attention="bf16"')
            cd = self.compute_dtype if q.dtype == torch.float32 else q.dtype
            # (.float(): module.to(bfloat16) narrows the parameter with the weights; the kernels take the sinks in fp32)
            out = ops.fa3_attention(q.to(cd), k.to(cd), v.to(cd), causal=is_causal, key_mask=key_mask, mask=mask, softmax_scale=self.scaling,
                                    out_dtype=q.dtype, sinks=self.sinks.float())
            return out, None
        if self.training and self.dropout > 0:
            # The reference applies attention dropout only in its dense branch (:174-175), i.e. when both sequence lengths
            # fit one tile of min(Sq, Sk, 512) (floor 32, :264-293); its tiled branch (:182-262) has no dropout at all.
            # Mirror that: longer sequences train with no attention dropout, exactly like the reference; the dense case runs
            # the fp32 kernels with a keep-mask drawn on the device (torch's generator: the reference's random stream itself
            # cannot be matched, its statistics are) and replayed by the fp32 backward.
            tile = max(32, min(q.shape[2], k.shape[2], 512))
            if q.shape[2] <= tile and k.shape[2] <= tile:
                if need_weights:
                    raise NotImplementedError("need_weights together with training-mode attention dropout is not supported")
                out = ops.fa3_attention_dropout(q, k, v, self.dropout, causal=is_causal, key_mask=key_mask, mask=mask,
                                                softmax_scale=self.scaling)
                return out, None
        if needs_grad:
            # differentiable path: HIP forward (with LSE) + HIP backward (pfa_fa3_bwd), masks included.  need_weights (the
            # default of the nn.MultiheadAttention-shaped facade) gets the softmax matrix from the second pass on the saved
            # LSE, DETACHED: the gradient flows through the output only.
            if q.dtype == torch.float32 and self.fp32_attention == "exact":
                out = ops.fa3_attention(q, k, v, causal=is_causal, key_mask=key_mask, mask=mask, softmax_scale=self.scaling)   # fp32 kernels, both directions
                w = None
                if need_weights:
                    cd = self.compute_dtype
                    with torch.no_grad():
                        w = ops.fa3_forward(q.to(cd), k.to(cd), v.to(cd), causal=is_causal, key_mask=key_mask, mask=mask,
                                            softmax_scale=self.scaling, out_dtype=torch.float32, weights_dtype=torch.float32,
                                            return_weights=True)[2]
                return out, w
            cd = self.compute_dtype if q.dtype == torch.float32 else q.dtype
            res = ops.fa3_attention(q.to(cd), k.to(cd), v.to(cd), causal=is_causal, key_mask=key_mask, mask=mask,
                                    softmax_scale=self.scaling, out_dtype=q.dtype, return_weights=need_weights,
                                    weights_dtype=torch.float32 if q.dtype == torch.float32 else None)
            return (res[0], res[1]) if need_weights else (res, None)

        kw = dict(causal=is_causal, key_mask=key_mask, mask=mask, softmax_scale=self.scaling,
                  return_weights=need_weights)
        if q.dtype == torch.float32 and self.fp32_attention == "exact":
            kw.pop("return_weights")
            out, _ = ops.fa3_forward(q, k, v, **kw)                            # exact fp32 core
            w = None
            if need_weights:                                                  # the softmax matrix: a 16-bit pass of its own
                cd = self.compute_dtype
                w = ops.fa3_forward(q.to(cd), k.to(cd), v.to(cd), out_dtype=torch.float32, weights_dtype=torch.float32,
                                    return_weights=True, **kw)[2]
            return out, w
        if q.dtype == torch.float32:
            cd = self.compute_dtype
            res = ops.fa3_forward(q.to(cd), k.to(cd), v.to(cd), out_dtype=torch.float32,
                                  weights_dtype=torch.float32, **kw)
        else:
            res = ops.fa3_forward(q, k, v, **kw)
        return res[0], (res[2] if need_weights else None)

    def get_performance_stats(self) -> dict:
        """Same keys as the reference (:295-302)."""
        return {
            "latency_ms": self.last_latency_ms,
            "memory_mb": self.last_memory_mb,
            "device": "cuda",
            "implementation": "flash_attention_3",
        }

#!/usr/bin/env python3
"""What does the Python layer hand to the library?  Every C call of a fixed list of public ``ops`` calls, with every argument block
passed by reference printed as ``field=value`` lines: pointer-typed fields as ``null`` / ``set``, everything else exactly
(``workspace_bytes`` included).  The calls go through to the real library, so the run needs the GPU; it takes a few seconds.

Two commits marshal alike iff their outputs are the same, line for line::

    python tools/ops_blocks.py > new.txt          # and the same file run from a checkout of the other commit
    diff parent.txt new.txt

Only the public API and ``_capi.load`` are used.  Shapes are the smallest the rules allow: B 2, H 4, Hkv 2, D 64, 128 cached keys
(or 2 pages of 64), 1 and 3 decode rows, 70 prefill rows, ``cu_seqlens_q = [0, 1, 70]``, ``shared_prefix=64``."""
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from photonic_flash_attention_amd import _capi, ops  # noqa: E402


def _value(ctype, v):
    if isinstance(v, C.Array):
        return "[" + " ".join(_value(v._type_, x) for x in v) + "]"
    if ctype is C.c_void_p:
        return "set" if v else "null"
    return repr(v)


class Recorder:
    """Stands in for the loaded library: prints each call, then forwards it."""

    def __init__(self, lib):
        self._lib = lib
        self.on = False                                          # off while main() prepares its operands

    def __getattr__(self, export):
        fn = getattr(self._lib, export)

        def call(*args):
            if not self.on:
                return fn(*args)
            print(f"  {export}")
            for i, x in enumerate(args):
                block = getattr(x, "_obj", None)                 # byref(block)
                if isinstance(block, C.Structure):
                    print(f"    arg {i}: {type(block).__name__}")
                    for field, ctype in block._fields_:
                        print(f"      {field}={_value(ctype, getattr(block, field))}")
                elif x is None or isinstance(x, C.c_void_p):
                    print(f"    arg {i}: {'set' if x is not None and x.value else 'null'}")
                else:
                    print(f"    arg {i}: {x!r}")
            return fn(*args)
        return call


def main():
    dev = torch.device("cuda:0")
    real = _capi.load()
    recorder = Recorder(real)
    _capi.load = lambda path=None: recorder
    g = torch.Generator(device=dev).manual_seed(5)
    B, H, Hkv, D, Smax, page = 2, 4, 2, 64, 128, 64
    bf = torch.bfloat16

    def rand(*shape, dtype=bf):
        return torch.randn(*shape, device=dev, generator=g).to(dtype)

    def bhsd(b, h, s, dtype=bf):                                 # [B,H,S,D]-shaped view of a [B,S,H,D] buffer, as the calls return it
        return rand(b, s, h, D, dtype=dtype).permute(0, 2, 1, 3)

    def i32(x):
        return torch.tensor(x, dtype=torch.int32, device=dev)

    lens, cu, table = i32([100, 128]), i32([0, 1, 70]), i32([[0, 1], [2, 3]])
    cos, sin = ops.rotary_tables(256, D, device=dev)
    rot = dict(rotary_cos=cos, rotary_sin=sin)
    ones_h, ones_bh = torch.ones(Hkv, device=dev), torch.ones(B, Hkv, device=dev)
    calls = []

    def add(label, fn):
        calls.append((label, fn))

    # --- the dense forward and backward ---------------------------------------------------------------------------------------------
    q, k, v = bhsd(B, H, Smax), bhsd(B, Hkv, Smax), bhsd(B, Hkv, Smax)
    kmask = torch.ones(B, Smax, dtype=torch.bool, device=dev)
    kmask[1, 100:] = False
    emask = torch.ones(B, 1, Smax, Smax, dtype=torch.bool, device=dev).tril()
    fwd = {"plain": {}, "causal": dict(causal=True), "seqlens_k": dict(seqlens_k=[100, 128]), "key_mask": dict(key_mask=kmask),
           "mask": dict(mask=emask), "return_lse": dict(return_lse=True), "out=": dict(out=torch.empty_like(q)),
           "fp32 output": dict(out_dtype=torch.float32), "return_weights": dict(return_weights=True)}
    for label, kw in fwd.items():
        add(f"fa3_forward {label}", lambda kw=kw: ops.fa3_forward(q, k, v, **kw))
    q32, k32, v32 = (bhsd(B, h, 64, torch.float32) for h in (H, H, H))
    drop = torch.rand(B, H, 64, 64, device=dev, generator=g) >= 0.1
    add("fa3_forward fp32 operands", lambda: ops.fa3_forward(q32, k32, v32))
    add("fa3_forward drop_mask", lambda: ops.fa3_forward(q32, k32, v32, drop_mask=drop, drop_scale=1 / 0.9))
    o, lse = ops.fa3_forward(q, k, v, return_lse=True)
    do = torch.randn(B, Smax, H, D, device=dev, generator=g).to(bf).permute(0, 2, 1, 3)
    bwd = {"plain": {}, "causal": dict(causal=True), "seqlens_k": dict(seqlens_k=[100, 128]), "key_mask": dict(key_mask=kmask),
           "mask": dict(mask=emask), "fp32 gradients": dict(grad_dtype=torch.float32)}
    for label, kw in bwd.items():
        add(f"fa3_backward {label}", lambda kw=kw: ops.fa3_backward(q, k, v, o, do, lse, **kw))

    # --- the calls over a KV cache, contiguous and paged ------------------------------------------------------------------------------
    def caches(paged, dtype=bf):
        if paged:
            pools = [rand(4, page, Hkv, D).transpose(1, 2) for _ in range(2)]
            kw = dict(block_table=table)
        else:
            pools = [rand(B, Smax, Hkv, D).transpose(1, 2) for _ in range(2)]
            kw = {}
        if dtype != bf:
            pools = [ops.quantize_kv(p, ones_h) for p in pools]
        return pools[0], pools[1], kw

    for paged in (False, True):
        where = "paged" if paged else "contiguous"
        kc, vc, tkw = caches(paged)
        k8, v8, _ = caches(paged, ops.FP8)
        fp8 = {"FP8 [Hkv]": dict(k_descale=ones_h, v_descale=ones_h), "FP8 [B,Hkv]": dict(k_descale=ones_bh, v_descale=ones_bh)}
        for Sq in (1, 3):
            qd, kn, vn = bhsd(B, H, Sq), bhsd(B, Hkv, Sq), bhsd(B, Hkv, Sq)
            words = ops.tree_mask_from_parents(torch.tensor([[-1, 0, 0][:Sq]] * B, device=dev))[0]
            mask = torch.ones(B, Smax, dtype=torch.bool, device=dev)
            dec = {"plain": {}, "key_mask alone": dict(key_mask=mask, cache_seqlens=None), "key_mask": dict(key_mask=mask),
                   "not causal": dict(causal=False), "return_lse": dict(return_lse=True), "out=": dict(out=torch.empty_like(qd)),
                   "fp32 output": dict(out_dtype=torch.float32), "window": dict(window=32), "tree_mask": dict(tree_mask=words),
                   "shared_prefix": dict(shared_prefix=64), "prefix_key_splits": dict(shared_prefix=64, prefix_key_splits=2),
                   "k_new / v_new": dict(k_new=kn, v_new=vn), "rotary": dict(k_new=kn, v_new=vn, **rot),
                   "rotary interleaved, offsets": dict(k_new=kn, v_new=vn, rotary_interleaved=True, pos_offsets=i32([1, 2]), **rot)}
            for label, kw in dec.items():
                add(f"fa3_decode {where} Sq {Sq} {label}",
                    lambda kw=kw, qd=qd, kc=kc, vc=vc, tkw=tkw: ops.fa3_decode(qd, kc, vc, **{"cache_seqlens": lens, **tkw, **kw}))
            for label, kw in fp8.items():
                add(f"fa3_decode {where} Sq {Sq} {label}",
                    lambda kw=kw, qd=qd, k8=k8, v8=v8, tkw=tkw: ops.fa3_decode(qd, k8, v8, cache_seqlens=lens, **tkw, **kw))
            add(f"fa3_decode {where} Sq {Sq} FP8 k_new / v_new",
                lambda qd=qd, kn=kn, vn=vn, k8=k8, v8=v8, tkw=tkw: ops.fa3_decode(qd, k8, v8, cache_seqlens=lens, k_new=kn, v_new=vn,
                                                                                    k_descale=ones_h, v_descale=ones_h, **tkw))
            add(f"kv_append {where} Sq {Sq}", lambda kn=kn, vn=vn, kc=kc, vc=vc, tkw=tkw: ops.kv_append(kn, vn, kc, vc, cache_seqlens=lens, **tkw))
            for label, kw in fp8.items():
                add(f"kv_append {where} Sq {Sq} {label}",
                    lambda kw=kw, kn=kn, vn=vn, k8=k8, v8=v8, tkw=tkw: ops.kv_append(kn, vn, k8, v8, cache_seqlens=lens, **tkw, **kw))
            rope = {"plain": {}, "q": dict(q=qd), "q in place": dict(q=qd.clone(), q_out="q"), "interleaved": dict(rotary_interleaved=True),
                    "pos_offsets": dict(pos_offsets=i32([1, 2]))}
            for label, kw in rope.items():
                def run(kw=kw, kn=kn, vn=vn, kc=kc, vc=vc, tkw=tkw):
                    kw = dict(kw)
                    if kw.get("q_out") == "q":
                        kw["q_out"] = kw["q"]
                    return ops.rope_append(kn, vn, kc, vc, cache_seqlens=lens, **rot, **tkw, **kw)
                add(f"rope_append {where} Sq {Sq} {label}", run)
        Sq = 70
        qp, kn, vn = bhsd(B, H, Sq), bhsd(B, Hkv, Sq), bhsd(B, Hkv, Sq)
        pre = {"plain": {}, "not causal": dict(causal=False), "return_lse": dict(return_lse=True), "out=": dict(out=torch.empty_like(qp)),
               "fp32 output": dict(out_dtype=torch.float32), "window": dict(window=32), "shared_prefix": dict(shared_prefix=64),
               "prefix_key_splits": dict(shared_prefix=64, prefix_key_splits=2), "prefix_key_splits auto": dict(shared_prefix=64, prefix_key_splits="auto"),
               "key_splits": dict(key_splits=2), "key_splits auto": dict(key_splits="auto"),
               "k_new / v_new": dict(k_new=kn, v_new=vn), "rotary": dict(k_new=kn, v_new=vn, **rot)}
        for label, kw in pre.items():
            add(f"fa3_prefill_cache {where} {label}", lambda kw=kw, kc=kc, vc=vc, tkw=tkw: ops.fa3_prefill_cache(qp, kc, vc, cache_seqlens=lens, **tkw, **kw))
        for label, kw in fp8.items():
            add(f"fa3_prefill_cache {where} {label}", lambda kw=kw, k8=k8, v8=v8, tkw=tkw: ops.fa3_prefill_cache(qp, k8, v8, cache_seqlens=lens, **tkw, **kw))
        add(f"fa3_prefill_cache {where} FP8 k_new / v_new",
            lambda k8=k8, v8=v8, tkw=tkw, kn=kn, vn=vn: ops.fa3_prefill_cache(qp, k8, v8, cache_seqlens=lens, k_new=kn, v_new=vn, k_descale=ones_h,
                                                                              v_descale=ones_h, **tkw))
        qr, knr, vnr = rand(70, H, D), rand(70, Hkv, D), rand(70, Hkv, D)
        rag = dict(cu_seqlens_q=cu, max_seqlen_q=69, cache_seqlens=lens)
        var = {"plain": {}, "not causal": dict(causal=False), "return_lse": dict(return_lse=True), "out=": dict(out=torch.empty_like(qr)),
               "fp32 output": dict(out_dtype=torch.float32), "window": dict(window=32), "k_new / v_new": dict(k_new=knr, v_new=vnr),
               "rotary": dict(k_new=knr, v_new=vnr, **rot)}
        for label, kw in var.items():
            add(f"fa3_prefill_varlen {where} {label}", lambda kw=kw, kc=kc, vc=vc, tkw=tkw: ops.fa3_prefill_varlen(qr, kc, vc, **rag, **tkw, **kw))
        for label, kw in fp8.items():
            add(f"fa3_prefill_varlen {where} {label}", lambda kw=kw, k8=k8, v8=v8, tkw=tkw: ops.fa3_prefill_varlen(qr, k8, v8, **rag, **tkw, **kw))
        add(f"fa3_prefill_varlen {where} FP8 k_new / v_new",
            lambda k8=k8, v8=v8, tkw=tkw: ops.fa3_prefill_varlen(qr, k8, v8, k_new=knr, v_new=vnr, k_descale=ones_bh, v_descale=ones_bh, **rag, **tkw))
        add(f"kv_append {where} cu_seqlens_q", lambda kc=kc, vc=vc, tkw=tkw: ops.kv_append(knr, vnr, kc, vc, **rag, **tkw))
        add(f"kv_append {where} cu_seqlens_q FP8 [B,Hkv]",
            lambda k8=k8, v8=v8, tkw=tkw: ops.kv_append(knr, vnr, k8, v8, k_descale=ones_bh, v_descale=ones_bh, **rag, **tkw))
        add(f"rope_append {where} cu_seqlens_q", lambda kc=kc, vc=vc, tkw=tkw: ops.rope_append(knr, vnr, kc, vc, **rot, **rag, **tkw))
        add(f"rope_append {where} cu_seqlens_q q", lambda kc=kc, vc=vc, tkw=tkw: ops.rope_append(knr, vnr, kc, vc, q=qr, **rot, **rag, **tkw))

    # --- page copy, merge, packed training -----------------------------------------------------------------------------------------
    kp, vp, _ = caches(True)
    add("page_copy plain", lambda: ops.page_copy(kp, vp, i32([[0, 1], [-1, 2]])))
    add("page_copy rows", lambda: ops.page_copy(kp, vp, i32([[0, 1], [2, 3]]), rows=i32([5, 64])))
    parts = [bhsd(B, H, 3, torch.float32) for _ in range(2)]
    lses = [rand(B, H, 3, dtype=torch.float32) for _ in range(2)]
    mrg = {"plain": {}, "return_lse": dict(return_lse=True), "out=": dict(out=torch.empty_like(parts[0])), "16-bit output": dict(out_dtype=bf)}
    for label, kw in mrg.items():
        add(f"attn_merge {label}", lambda kw=kw: ops.attn_merge(parts, lses, **kw))
    add("attn_merge 16-bit parts, strided LSE", lambda: ops.attn_merge([p.to(bf) for p in parts], [x.transpose(1, 2).contiguous().transpose(1, 2) for x in lses]))
    qv, kv_, vv = rand(70, H, D), rand(70, Hkv, D), rand(70, Hkv, D)
    pk = dict(cu_seqlens_q=cu, cu_seqlens_k=cu, max_seqlen_q=69, max_seqlen_k=69)
    vf = {"plain": {}, "causal": dict(causal=True), "return_lse": dict(return_lse=True), "out=": dict(out=torch.empty_like(qv)),
          "fp32 output": dict(out_dtype=torch.float32)}
    for label, kw in vf.items():
        add(f"fa3_varlen_forward {label}", lambda kw=kw: ops.fa3_varlen_forward(qv, kv_, vv, **pk, **kw))
    ov, lv = ops.fa3_varlen_forward(qv, kv_, vv, return_lse=True, **pk)
    dov = rand(70, H, D)
    for label, kw in {"plain": {}, "causal": dict(causal=True), "fp32 gradients": dict(grad_dtype=torch.float32)}.items():
        add(f"fa3_varlen_backward {label}", lambda kw=kw: ops.fa3_varlen_backward(qv, kv_, vv, ov, dov, lv, **pk, **kw))

    torch.cuda.synchronize()
    recorder.on = True
    for label, fn in calls:
        print(label)
        try:
            fn()
        except (ValueError, TypeError) as e:                     # a refusal in front of the launch is part of the record; anything else ends the run
            print(f"  raised {type(e).__name__}: {e}")
    torch.cuda.synchronize()
    print(f"{len(calls)} calls")


if __name__ == "__main__":
    main()

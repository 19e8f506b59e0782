"""GPU tests of the calls over a KV cache on tensors spread past 4 and 8 GiB: every case runs one tiny problem twice, on ordinary
tensors and on far views of one 12.5 GiB arena (tests/far_testlib.py), and ``far_testlib.two_runs`` asserts

  (a) the library saw the far view, not a copy: the argument block ``ops`` built carries the view's pointer and strides;
  (b) ``_capi.describe*`` names the same kernel for both runs;
  (c) every output of the far run -- O, LSE, appended or copied cache rows, rotated q -- is bit-equal to the near run's;
  (d) the near run lies inside the existing bounds of tests/kvcache_testlib.py (attention; an FP8 cache against fp64 on the dequantised
      cache) and of tests/test_hip_attn_merge.py (the merge), or equals ``ops``' own CPU model (the appends and the page copy: the
      executable specification their own GPU tests compare with);
  (e) nothing in the arena outside the declared output regions changed, and no input did.

Inputs live in the arena too, among NaN: a truncated read returns NaN or other elements and fails (c), a truncated write fails (e).
H 4, Hkv 2, pages of 64 keys (128 at D 64: the same 32 KiB), Smax 256, lengths ``[256, 65, 130]`` (five sequences for the narrow stride,
two where a one- or four-byte tensor is placed wide).  bf16 with D 128 and fp16 with D 64 alternate.  fp32 tensors (the rotary tables)
are placed to 4 GiB only and claim the two byte models alone (tests/far_testlib.py says why).  ``CASES`` is built on the host:
tests/test_far_testlib.py checks every layout below without a GPU."""

from __future__ import annotations

import pytest
import torch

import far_testlib as F
from far_testlib import FarCase, Spec, saw_view
from kvcache_testlib import check_lse, check_out, folded_reference, guard, merge_ref64, poisoned, reference, window_lo, with_sink
from photonic_flash_attention_amd import _capi, ops

BF, FP, FP8 = torch.bfloat16, torch.float16, torch.float8_e4m3fn
H, HKV, NUM_PAGES = 4, 2, 2 ** 18 + 64
LENS, LENS5, LENS2 = [256, 65, 130], [256, 65, 130, 1, 200], [256, 65]
ROW_STRIDE, ROW_LENS = 2 ** 22 + 8, [255, 255, 255, 255, 4, 40]         # packed rows: sequences start at rows 0, 255, 510, 765, 1020, 1024
ANCHORS = (2 ** 16, 2 ** 17, 2 ** 17 + 2 ** 16, 2 ** 18, 2 ** 15, 2 ** 16 + 2 ** 15, 2 ** 17 + 2 ** 15, 2 ** 17 + 2 ** 16 + 2 ** 15)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _i32(x):
    return torch.tensor(x, dtype=torch.int32)


def _cu(lens):
    out = [0]
    for n in lens:
        out.append(out[-1] + n)
    return out


def _problem(B, Sq, Smax, D, dtype, seed):
    """q as a [B,H,Sq,D] view of a [B,Sq,H,D] array, contiguous k, v [B,Hkv,Smax,D]; on the host"""
    g = _gen(seed)
    q = torch.randn(B, Sq, H, D, generator=g).to(dtype).permute(0, 2, 1, 3)
    k, v = (torch.randn(B, HKV, Smax, D, generator=g).to(dtype) for _ in range(2))
    return q, k, v


def _out_like(q, dtype=None):
    B, Hq, Sq, D = q.shape
    return torch.empty(B, Sq, Hq, D, dtype=dtype or q.dtype).permute(0, 2, 1, 3)


def page_ids(n):
    """n distinct page ids around 2^15 .. 2^18 in steps of 2^15: 1, 2, 3, ... 8 GiB into a pool of 32 KiB pages, and above 2^18"""
    assert n <= 30
    return [ANCHORS[i % 8] + 3 + 2 * i for i in range(n)]


def page_table(lens, page, Smax, seed, lo=None, ids=None):
    """The pages a batch of sequences needs -> ([(b, j, position in the near run's small pool, id in the far pool)], the sorted live ids,
    the near run's table (positions), the far run's table (ids)).  Entries behind a length, and below ``lo_b // page``, stay -1 and get
    no page."""
    need = [(b, j) for b in range(len(lens)) for j in range((lo[b] if lo else 0) // page, -(-lens[b] // page))]
    ids = page_ids(len(need)) if ids is None else ids
    live = sorted(ids)
    order = torch.randperm(len(need), generator=_gen(seed)).tolist()
    tn = torch.full((len(lens), Smax // page), -1, dtype=torch.int32)
    tf = tn.clone()
    where = []
    for n, (b, j) in enumerate(need):
        pid = ids[order[n]]
        where.append((b, j, live.index(pid), pid))
        tn[b, j], tf[b, j] = live.index(pid), pid
    return where, live, tn, tf


def paged(kn, vn, lens, page, seed, lo=None, ids=None):
    """Contiguous caches over pools -> (k pages [n,Hkv,page,D], v pages, ``page_table``'s live ids and two tables)"""
    B, Hkv, Smax, D = kn.shape
    where, live, tn, tf = page_table(lens, page, Smax, seed, lo, ids)
    kp, vp = (torch.empty(len(where), Hkv, page, D, dtype=kn.dtype) for _ in range(2))
    for b, j, pos, _ in where:
        kp[pos], vp[pos] = kn[b, :, j * page:(j + 1) * page], vn[b, :, j * page:(j + 1) * page]
    return kp, vp, live, tn, tf


def _put_pools(case, kp, vp, live, num_pages=NUM_PAGES, role="in"):
    for name, t in (("k", kp), ("v", vp)):
        case.put_at(name, t, case.layout.pages(name, num_pages, tuple(t.shape[1:]), t.element_size(), live), role)


def _saw_table(a, t):
    assert a.block_table == t["table"].data_ptr() and a.block_table_stride_b == t["table"].stride(0)
    assert a.num_pages == t["k"].shape[0]


# --- the decode and the forward over a cache (both take pfa_fa3_decode_args) -------------------------------------------------------------

def attention(entry, place, *, Sq, D, dtype, seed, lens=LENS, Smax=256, window=None, key_mask=False, tree=False, sinks=False, fp8=False,
              key_splits=None, table_kind=None, kv_axis=0, expect=None):
    """``ops.fa3_decode`` / ``ops.fa3_prefill_cache``.  place: "wide" / "narrow" (contiguous caches, far along ``kv_axis``), "pages" (a
    dense pool of 2^18 + 64 pages), "pool3" (three pages, a wide stride between them).  q and o are far along the batch.  ``expect``: what
    the kernel's name must contain ("_paged" with a table)."""
    B, page = len(lens), 64 * 128 // D
    fn = ops.fa3_decode if entry == "decode" else ops.fa3_prefill_cache
    q, k, v = _problem(B, Sq, Smax, D, dtype, seed)
    g = _gen(seed + 1)
    lens_t = _i32(lens)
    case = FarCase()
    dk = dv = None
    if fp8:
        dk, dv = (0.5 + torch.rand(B, HKV, generator=g) for _ in range(2))
        k8, v8 = ops.quantize_kv(k.float(), dk), ops.quantize_kv(v.float(), dv)
        k, v = ops.dequantize_kv(k8, dk, torch.float64), ops.dequantize_kv(v8, dv, torch.float64)      # what the reference attends over
        kn, vn = poisoned(k8, lens), poisoned(v8, lens)
    else:
        kn, vn = guard(k, v, lens, Sq, window)
    kind_q = "narrow" if place == "narrow" else "wide"
    case.put("q", q, kind_q)
    case.put("o", _out_like(q), kind_q, role="out")
    paging = place in ("pages", "pool3")
    if paging:
        lo = window_lo(lens, Sq, window)
        if place == "pages":
            kp, vp, live, tn, tf = paged(kn, vn, lens, page, seed, lo)
            _put_pools(case, kp, vp, live)
        else:
            kp, vp, live, tn, tf = paged(kn, vn, lens, page, seed, lo, ids=[0, 1, 2])
            case.put("k", kp, "wide")
            case.put("v", vp, "wide")
        if table_kind:
            case.put("table", tn, table_kind, far=tf)
        else:
            case.plain("table", tn, tf)
    else:
        case.put("k", kn, place, axis=kv_axis)
        case.put("v", vn, place, axis=kv_axis)
    km = words = snk = None
    if key_mask:
        km = torch.rand(B, Smax, generator=g) > 0.3
        case.put("key_mask", km, "wide")
    if tree:
        words = torch.randint(0, 2 ** Sq, (B, Sq), generator=g, dtype=torch.int64) | (1 << torch.arange(Sq))[None, :]
        case.put("words", words, "wide")
    if sinks:
        snk = torch.randn(H, generator=g)

    def call(t):
        dev = t["q"].device
        kw = dict(cache_seqlens=lens_t.to(dev), causal=True, return_lse=True, out=t["o"])
        if paging:
            kw["block_table"] = t["table"]
        for name, x in (("window", window), ("key_splits", key_splits)):
            if x is not None:
                kw[name] = x
        if key_mask:
            kw["key_mask"] = t["key_mask"]
        if tree:
            kw["tree_mask"] = t["words"]
        if sinks:
            kw["sinks"] = snk.to(dev)
        if fp8:
            kw.update(k_descale=dk.to(dev), v_descale=dv.to(dev))
        o, lse = fn(t["q"], t["k"], t["v"], **kw)
        assert o is t["o"]
        return {"lse": lse}

    def seen(blocks, t):
        a = blocks.of("PfaFa3DecodeArgs")
        for field, name in (("q", "q"), ("k_cache", "k"), ("v_cache", "v"), ("o", "o")):
            saw_view(a, field, t[name])
        if paging:
            _saw_table(a, t)
        if key_mask:
            assert a.key_mask == t["key_mask"].data_ptr() and a.key_mask_stride_b == t["key_mask"].stride(0)
        if tree:
            tm = blocks.of("PfaFa3TreeMask")
            assert tm.words == t["words"].data_ptr() and tm.stride_b == t["words"].stride(0)

    def describe(blocks):
        a, ext = blocks.of("PfaFa3DecodeArgs"), blocks.of("PfaFa3CacheExt")
        if entry == "decode":
            if tree:
                return _capi.describe_decode_tree(a, ext, blocks.of("PfaFa3TreeMask"))
            if fp8:
                return _capi.describe_decode_q8(a, ext, blocks.of("PfaFa3KvQuant"))
            if sinks:
                return _capi.describe_decode_sink(a, ext, blocks.of("PfaFa3Sinks"))
            return _capi.describe_decode_ex(a, ext)
        if key_splits is not None:
            return _capi.describe_prefill_split(a, key_splits)
        if fp8:
            return _capi.describe_prefill_q8(a, ext, blocks.of("PfaFa3KvQuant"))
        return _capi.describe_prefill_ex(a, ext)

    def check(near, ex):
        dev = near["q"].device
        kc, vc, L = k.to(dev), v.to(dev), lens_t.to(dev)
        kmd = None if km is None else km.to(dev)
        if tree:
            ref = folded_reference(dict(q=near["q"], B=B, Sq=Sq, Smax=Smax, lens=L, k=kc, v=vc), words.to(dev), kmd)
        else:
            ref = reference(near["q"], kc, vc, seqlens=L, key_mask=kmd, causal=True, window=window)
        if sinks:
            ref = with_sink(ref, snk)
        check_out(near["o"], ref[0], ref[2], float(vc.abs().max()), dtype, entry)
        check_lse(near["o"], ex["lse"], ref[1], entry)

    return Spec(case, call, seen, describe, check, expect if expect is not None else "_paged" if paging else "")


# --- the ragged forward over a cache ------------------------------------------------------------------------------------------------------

def prefill_varlen(rows, *, D, dtype, seed, q_lens, kv_lens, fp8=False):
    """``ops.fa3_prefill_varlen`` over a pool of pages.  rows "far": the packed q / o rows 2^22 + 8 elements apart (``ROW_LENS``);
    "near": rows H * D apart, in the arena all the same."""
    B, page, Smax = len(q_lens), 64 * 128 // D if not fp8 else 128, 256
    cu = _cu(q_lens)
    total = cu[-1]
    g = _gen(seed)
    q = torch.randn(total, H, D, generator=g).to(dtype)
    k, v = (torch.randn(B, HKV, Smax, D, generator=g).to(dtype) for _ in range(2))
    dk = dv = None
    if fp8:
        dk, dv = (0.5 + torch.rand(B, HKV, generator=g) for _ in range(2))
        k8, v8 = ops.quantize_kv(k.float(), dk), ops.quantize_kv(v.float(), dv)
        k, v = ops.dequantize_kv(k8, dk, torch.float64), ops.dequantize_kv(v8, dv, torch.float64)
        kn, vn = poisoned(k8, kv_lens), poisoned(v8, kv_lens)
    else:
        kn, vn = guard(k, v, kv_lens)
    case = FarCase()
    stride = ROW_STRIDE if rows == "far" else H * D
    for name, role in (("q", "in"), ("o", "out")):
        case.put_at(name, q, case.layout.rows(name, total, (H, D), (D, 1), 2, stride, range(total)), role)
    kp, vp, live, tn, tf = paged(kn, vn, kv_lens, page, seed)
    _put_pools(case, kp, vp, live)
    case.plain("table", tn, tf)
    lens_t, cu_t = _i32(kv_lens), _i32(cu)

    def call(t):
        dev = t["q"].device
        kw = dict(k_descale=dk.to(dev), v_descale=dv.to(dev)) if fp8 else {}
        o, lse = ops.fa3_prefill_varlen(t["q"], t["k"], t["v"], cu_seqlens_q=cu_t.to(dev), max_seqlen_q=max(q_lens), cache_seqlens=lens_t.to(dev),
                                        block_table=t["table"], causal=True, return_lse=True, out=t["o"], **kw)
        assert o is t["o"]
        return {"lse": lse}

    def seen(blocks, t):
        a = blocks.of("PfaFa3PrefillVarlenArgs")
        for field, name, axes in (("q", "q", "sh"), ("o", "o", "sh"), ("k_cache", "k", "bhs"), ("v_cache", "v", "bhs")):
            saw_view(a, field, t[name], axes)
        _saw_table(a, t)

    def describe(blocks):
        a = blocks.of("PfaFa3PrefillVarlenArgs")
        return _capi.describe_prefill_varlen_q8(a, None, blocks.of("PfaFa3KvQuant")) if fp8 else _capi.describe_prefill_varlen_ex(a, None)

    def check(near, ex):
        dev = near["q"].device
        for b in range(B):
            rows_b = slice(cu[b], cu[b + 1])
            qb, ob = (near[n][rows_b].permute(1, 0, 2)[None] for n in ("q", "o"))
            ref = reference(qb, k[b:b + 1].to(dev), v[b:b + 1].to(dev), seqlens=lens_t[b:b + 1].to(dev), causal=True)
            check_out(ob, ref[0], ref[2], float(v.abs().max()), dtype, f"sequence {b}")
            check_lse(ob, ex["lse"][None, :, rows_b], ref[1], f"sequence {b}")

    return Spec(case, call, seen, describe, check, "_paged")


# --- the appends ----------------------------------------------------------------------------------------------------------------------------

def append(entry, place, *, D, dtype, seed, q_lens=None, Sq=None, lens=LENS, fp8=False):
    """``ops.kv_append`` / ``ops.rope_append`` (with q, q_out and far rotary tables).  place "wide": the uniform call, new rows and the
    caches far along the batch; "pages": the ragged call into a pool, rows H * D apart; "rows": the ragged call, packed rows far."""
    B, page, Smax = len(lens), 64 * 128 // D, 256
    ragged = place != "wide"
    rope = entry == "rope"
    g = _gen(seed)
    cdt = FP8 if fp8 else dtype
    case = FarCase()
    if ragged:
        cu = _cu(q_lens)
        total = cu[-1]
        stride = ROW_STRIDE if place == "rows" else None
        new = {"k_new": torch.randn(total, HKV, D, generator=g).to(dtype), "v_new": torch.randn(total, HKV, D, generator=g).to(dtype)}
        if rope:
            new["q"] = torch.randn(total, H, D, generator=g).to(dtype)
        for name, t in new.items():
            case.put_at(name, t, case.layout.rows(name, total, tuple(t.shape[1:]), (D, 1), 2, stride or t.shape[1] * D, range(total)))
        if rope:
            case.put_at("q_out", new["q"], case.layout.rows("q_out", total, (H, D), (D, 1), 2, stride or H * D, range(total)), "out")
        # the destination pages: those the new rows fall into
        _, live, tn, tf = page_table(lens, page, Smax, seed, [max(0, n - r) for n, r in zip(lens, q_lens)])
        kp, vp = (torch.empty(len(live), HKV, page, D, dtype=cdt) for _ in range(2))
        _put_pools(case, kp, vp, live, role="out")
        case.plain("table", tn, tf)
    else:
        new = {"k_new": torch.randn(B, HKV, Sq, D, generator=g).to(dtype), "v_new": torch.randn(B, HKV, Sq, D, generator=g).to(dtype)}
        if rope:
            new["q"] = torch.randn(B, Sq, H, D, generator=g).to(dtype).permute(0, 2, 1, 3)
        for name, t in new.items():
            case.put(name, t, "wide")
        if rope:
            case.put("q_out", _out_like(new["q"]), "wide", role="out")
        for name in ("k", "v"):
            case.put(name, torch.empty(B, HKV, Smax, D, dtype=cdt), "wide", role="out")
    dk = dv = cos = sin = None
    if fp8:
        dk, dv = (0.5 + torch.rand(B, HKV, generator=g) for _ in range(2))
    if rope:                                             # fp32 tables, 300 positions 2^22 + 8 elements apart: position 255 lies 4 GiB out
        cos, sin = ops.rotary_tables(300, 64)
        for name, t in (("cos", cos), ("sin", sin)):
            case.put_at(name, t, case.layout.rows(name, 300, (32,), (1,), 4, ROW_STRIDE, range(300)))
    lens_t = _i32(lens)
    cu_t = _i32(cu) if ragged else None

    def kwargs(t, dev):
        kw = dict(cache_seqlens=lens_t.to(dev))
        if ragged:
            kw.update(cu_seqlens_q=cu_t.to(dev), max_seqlen_q=max(q_lens), block_table=t["table"])
        if fp8:
            kw.update(k_descale=dk.to(dev), v_descale=dv.to(dev))
        if rope:
            kw.update(rotary_cos=t["cos"], rotary_sin=t["sin"], q=t["q"], q_out=t["q_out"])
        return kw

    def call(t):
        dev = t["k_new"].device
        (ops.rope_append if rope else ops.kv_append)(t["k_new"], t["v_new"], t["k"], t["v"], **kwargs(t, dev))
        return {}

    block = "PfaRopeAppendArgs" if rope else "PfaKvAppendArgs"

    def seen(blocks, t):
        a = blocks.of(block)
        rows = "sh" if ragged else "bsh"
        for field, name, axes in (("k_new", "k_new", rows), ("v_new", "v_new", rows), ("k_cache", "k", "bhs"), ("v_cache", "v", "bhs")) + \
                ((("q", "q", rows), ("q_out", "q_out", rows)) if rope else ()):
            saw_view(a, field, t[name], axes)
        if ragged:
            _saw_table(a, t)
        if rope:
            assert a.cos == t["cos"].data_ptr() and a.sin == t["sin"].data_ptr() and a.cs_stride == t["cos"].stride(0)

    def describe(blocks):
        a = blocks.of(block)
        return _capi.describe_rope_append(a) if rope else _capi.describe_kv_append(a)

    def check(near, ex):
        """the near run against ``ops``' CPU model of the same call, bit for bit"""
        cpu = case.near_inputs(torch.device("cpu"))
        (ops.rope_append if rope else ops.kv_append)(cpu["k_new"], cpu["v_new"], cpu["k"], cpu["v"], **kwargs(cpu, "cpu"))
        for n in ("k", "v") + (("q_out",) if rope else ()):
            assert torch.equal(F.bits(near[n].cpu()), F.bits(cpu[n])), f"{n}: the near run is not the CPU model's"
        assert not bool((F.bits(cpu["k"]).view(torch.uint8) == F.FILL).all()), "nothing was appended"

    return Spec(case, call, seen, describe, check)


# --- the page copy and the merge -------------------------------------------------------------------------------------------------------------

def page_copy(*, D, dtype, seed):
    """``ops.page_copy`` inside a pool of 2^18 + 64 pages: two pairs whose ids lie past 2^17 and 2^18, the pair list's rows a wide stride
    apart, the second pair a partial page."""
    page = 64 * 128 // D
    g = _gen(seed)
    ids = sorted(page_ids(8))
    src, dst = [ids[3], ids[7]], [ids[6], ids[4]]                # sources and destinations on both sides of 2^17 and 2^18
    assert max(src + dst) > 2 ** 18 and min(src + dst) > 2 ** 16
    live = sorted(src + dst)
    kp, vp = (torch.randn(4, HKV, page, D, generator=g).to(dtype) for _ in range(2))
    case = FarCase()
    _put_pools(case, kp, vp, live, role="inout")
    pos = {pid: n for n, pid in enumerate(live)}
    pairs_far = _i32([[src[0], dst[0]], [src[1], dst[1]]])
    pairs_near = _i32([[pos[src[0]], pos[dst[0]]], [pos[src[1]], pos[dst[1]]]])
    case.put("pairs", pairs_near, "wide", far=pairs_far)
    rows = _i32([page, 37])

    def call(t):
        ops.page_copy(t["k"], t["v"], t["pairs"], rows=rows.to(t["k"].device))
        return {}

    def seen(blocks, t):
        a = blocks.of("PfaPageCopyArgs")
        saw_view(a, "k_pool", t["k"])
        saw_view(a, "v_pool", t["v"])
        assert a.pairs == t["pairs"].data_ptr() and a.pairs_stride == t["pairs"].stride(0) and a.num_pages == t["k"].shape[0]

    def check(near, ex):
        ck, cv = kp.clone(), vp.clone()
        ops.page_copy(ck, cv, pairs_near, rows=rows)
        assert torch.equal(F.bits(near["k"].cpu()), F.bits(ck)) and torch.equal(F.bits(near["v"].cpu()), F.bits(cv)), "not the CPU model's pools"
        assert not torch.equal(F.bits(ck), F.bits(kp)), "nothing was copied"

    return Spec(case, call, seen, lambda blocks: _capi.describe_page_copy(blocks.of("PfaPageCopyArgs")), check)


def merge(*, D, seed):
    """``ops.attn_merge`` of three fp32 parts with their LSEs into a bf16 output and an LSE: every part, every LSE and the output far
    along the batch (B 2: fp32 tensors take two indices)."""
    B, Sq, N = 2, 5, 3
    g = _gen(seed)
    case = FarCase()
    parts = [torch.randn(B, Sq, H, D, generator=g).permute(0, 2, 1, 3) for _ in range(N)]
    lses = [torch.randn(B, H, Sq, generator=g) * 3 for _ in range(N)]
    lses[1][0, 1, 2] = lses[2][1, 0, :] = float("-inf")
    for n in range(N):
        case.put(f"part{n}", parts[n], "wide")
        case.put(f"lse{n}", lses[n], "wide")
    case.put("o", _out_like(parts[0], BF), "wide", role="out")

    def call(t):
        o, lse = ops.attn_merge([t[f"part{n}"] for n in range(N)], [t[f"lse{n}"] for n in range(N)], out=t["o"], return_lse=True)
        assert o is t["o"]
        return {"lse": lse}

    def seen(blocks, t):
        a = blocks.of("PfaAttnMergeArgs")
        saw_view(a, "o", t["o"])
        for n in range(N):
            p, l = t[f"part{n}"], t[f"lse{n}"]
            assert a.o_part[n] == p.data_ptr() and (a.op_stride_b[n], a.op_stride_h[n], a.op_stride_s[n]) == p.stride()[:3]
            assert a.lse_part[n] == l.data_ptr() and (a.lp_stride_b[n], a.lp_stride_h[n], a.lp_stride_s[n]) == l.stride()

    def check(near, ex):
        """the bounds of tests/test_hip_attn_merge.py (``_check_merge``)"""
        ro, rl = merge_ref64(parts, lses)
        o, lse = near["o"].cpu().double(), ex["lse"].cpu().double()
        assert bool(torch.isfinite(o).all())
        bound = 1e-5 * torch.stack([p.double().abs() for p in parts]).max(dim=0).values + 2.0 ** -8 * ro.abs()
        assert bool(((o - ro).abs() <= bound).all()), float(((o - ro).abs() - bound).max())
        fin = torch.isfinite(rl)
        assert torch.equal(torch.isfinite(lse), fin) and bool(((lse - rl)[fin].abs() <= 4e-6 * rl[fin].abs().clamp_min(1.0)).all())

    return Spec(case, call, seen, lambda blocks: _capi.describe_attn_merge(blocks.of("PfaAttnMergeArgs")), check)


# --- the cases: name -> a function that builds the Spec on the host --------------------------------------------------------------------

CASES = {
    # fa3_decode, contiguous: k / v batch, k / v head, q and o batch; wide and narrow
    "decode-wide-batch": lambda: attention("decode", "wide", Sq=1, D=128, dtype=BF, seed=1),
    "decode-narrow-batch": lambda: attention("decode", "narrow", Sq=4, D=64, dtype=FP, seed=2, lens=LENS5),
    "decode-wide-head": lambda: attention("decode", "wide", Sq=4, D=128, dtype=BF, seed=3, kv_axis=1),
    # fa3_decode, paged: the dense pool with high ids; a wide page stride with 3 pages and a wide table row stride
    "decode-pages": lambda: attention("decode", "pages", Sq=1, D=64, dtype=FP, seed=4),
    "decode-pool3-wide-table": lambda: attention("decode", "pool3", Sq=4, D=128, dtype=BF, seed=5, lens=[65, 40], Smax=128, table_kind="wide"),
    # the decode's variants, one placement each
    "decode-splits-pages": lambda: attention("decode", "pages", Sq=1, D=128, dtype=BF, seed=6, lens=[500, 65, 130], Smax=512,
                                             expect="+combine_paged"),
    "decode-window-released-pages": lambda: attention("decode", "pages", Sq=1, D=128, dtype=BF, seed=7, window=70),
    "decode-key-mask-wide": lambda: attention("decode", "wide", Sq=1, D=64, dtype=FP, seed=8, lens=LENS2, key_mask=True),
    "decode-tree-wide": lambda: attention("decode", "wide", Sq=4, D=128, dtype=BF, seed=9, lens=LENS2, tree=True),
    "decode-sinks-pages": lambda: attention("decode", "pages", Sq=4, D=64, dtype=FP, seed=10, sinks=True),
    "decode-fp8-wide": lambda: attention("decode", "wide", Sq=1, D=128, dtype=BF, seed=11, lens=LENS2, fp8=True),
    # fa3_prefill_cache, its split form, FP8
    "prefill-pages": lambda: attention("prefill", "pages", Sq=96, D=128, dtype=BF, seed=12),
    "prefill-wide-batch": lambda: attention("prefill", "wide", Sq=96, D=64, dtype=FP, seed=13),
    "prefill-split-pages": lambda: attention("prefill", "pages", Sq=96, D=64, dtype=FP, seed=14, key_splits=2),
    "prefill-split-wide-batch": lambda: attention("prefill", "wide", Sq=96, D=128, dtype=BF, seed=15, key_splits=2),
    "prefill-fp8-wide": lambda: attention("prefill", "wide", Sq=96, D=64, dtype=FP, seed=16, lens=LENS2, fp8=True),
    # fa3_prefill_varlen (+ FP8): a pool of pages; packed q / o rows far
    "prefill-varlen-pages": lambda: prefill_varlen("near", D=128, dtype=BF, seed=17, q_lens=[96, 1, 33], kv_lens=LENS),
    "prefill-varlen-packed-rows": lambda: prefill_varlen("far", D=64, dtype=FP, seed=18, q_lens=ROW_LENS, kv_lens=[256, 255, 256, 256, 65, 130]),
    "prefill-varlen-fp8-packed-rows": lambda: prefill_varlen("far", D=128, dtype=BF, seed=19, q_lens=ROW_LENS, kv_lens=[256, 255, 256, 256, 65, 130],
                                                             fp8=True),
    # kv_append, the quantising append, rope_append
    "kv-append-pages": lambda: append("kv", "pages", D=128, dtype=BF, seed=20, q_lens=[96, 1, 33]),
    "kv-append-wide-batch": lambda: append("kv", "wide", D=64, dtype=FP, seed=21, Sq=4),
    "kv-append-packed-rows": lambda: append("kv", "rows", D=64, dtype=FP, seed=22, q_lens=ROW_LENS, lens=[256, 255, 256, 256, 65, 130]),
    "kv-append-fp8-wide-batch": lambda: append("kv", "wide", D=128, dtype=BF, seed=23, Sq=4, lens=LENS2, fp8=True),
    "rope-append-wide-batch": lambda: append("rope", "wide", D=128, dtype=BF, seed=24, Sq=4),
    "rope-append-pages": lambda: append("rope", "pages", D=64, dtype=FP, seed=25, q_lens=[96, 1, 33]),
    "rope-append-packed-rows": lambda: append("rope", "rows", D=128, dtype=BF, seed=26, q_lens=ROW_LENS, lens=[256, 255, 256, 256, 65, 130]),
    # page_copy, attn_merge
    "page-copy-pages": lambda: page_copy(D=128, dtype=BF, seed=27),
    "attn-merge-wide-batch": lambda: merge(D=128, seed=28),
}


@pytest.fixture(scope="module")
def arena():
    """The module's one arena.  Less than the arena plus 2 GiB free: the module skips, and says how much there was."""
    free = torch.cuda.mem_get_info()[0]
    if free < F.ARENA_BYTES + 2 * 2 ** 30:
        pytest.skip(f"{free / 2 ** 30:.1f} GiB of device memory free: the far-address tests need {F.ARENA_BYTES / 2 ** 30 + 2:.1f} GiB")
    torch.cuda.reset_peak_memory_stats()
    a = F.make_arena(torch.device("cuda:0"))
    yield a
    print(f"\ntests/test_hip_far_cache.py: peak device memory {torch.cuda.max_memory_allocated() / 2 ** 30:.3f} GiB")
    del a
    torch.cuda.empty_cache()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_far(name, arena):
    F.two_runs(arena, CASES[name]())

"""GPU tests of WHICH KEYS A ROW SEES in the calls over a KV cache -- ``ops.fa3_decode``, ``ops.fa3_prefill_cache`` (``key_splits``
None and 1 .. 8) and ``ops.fa3_prefill_varlen`` -- with the exact probes of tests/probe_testlib.py: ``count`` (every score 0, V of 0 and
1: the answer is a count of keys) and ``stair`` (integer scores in log2 units: every weight a power of two, the running maximum
jumps where the test puts it).  One key too many or too few in one row of 32768 is 30 x over the tolerance, and ``check_probe`` names
the row and, for a single key, the key.  The random-data tests of these calls (tests/kvcache_testlib.py's bounds) measure the
arithmetic; here the arithmetic is exact and the visibility is what is measured.

Every case runs contiguous and paged (``scatter``: pages of 64 and 128 keys in a random order, page 0 unnamed), with fp32 and 16-bit
outputs (the off-by-one test at 32768 keys: contiguous, fp32); bf16 / fp16 and D 64 / 128 are shared out over the cases.  Caches carry
``guard``'s NaN wherever a kernel promises not to read.
Each case takes its kernel's name, and the decode its split count, from ``_capi.describe*`` and asserts them; the lengths sit on both
sides of the split, tile and page boundaries that follow from that count (``edge_lens``)."""

from __future__ import annotations

import pytest
import torch

from kvcache_testlib import (INF, _paged, _with_nan, device, guard, i32, poisoned, quant, scatter, scatter_fp8, share_prefix_pages, window_lo)
from photonic_flash_attention_amd import _capi, ops
from probe_testlib import cache_visible, check_probe, count, expected, probe_v, stair, unseen_keys

pytestmark = pytest.mark.gpu

BF, FP, F32 = torch.bfloat16, torch.float16, torch.float32
# (page size or None, fp32 output?) of the three calls a case makes per probe
VARIANTS = {"count": ((None, True), (64, False), (128, True)), "stair": ((None, False), (64, True), (128, False))}
PROBES = ("count", "stair")


def roundup(x, m):
    return -(-x // m) * m


def decode_splits(B, H, Hkv, Sq, Smax, window=None):
    """The documented plan of ``pfa_fa3_decode`` (include/pfa_hip.h): 512 workgroups over B * Hkv * ceil(Sq * H / Hkv / 16) row blocks,
    at least 256 keys of the (windowed) span a split, at most 128 splits."""
    base = B * Hkv * -(-Sq * (H // Hkv) // 16)
    keys = Smax if window is None else min(Smax, roundup(window + Sq - 1, 64))
    return max(1, min(-(-512 // base), max(1, keys // 256), 128))


def edge_lens(Smax, ns):
    """Eight lengths around the boundaries of a decode of ``ns`` splits: split b of a length covers ``c = roundup(ceil(len / ns), 64)``
    keys from ``b * c``.  ``ns * 64 * t`` fills every split with t tiles, one key more moves c up and empties the last splits, one key
    fewer shortens the last split; ``(ns - 1) * c + 1`` leaves the last split one key; 128 and 129 are a page of 128 and one key more."""
    unit, c = ns * 64, roundup(-(-Smax // ns), 64)
    return [unit - 1, unit, 2 * unit - 1, 2 * unit, 3 * unit + 1, (ns - 1) * c + 1, 129, 128]


def _name(fn, q, k, v, *, out_dtype, table=None, window=None, tree=False, fp8=False, sinks=False, key_splits=None, causal=True):
    """(kernel name, split count or None) of the call, from ``_capi.describe*`` on the call's own argument block."""
    decode = fn is ops.fa3_decode
    a = ops._cache_call_args("pfa_fa3_decode" if decode else "pfa_fa3_prefill", q, k, v, causal, None, out_dtype, None, table, fp8)[0]
    a.workspace, a.workspace_bytes = 0x1000, 1 << 40
    ext = None if window is None else _capi.make_cache_ext(window=window)
    quant_ = _capi.make_kv_quant(k_descale=0x7000, v_descale=0x7400) if fp8 else None
    snk = _capi.make_sinks(sinks=0x9000) if sinks else None
    if decode:
        if tree:
            r = _capi.describe_decode_tree(a, ext, _capi.make_tree_mask(words=0x7000, stride_b=q.shape[2]))
        elif fp8:
            r = _capi.describe_decode_q8(a, ext, quant_)
        else:
            r = _capi.describe_decode_sink(a, ext, snk)
        return r[0], r[2]
    if key_splits is not None:
        r = _capi.describe_prefill_split_sink(a, 0 if key_splits == "auto" else key_splits, snk)
        return r[0], r[2]
    if fp8:
        return _capi.describe_prefill_q8(a, ext, quant_)[0], None
    return _capi.describe_prefill_sink(a, ext, snk)[0], None


def _want_name(fn, dtype, D, o32, *, paged, window=None, tree=False, fp8=False, sinks=False, nsplit=1, causal=True):
    dt, o = ("bf16" if dtype == BF else "fp16"), ("o32" if o32 else "o16")
    if fn is ops.fa3_decode:
        return (f"fa3_decode_{dt}_d{D}_{o}{'_tree' if tree else '_win' if window else ''}{'_kv8' if fp8 else ''}{'_sink' if sinks else ''}"
                f"{'+combine' if nsplit > 1 else ''}{'_paged' if paged else ''}")
    return (f"fa3_prefill_{dt}_d{D}_{o}{'_causal' if causal else ''}{'_win' if window else ''}{'_kv8' if fp8 else ''}{'_sink' if sinks else ''}"
            f"{f'_split{nsplit}+merge' if nsplit > 1 else ''}{'_paged' if paged else ''}")


def _problem(kind, B, H, Hkv, Sq, S, D, dtype, vis, steps, shared=None):
    """The probe's operands on the CPU: (pr, v).  shared: P, the keys every sequence has from sequence 0."""
    pr = count(B, H, Hkv, Sq, S, D, dtype) if kind == "count" else stair(B, H, Hkv, Sq, S, D, dtype, steps)
    v = probe_v(B, Hkv, S, D, dtype, unseen_keys(vis, Hkv))
    if shared:
        v[:, :, :shared] = v[:1, :, :shared]
        pr["k"][:, :, :shared] = pr["k"][:1, :, :shared]
        if pr["steps"] is not None:
            pr["steps"][:, :, :shared] = pr["steps"][:1, :, :shared]
    return pr, v


def run_case(fn, what, *, B, H, Hkv, Sq, S, D, dtype, lens, steps, window=None, key_mask=None, tree=None, sinks=None, fp8=None,
             key_splits=None, causal=True, nsplit=None, merged=False, probes=PROBES, variants=None):
    """Both probes through ``fn`` in the three variants: guard, (scatter,) call, ``check_probe``; the kernel's name and split count
    asserted.  fp8: (k_descale, v_descale) as CPU tensors.  nsplit: the split count the case expects (decode: the plan's; prefill: the
    resolved ``key_splits``)."""
    dev = device()
    vis = cache_visible(B, H, Sq, S, lens, causal=causal, window=window, key_mask=key_mask, tree=tree)
    kw = {}
    if key_mask is not None:
        kw["key_mask"] = key_mask.to(dev)
    if tree is not None:
        kw["tree_mask"] = tree.to(dev)
    if sinks is not None:
        kw["sinks"] = sinks.to(dev)
    if key_splits is not None:
        kw["key_splits"] = key_splits
    if window is not None:
        kw["window"] = window
    for kind in probes:
        pr, v = _problem(kind, B, H, Hkv, Sq, S, D, dtype, vis, steps)
        exp = expected(vis, v, pr["steps"], sinks, None if fp8 is None else fp8[1])
        q = pr["q"].to(dev)
        for page, o32 in (variants or VARIANTS[kind]):
            odt = F32 if o32 else dtype
            tag = f"{what} {kind} {'contiguous' if page is None else f'page {page}'} {'o32' if o32 else 'o16'}"
            if fp8 is None:
                kn, vn = guard(pr["k"].to(dev), v.to(dev), lens, Sq, window)
                table = None
                if page is not None:
                    kn, vn, table = scatter(kn, vn, page, seed=page + Sq, first=1, lo=window_lo(lens, Sq, window) if window else None)
            else:
                ones = torch.ones_like(fp8[0])
                k8, v8 = quant(pr["k"].float(), ones).to(dev), quant(v.float(), ones).to(dev)
                kw["k_descale"], kw["v_descale"] = fp8[0].to(dev), fp8[1].to(dev)
                kn, vn, table = poisoned(k8, lens), poisoned(v8, lens), None
                if page is not None:
                    kn, vn, table = scatter_fp8(k8, v8, page, page + Sq, lens)
            name, ns = _name(fn, q, kn, vn, out_dtype=odt, table=table, window=window, tree=tree is not None, fp8=fp8 is not None,
                             sinks=sinks is not None, key_splits=key_splits, causal=causal)
            want_ns = nsplit if nsplit is not None else 1
            assert name == _want_name(fn, dtype, D, o32, paged=page is not None, window=window, tree=tree is not None, fp8=fp8 is not None,
                                      sinks=sinks is not None, nsplit=want_ns, causal=causal), name
            assert ns is None or ns == want_ns, (name, ns, want_ns)
            o, lse = fn(q, kn, vn, cache_seqlens=i32(lens), block_table=table, causal=causal, softmax_scale=pr["scale"], out_dtype=odt,
                        return_lse=True, **kw)
            torch.cuda.synchronize()
            check_probe(o, lse, exp, odt, tag, kind == "count", merged=merged)


# --- 1. decode: the splits ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [32768, 32513, 24577, 127 * 64 + 1])
def test_decode_128_splits(n):
    """B 1, H 8 / Hkv 1, one 32768-key cache: 128 splits of 256 keys.  32513 leaves the last split one key, 24577 = 128 * 192 + 1 moves
    c from 192 to 256 (the last 32 splits empty), 8129 = 127 * 64 + 1 leaves split 127 one key of one tile a split.  A span of 8
    keeps 2^8 * 2^15 < 2^24; steps in the first, a middle and the last split, the newest key and the first key of a split."""
    ns = decode_splits(1, 8, 1, 1, 32768)
    c = roundup(-(-n // ns), 64)
    steps = {3: 2, (n // c // 2) * c: 5, n - 1: 8, (n - 1) // c * c: 7}
    assert ns == 128
    run_case(ops.fa3_decode, f"decode 128 splits len {n}", B=1, H=8, Hkv=1, Sq=1, S=32768, D=128, dtype=BF, lens=[n], steps=steps, nsplit=ns,
             variants=None if n == 32768 else ((None, True), (128, False)))


def test_one_key_too_many_or_too_few_is_seen_and_named_at_32768_keys():
    """The probes against the kernel's own noise: the decode is handed a length one above and one below the 32767 keys the expectation
    is for.  ``count`` names the key and the direction; ``stair`` (the extra key weighs 2^-8 of the newest) is over the tolerance."""
    B, H, Hkv, Sq, S, D, n = 1, 8, 1, 1, 32768, 128, 32767
    dev = device()
    vis = cache_visible(B, H, Sq, S, [n])
    for kind in PROBES:
        pr, v = _problem(kind, B, H, Hkv, Sq, S, D, BF, vis, {3: 2, n - 1: 8})
        exp = expected(vis, v, pr["steps"])
        for given, blame in ((n, None), (n + 1, f"32767 keys expected, 32768 found .* key {n} is extra"),
                             (n - 1, f"32767 keys expected, 32766 found .* key {n - 1} is missing")):
            kn, vn = guard(pr["k"].to(dev), v.to(dev), [given], Sq)
            name, ns = _name(ops.fa3_decode, pr["q"].to(dev), kn, vn, out_dtype=F32)
            assert name == _want_name(ops.fa3_decode, BF, D, True, paged=False, nsplit=128) and ns == decode_splits(B, H, Hkv, Sq, S) == 128
            o, lse = ops.fa3_decode(pr["q"].to(dev), kn, vn, cache_seqlens=i32([given]), softmax_scale=pr["scale"], out_dtype=F32, return_lse=True)
            torch.cuda.synchronize()
            if blame is None:
                check_probe(o, lse, exp, F32, f"decode 32767 keys {kind} o32", kind == "count")
                continue
            with pytest.raises(AssertionError, match=blame if kind == "count" else "over the tolerance"):
                check_probe(o, lse, exp, F32, f"decode handed {given} keys {kind}", kind == "count")


@pytest.mark.parametrize("which", ["issue", "edges", "every256"])
def test_decode_16_splits_ragged_lengths(which):
    """B 8, H 8 / Hkv 1 over 4096 keys: 16 splits; every sequence its own length, on both sides of the split, tile and page edges.
    ``every256``: the 16 multiples of 256 keys, the split size of a full cache, and one key more."""
    ns = decode_splits(8, 8, 1, 1, 4096)
    assert ns == 16
    lens = {"issue": [4096, 4095, 4033, 4032, 2049, 1025, 65, 0], "edges": edge_lens(4096, ns),
            "every256": [256 * s + d for s in range(1, 17) for d in (0, 1)][:-1]}[which]     # 31 sequences: 512 / 31 is still above 16
    B = len(lens)
    assert decode_splits(B, 8, 1, 1, 4096) == ns
    steps = []
    for n in lens:
        c = max(64, roundup(-(-n // ns), 64))
        steps.append({j: h for j, h in ((0, 3), (n - 2, 1), (min(c, n - 1), 6), (n // 2, 11), (n - 1, 9)) if 0 <= j < n})
    run_case(ops.fa3_decode, f"decode 16 splits {which}", B=B, H=8, Hkv=1, Sq=1, S=4096, D=64, dtype=FP, lens=lens, steps=steps, nsplit=ns)


@pytest.mark.parametrize("Sq,lens", [(5, [1000, 517, 4]), (2, [1, 300, 1024]), (8, [5, 1024, 65]), (64, [40, 1024, 64])],
                         ids=["sq5-35rows", "sq2", "sq8", "sq64"])
def test_decode_row_blocks_and_rows_that_see_nothing(Sq, lens):
    """H 28 / Hkv 4: G 7, so Sq 5 is 35 rows in 3 row blocks of 16, the last partial.  A length below Sq leaves rows without a key."""
    ns = decode_splits(3, 28, 4, Sq, 1024)
    steps = [{j: h for j, h in ((0, 2), (n - 1, 9), (max(n - Sq, 0), 4), (n // 2, 12)) if 0 <= j < n} for n in lens]
    run_case(ops.fa3_decode, f"decode rows Sq {Sq}", B=3, H=28, Hkv=4, Sq=Sq, S=1024, D=128 if Sq != 8 else 64, dtype=FP if Sq == 5 else BF,
             lens=lens, steps=steps, nsplit=ns)
    assert min(lens) < Sq


# --- 2. decode: the modes -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W", [1, 64, 65, 96, 5000])
def test_decode_window(W):
    """lo_b = len - Sq - W + 1 at a tile edge (len = 640 + Sq + W - 1), one past it, inside a page of 128, and a window wider than the
    sequence.  The step on lo's own key is seen by row 0 alone; the 12 on the key below it by nobody."""
    B, H, Hkv, Sq, S, D = 4, 8, 2, 3, 2048, 64
    lens = [min(S, 640 + Sq + W - 1), min(S, 641 + Sq + W - 1), min(S, 700 + Sq + W - 1), 50]
    steps = []
    for n in lens:
        lo = max(0, n - Sq - W + 1)
        steps.append({j: h for j, h in ((lo, 2), (lo - 1, 12), (n - 1, 9), (n - 2, 4), (lo + 1, 5)) if 0 <= j < n})
    run_case(ops.fa3_decode, f"decode window {W}", B=B, H=H, Hkv=Hkv, Sq=Sq, S=S, D=D, dtype=BF if W % 2 else FP, lens=lens, steps=steps,
             window=W, nsplit=decode_splits(B, H, Hkv, Sq, S, W))


@pytest.mark.parametrize("Sq", [8, 64])
def test_decode_tree_mask(Sq):
    """Random words, the chain, all ones, an empty word with and without a prefix, bit 63 alone."""
    B, H, Hkv, S, D = 5, 8, 2, 1024, 128 if Sq == 8 else 64
    lens = [1000, 517, Sq, Sq + 70, 900]
    g = torch.Generator().manual_seed(40 + Sq)
    words = torch.randint(-2 ** 63, 2 ** 63 - 1, (B, Sq), generator=g, dtype=torch.int64)
    words[1] = torch.tensor([(1 << (i + 1)) - 1 if i < 63 else -1 for i in range(Sq)])
    words[2] = -1
    words[2, 1] = 0                                                   # empty, no prefix: the row sees nothing
    words[3, 2] = 0                                                   # empty behind a prefix of 70 keys
    words[4, 0] = -2 ** 63                                            # bit 63: key off + 63 if Sq is 64, else nothing of the step
    steps = [{j: h for j, h in ((n - 1, 9), (n - Sq, 5), (max(n - Sq - 1, 0), 3), (n - Sq // 2, 12)) if 0 <= j < n} for n in lens]
    run_case(ops.fa3_decode, f"decode tree Sq {Sq}", B=B, H=H, Hkv=Hkv, Sq=Sq, S=S, D=D, dtype=BF if Sq == 8 else FP, lens=lens, steps=steps,
             tree=words, nsplit=decode_splits(B, H, Hkv, Sq, S))


def test_decode_key_mask():
    """A hole, left padding, a fully hidden batch, a random mask."""
    B, H, Hkv, Sq, S, D = 4, 8, 2, 2, 1024, 128
    lens = [1000, 1024, 600, 777]
    km = torch.ones(B, S, dtype=torch.bool)
    km[0, 300:431] = False
    km[1, :257] = False
    km[2] = False
    km[3] = torch.rand(S, generator=torch.Generator().manual_seed(5)) > 0.4
    steps = [{299: 4, 300: 13, 431: 9, 999: 2}, {256: 13, 257: 9, 1023: 6}, {5: 9}, {776: 9, 400: 5}]
    run_case(ops.fa3_decode, "decode key mask", B=B, H=H, Hkv=Hkv, Sq=Sq, S=S, D=D, dtype=BF, lens=lens, steps=steps, key_mask=km,
             nsplit=decode_splits(B, H, Hkv, Sq, S))


@pytest.mark.parametrize("S,W", [(256, None), (4096, None), (2048, 96), (4096, 700)], ids=["1split", "splits", "window", "window-splits"])
def test_decode_sinks(S, W):
    """0.0 on some heads and -inf on others; one split and many; a sequence of length 0, whose rows are O = 0, LSE = sink."""
    B, H, Hkv, Sq, D = 3, 8, 2, 2, 64
    lens = [S, 0, S // 2 + 1]
    sinks = torch.tensor([0.0, -INF, 0.0, 0.0, -INF, -INF, 0.0, -INF])
    ns = decode_splits(B, H, Hkv, Sq, S, W)
    assert (ns > 1) == (S == 4096)
    steps = [{j: h for j, h in ((n - 1, 6), (n // 2, 9), (1, 3), (n - 2, -2)) if 0 <= j < n} for n in lens]
    run_case(ops.fa3_decode, f"decode sinks S {S} W {W}", B=B, H=H, Hkv=Hkv, Sq=Sq, S=S, D=D, dtype=FP if W else BF, lens=lens, steps=steps,
             window=W, sinks=sinks, nsplit=ns)


@pytest.mark.parametrize("per_batch", [False, True], ids=["per-head", "per-batch"])
def test_decode_fp8(per_batch):
    """k_descale 1 and v_descale 0.5 / 0.25 / 2: powers of two, so the dequantised V and the result stay exact."""
    B, H, Hkv, Sq, S, D = 3, 8, 2, 2, 2048, 128 if per_batch else 64
    lens = [2048, 1025, 64]
    vd = torch.tensor([[0.5, 0.25], [2.0, 0.5], [0.5, 1.0]]) if per_batch else torch.tensor([0.5, 0.25])
    steps = [{j: h for j, h in ((n - 1, 9), (n // 2, 12), (1, 3)) if 0 <= j < n} for n in lens]
    run_case(ops.fa3_decode, f"decode fp8 {'per-batch' if per_batch else 'per-head'}", B=B, H=H, Hkv=Hkv, Sq=Sq, S=S, D=D,
             dtype=BF if per_batch else FP, lens=lens, steps=steps, fp8=(torch.ones_like(vd), vd), nsplit=decode_splits(B, H, Hkv, Sq, S))


def _assert_prefix_step_kernels(q, kk, vv, tb, P, dtype, splits):
    """The two attention passes ``shared_prefix`` makes (``ops._shared_prefix_step``), on the argument blocks it builds: all rows as one
    sequence over sequence 0's first P keys (the decode up to 64 rows, else the prefill with ``prefix_key_splits``), and each sequence
    over its own keys from P on; both with an fp32 store.  Name and split count of each, by ``describe``."""
    B, H, Sq, D = q.shape
    Hkv, rows, page = kk.shape[1], B * Sq, None if tb is None else kk.shape[2]
    q_all = q.transpose(1, 2).reshape(1, rows, H, D).transpose(1, 2)
    pre = (kk[:1, :, :P], vv[:1, :, :P], None) if tb is None else (kk, vv, tb[:1, :P // page])
    own = (kk[:, :, P:], vv[:, :, P:], None) if tb is None else (kk, vv, tb[:, P // page:])
    S_own = own[0].shape[2] if tb is None else own[2].shape[1] * page
    fn = ops.fa3_decode if rows <= 64 else ops.fa3_prefill_cache
    want = decode_splits(1, H, Hkv, rows, P) if rows <= 64 else (splits or 1)
    name, ns = _name(fn, q_all, pre[0], pre[1], out_dtype=F32, table=pre[2], causal=False, key_splits=None if rows <= 64 else splits)
    assert name == _want_name(fn, dtype, D, True, paged=tb is not None, nsplit=want, causal=False) and ns in (None, want), (name, ns)
    want = decode_splits(B, H, Hkv, Sq, S_own)
    name, ns = _name(ops.fa3_decode, q, own[0], own[1], out_dtype=F32, table=own[2])
    assert name == _want_name(ops.fa3_decode, dtype, D, True, paged=tb is not None, nsplit=want) and ns == want, (name, ns)


@pytest.mark.parametrize("Sq", [5, 20], ids=["20rows-decode", "80rows-prefill"])
def test_decode_shared_prefix(Sq):
    """P 128 (two pages of 64, one of 128): the prefix pass is the decode up to 64 rows and the prefill (``prefix_key_splits`` 2 and
    None) past them, and ``attn_merge`` joins it with the own-keys pass: the merged tolerance, and the integer check all the same."""
    B, H, Hkv, S, D, P = 4, 8, 2, 384, 64 if Sq == 5 else 128, 128
    dtype = BF if Sq == 5 else FP
    lens = [P + n for n in (Sq, 130, 200, 77)]
    dev = device()
    vis = cache_visible(B, H, Sq, S, lens)
    steps = [{j: h for j, h in ((n - 1, 9), (P - 1, 5), (P, 12), (3, 2), (n - Sq, 4)) if 0 <= j < n} for n in lens]
    steps = [{**s, **{j: h for j, h in steps[0].items() if j < P}} for s in steps]
    sl = torch.tensor(lens, dtype=torch.int32)
    for kind in PROBES:
        pr, v = _problem(kind, B, H, Hkv, Sq, S, D, dtype, vis, steps, shared=P)
        exp = expected(vis, v, pr["steps"])
        q = pr["q"].to(dev)
        kc, vc = _with_nan(pr["k"].to(dev), sl, P), _with_nan(v.to(dev), sl, P)
        perm = torch.randperm(P // 64 + B * ((S - P) // 64) + 3, generator=torch.Generator().manual_seed(Sq)).tolist()
        kp, table = _paged(kc, sl, P, perm)
        vp, _ = _paged(vc, sl, P, perm)
        kp2, vp2, table2 = scatter(kc, vc, 128, seed=Sq, first=1)          # pages of 128: the prefix page held once, sequence 0's
        for b in range(1, B):
            share_prefix_pages(kp2, vp2, table2, 0, b, P // 128)
        for (kk, vv, tb), o32 in (((kc, vc, None), kind == "count"), ((kp, vp, table), kind != "count"), ((kp2, vp2, table2), kind == "count")):
            odt = F32 if o32 else dtype
            splits = 2 if Sq == 20 and tb is None else None
            _assert_prefix_step_kernels(q, kk, vv, tb, P, dtype, splits)
            o, lse = ops.fa3_decode(q, kk, vv, cache_seqlens=sl.to(dev), block_table=tb, shared_prefix=P, softmax_scale=pr["scale"],
                                    out_dtype=odt, return_lse=True, **({} if splits is None else dict(prefix_key_splits=splits)))
            torch.cuda.synchronize()
            check_probe(o, lse, exp, odt, f"decode shared prefix Sq {Sq} {kind} {'contiguous' if tb is None else f'page {kk.shape[2]}'} "
                        f"{'o32' if o32 else 'o16'}", kind == "count", merged=True)


# --- 3. prefill -------------------------------------------------------------------------------------------------------------------------

def _prefill_steps(lens, Sq):
    """The kernel moves a row's running maximum only on a jump above 8 and otherwise keeps the stale one.  Even sequences: 9 on a late
    key every row sees (the rescale branch), 11 in the rows' own keys (2 more: deferred; seen by the rows behind it only), 6 on the
    newest key, 1 on the first row's diagonal key.  Odd sequences: a jump of exactly 8 (deferred), then 11 (the rescale), 3 on the
    newest key."""
    out = []
    for b, n in enumerate(lens):
        marks = ((max(n - Sq - 70, 0), 9), (n - Sq // 2 - 1, 11), (n - 1, 6), (n - Sq, 1)) if b % 2 == 0 else \
            ((max(n - Sq - 70, 0), 8), (n - Sq // 2 - 1, 11), (n - 1, 3))
        out.append({j: h for j, h in marks if 0 <= j < n})
    return out


@pytest.mark.parametrize("Sq,S", [(300, 1024), (300, 4096), (1, 1024)], ids=["sq300-1024", "sq300-4096", "sq1"])
def test_prefill_row_blocks(Sq, S):
    """Sq 300: a block of 256 rows and one of 44.  The second sequence is shorter than Sq: its first rows see nothing."""
    B, H, Hkv, D = 2, 4, 2, 128 if S == 1024 else 64
    lens = [S - 37, 250 if Sq == 300 else 0]
    run_case(ops.fa3_prefill_cache, f"prefill Sq {Sq} S {S}", B=B, H=H, Hkv=Hkv, Sq=Sq, S=S, D=D, dtype=BF if S == 1024 else FP, lens=lens,
             steps=_prefill_steps(lens, Sq))


@pytest.mark.parametrize("N", [1, 2, 3, 4, 5, 6, 7, 8])
def test_prefill_key_splits(N):
    """Sq 70 over 1024 keys: 16 tiles, ``per = ceil(16 / N)``; N 7 gives per 3 and leaves the last split empty, N 5 and 6 too.  The
    second sequence ends one key behind a split boundary of N 2, 4 and 8 (513 = 8 tiles + 1)."""
    B, H, Hkv, Sq, S, D = 2, 4, 2, 70, 1024, 64 if N % 2 else 128
    lens = [1024, 513]
    steps = [{1: 3, 200: 9, 1023: 6, 1024 - 36: 12, 512: 5, 511: 2}, {1: 3, 200: 9, 512: 6, 511: 2, 480: 12}]
    run_case(ops.fa3_prefill_cache, f"prefill key_splits {N}", B=B, H=H, Hkv=Hkv, Sq=Sq, S=S, D=D, dtype=BF if N % 2 else FP, lens=lens,
             steps=steps, key_splits=N, nsplit=N, merged=N > 1, sinks=torch.tensor([0.0, -INF, -INF, 0.0]) if N in (3, 7, 8) else None)


def test_prefill_key_splits_auto_resolves_like_the_plan():
    B, H, Hkv, Sq, S, D = 1, 4, 2, 70, 4096, 128
    q = torch.zeros(B, H, Sq, D, dtype=BF, device=device())
    k = torch.zeros(B, Hkv, S, D, dtype=BF, device=device())
    ns = _name(ops.fa3_prefill_cache, q, k, k, out_dtype=BF, key_splits=0)[1]
    assert ns == min(8, S // 1024, 512 // (B * H))
    lens = [4096 - 63]
    run_case(ops.fa3_prefill_cache, "prefill key_splits auto", B=B, H=H, Hkv=Hkv, Sq=Sq, S=S, D=D, dtype=BF, lens=lens, steps=_prefill_steps(lens, Sq),
             key_splits="auto", nsplit=ns, merged=True)


@pytest.mark.parametrize("W", [1, 64, 65, 96, 5000])
def test_prefill_window(W):
    B, H, Hkv, Sq, S, D = 3, 4, 2, 130, 2048, 128
    lens = [min(S, 640 + Sq + W - 1), min(S, 641 + Sq + W - 1), 100]
    steps = []
    for n in lens:
        lo = max(0, n - Sq - W + 1)
        steps.append({j: h for j, h in ((lo, 2), (lo - 1, 12), (n - 1, 9), (n - Sq, 4), (lo + 1, 5)) if 0 <= j < n})
    run_case(ops.fa3_prefill_cache, f"prefill window {W}", B=B, H=H, Hkv=Hkv, Sq=Sq, S=S, D=D, dtype=FP if W % 2 else BF, lens=lens, steps=steps,
             window=W, sinks=torch.tensor([0.0, -INF, 0.0, -INF]) if W in (65, 5000) else None)


def test_prefill_sinks_and_fp8():
    B, H, Hkv, Sq, S, D = 3, 4, 2, 70, 1024, 64
    lens = [1000, 30, 0]
    run_case(ops.fa3_prefill_cache, "prefill sinks", B=B, H=H, Hkv=Hkv, Sq=Sq, S=S, D=D, dtype=FP, lens=lens, steps=_prefill_steps(lens, Sq),
             sinks=torch.tensor([0.0, -INF, -INF, 0.0]))
    run_case(ops.fa3_prefill_cache, "prefill sinks full", B=B, H=H, Hkv=Hkv, Sq=Sq, S=S, D=D, dtype=FP, lens=lens, steps=_prefill_steps(lens, Sq),
             sinks=torch.tensor([0.0, -INF, -INF, 0.0]), causal=False, variants=((None, True), (64, False)))
    vd = torch.tensor([[0.5, 0.25], [2.0, 0.5], [0.5, 1.0]])
    run_case(ops.fa3_prefill_cache, "prefill fp8", B=B, H=H, Hkv=Hkv, Sq=Sq, S=S, D=128, dtype=BF, lens=lens, steps=_prefill_steps(lens, Sq),
             fp8=(torch.ones_like(vd), vd))


# --- 4. the ragged prefill --------------------------------------------------------------------------------------------------------------

Q_ROWS = [1, 0, 33, 300, 64]
KV_LENS = [700, 50, 33, 1024, 40]                      # the last sequence is shorter than its rows


@pytest.mark.parametrize("mode", ["plain", "window", "sinks", "fp8", "capped"])
def test_prefill_varlen(mode):
    """q rows 1, 0, 33, 300 and 64 with their own cache lengths; ``capped``: ``max_seqlen_q`` 256 computes the first 256 rows of the 300
    as a sequence of 256 rows and writes none of the others."""
    H, Hkv, S, D = 4, 2, 1024, 128 if mode in ("plain", "fp8") else 64
    dtype = BF if mode in ("plain", "sinks") else FP
    dev = device()
    B = len(Q_ROWS)
    W = 96 if mode == "window" else None
    cap = 256 if mode == "capped" else max(Q_ROWS)
    rows = [min(n, cap) for n in Q_ROWS]
    sinks = torch.tensor([0.0, -INF, -INF, 0.0]) if mode == "sinks" else None
    vd = torch.tensor([0.5, 0.25]) if mode == "fp8" else None
    cu = [0]
    for n in Q_ROWS:
        cu.append(cu[-1] + n)
    vis = [cache_visible(1, H, max(n, 1), S, [KV_LENS[b]], window=W) for b, n in enumerate(rows)]
    unseen = torch.cat([unseen_keys(vb, Hkv) if rows[b] else torch.ones(1, Hkv, S, dtype=torch.bool) for b, vb in enumerate(vis)])
    steps = []
    for n, sq in zip(KV_LENS, rows):
        lo = max(0, n - sq - (W or n) + 1)
        steps.append({j: h for j, h in ((lo, 2), (lo - 1, 13), (n - 1, 9), (n - sq, 4), (n // 2, 5)) if 0 <= j < n})
    for kind in PROBES:
        pr = count(B, H, Hkv, 1, S, D, dtype) if kind == "count" else stair(B, H, Hkv, 1, S, D, dtype, steps)
        v = probe_v(B, Hkv, S, D, dtype, unseen)
        q = torch.zeros(cu[-1], H, D, dtype=dtype)
        q[..., 0] = 0.0 if kind == "count" else 1.0
        for page, o32 in VARIANTS[kind]:
            odt = F32 if o32 else dtype
            kw = {}
            if mode == "fp8":
                ones = torch.ones_like(vd)
                k8, v8 = quant(pr["k"].float(), ones).to(dev), quant(v.float(), ones).to(dev)
                kn, vn, table = (poisoned(k8, KV_LENS), poisoned(v8, KV_LENS), None) if page is None else scatter_fp8(k8, v8, page, 7, KV_LENS)
                kw = dict(k_descale=ones.to(dev), v_descale=vd.to(dev))
            else:
                kn, vn = guard(pr["k"].to(dev), v.to(dev), KV_LENS, rows, W)
                table = None
                if page is not None:
                    kn, vn, table = scatter(kn, vn, page, seed=9, first=1, lo=window_lo(KV_LENS, rows, W) if W else None)
            a = _capi.make_prefill_varlen_args(B=B, H=H, Hkv=Hkv, total_q=cu[-1], max_seqlen_q=cap, Smax=S, D=D, dtype_in=0 if dtype == BF else 1,
                                               dtype_out=2 if o32 else (0 if dtype == BF else 1), causal=1, softmax_scale=1.0, q=0x1000, o=0x2000,
                                               cu_seqlens_q=0x3000, q_stride_s=H * D, q_stride_h=D, o_stride_s=H * D, o_stride_h=D)
            ops._set_view(a, "k_cache", kn)
            ops._set_view(a, "v_cache", vn)
            ops._set_block_table(a, table, 0 if table is None else kn.shape[2], 0 if table is None else kn.shape[0])
            ext = None if W is None else _capi.make_cache_ext(window=W)
            name = (_capi.describe_prefill_varlen_q8(a, ext, _capi.make_kv_quant(k_descale=0x7000, v_descale=0x7400)) if mode == "fp8" else
                    _capi.describe_prefill_varlen_sink(a, ext, _capi.make_sinks(sinks=0x9000) if sinks is not None else None))[0]
            assert name == (f"fa3_prefill_{'bf16' if dtype == BF else 'fp16'}_d{D}_{'o32' if o32 else 'o16'}_causal{'_win' if W else ''}"
                            f"{'_kv8' if mode == 'fp8' else ''}{'_sink' if sinks is not None else ''}_varlen{'_paged' if page else ''}"), name
            out = torch.full((cu[-1], H, D), 7.0, dtype=odt, device=dev)
            if W is not None:
                kw["window"] = W
            if sinks is not None:
                kw["sinks"] = sinks.to(dev)
            o, lse = ops.fa3_prefill_varlen(q.to(dev), kn, vn, cu_seqlens_q=i32(cu), max_seqlen_q=cap, cache_seqlens=i32(KV_LENS), block_table=table,
                                            softmax_scale=pr["scale"], out_dtype=odt, return_lse=True, out=out, **kw)
            torch.cuda.synchronize()
            for b, n in enumerate(rows):
                if n == 0:
                    continue
                exp = expected(vis[b], v[b:b + 1], None if pr["steps"] is None else pr["steps"][b:b + 1], sinks, None if vd is None else vd)
                check_probe(o[cu[b]:cu[b] + n].permute(1, 0, 2)[None], lse[None, :, cu[b]:cu[b] + n], exp, odt,
                            f"varlen {mode} {kind} {'contiguous' if page is None else f'page {page}'} {'o32' if o32 else 'o16'} sequence {b}", kind == "count")
                assert bool((o[cu[b] + n:cu[b + 1]] == 7.0).all()), f"sequence {b}: a row past max_seqlen_q was written"

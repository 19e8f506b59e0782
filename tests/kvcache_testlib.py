"""What the KV-cache tests share.  Plain functions and constants; pytest collects nothing from here, and tests/test_kvcache_testlib.py
tests it on the CPU, the runner with a stand-in kernel.  A new mode's GPU tests are its cases and its own assertions around these:

  ``reference`` / ``check_out`` / ``check_lse``     the fp64 attention, the bound on O, the rule for the LSE (below); ``merge_ref64``
  ``with_sink`` / ``tree_visible`` / ``folded_reference``   the reference of a call with sinks, and of a tree step (rows folded into the batch)
  ``problem`` / ``gen`` / ``i32`` / ``device``      device draws of q, k, v; small tensors
  ``guard(k, v, lens, sqs, window)``                the one NaN rule: copies with NaN wherever a kernel promises not to read (``window_lo``)
  ``scatter`` / ``share_prefix_pages``              caches over pools in a random page order (page 0 unnamed, pages released below a window),
                                                    a prefix held once; ``contiguous_of`` gathers a ``PagedKVCache`` back
  ``run_and_check(call, q, k, v, lens, ...)``       guard, call, synchronise, fp64 reference (``with_ref`` makes it the mode's), dtype, bounds
  ``both(call, q, kn, vn, kp, vp, table, ...)``     contiguous call == paged call, bit for bit and finite
  ``seq_rows`` / ``ragged_equals_uniform``          ragged call == per-sequence uniform calls, bit for bit
  ``capture(step)`` / ``check_against_cache``       warm-up and graph capture; a replay over a ``PagedKVCache`` against fp64
  ``FP8, NANB, b8, quant, dequant, to16, poisoned, scatter_fp8``     the same small change for e4m3 caches, as bytes
  ``prefix_problem`` / ``check_step`` / ``both_prefix_caches``       the shared-prefix step

Every helper that runs a kernel takes the attention function as its first argument and its device from the tensors.

The reference is fp64 attention of ``q [B,H,Sq,D]`` over ``k/v [B,Hkv,Smax,D]`` with the bottom-right causal rule per batch: with
``off_b = len_b - Sq``, row i sees key j iff ``j < len_b``, ``j <= i + off_b`` (causal), ``j > i + off_b - W`` (window) and the key mask
allows it.  It is computed from CLEAN caches: the NaN a test puts where a kernel must not read goes to the kernel only.

The bounds: ``|err| <= eps |ref| + 3 eps max|v| ||p_row||_2 + 2e-6`` per element of a 16-bit output (eps 2^-9 bf16, 2^-11 fp16: the
bound of the fast variant in tests/test_hip_parity.py's docstring), 1e-3 max-abs for an fp32 output, 2e-3 on the LSE with exact
agreement on which rows are -inf, and O exactly zero on those rows.  Every output must be finite.

These bounds measure the arithmetic.  WHICH KEYS a row sees they measure poorly: one wrong key among n random ones moves O by about
``|v| / n`` and the LSE by about ``1 / n``, below every bound above at a few thousand keys.  Visibility -- lengths, the causal diagonal,
windows, tree words, masks, split, tile and page edges, sinks, the shared-prefix cut -- is checked by the exact probes of
tests/probe_testlib.py (tests/test_hip_cache_probes.py), on inputs whose answer is a count of keys.  WHERE a kernel reads and writes once
index times stride passes 2^31 and 2^32 is tests/far_testlib.py's (tests/test_hip_far_cache.py, tests/test_hip_far_dense.py)."""

from __future__ import annotations

import functools

import torch

from capi_testlib import built_lib  # noqa: F401  (kept here for the users of this module)

EPS = {torch.bfloat16: 2.0 ** -9, torch.float16: 2.0 ** -11}
INF, NAN = float("inf"), float("nan")


def device():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def i32(x, dev=None):
    return torch.tensor(x, dtype=torch.int32, device=device() if dev is None else dev)


# --- the fp64 reference and the bounds -----------------------------------------------------------------------------------------------

def reference(q, k, v, *, seqlens=None, key_mask=None, causal=True, window=None, scale=None):
    """fp64 on q's device: q [B,H,Sq,D], k/v [B,Hkv,Smax,D] -> (o, lse, ||p_row||_2).  A row that sees no key has o = 0, lse = -inf."""
    assert window is None or causal, "a window is defined against the causal diagonal"
    B, H, Sq, D = q.shape
    Hkv, Smax = k.shape[1], k.shape[2]
    g = H // Hkv
    kd = k.double().repeat_interleave(g, dim=1)
    vd = v.double().repeat_interleave(g, dim=1)
    s = (q.double() @ kd.transpose(-1, -2)) * (D ** -0.5 if scale is None else scale)        # [B,H,Sq,Smax]
    j = torch.arange(Smax, device=q.device)
    i = torch.arange(Sq, device=q.device)
    L = seqlens.to(q.device).long() if seqlens is not None else torch.full((B,), Smax, device=q.device)
    vis = (j[None, None, :] < L[:, None, None]).expand(B, Sq, Smax)
    if causal:
        diag = L[:, None, None] - Sq + i[None, :, None]                                       # i + off_b: bottom-right, per batch
        vis = vis & (j[None, None, :] <= diag)
        if window is not None:
            vis = vis & (j[None, None, :] > diag - window)
    if key_mask is not None:
        vis = vis & key_mask.to(q.device).bool()[:, None, :]
    s = s.masked_fill(~vis[:, None], -INF)
    m = s.amax(-1, keepdim=True)
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    p = torch.exp(s - m)
    l = p.sum(-1, keepdim=True)
    safe = torch.where(l > 0, l, torch.ones_like(l))
    pn = p / safe
    o = pn @ vd
    lse = torch.where(l > 0, m + torch.log(safe), torch.full_like(l, -INF))[..., 0]
    return o, lse, pn.norm(dim=-1, keepdim=True)


def check_out(got, ref, pnorm, vmax, dtype, what=""):
    """``got`` against the reference's ``o``: finite, and within the bound of ``dtype`` (the input dtype) or 1e-3 if ``got`` is fp32."""
    tag = f"{what}: " if what else ""
    assert bool(torch.isfinite(got).all()), f"{tag}non-finite output -- a key or a page the call must never read was read"
    err = (got.double() - ref).abs()
    if got.dtype == torch.float32:
        print(f"{tag}max-abs {float(err.max()):.3e} (fp32, bound 1e-3)")
        assert float(err.max()) <= 1e-3, (what, float(err.max()))
        return
    eps = EPS[dtype]
    bound = eps * ref.abs() + 3 * eps * vmax * pnorm + 2e-6
    worst = float((err - bound).max())
    print(f"{tag}max-abs {float(err.max()):.3e}, closest to the bound {worst:.3e}")
    assert worst <= 0, f"{tag}max-abs {float(err.max()):.3e}, over the bound by {worst:.3e}"


def check_lse(o, lse, rlse, what=""):
    """``lse`` against the reference's: -inf on exactly the reference's rows (and ``o`` zero there), within 2e-3 on the others."""
    tag = f"{what}: " if what else ""
    fin = torch.isfinite(rlse)
    assert torch.equal(torch.isfinite(lse), fin), f"{tag}the rows with a finite LSE are not the reference's"
    assert not bool(torch.isnan(lse).any()), f"{tag}NaN in the LSE"
    assert bool((lse[~fin] == -INF).all()), f"{tag}a row with no visible key has an LSE other than -inf"
    assert bool((o[~fin[..., None].expand_as(o)] == 0).all()), f"{tag}a row with no visible key is not exactly zero"
    if bool(fin.any()):
        d = float((lse.double() - rlse)[fin].abs().max())
        print(f"{tag}LSE max-abs {d:.3e}")
        assert d <= 2e-3, (what, d)


def merge_ref64(outs, lses):
    """The merge rule of partial attention results in fp64, for LSEs that are finite or -inf -> (O, LSE)."""
    L = torch.stack([l.double() for l in lses])
    m = L.max(dim=0).values
    w = torch.exp(L - torch.where(m == -INF, torch.zeros_like(m), m))
    s = w.sum(dim=0)
    o = sum(torch.where(w[n][..., None] > 0, w[n][..., None] * outs[n].double(), torch.zeros_like(outs[n], dtype=torch.float64))
            for n in range(len(outs)))
    o = torch.where(s[..., None] > 0, o / s[..., None].clamp_min(1e-300), torch.zeros_like(o))
    return o, torch.where(s > 0, m + torch.log(s), torch.full_like(m, -INF))


# --- the references of two modes: attention sinks (tests/test_hip_attn_sinks.py) and the tree step (tests/test_hip_decode_tree.py) ------

def with_sink(ref, sinks):
    """``reference()``'s ``(o [B,H,Sq,D], lse [B,H,Sq], pnorm [B,H,Sq,1])`` and ``sinks [H]`` -> the same three with the sink, in fp64."""
    o, lse, pn = ref
    s = sinks.to(lse.device).double().view(1, -1, 1).expand_as(lse)
    dead = torch.isneginf(lse)
    w = torch.where(torch.isneginf(s), torch.ones_like(lse), torch.sigmoid(lse - s))
    w = torch.where(dead, torch.zeros_like(w), w)
    lse2 = torch.where(dead, s, torch.logaddexp(lse, s))
    return o * w[..., None], lse2, pn * w[..., None]


def tree_visible(words, lens, Sq, Smax):
    """The rule of the specification, from the words: bool [B, Sq, Smax]."""
    j = torch.arange(Smax, device=words.device)
    L = lens.long()
    rel = j[None, :] - (L - Sq)[:, None]                                     # j - off_b, [B, Smax]
    bit = ((words[:, :, None] >> rel.clamp(0, 63)[:, None, :]) & 1).bool()   # an arithmetic shift: the bit asked for is still bit 0
    return (j[None, None, :] < L[:, None, None]) & ((rel < 0)[:, None, :] | bit)


def folded_reference(pr, words, key_mask=None):
    """fp64 reference of the tree step, the rows folded into the batch -> (o [B,H,Sq,D], lse [B,H,Sq], pnorm [B,H,Sq,1])."""
    q, B, Sq, Smax = pr["q"], pr["B"], pr["Sq"], pr["Smax"]
    H, D = q.shape[1], q.shape[3]
    vis = tree_visible(words, pr["lens"], Sq, Smax)
    if key_mask is not None:
        vis = vis & key_mask.bool()[:, None, :]
    qf = q.permute(0, 2, 1, 3).reshape(B * Sq, H, 1, D)
    o, lse, pn = reference(qf, pr["k"].repeat_interleave(Sq, dim=0), pr["v"].repeat_interleave(Sq, dim=0),
                           seqlens=pr["lens"].repeat_interleave(Sq), key_mask=vis.reshape(B * Sq, Smax), causal=False)
    unfold = lambda t, last: t.reshape(B, Sq, H, last).permute(0, 2, 1, 3)
    return unfold(o, D), lse.reshape(B, Sq, H).permute(0, 2, 1), unfold(pn, 1)


# --- caches and pools ----------------------------------------------------------------------------------------------------------------

def gen(seed):
    return torch.Generator(device=device()).manual_seed(seed)


def problem(B, H, Hkv, Sq, Smax, D, dtype, seed):
    """q as a [B,H,Sq,D] view of a [B,Sq,H,D] buffer and contiguous k, v [B,Hkv,Smax,D], drawn on the device from one generator."""
    g = gen(seed)
    dev = device()
    q = torch.randn(B, Sq, H, D, generator=g, device=dev).to(dtype).permute(0, 2, 1, 3)
    k = torch.randn(B, Hkv, Smax, D, generator=g, device=dev).to(dtype)
    v = torch.randn(B, Hkv, Smax, D, generator=g, device=dev).to(dtype)
    return q, k, v


def window_lo(lens, sqs, window):
    """Per sequence the first key a window lets any row see, ``max(0, len_b - Sq_b - W + 1)`` (0 without a window).  sqs: an int or a list."""
    if window is None:
        return [0] * len(lens)
    return [max(0, n - (sqs if isinstance(sqs, int) else sqs[b]) - window + 1) for b, n in enumerate(lens)]


def guard(k, v, lens, sqs=None, window=None):
    """Copies of the caches with NaN wherever the kernels promise not to read: at and past ``len_b`` (what an unfilled tail may hold) and,
    under a window, below ``floor64(max(0, len_b - Sq_b - W + 1))``.  sqs: the row count, or one per sequence; needed with a window only."""
    kn, vn = k.clone(), v.clone()
    for b, (n, lo) in enumerate(zip(lens, window_lo(lens, sqs, window))):
        for t in (kn, vn):
            t[b, :, n:] = NAN
            t[b, :, :lo // 64 * 64] = NAN
    return kn, vn


def scatter(k, v, page, seed, layout="phsd", spare=5, first=0, lo=None):
    """Scatter contiguous [B, Hkv, Smax, D] caches over pools in a random page order.  -> (k_pool, v_pool, table) with the pools as
    [num_pages, Hkv, page, D] views; pages no table entry names hold NaN (and so does whatever NaN the caches carry).  first: the first
    page a table may name (1 leaves page 0, where a clamped -1 lands, unnamed).  lo: per sequence the first key that is read
    (``window_lo``); the table entries below ``lo_b // page`` become -1 and their pages NaN."""
    B, Hkv, Smax, D = k.shape
    assert Smax % page == 0
    pages = Smax // page
    NP = first + B * pages + spare
    dev = k.device
    perm = torch.randperm(NP - first, generator=torch.Generator().manual_seed(seed))[:B * pages] + first
    table = perm.to(torch.int32).reshape(B, pages).to(dev)
    pools = []
    for src in (k, v):
        if layout == "phsd":        # flash-attn style [num_pages, page, Hkv, D], passed transposed
            pool = torch.full((NP, page, Hkv, D), NAN, dtype=k.dtype, device=dev).transpose(1, 2)
        elif layout == "hpsd":
            pool = torch.full((NP, Hkv, page, D), NAN, dtype=k.dtype, device=dev)
        else:                       # every second page of a larger pool, whose pages also have room for 64 more keys
            pool = torch.full((2 * NP, Hkv, page + 64, D), NAN, dtype=k.dtype, device=dev)[::2, :, :page]
        pool[perm.to(dev)] = src.reshape(B, Hkv, pages, page, D).permute(0, 2, 1, 3, 4).reshape(B * pages, Hkv, page, D)
        pools.append(pool)
    for b, n in enumerate(lo or ()):
        dead = table[b, :n // page].long()
        table[b, :n // page] = -1
        for pool in pools:
            pool[dead] = NAN
    return pools[0], pools[1], table


def share_prefix_pages(kp, vp, table, src, dst, n_pages):
    """Sequence ``dst`` names ``src``'s first ``n_pages`` pages from now on -- a prefix held once -- and its own copies turn to NaN."""
    freed = table[dst, :n_pages].clone()
    table[dst, :n_pages] = table[src, :n_pages]
    for pool in (kp, vp):
        pool[freed.long()] = NAN


def contiguous_of(cache, Smax):
    """A PagedKVCache's sequences gathered into contiguous [max_batch, Hkv, Smax, D] K and V (zeros past each length)."""
    B = cache.max_batch
    k = torch.zeros(B, cache.Hkv, Smax, cache.D, dtype=cache.k_pool.dtype, device=cache.device)
    v = torch.zeros_like(k)
    for s in range(B):
        gk, gv = cache.gather(s)
        k[s, :, :gk.shape[1]] = gk
        v[s, :, :gv.shape[1]] = gv
    return k, v


def capture(step):
    """``step()`` once on a side stream (allocator warm-up), then captured -> (graph, what the captured call returned)."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = step()
    return graph, res


# --- run, synchronise, check: what a mode's GPU tests are made of ---------------------------------------------------------------------
# Every helper takes the attention function as ``call`` and its device from the tensors, so the CPU tests drive them with a stand-in.

def _sync(t):
    if t.is_cuda:
        torch.cuda.synchronize()


def run_and_check(call, q, k, v, lens, *, causal=True, window=None, key_mask=None, out_dtype=None, ref=None, sqs=None, guarded=True,
                  with_ref=None, what="", **kw):
    """``call`` on the guarded caches against fp64 on the clean ones -> (o, lse).  lens: a list, an int32 tensor or None (the whole cache;
    then nothing is guarded).  guarded=False hands the clean caches over.  ref: ``reference(...)``'s triple if the caller has it; with_ref
    turns it into the mode's own (``with_sink``).  sqs: the rows of each sequence where q's shape does not say (a ragged call)."""
    sl = lens if lens is None or torch.is_tensor(lens) else i32(list(lens), q.device)
    kn, vn = (k, v) if lens is None or not guarded else guard(k, v, sl.tolist(), q.shape[2] if sqs is None else sqs, window)
    opt = {n: x for n, x in (("window", window), ("key_mask", key_mask), ("out_dtype", out_dtype)) if x is not None}
    o, lse = call(q, kn, vn, cache_seqlens=sl, causal=causal, return_lse=True, **opt, **kw)
    _sync(o)
    if ref is None:
        ref = reference(q, k, v, seqlens=sl, key_mask=key_mask, causal=causal, window=window)
    ref = tuple(t.to(o.device) for t in (ref if with_ref is None else with_ref(ref)))
    assert o.dtype == (out_dtype or q.dtype), f"{what}: the output is {o.dtype}"
    check_out(o, ref[0], ref[2], float(v.abs().max()), q.dtype, what)
    check_lse(o, lse, ref[1], what)
    return o, lse


def both(call, q, kn, vn, kp, vp, table, **kw):
    """The contiguous and the paged call: both finite, O and LSE bit-equal -> the paged (o, lse)."""
    kw.setdefault("return_lse", True)
    oc, lc = call(q, kn, vn, **kw)
    op, lp = call(q, kp, vp, block_table=table, **kw)
    _sync(op)
    assert bool(torch.isfinite(op).all()) and bool(torch.isfinite(oc).all()), "a key or a page the call must never read was read"
    assert torch.equal(op, oc), f"O differs: max-abs {float((op.double() - oc.double()).abs().max()):.3e}"
    assert torch.equal(lp, lc), "LSE differs"
    return op, lp


def seq_rows(t, cu, b):
    """Sequence b's rows of a packed [total, H, D] tensor as the uniform call's [1, H, Sq_b, D] view."""
    return t[cu[b]:cu[b + 1]].permute(1, 0, 2)[None]


def ragged_equals_uniform(uniform_call, o, lse, q, kn, vn, cu, kv_lens, **kw):
    """The ragged result ``o [total,H,D]``, ``lse [H,total]`` against ``uniform_call`` per sequence with rows, on that sequence's rows,
    cache and length: the uniform result is finite and O and LSE are bit-equal."""
    for b in range(len(cu) - 1):
        if cu[b + 1] == cu[b]:
            continue
        ou, lu = uniform_call(seq_rows(q, cu, b), kn[b:b + 1], vn[b:b + 1], cache_seqlens=i32(list(kv_lens[b:b + 1]), q.device),
                              return_lse=True, **kw)
        _sync(ou)
        assert bool(torch.isfinite(ou).all()), f"sequence {b}: non-finite output of the per-sequence call"
        got = seq_rows(o, cu, b)
        assert torch.equal(got, ou), f"sequence {b}: O differs, max-abs {float((got.double() - ou.double()).abs().max()):.3e}"
        assert torch.equal(lse[None, :, cu[b]:cu[b + 1]], lu), f"sequence {b}: LSE differs from the per-sequence call"


def check_against_cache(cache, q, o, lse, Smax, what="", **ref_kw):
    """A result over a ``PagedKVCache`` (after a replay, say) against fp64 on the cache's sequences gathered as they are now."""
    kc, vc = contiguous_of(cache, Smax)
    ref = reference(q, kc, vc, seqlens=cache.cache_seqlens, **ref_kw)
    check_out(o, ref[0], ref[2], float(vc.abs().max()), q.dtype, what)
    check_lse(o, lse, ref[1], what)


# --- FP8 (e4m3fn) caches: bytes, made on the CPU and moved as bytes ---------------------------------------------------------------------

FP8 = torch.float8_e4m3fn
NANB = 0x7f                       # a NaN byte


def b8(x):
    return x.view(torch.uint8)


def quant(x, d):
    """``ops.quantize_kv`` on the CPU -> the FP8 tensor on x's device."""
    from photonic_flash_attention_amd import ops
    return ops.quantize_kv(x.detach().cpu().float(), d.cpu()).to(x.device)


def dequant(x8, d, dtype):
    from photonic_flash_attention_amd import ops
    return ops.dequantize_kv(x8.cpu(), d.cpu(), dtype).to(x8.device)


def to16(x8, dtype):
    """``x8.to(dtype)`` through the CPU, strides kept: every e4m3 value is a value of dtype, a NaN byte a NaN."""
    out = torch.empty_strided(x8.shape, x8.stride(), dtype=dtype, device=x8.device)
    out.copy_(x8.cpu().float().to(dtype))
    return out


def poisoned(x8, lens):
    """A copy with NaN bytes at and past each sequence's length: ``guard`` for an FP8 cache."""
    y = b8(x8).clone()
    for b, n in enumerate(lens):
        y[b, :, n:] = NANB
    return y.view(FP8)


def scatter_fp8(k8, v8, page, seed, lens, layout="phsd"):
    """``scatter`` of FP8 caches (through fp16 carriers of the bytes): pools in a random page order whose unnamed pages are NaN bytes,
    page 0 among them, and the table entries behind each length name page 0."""
    kp, vp, table = scatter(b8(k8).to(torch.float16), b8(v8).to(torch.float16), page, seed, layout)
    spare = next(p for p in range(kp.shape[0]) if p not in set(table.flatten().tolist()))
    if bool((table == 0).any()):                                                # move page 0's keys to a spare page: page 0 becomes NaN
        for pool in (kp, vp):
            pool[spare] = pool[0]
            pool[0] = NAN
        table[table == 0] = spare
    for b, n in enumerate(lens):
        table[b, -(-n // page):] = 0
    out = []
    for pool in (kp, vp):
        raw = torch.empty_strided(pool.shape, pool.stride(), dtype=torch.uint8, device=pool.device)
        raw.copy_(torch.nan_to_num(pool, nan=float(NANB)))
        out.append(raw.view(FP8))
    assert bool((b8(out[0])[0] == NANB).all())
    return out[0], out[1], table


# --- the shared-prefix step (tests/test_hip_attn_merge.py, tests/test_hip_prefill_split.py) -----------------------------------------

PREFIX_PAGE = 64


def _with_nan(kl, lens, P):
    """The contiguous cache of the logical one: NaN behind every length and over every prefix copy but sequence 0's."""
    kc = kl.clone()
    for b, n in enumerate(lens.tolist()):
        kc[b, :, n:] = NAN
        if b:
            kc[b, :, :P] = NAN
    return kc


def _paged(kc, lens, P, perm):
    """Pool and table of the contiguous cache ``kc`` (NaN tails included): the prefix pages named once, by every sequence; NaN in the
    pages nobody names; the table entries past a sequence's last page name one of those."""
    Bc, Hkv, Smax, D = kc.shape
    n_pre, per = P // PREFIX_PAGE, (Smax - P) // PREFIX_PAGE
    pool = torch.full((len(perm), Hkv, PREFIX_PAGE, D), NAN, dtype=kc.dtype, device=kc.device)
    table = torch.empty(Bc, n_pre + per, dtype=torch.int32)
    for jp in range(n_pre):
        pool[perm[jp]] = kc[0, :, jp * PREFIX_PAGE:(jp + 1) * PREFIX_PAGE]
        table[:, jp] = perm[jp]
    for b, n in enumerate(lens.tolist()):
        for jp in range(per):
            pid = perm[n_pre + b * per + jp]
            if P + jp * PREFIX_PAGE < n:
                pool[pid] = kc[b, :, P + jp * PREFIX_PAGE:P + (jp + 1) * PREFIX_PAGE]
                table[b, n_pre + jp] = pid
            else:
                table[b, n_pre + jp] = perm[-1]                                # never read: a page of NaN
    return pool, table.to(kc.device)


@functools.lru_cache(maxsize=None)
def prefix_problem(Bc, Sq, D, private, Smax, dtype, causal=True, P=128, Hq=8, Hkv=2):
    """One shared-prefix step and its fp64 reference, built once: q, the logical caches (every sequence's first P keys are sequence
    0's), the lengths P + private, the contiguous caches with NaN, the pools with their table."""
    g = torch.Generator().manual_seed(Bc * 1000 + Sq * 10 + D + sum(private))
    dev = device()
    q = torch.randn(Bc, Sq, Hq, D, generator=g).to(dev, dtype).permute(0, 2, 1, 3)
    kl, vl = (torch.randn(Bc, Hkv, Smax, D, generator=g).to(dev, dtype) for _ in range(2))
    kl[:, :, :P], vl[:, :, :P] = kl[:1, :, :P], vl[:1, :, :P]
    lens = torch.tensor([P + n for n in private], dtype=torch.int32, device=dev)
    assert all(n >= Sq for n in private) and P + max(private) <= Smax            # the caller's promise: every row lies behind the prefix
    n_pages = P // PREFIX_PAGE + Bc * ((Smax - P) // PREFIX_PAGE) + 3
    perm = torch.randperm(n_pages, generator=g).tolist()
    kc, vc = _with_nan(kl, lens, P), _with_nan(vl, lens, P)
    kp, table = _paged(kc, lens, P, perm)
    vp, _ = _paged(vc, lens, P, perm)
    return dict(q=q, kl=kl, vl=vl, lens=lens, kc=kc, vc=vc, kp=kp, vp=vp, table=table, P=P, causal=causal, dtype=dtype,
                ref=reference(q, kl, vl, seqlens=lens, causal=causal), vmax=float(vl.abs().max()))


def check_step(o, lse, ref, dtype, vmax, what):
    """A shared-prefix step against ``ref = reference(...)``: every row lies behind the prefix, so every LSE is finite."""
    check_out(o, ref[0], ref[2], vmax, dtype, what)
    assert bool(torch.isfinite(lse).all()), f"{what}: a non-finite LSE"
    check_lse(o, lse, ref[1], what)


def both_prefix_caches(fn, pr, what, **kw):
    """``fn`` with shared_prefix on the contiguous and on the paged cache: each within the bound, the two bit-equal -> (o, lse)."""
    o_c, lse_c = fn(pr["q"], pr["kc"], pr["vc"], cache_seqlens=pr["lens"], causal=pr["causal"], shared_prefix=pr["P"], return_lse=True, **kw)
    o_p, lse_p = fn(pr["q"], pr["kp"], pr["vp"], cache_seqlens=pr["lens"], block_table=pr["table"], causal=pr["causal"],
                    shared_prefix=pr["P"], return_lse=True, **kw)
    torch.cuda.synchronize()
    assert o_c.dtype == pr["dtype"] and o_c.shape == pr["q"].shape and lse_c.shape == pr["q"].shape[:3]
    check_step(o_c, lse_c, pr["ref"], pr["dtype"], pr["vmax"], what + " contiguous")
    check_step(o_p, lse_p, pr["ref"], pr["dtype"], pr["vmax"], what + " paged")
    assert torch.equal(o_c, o_p) and torch.equal(lse_c, lse_p)
    return o_c, lse_c

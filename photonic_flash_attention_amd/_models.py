"""The executable specifications of the native calls, in plain torch: what the entry points of ``ops`` run on CPU tensors and what the
host tests compare against.  Nothing here launches a kernel or touches the native library; ``ops`` imports every name below."""

from __future__ import annotations

import torch

FP8 = torch.float8_e4m3fn           # the element type of an FP8 KV cache: OCP e4m3fn (max finite 448, 0x7f / 0xff NaN, no infinities)
FP8_MAX = 448.0


def _descale_like(x: torch.Tensor, descale: torch.Tensor) -> torch.Tensor:
    """``descale`` ``[Hkv]`` or ``[B, Hkv]`` (fp32) shaped to broadcast over ``x`` ``[B, Hkv, S, D]`` (pools: ``[num_pages, Hkv, page, D]``)."""
    if not isinstance(descale, torch.Tensor) or descale.dtype != torch.float32 or descale.dim() not in (1, 2):
        raise ValueError("a descale must be an fp32 tensor [Hkv] or [B, Hkv]")
    if x.dim() != 4 or descale.shape[-1] != x.shape[1] or (descale.dim() == 2 and descale.shape[0] != x.shape[0]):
        raise ValueError(f"descale {tuple(descale.shape)} does not match a [B, Hkv, S, D] tensor of shape {tuple(x.shape)}")
    return descale[..., None, None]


def quantize_kv(x: torch.Tensor, descale: torch.Tensor) -> torch.Tensor:
    """``x`` ``[B, Hkv, S, D]`` (any floating dtype) as the FP8 cache holds it: ``e4m3fn(clamp(float(x) / descale, -448, 448))``, descale
    fp32 ``[Hkv]`` or ``[B, Hkv]`` -- the rule of ``kv_append`` into an FP8 cache, in plain torch (a first prompt's K / V, the tests).
    The division is fp32, the cast rounds to nearest even, NaN stays NaN; without the clamp the cast would turn 500.0 into NaN."""
    d = _descale_like(x, descale)
    return (x.to(torch.float32) / d).clamp(-FP8_MAX, FP8_MAX).to(FP8)


def dequantize_kv(x8: torch.Tensor, descale: torch.Tensor, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """The values an FP8 cache ``x8`` ``[B, Hkv, S, D]`` stands for, ``e4m3(x8) * descale``, as ``dtype``: computed in fp64 for
    ``torch.float64`` (exact: what a reference takes), else in fp32 and rounded once."""
    if x8.dtype != FP8:
        raise ValueError("dequantize_kv takes a torch.float8_e4m3fn tensor")
    d = _descale_like(x8, descale)
    w = torch.float64 if dtype == torch.float64 else torch.float32
    return (x8.to(torch.float32).to(w) * d.to(w)).to(dtype)


def _kv_append_model(k_new, v_new, k_cache, v_cache, lens, cu, max_seqlen_q, block_table) -> None:
    """``pfa_kv_append``'s rule in plain torch, every clamp and drop included: the executable specification, and what ``kv_append``
    runs on CPU tensors.  ``lens`` / ``cu`` are host lists; k_new ``[total, Hkv, D]`` with ``cu``, else ``[B, Hkv, Sq, D]``."""
    paged = block_table is not None
    Smax = block_table.shape[1] * k_cache.shape[2] if paged else k_cache.shape[2]
    page_size, num_pages, total = k_cache.shape[2], k_cache.shape[0], k_new.shape[0]
    for b, n in enumerate(lens):
        len_b = min(max(n, 0), Smax)
        if cu is not None:
            s_b = min(max(cu[b], 0), total)
            e_b = min(max(cu[b + 1], s_b), total)
            sq = min(e_b - s_b, max_seqlen_q)
            rows = [t[s_b:s_b + sq] for t in (k_new, v_new)]                 # [Sq_b, Hkv, D]
        else:
            sq = max_seqlen_q
            rows = [t[b].transpose(0, 1) for t in (k_new, v_new)]
        first = max(0, sq - len_b)                                            # rows in front of key 0 are dropped
        if first >= sq:
            continue
        pos = torch.arange(len_b - sq + first, len_b)
        rows = [r[first:sq] for r in rows]
        if not paged:
            for cache, r in zip((k_cache, v_cache), rows):
                cache[b][:, pos] = r.transpose(0, 1)
            continue
        pg = block_table[b, pos // page_size].to(torch.int64)
        ok = (pg >= 0) & (pg < num_pages)                                     # a page id outside the pool drops the write
        for pool, r in zip((k_cache, v_cache), rows):
            pool[pg[ok], :, (pos % page_size)[ok]] = r[ok]


def _kv_append_q8_model(k_new, v_new, k_cache, v_cache, k_descale, v_descale, lens, cu, max_seqlen_q, block_table) -> None:
    """``pfa_kv_append_q8``'s rule in plain torch: every source element as ``quantize_kv`` stores it, then ``_kv_append_model``'s
    placement, on the caches' bytes.  The executable specification, and what ``kv_append`` runs on CPU tensors with FP8 caches."""
    def rows8(x, d):
        if cu is None:                                    # [B, Hkv, Sq, D]
            return quantize_kv(x, d)
        if d.dim() == 2:                                  # packed rows: each row takes its sequence's scales
            seq = torch.zeros(x.shape[0], dtype=torch.int64)
            for b in range(len(lens)):
                s_b = min(max(cu[b], 0), x.shape[0])
                seq[s_b:min(max(cu[b + 1], s_b), x.shape[0])] = b
            d = d[seq]                                    # [total, Hkv]
        return (x.to(torch.float32) / d[..., None]).clamp(-FP8_MAX, FP8_MAX).to(FP8)
    _kv_append_model(rows8(k_new, k_descale).view(torch.uint8), rows8(v_new, v_descale).view(torch.uint8), k_cache.view(torch.uint8),
                     v_cache.view(torch.uint8), lens, cu, max_seqlen_q, block_table)


def _page_copy_model(k_pool, v_pool, pairs, rows) -> None:
    """``pfa_page_copy``'s rule in plain torch, pair by pair in order, every range check and clamp included: the executable
    specification, and what ``page_copy`` runs on CPU tensors.  ``pairs`` is a host list of ``(src, dst)``, ``rows`` one of counts or
    None; the pools are ``[num_pages, Hkv, page_size, D]``-shaped views."""
    num_pages, page_size = k_pool.shape[0], k_pool.shape[2]
    for i, (s, d) in enumerate(pairs):
        if not 0 <= s < num_pages or not 0 <= d < num_pages or s == d:       # the empty pair: nothing read, nothing written
            continue
        r = page_size if rows is None else min(max(rows[i], 0), page_size)
        for pool in (k_pool, v_pool):
            pool[d, :, :r] = pool[s, :, :r].clone()


def _rope_rotate(x: torch.Tensor, c: torch.Tensor, s: torch.Tensor, interleaved: bool) -> torch.Tensor:
    """Rows ``x [n, heads, D]`` rotated by their table rows ``c`` / ``s`` (fp32 ``[n, half]``), as ``pfa_rope_append`` rounds: operands
    widened to fp32, the two products and the add / subtract separate fp32 operations, one rounding to the dtype.  Elements at and
    past ``2 * half`` are copied.  -> a new tensor."""
    half = c.shape[-1]
    R = 2 * half
    c, s = c[:, None, :], s[:, None, :]
    x1, x2 = (x[..., 0:R:2], x[..., 1:R:2]) if interleaved else (x[..., :half], x[..., half:R])
    y1 = (x1.float() * c - x2.float() * s).to(x.dtype)
    y2 = (x2.float() * c + x1.float() * s).to(x.dtype)
    out = x.clone()
    if interleaved:
        out[..., 0:R:2], out[..., 1:R:2] = y1, y2
    else:
        out[..., :half], out[..., half:R] = y1, y2
    return out


def _rope_append_model(k_new, v_new, k_cache, v_cache, cos, sin, lens, cu, max_seqlen_q, block_table, offsets, interleaved,
                       q=None, q_out=None) -> None:
    """``pfa_rope_append``'s rule in plain torch, every clamp and drop included: the executable specification, and what
    ``rope_append`` runs on CPU tensors.  The placement is ``_kv_append_model``'s, one sequence at a time, on that sequence's rotated K
    rows.  ``lens`` / ``cu`` / ``offsets`` are host lists (``offsets`` or None); the tensors as in ``rope_append``."""
    paged = block_table is not None
    Smax = block_table.shape[1] * k_cache.shape[2] if paged else k_cache.shape[2]
    total, max_pos = k_new.shape[0], cos.shape[0]
    q_src = None if q is None else q.clone()                                   # q_out may be q
    k_rot = k_new.clone()                                                      # rows no sequence covers stay as they are, unread
    for b, n in enumerate(lens):
        len_b = min(max(n, 0), Smax)
        if cu is not None:
            s_b = min(max(cu[b], 0), total)
            e_b = min(max(cu[b + 1], s_b), total)
            sq = min(e_b - s_b, max_seqlen_q)
        else:
            sq = max_seqlen_q
        if sq < 1:
            continue
        pos = torch.arange(len_b - sq, len_b, dtype=torch.int64) + (0 if offsets is None else offsets[b])
        pos.clamp_(0, max_pos - 1)                                             # rows in front of key 0 too: their Q is still written
        c, s = cos[pos], sin[pos]
        if cu is not None:
            rows = slice(s_b, s_b + sq)
            k_rot[rows] = _rope_rotate(k_new[rows], c, s, interleaved)
            if q is not None:
                q_out[rows] = _rope_rotate(q_src[rows], c, s, interleaved)
            one = (k_rot, v_new)
        else:
            k_rot[b] = _rope_rotate(k_new[b].transpose(0, 1), c, s, interleaved).transpose(0, 1)
            if q is not None:
                q_out[b] = _rope_rotate(q_src[b].transpose(0, 1), c, s, interleaved).transpose(0, 1)
            one = (k_rot[b:b + 1], v_new[b:b + 1])
        caches = (k_cache, v_cache) if paged else (k_cache[b:b + 1], v_cache[b:b + 1])
        _kv_append_model(*one, *caches, [n], None if cu is None else [cu[b], cu[b + 1]], max_seqlen_q,
                         block_table[b:b + 1] if paged else None)


def _rotary_model(xs, outs, cos, sin, interleaved, conjugate, cu, max_seqlen, offsets, position_ids) -> None:
    """``pfa_rotary``'s rule in plain torch, every clamp included: the executable specification, and what ``apply_rotary`` runs on CPU
    tensors.  ``xs``: one or two tensors over the same rows, ``[total, H, D]`` with ``cu`` (a host list), else ``[B, H, S, D]``;
    ``outs``: where each goes, the tensor itself for the in-place call, which touches nothing at and past ``rot_dim``.  ``offsets``: a
    host list or None; ``position_ids``: int32 ``[total]`` / ``[B, S]`` or None.  The conjugate rotation is the rule at ``-sin``."""
    max_pos, R = cos.shape[0], 2 * cos.shape[1]
    if conjugate:
        sin = -sin
    src = [x.clone() for x in xs]                                              # an output may be its input
    packed = cu is not None
    total = xs[0].shape[0]
    for b in range(len(cu) - 1 if packed else xs[0].shape[0]):
        s_b, rows = 0, max_seqlen
        if packed:
            s_b = min(max(cu[b], 0), total)
            rows = min(min(max(cu[b + 1], s_b), total) - s_b, max_seqlen)
        if rows < 1:
            continue
        if position_ids is not None:
            pos = (position_ids[s_b:s_b + rows] if packed else position_ids[b, :rows]).to(torch.int64)
        else:
            pos = torch.arange(rows, dtype=torch.int64) + (0 if offsets is None else offsets[b])
        pos = pos.clamp(0, max_pos - 1)
        c, s = cos[pos], sin[pos]
        for x, o in zip(src, outs):
            cut = R if any(o is t for t in xs) else x.shape[-1]
            if packed:
                o[s_b:s_b + rows, :, :cut] = _rope_rotate(x[s_b:s_b + rows], c, s, interleaved)[..., :cut]
            else:
                o[b, :, :rows, :cut] = _rope_rotate(x[b, :, :rows].transpose(0, 1), c, s, interleaved).transpose(0, 1)[..., :cut]


QKNORM_BWD_ROWS = 32      # rows of one sequence a stage-1 workgroup of pfa_qk_norm_bwd walks (csrc/qk_norm_kernel.h)
_QKNORM_THREADS = 256


def _qkn_order(D: int, R: int, interleaved: bool) -> torch.Tensor:
    """``[D / 16, 2]``: the two 8-element chunks of every 16-element unit of a head -- ``(u, u + R / 16)`` in the rotated region of the
    half pairing, ``(2u, 2u + 1)`` everywhere else (csrc/rotary_kernel.h)."""
    ru = R // 16
    return torch.tensor([(u, u + ru) if (not interleaved and u < ru) else (2 * u, 2 * u + 1) for u in range(D // 16)], dtype=torch.int64)


def _qkn_head_sum(p: torch.Tensor, order: torch.Tensor) -> torch.Tensor:
    """The kernels' sum tree over the head dim of the fp32 products ``p [..., D]`` -> ``[..., 1]``: every 8-element chunk left to
    right, a unit's two chunk sums in the order of its pair, the D / 16 unit sums by an xor butterfly (masks 1, 2, .. D / 32)."""
    ch = p.contiguous().reshape(*p.shape[:-1], p.shape[-1] // 8, 8)
    s = ch[..., 0]
    for k in range(1, 8):
        s = s + ch[..., k]
    lane = s[..., order[:, 0]] + s[..., order[:, 1]]
    G, m = order.shape[0], 1
    idx = torch.arange(G)
    while m < G:
        lane = lane + lane[..., idx ^ m]
        m <<= 1
    return lane[..., :1]


def _qkn_scale(w: torch.Tensor, unit_offset: bool) -> torch.Tensor:
    s = w.to(torch.float32)
    return 1.0 + s if unit_offset else s


def _qkn_r(xf: torch.Tensor, eps: float, order: torch.Tensor) -> torch.Tensor:
    """``r = 1 / sqrt(mean(x^2) + eps)`` of every head of the fp32 ``xf [..., D]`` -> ``[..., 1]``, as the kernels round it: the IEEE
    fp32 square root, then the IEEE fp32 divide.  torch's fp32 ``sqrt`` on the CPU comes from a vector math library and is NOT
    correctly rounded (it misses by one unit in the last place in about one value in 150), so each of the two operations is taken in
    fp64 and rounded once to fp32 -- which is the correctly rounded fp32 result, for the square root and for the quotient alike,
    because fp64 carries 53 >= 2 * 24 + 2 bits."""
    ms = _qkn_head_sum(xf * xf, order) * (1.0 / xf.shape[-1])
    root = torch.sqrt((ms + torch.tensor(eps, dtype=torch.float32)).to(torch.float64)).to(torch.float32)
    return (1.0 / root.to(torch.float64)).to(torch.float32)


def _qkn_rotate32(n: torch.Tensor, c, s, interleaved: bool) -> torch.Tensor:
    """``_rope_rotate`` on fp32 rows ``n [rows, heads, D]`` with no narrowing: the three roundings of a pair, elements at and past
    ``2 * half`` as they are.  ``c`` None: no rotation."""
    if c is None:
        return n
    half = c.shape[-1]
    R = 2 * half
    c, s = c[:, None, :], s[:, None, :]
    n1, n2 = (n[..., 0:R:2], n[..., 1:R:2]) if interleaved else (n[..., :half], n[..., half:R])
    y1, y2 = n1 * c - n2 * s, n2 * c + n1 * s
    out = n.clone()
    if interleaved:
        out[..., 0:R:2], out[..., 1:R:2] = y1, y2
    else:
        out[..., :half], out[..., half:R] = y1, y2
    return out


def _qkn_forward_rows(x, w, eps, unit_offset, c, s, interleaved) -> torch.Tensor:
    """Rows ``x [rows, heads, D]`` normalised and rotated: ``pfa_qk_norm``'s rule for one tensor of one sequence.  -> a new tensor."""
    order = _qkn_order(x.shape[-1], 0 if c is None else 2 * c.shape[-1], interleaved)
    xf = x.to(torch.float32)
    n = (xf * _qkn_r(xf, eps, order)) * _qkn_scale(w, unit_offset)
    return _qkn_rotate32(n, c, s, interleaved).to(x.dtype)


def _qkn_backward_rows(x, dy, w, eps, unit_offset, c, s, interleaved):
    """``pfa_qk_norm_bwd``'s rule for rows ``x`` / ``dy [rows, heads, D]`` -> (``dx`` in the dtype, the fp32 terms ``g * xh`` of the
    weight gradient)."""
    order = _qkn_order(x.shape[-1], 0 if c is None else 2 * c.shape[-1], interleaved)
    xf = x.to(torch.float32)
    r = _qkn_r(xf, eps, order)
    g = _qkn_rotate32(dy.to(torch.float32), c, None if s is None else -s, interleaved)      # the conjugate: the rule at -sin, exact
    xh = xf * r
    a = g * _qkn_scale(w, unit_offset)
    cc = _qkn_head_sum(a * xh, order) * (1.0 / x.shape[-1])
    return (r * (a - xh * cc)).to(x.dtype), g * xh


def _qkn_sequences(first, cos, sin, cu, max_seqlen, offsets, position_ids):
    """(b, first packed row, rows, cos rows, sin rows) of every sequence, with ``pfa_rotary``'s clamps; the table rows are None without
    tables.  ``first``: the first tensor, ``[total, H, D]`` with ``cu`` else ``[B, H, S, D]``."""
    packed = cu is not None
    total = first.shape[0]
    for b in range(len(cu) - 1 if packed else first.shape[0]):
        s_b, rows = 0, max_seqlen
        if packed:
            s_b = min(max(cu[b], 0), total)
            rows = min(min(max(cu[b + 1], s_b), total) - s_b, max_seqlen)
        c = s = None
        if cos is not None and rows >= 1:
            if position_ids is not None:
                pos = (position_ids[s_b:s_b + rows] if packed else position_ids[b, :rows]).to(torch.int64)
            else:
                pos = torch.arange(rows, dtype=torch.int64) + (0 if offsets is None else offsets[b])
            pos = pos.clamp(0, cos.shape[0] - 1)
            c, s = cos[pos], sin[pos]
        yield b, s_b, rows, c, s


def _qk_norm_model(xs, outs, ws, eps, unit_offset, cos, sin, interleaved, cu, max_seqlen, offsets, position_ids) -> None:
    """``pfa_qk_norm``'s rule in plain torch, every clamp and every rounding included: the executable specification, and what
    ``qk_norm`` runs on CPU tensors.  ``xs``: one or two tensors over the same rows, ``[total, H, D]`` with ``cu`` (a host list), else
    ``[B, H, S, D]``; ``outs``: where each goes (the tensor itself in place); ``ws``: their weights ``[D]``; ``cos`` / ``sin`` None:
    the norm alone.  All arithmetic is fp32 on widened operands, every product and sum an op of its own; the sum over the head dim is
    ``_qkn_head_sum``'s tree, spelled out in slices and index tables."""
    src = [x.clone() for x in xs]                                              # an output may be its input
    packed = cu is not None
    for b, s_b, rows, c, s in _qkn_sequences(xs[0], cos, sin, cu, max_seqlen, offsets, position_ids):
        if rows < 1:
            continue
        for x, o, w in zip(src, outs, ws):
            if packed:
                o[s_b:s_b + rows] = _qkn_forward_rows(x[s_b:s_b + rows], w, eps, unit_offset, c, s, interleaved)
            else:
                o[b, :, :rows] = _qkn_forward_rows(x[b, :, :rows].transpose(0, 1), w, eps, unit_offset, c, s, interleaved).transpose(0, 1)


def _qk_norm_bwd_model(xs, dys, dxs, ws, dws, eps, unit_offset, cos, sin, interleaved, cu, max_seqlen, offsets, position_ids) -> None:
    """``pfa_qk_norm_bwd``'s rule in plain torch: ``dxs`` (the dtype) and ``dws`` (fp32 ``[D]``, overwritten) from ``xs``, ``dys`` and
    the forward's other operands.  The weight gradient is summed in the kernels' order: per tensor and sequence, chunks of
    ``QKNORM_BWD_ROWS`` rows; inside a chunk the heads in ``[row][head]`` order are dealt to ``256 / (D / 16)`` slots, every slot adds
    its heads in order, the slots are added in order into the chunk's partial (zeros for a chunk past its sequence); the partials
    ``k, k + 16, ...`` are added in order for every ``k`` in 0 .. 15 and those 16 sums in order."""
    packed = cu is not None
    D = xs[0].shape[-1]
    slots, groups = _QKNORM_THREADS // (D // 16), 16
    nrc = -(-max_seqlen // QKNORM_BWD_ROWS)
    partials = [[] for _ in xs]
    for b, s_b, rows, c, s in _qkn_sequences(xs[0], cos, sin, cu, max_seqlen, offsets, position_ids):
        for t, (x, dy, dx, w) in enumerate(zip(xs, dys, dxs, ws)):
            terms = None
            if rows >= 1:
                if packed:
                    got, terms = _qkn_backward_rows(x[s_b:s_b + rows], dy[s_b:s_b + rows], w, eps, unit_offset, c, s, interleaved)
                    dx[s_b:s_b + rows] = got
                else:
                    got, terms = _qkn_backward_rows(x[b, :, :rows].transpose(0, 1), dy[b, :, :rows].transpose(0, 1), w, eps, unit_offset, c, s,
                                                    interleaved)
                    dx[b, :, :rows] = got.transpose(0, 1)
            for ch in range(nrc):
                r0 = ch * QKNORM_BWD_ROWS
                if r0 >= rows:
                    partials[t].append(torch.zeros(D))
                    continue
                heads = terms[r0:r0 + QKNORM_BWD_ROWS].reshape(-1, D)          # [row][head]
                acc = torch.zeros(slots, D)
                for at in range(0, heads.shape[0], slots):
                    step = heads[at:at + slots]
                    acc[:step.shape[0]] = acc[:step.shape[0]] + step
                part = acc[0]
                for q in range(1, slots):
                    part = part + acc[q]
                partials[t].append(part)
    for t, dw in enumerate(dws):
        sums = []
        for k in range(groups):
            v = torch.zeros(D)
            for part in partials[t][k::groups]:
                v = v + part
            sums.append(v)
        v = sums[0]
        for other in sums[1:]:
            v = v + other
        dw.copy_(v)


def _attn_merge_model(outs, lses, out, lse_out) -> None:
    """``pfa_attn_merge``'s rule in plain fp32 torch ops, in part order: the executable specification, and what ``attn_merge`` runs on
    CPU tensors.  A part whose LSE is -inf is selected away, never multiplied in; a NaN LSE makes the row NaN."""
    neg_inf = float("-inf")
    L = torch.stack([l.to(torch.float32) for l in lses])                      # [N, B, H, Sq]
    live = L > neg_inf                                                        # False for -inf and for NaN
    m = torch.where(live, L, torch.full_like(L, neg_inf)).max(dim=0).values
    s = torch.zeros_like(m)
    acc = torch.zeros(outs[0].shape, dtype=torch.float32, device=m.device)
    for n, o_n in enumerate(outs):
        w = torch.exp(L[n] - m)
        s = torch.where(live[n], s + w, s)
        acc = torch.where(live[n][..., None], acc + w[..., None] * o_n.to(torch.float32), acc)
    none = ~(m > neg_inf)                                                     # no part with a visible key
    o = torch.where(none[..., None], torch.zeros_like(acc), acc / s[..., None])
    lse = torch.where(none, torch.full_like(m, neg_inf), m + torch.log(s))
    nan = torch.isnan(L).any(dim=0)
    o = torch.where(nan[..., None], torch.full_like(o, float("nan")), o)
    lse = torch.where(nan, torch.full_like(lse, float("nan")), lse)
    out.copy_(o)                                                              # 16-bit: round to nearest even
    if lse_out is not None:
        lse_out.copy_(lse)


def _packed_seqs(cu_q, cu_k, total_q: int, total_k: int, max_seqlen_q: int, max_seqlen_k: int):
    """The kernels' reading of two host ``cu_seqlens`` lists: per sequence ``(s_q, Sq_b, s_k, Sk_b)`` with ``s = clamp(cu[b], 0,
    total)``, ``e = clamp(cu[b + 1], s, total)``, ``S_b = min(e - s, max_seqlen)`` -- the rule of ``pfa_fa3_prefill_varlen_args``."""
    def one(cu, b, total, cap):
        s = min(max(cu[b], 0), total)
        e = min(max(cu[b + 1], s), total)
        return s, min(e - s, cap)
    return [one(cu_q, b, total_q, max_seqlen_q) + one(cu_k, b, total_k, max_seqlen_k) for b in range(len(cu_q) - 1)]


def _packed_probs(qb, kb, lse_b, causal: bool, scale: float):
    """fp32 scores of one sequence ``[H, Sq_b, Sk_b]`` (top-left causal: row i sees key j iff j <= i) and, given the rows' LSE, the
    softmax weights ``exp(s - lse)`` (0 where masked or where the row has no key)."""
    s = torch.matmul(qb, kb.transpose(1, 2)) * scale
    if causal:
        i, j = torch.arange(s.shape[1])[:, None], torch.arange(s.shape[2])[None, :]
        s = s.masked_fill(j > i, float("-inf"))
    if lse_b is None:
        return s, None
    p = torch.exp(s - lse_b[:, :, None])
    return s, torch.where(torch.isfinite(lse_b)[:, :, None] & torch.isfinite(s), p, torch.zeros_like(p))


def _varlen_forward_model(q, k, v, out, lse, cu_q, cu_k, max_seqlen_q, max_seqlen_k, causal, scale) -> None:
    """``pfa_fa3_varlen_fwd``'s rule in plain torch, per sequence in fp32, every clamp included: the executable specification, and
    what ``fa3_varlen_forward`` runs on CPU tensors.  ``cu_q`` / ``cu_k`` are host lists; writes the covered rows of out / lse only."""
    g = q.shape[1] // k.shape[1]
    for sq, nq, sk, nk in _packed_seqs(cu_q, cu_k, q.shape[0], k.shape[0], max_seqlen_q, max_seqlen_k):
        if nq == 0:
            continue
        if nk == 0:                                                     # rows without a key: O = 0, LSE = -inf
            out[sq:sq + nq] = 0
            if lse is not None:
                lse[:, sq:sq + nq] = float("-inf")
            continue
        qb = q[sq:sq + nq].float().transpose(0, 1)
        kb, vb = (t[sk:sk + nk].float().transpose(0, 1).repeat_interleave(g, dim=0) for t in (k, v))
        s, _ = _packed_probs(qb, kb, None, causal, scale)
        lse_b = torch.logsumexp(s, dim=-1)                              # (top-left causal: every row sees key 0)
        out[sq:sq + nq] = torch.matmul(torch.exp(s - lse_b[:, :, None]), vb).transpose(0, 1).to(out.dtype)
        if lse is not None:
            lse[:, sq:sq + nq] = lse_b


def _varlen_backward_model(q, k, v, out, dout, lse, dq, dk, dv, cu_q, cu_k, max_seqlen_q, max_seqlen_k, causal, scale) -> None:
    """``pfa_fa3_varlen_bwd``'s rule in plain torch (see ``_varlen_forward_model``): writes rows ``[s_q, s_q + Sq_b)`` of dq and
    ``[s_k, s_k + Sk_b)`` of dk / dv of every sequence, and nothing else."""
    Hkv = k.shape[1]
    g = q.shape[1] // Hkv
    for sq, nq, sk, nk in _packed_seqs(cu_q, cu_k, q.shape[0], k.shape[0], max_seqlen_q, max_seqlen_k):
        if nq == 0 or nk == 0:                                          # no key: dQ = 0; no row: dK = dV = 0
            dq[sq:sq + nq] = 0
            dk[sk:sk + nk] = 0
            dv[sk:sk + nk] = 0
            continue
        qb, ob, gb = (t[sq:sq + nq].float().transpose(0, 1) for t in (q, out, dout))
        kb, vb = (t[sk:sk + nk].float().transpose(0, 1).repeat_interleave(g, dim=0) for t in (k, v))
        _, p = _packed_probs(qb, kb, lse[:, sq:sq + nq], causal, scale)
        delta = (gb * ob).sum(-1)
        ds = p * (torch.matmul(gb, vb.transpose(1, 2)) - delta[:, :, None])
        dq[sq:sq + nq] = (torch.matmul(ds, kb) * scale).transpose(0, 1).to(dq.dtype)
        dkb = torch.matmul(ds.transpose(1, 2), qb) * scale              # [H, Sk_b, D] -> summed over each group of query heads
        dvb = torch.matmul(p.transpose(1, 2), gb)
        dk[sk:sk + nk] = dkb.reshape(Hkv, g, nk, -1).sum(1).transpose(0, 1).to(dk.dtype)
        dv[sk:sk + nk] = dvb.reshape(Hkv, g, nk, -1).sum(1).transpose(0, 1).to(dv.dtype)


def _sink_grad_model(lse, delta, sinks, d_sinks, rows=None) -> None:
    """``pfa_fa3_sink_grad``'s rule in plain torch, fp32: ``d_sinks[h] = - sum exp(sinks[h] - lse) * delta`` over the rows of head h --
    the executable specification, and what ``fa3_sink_grad`` runs on CPU tensors.  Dense ``[B, H, Sq]`` arrays (``rows`` None), or packed
    ``[H, total_q]`` ones with ``rows`` the host list of ``(start, count)`` per sequence: rows no sequence covers are not read.  A row
    with ``lse = -inf`` is SKIPPED (``delta`` there may hold anything, NaN included), and a ``-inf`` sink skips every row of its head."""
    H = sinks.shape[0]
    if rows is None:
        l, d = lse.transpose(0, 1).reshape(H, -1), delta.transpose(0, 1).reshape(H, -1)
    else:
        idx = torch.cat([torch.arange(s, s + n) for s, n in rows] + [torch.zeros(0, dtype=torch.long)])
        l, d = lse[:, idx], delta[:, idx]
    s = sinks.float()[:, None]
    live = (l > float("-inf")) & (s > float("-inf"))
    terms = torch.exp(torch.where(live, s - l.float(), torch.zeros_like(l))) * torch.where(live, d.float(), torch.zeros_like(d))
    d_sinks.copy_(-torch.where(live, terms, torch.zeros_like(terms)).sum(dim=1) + 0.0)

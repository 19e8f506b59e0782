"""What the host and the GPU tests of QK-norm (``ops.qk_norm``, ``pfa_qk_norm*``) share: the fp64 evaluation of the rule, its mutants, and
the error bounds with their derivation.  Plain functions; pytest collects nothing from here.

All bounds are first-order counts of fp32 roundings, u = 2^-24 each (second-order terms are below 1e-5 of any slack here):

forward, ``2^-8 |y| + K u (|n1| + |n2|)`` (fp16: ``2^-11 |y| + 2^-25`` for the first term; ``n2 = 0`` outside the rotated region):
  the sum of squares carries 1 (a product) + 7 (a chunk, left to right) + 1 (the chunk pair) + log2(D / 16) = 3 (the butterfly) = 12
  roundings at D 128, all on positive terms, so 12 u relative; then ``+ eps``, the square root and the divide: 15 u on ``r`` (the square
  root halves what it is handed; the count does not use that).  ``x * r``: 16, ``* s``: 17, and with the unit offset ``1 + w``: 18 -- the
  relative error of ``n``.  A rotated element ``n1 c - n2 s`` adds one rounding to each product (19, on ``|n1 c| + |n2 s| <= |n1| +
  |n2|``) and one for the subtraction (on ``|y| <= |n1| + |n2|``): K = 20.

backward dx, ``2^-8 |dx| + K' u r (A_j + |xh_j| C)`` with ``A_j = (|dy1 c| + |dy2 s|) |s_j| >= |a_j|`` and ``C = sum_j A_j |xh_j| / D``:
  ``a``: 2 (the rotation, on ``|dy1 c| + |dy2 s|``) + 1 (``* s``) + 1 (unit offset) = 4; ``xh``: 15 + 1 = 16; a term ``a xh``: 4 + 16 + 1 =
  21, the tree over them 7 + 1 + 3 = 11 more: 32 on ``C``; ``xh c``: 16 + 32 + 1 = 49; the subtraction 1; ``r *``: 15 + 1.  K' = 49 + 1 +
  16 = 66.

backward dw, ``(N + 19) u sum (|dy1 c| + |dy2 s|) |xh|`` over the N = rows x heads terms of an element: a term ``g xh`` carries 2 + 16 + 1 =
  19 roundings, and N terms added in ANY order carry at most N - 1 more on the sum of their magnitudes."""

from __future__ import annotations

import torch

U = 2.0 ** -24
K_FWD, K_DX, K_DW_TERM = 20, 66, 19


def pairs(t, R, interleaved):
    return (t[..., 0:R:2], t[..., 1:R:2]) if interleaved else (t[..., :R // 2], t[..., R // 2:R])


def put_pairs(t, y1, y2, R, interleaved):
    out = t.clone()
    if interleaved:
        out[..., 0:R:2], out[..., 1:R:2] = y1, y2
    else:
        out[..., :R // 2], out[..., R // 2:R] = y1, y2
    return out


def rotate64(n, c, s, interleaved):
    """fp64 rotation of ``n [B, H, S, D]`` by table rows ``c`` / ``s`` ``[B, 1, S, R / 2]`` (None: none)."""
    if c is None:
        return n
    R = 2 * c.shape[-1]
    n1, n2 = pairs(n, R, interleaved)
    return put_pairs(n, n1 * c - n2 * s, n2 * c + n1 * s, R, interleaved)


def partner_abs(n, c, interleaved):
    """``|n1| + |n2|`` at every element: its own magnitude plus its pair's inside the rotated region, its own outside."""
    a = n.abs()
    if c is None:
        return a
    R = 2 * c.shape[-1]
    a1, a2 = pairs(a, R, interleaved)
    return put_pairs(a, a1 + a2, a1 + a2, R, interleaved)


def each_sequence(ts, cos, sin, cu=None, max_seqlen=None, offsets=None, position_ids=None):
    """Every sequence of at least one row as a dense problem: -> (the tensors' rows as ``[1, H, rows, D]`` views, the fp64 table rows
    ``[1, 1, rows, R / 2]`` twice -- or None, None without tables), with the clamps of the packed kernels.  ``ts``: ``[total, H, D]``
    tensors with ``cu`` (a host list), else ``[B, H, S, D]``."""
    packed = cu is not None
    total = ts[0].shape[0]
    for b in range(len(cu) - 1 if packed else ts[0].shape[0]):
        s_b, rows = 0, ts[0].shape[2] if not packed else max_seqlen
        if packed:
            s_b = min(max(cu[b], 0), total)
            rows = min(min(max(cu[b + 1], s_b), total) - s_b, max_seqlen)
        if rows < 1:
            continue
        views = [t[s_b:s_b + rows].transpose(0, 1)[None] if packed else t[b:b + 1] for t in ts]
        c = s = None
        if cos is not None:
            if position_ids is not None:
                pos = (position_ids[s_b:s_b + rows] if packed else position_ids[b, :rows]).to(torch.int64)
            else:
                pos = torch.arange(rows) + (0 if offsets is None else int(offsets[b]))
            pos = pos.clamp(0, cos.shape[0] - 1)
            c, s = cos[pos][None, None].double(), sin[pos][None, None].double()
        yield views, c, s


def forward64(x, w, eps, unit_offset, c, s, interleaved, mutant=None):
    """The rule in fp64 on ``x [B, H, S, D]`` (fp64), ``w [D]`` (fp64) -> (y, n).  ``mutant``: one deliberate mistake."""
    D = x.shape[-1]
    sc = 1.0 + w if bool(unit_offset) != (mutant == "unit") else w          # the mutant: 1 + w without the flag (and w with it)
    src = x * sc if mutant == "weight_first" else x
    R = D if c is None else 2 * c.shape[-1]
    ms = (src * src)[..., :R].mean(-1, keepdim=True) if mutant == "mean_over_R" else (src * src).mean(-1, keepdim=True)
    r = 1.0 / torch.sqrt(ms + (0.0 if mutant == "no_eps" else eps))
    n = src * r if mutant == "weight_first" else (x * r) * sc
    return rotate64(n, c, s, interleaved), n


def forward_ratio(got, x, w, eps, unit_offset, c, s, interleaved):
    """max |got - y64| / bound over every element (the forward bound of this file's docstring)."""
    y, n = forward64(x.double(), w.double(), eps, unit_offset, c, s, interleaved)
    first = 2.0 ** -8 * y.abs() if got.dtype == torch.bfloat16 else 2.0 ** -11 * y.abs() + 2.0 ** -25
    bound = first + K_FWD * U * partner_abs(n, c, interleaved)
    return float(((got.double() - y).abs() / bound).max())


def backward64(x, dy, w, eps, unit_offset, c, s, interleaved):
    """fp64 autograd of ``forward64`` -> (dx, dw): the guard of the backward formula itself."""
    x, w = x.double().requires_grad_(True), w.double().requires_grad_(True)
    y, _ = forward64(x, w, eps, unit_offset, c, s, interleaved)
    return torch.autograd.grad(y, (x, w), dy.double())


def backward_bounds(x, dy, w, eps, unit_offset, c, s, interleaved, dx64, dtype):
    """(bound of dx per element, ``sum (|dy1 c| + |dy2 s|) |xh|`` per element of the head dim: what ``dw_bound`` scales) of this
    file's docstring, from fp64 quantities."""
    x, dy, w = x.double(), dy.double(), w.double()
    D = x.shape[-1]
    sc = 1.0 + w if unit_offset else w
    r = 1.0 / torch.sqrt((x * x).mean(-1, keepdim=True) + eps)
    xh = (x * r).abs()
    g_abs = dy.abs()
    if c is not None:                                       # |dy1 c| + |dy2 s| for both members of a pair
        R = 2 * c.shape[-1]
        d1, d2 = pairs(g_abs, R, interleaved)
        g_abs = put_pairs(g_abs, d1 * c.abs() + d2 * s.abs(), d2 * c.abs() + d1 * s.abs(), R, interleaved)
    A = g_abs * sc.abs()
    Cm = (A * xh).sum(-1, keepdim=True) / D
    first = 2.0 ** -8 * dx64.abs() if dtype == torch.bfloat16 else 2.0 ** -11 * dx64.abs() + 2.0 ** -25
    dx_bound = first + K_DX * U * r * (A + xh * Cm)
    return dx_bound, (g_abs * xh).sum((0, 1, 2))


def dw_bound(n_terms: int, magnitude):
    """The bound of a weight gradient of ``n_terms`` (rows x heads) terms whose magnitudes sum to ``magnitude`` (``backward_bounds``)."""
    return (n_terms + K_DW_TERM) * U * magnitude


def dw_reference(x, dy, w, eps, unit_offset, cos, sin, interleaved, cu=None, max_seqlen=None, offsets=None, position_ids=None):
    """(the weight gradient in fp64, its bound per element) of one tensor of a dense or packed call: fp64 autograd sequence by sequence,
    N counted over every row and head that contributes."""
    want, mag, terms = torch.zeros(x.shape[-1], dtype=torch.float64), torch.zeros(x.shape[-1], dtype=torch.float64), 0
    for (xb, dyb), c, s in each_sequence([x, dy], cos, sin, cu, max_seqlen, offsets, position_ids):
        dx64, dw64 = backward64(xb, dyb, w, eps, unit_offset, c, s, interleaved)
        want += dw64
        mag += backward_bounds(xb, dyb, w, eps, unit_offset, c, s, interleaved, dx64, x.dtype)[1]
        terms += xb.shape[1] * xb.shape[2]
    return want, dw_bound(terms, mag)


def backward_mutant64(x, dy, w, eps, unit_offset, c, s, interleaved, mutant):
    """The closed form of the backward in fp64 with one deliberate mistake -> dx: ``"sign"`` rotates dy forward instead of by the
    conjugate, ``"no_c"`` drops the ``xh c`` term.  ``None``: the closed form itself."""
    x, dy, w = x.double(), dy.double(), w.double()
    sc = 1.0 + w if unit_offset else w
    r = 1.0 / torch.sqrt((x * x).mean(-1, keepdim=True) + eps)
    g = rotate64(dy, c, None if c is None else (s if mutant == "sign" else -s), interleaved)
    xh, a = x * r, g * sc
    cc = 0.0 if mutant == "no_c" else (a * xh).mean(-1, keepdim=True)
    return r * (a - xh * cc)

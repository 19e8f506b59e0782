"""What the far-address tests share (tests/test_hip_far_cache.py, tests/test_hip_far_dense.py).  Plain functions, constants and small
records; pytest collects nothing from here, and tests/test_far_testlib.py tests it on the CPU, the checks with a NumPy stand-in kernel
that truncates its addresses in one way each.  The counterpart of tests/kvcache_testlib.py for WHERE a kernel reads and writes.

A kernel that drops one ``(int64_t)``, loses one carry or trusts a host limit that is off by a factor of two computes every small
problem right: index times stride stays below 2^31.  These helpers put a tiny problem's tensors gigabytes from their base pointers:

  ``make_arena``                one flat uint8 allocation (12.5 GiB on the device) filled with 0xFF: NaN as bf16, fp16, fp32 and e4m3fn,
                                -1 as an int32 table entry.  One per test module.
  ``Layout`` / ``Placement``    the bookkeeping of one case, on the host: where each tensor's element [0, ..., 0] lies, its element
                                strides, which axes are far and which indices along them are live.  ``Layout.like`` places a tensor
                                with one far axis (``KINDS``: wide, narrow, u32max), ``Layout.pages`` a dense pool of which a table
                                names a few pages, ``Layout.rows`` packed rows; each call searches the first phase at which
                                ``Layout.problems`` stays empty.
  ``aliases(p)``                where each live index would land under the four truncation ``MODELS``
  ``far_view`` / ``write`` / ``read`` / ``restore``     ``torch.as_strided`` over the arena (metadata only); data moves slab by slab
                                through contiguous slices of the flat arena at host-computed byte offsets, never through one strided
                                torch op over the arena: the tests do not depend on torch's own large-index paths.
  ``untouched(arena, regions)``   every byte outside the regions still holds the fill, else the first offender's byte offset
  ``FarCase``                   a case's near tensors and their placements: ``put`` on the host, ``upload`` / ``near_inputs`` /
                                ``finish`` around the two runs on the device
  ``standin_copy``              the NumPy gather / scatter "kernel" of the CPU test, honest or with one truncation model

The truncation models.  With ``x = sum(index * stride)`` in elements, ``e`` the element size and W = 32 the width:

  int32 bytes      wrap_signed(x * e, W)              uint32 bytes      (x * e) mod 2^W
  int32 elements   wrap_signed(x, W) * e              uint32 elements   (x mod 2^W) * e

each applied to the whole offset and to the product of each far axis alone.  An index ALIASES under a model when the truncated
address differs from the true one.  Every far tensor starts at least 4 GiB (``LEAD``) into the arena, so an offset truncated to a
negative number still falls inside the arena and reads NaN or hits a watched byte instead of leaving the allocation.  A layout is
sound (``Layout.problems`` empty) when no two live regions overlap, every alias lies inside the arena with room for its slab, and no
alias starts inside a live region of any tensor placed in it: a truncated read then returns the fill (NaN) or, where it starts a few
bytes in front of a live region, other elements of distinct random data; a truncated write changes a watched byte.  Tensors that
share an arena therefore sit at different phases of the stride period, and the excess of a far stride over 2^32 bytes must exceed
the slabs that share it: this check is what shows it.

fp32 tensors are placed to 4 GiB only (wide, indices 0 .. 1): the int32-elements alias of an fp32 tensor 8 GiB out would fall 8 GiB in
front of its base, outside the arena.  The two element models are not claimed for them.

``wrap`` scales everything down for the CPU test: a layout of width W has its lead at 2^W, strides around 2^W and 2^(W-1) bytes and an
arena of 3.125 * 2^W bytes, and the models wrap at W bits."""

from __future__ import annotations

import dataclasses
import itertools

import numpy as np
import torch

FILL = 0xFF
MODELS = ("int32 bytes", "uint32 bytes", "int32 elements", "uint32 elements")


def arena_bytes(wrap=32):
    return 25 * (1 << wrap) // 8                    # 3.125 x 2^W: 12.5 GiB at W = 32


def lead_bytes(wrap=32):
    return 1 << wrap                                # 4 GiB at W = 32


ARENA_BYTES, LEAD = arena_bytes(), lead_bytes()


def stride_bytes(kind, wrap=32):
    """The far strides, in bytes.  wide: the stride alone does not fit an int; narrow: it does, only index x stride overflows; u32max:
    the largest byte stride of W unsigned bits that keeps 16-byte alignment."""
    return {"wide": (1 << wrap) + (1 << (wrap - 11)), "narrow": (1 << (wrap - 1)) - 16, "u32max": (1 << wrap) - 16}[kind]


KINDS = ("wide", "narrow", "u32max")
# the most indices a far axis of each kind takes (the last one lands just past or just under 8 GiB), by element size
MAX_INDICES = {("wide", 1): 2, ("wide", 2): 3, ("wide", 4): 2, ("wide", 8): 2, ("narrow", 1): 5, ("narrow", 2): 5, ("narrow", 4): 5,
               ("u32max", 1): 3, ("u32max", 2): 3}


def _wrap_signed(x, w):
    x &= (1 << w) - 1
    return x - (1 << w) if x >> (w - 1) else x


def truncated(model, elems, esize, wrap=32):
    """The byte offset a kernel that computes ``elems`` (an element offset) under ``model`` arrives at."""
    if model is None:
        return elems * esize
    if model == "int32 bytes":
        return _wrap_signed(elems * esize, wrap)
    if model == "uint32 bytes":
        return (elems * esize) & ((1 << wrap) - 1)
    if model == "int32 elements":
        return _wrap_signed(elems, wrap) * esize
    if model == "uint32 elements":
        return (elems & ((1 << wrap) - 1)) * esize
    raise ValueError(model)


@dataclasses.dataclass(frozen=True)
class Alias:
    model: str
    index: tuple           # the live index along each far axis
    axis: object           # the far axis whose product was truncated, or None: the whole offset
    address: int           # byte offset in the arena


@dataclasses.dataclass(frozen=True)
class Placement:
    """One tensor in the arena.  ``far``: ((axis, live indices), ...).  A SLAB is what the other (near) axes span around one
    combination of far indices; the live regions are the slabs of the live combinations."""
    name: str
    base: int              # byte offset of element [0, ..., 0]
    esize: int
    shape: tuple
    strides: tuple         # elements
    far: tuple
    kind: str = ""
    wrap: int = 32

    @property
    def far_axes(self):
        return tuple(ax for ax, _ in self.far)

    @property
    def near_axes(self):
        return tuple(ax for ax in range(len(self.shape)) if ax not in self.far_axes)

    @property
    def slab_bytes(self):
        return (sum((self.shape[ax] - 1) * self.strides[ax] for ax in self.near_axes) + 1) * self.esize

    @property
    def near_shape(self):
        """The shape of the near tensor that holds the live data: a far axis shrinks to its live indices."""
        live = dict(self.far)
        return tuple(len(live[ax]) if ax in live else n for ax, n in enumerate(self.shape))

    def live(self):
        """-> [(position along the far axes in the near tensor, index along them in the arena, element offset)]"""
        out = []
        for pos in itertools.product(*(range(len(ix)) for _, ix in self.far)):
            idx = tuple(ix[k] for (_, ix), k in zip(self.far, pos))
            out.append((pos, idx, sum(i * self.strides[ax] for ax, i in zip(self.far_axes, idx))))
        return out

    def regions(self):
        """int64 [n, 2]: first byte and end of every live region, in the order of ``live()``"""
        return np.array([(self.base + off * self.esize, self.base + off * self.esize + self.slab_bytes) for _, _, off in self.live()],
                        dtype=np.int64).reshape(-1, 2)

    def moved(self, base):
        return dataclasses.replace(self, base=base)


def aliases(p, models=MODELS):
    """Every (model, live index) whose truncated address differs from the true one -> [Alias].  The whole offset and each far axis'
    own product are truncated in turn."""
    out, seen = [], set()
    for _, idx, off in p.live():
        true = p.base + off * p.esize
        for model in models:
            cands = [(None, p.base + truncated(model, off, p.esize, p.wrap))]
            for ax, i in zip(p.far_axes, idx):
                term = i * p.strides[ax]
                cands.append((ax, p.base + (off - term) * p.esize + truncated(model, term, p.esize, p.wrap)))
            for ax, addr in cands:
                if addr != true and (model, idx, addr) not in seen:
                    seen.add((model, idx, addr))
                    out.append(Alias(model, idx, ax, addr))
    return out


def claims(p):
    """The models under which at least one live index of ``p`` aliases."""
    got = {a.model for a in aliases(p)}
    return tuple(m for m in MODELS if m in got)


def _inside(points, regions):
    """bool per point: it lies in one of the sorted, disjoint regions [n, 2]"""
    if len(regions) == 0 or len(points) == 0:
        return np.zeros(len(points), dtype=bool)
    j = np.searchsorted(regions[:, 0], points, side="right") - 1
    return (j >= 0) & (points < regions[np.maximum(j, 0), 1])


class Layout:
    """The placements of one case and the rule they obey.  Host arithmetic only: the CPU test builds every layout the GPU tests use."""

    def __init__(self, wrap=32, nbytes=None, lead=None, step=None):
        self.wrap = wrap
        self.nbytes = arena_bytes(wrap) if nbytes is None else nbytes
        self.lead = lead_bytes(wrap) if lead is None else lead
        self.step = max(256, 1 << (wrap - 20)) if step is None else step           # 4 KiB phases at W = 32
        self.placements = []
        self._seen = {}

    # --- the rule ---------------------------------------------------------------------------------------------------------------------

    def _facts(self, p):
        al = aliases(p)
        return p.regions(), np.array([a.address for a in al], dtype=np.int64), p.slab_bytes

    def problems(self, extra=None):
        """What is wrong with the layout (with ``extra`` placed too): a list of sentences, empty for a sound one."""
        ps = self.placements + ([extra] if extra is not None else [])
        facts = []
        for p in ps:
            zero = p.moved(0)                              # regions and aliases move with the base: computed once per tensor
            if zero not in self._seen:
                self._seen[zero] = self._facts(zero)
            r, a, slab = self._seen[zero]
            facts.append((r + p.base, a + p.base, slab))
        out = []
        allr = np.concatenate([f[0] for f in facts]) if facts else np.zeros((0, 2), dtype=np.int64)
        owner = np.concatenate([np.full(len(f[0]), n) for n, f in enumerate(facts)]) if facts else np.zeros(0, dtype=np.int64)
        order = np.argsort(allr[:, 0], kind="stable")
        allr, owner = allr[order], owner[order]
        if len(allr) and (allr[0, 0] < self.lead or allr[:, 1].max() > self.nbytes):
            out.append(f"a live region lies outside [{self.lead}, {self.nbytes})")
        clash = np.nonzero(allr[1:, 0] < allr[:-1, 1])[0]
        if len(clash):
            n = int(clash[0])
            out.append(f"live regions of {ps[owner[n]].name} and {ps[owner[n + 1]].name} overlap at byte {int(allr[n + 1, 0])}")
            return out
        for p, (_, addr, slab) in zip(ps, facts):
            if len(addr) == 0:
                continue
            if addr.min() < 0 or addr.max() + slab > self.nbytes:
                out.append(f"an alias of {p.name} leaves the arena: {int(addr.min())} .. {int(addr.max()) + slab}")
            hit = _inside(addr, allr)
            if hit.any():
                a = int(addr[np.nonzero(hit)[0][0]])
                j = int(np.searchsorted(allr[:, 0], a, side="right") - 1)
                out.append(f"an alias of {p.name} at byte {a} starts inside a live region of {ps[owner[j]].name}")
        return out

    # --- placing ----------------------------------------------------------------------------------------------------------------------

    def place(self, name, shape, strides, esize, far, kind=""):
        """The first phase (``lead + n * step``) at which the tensor joins the layout without a problem -> its Placement."""
        cand = Placement(name, 0, esize, tuple(shape), tuple(strides), tuple((ax, tuple(ix)) for ax, ix in far), kind, self.wrap)
        span = max(off for _, _, off in cand.live()) * esize + cand.slab_bytes
        for n in range(4096):
            base = self.lead + n * self.step
            if base + span > self.nbytes:
                break
            p = cand.moved(base)
            if not self.problems(p):
                self.placements.append(p)
                return p
        raise AssertionError(f"no phase takes {name}: {self.problems(cand.moved(self.lead))}")

    def like(self, name, t, kind, axis=0):
        """``t``'s shape and strides with the stride of ``axis`` made far (``KINDS``), every index along it live."""
        e = t.element_size()
        sb = stride_bytes(kind, self.wrap)
        assert sb % e == 0 and t.shape[axis] <= MAX_INDICES[kind, e], (kind, e, t.shape[axis])
        strides = list(t.stride())
        strides[axis] = sb // e
        return self.place(name, t.shape, strides, e, [(axis, range(t.shape[axis]))], kind)

    def pages(self, name, num_pages, page_shape, esize, ids):
        """A dense pool ``[num_pages, *page_shape]`` of which only the pages ``ids`` are live."""
        strides = [1]
        for n in reversed(page_shape):
            strides.insert(0, strides[0] * n)
        return self.place(name, (num_pages, *page_shape), strides, esize, [(0, sorted(set(ids)))], "pages")

    def rows(self, name, total, inner_shape, inner_strides, esize, row_stride, live_rows):
        """Packed rows ``[total, *inner_shape]`` with ``row_stride`` elements between rows; kind "near" where the last row lies below
        2^31 bytes: such a tensor lives in the arena, among NaN, and claims no model."""
        kind = "rows" if (total - 1) * row_stride * esize >= 1 << (self.wrap - 1) else "near"
        return self.place(name, (total, *inner_shape), (row_stride, *inner_strides), esize, [(0, list(live_rows))], kind)

    def table(self):
        """One line per placement: kind, base, far strides and indices, the models it catches, where its aliases fall."""
        lines = []
        for p in self.placements:
            al = aliases(p)
            span = f"{min(a.address for a in al) / 2 ** 30:.3f} .. {max(a.address for a in al) / 2 ** 30:.3f} GiB" if al else "-"
            far = ", ".join(f"axis {ax}: stride {p.strides[ax]} x {len(ix)} indices up to {max(ix)}" for ax, ix in p.far)
            lines.append(f"{p.name:10s} {p.kind:7s} e{p.esize} base {p.base / 2 ** 30:.6f} GiB  slab {p.slab_bytes} B  {far}  "
                         f"catches [{', '.join(claims(p))}]  aliases {len(al)} at {span}")
        return lines


# --- the arena: views, data in and out, the watch -----------------------------------------------------------------------------------------

def make_arena(device, nbytes=ARENA_BYTES):
    """The flat allocation, filled.  On the device: only where ``nbytes`` + 2 GiB are free (the caller skips otherwise)."""
    arena = torch.empty(nbytes, dtype=torch.uint8, device=device)
    arena.fill_(FILL)
    return arena


def far_view(arena, p, dtype):
    """The tensor a kernel is handed: ``p``'s shape and strides over the arena.  Metadata only."""
    assert dtype.itemsize == p.esize and p.base % p.esize == 0
    return torch.as_strided(arena.view(dtype), p.shape, p.strides, p.base // p.esize)


def _slab(arena, p, off, dtype):
    """The slab at element offset ``off`` as a small strided view of a contiguous slice of the flat arena."""
    start = p.base + off * p.esize
    flat = arena[start:start + p.slab_bytes].view(dtype)
    near = p.near_axes
    return torch.as_strided(flat, tuple(p.shape[ax] for ax in near), tuple(p.strides[ax] for ax in near))


def _near_index(p, pos):
    ix = [slice(None)] * len(p.shape)
    for ax, k in zip(p.far_axes, pos):
        ix[ax] = k
    return tuple(ix)


def write(arena, p, src):
    """``src`` (shape ``p.near_shape``) into the live regions, slab by slab."""
    assert tuple(src.shape) == p.near_shape and src.element_size() == p.esize, (tuple(src.shape), p.near_shape)
    for pos, _, off in p.live():
        _slab(arena, p, off, src.dtype).copy_(src[_near_index(p, pos)])


def read(arena, p, dtype):
    """The live regions, slab by slab -> a fresh contiguous tensor of shape ``p.near_shape`` on the arena's device."""
    out = torch.empty(p.near_shape, dtype=dtype, device=arena.device)
    for pos, _, off in p.live():
        out[_near_index(p, pos)].copy_(_slab(arena, p, off, dtype))
    return out


def restore(arena, placements):
    """The fill back over every live region."""
    for p in placements:
        for s, e in p.regions().tolist():
            arena[s:e].fill_(FILL)


def bits(t):
    """A tensor's bits as integers, for ``torch.equal`` (NaN == NaN, -0 != 0)."""
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def untouched(arena, regions, fill=FILL, chunk=1 << 28):
    """Asserts that every byte of ``arena`` outside ``regions`` ([(first byte, end)], any order, may touch) still holds ``fill``; the
    message names the first offender's byte offset.  The arena is scanned in chunks, eight bytes a comparison where aligned."""
    word = int.from_bytes(bytes([fill]) * 8, "little", signed=True)
    n = arena.numel()
    gaps, at = [], 0
    for s, e in sorted((int(s), int(e)) for s, e in regions):
        assert 0 <= s <= e <= n, (s, e)
        if s > at:
            gaps.append((at, s))
        at = max(at, e)
    if at < n:
        gaps.append((at, n))
    flags = []                                       # (first byte, end, device count of bytes / words that differ)
    for lo, hi in gaps:
        a, b = min(hi, -(-lo // 8) * 8), max(lo, hi // 8 * 8)
        if a >= b:
            a = b = hi
        for s, e in ((lo, a), (b, hi)):
            if e > s:
                flags.append((s, e, (arena[s:e] != fill).sum()))
        for s in range(a, b, chunk):
            e = min(b, s + chunk)
            flags.append((s, e, (arena[s:e].view(torch.int64) != word).sum()))
    if not flags:
        return
    counts = torch.stack([f[2] for f in flags]).cpu().tolist()
    for (s, e, _), c in zip(flags, counts):
        if c:
            first = s + int(torch.nonzero(arena[s:e] != fill)[0, 0])
            raise AssertionError(f"byte {first} of the arena ({first / 2 ** 30:.6f} GiB) holds {int(arena[first]):#x}, not the fill "
                                 f"{fill:#x}: something wrote outside the declared regions")


# --- one case: near tensors, their placements, the two runs ----------------------------------------------------------------------------

class FarCase:
    """The tensors of one far run.  On the host: ``put(name, t, kind, axis)`` records a near tensor with the placement ``Layout.like``
    finds; ``put_at`` records one whose placement the caller made (``Layout.pages`` / ``Layout.rows``); ``plain`` one that stays outside
    the arena (lengths, a table).  role "in": ``t``'s data is written and must come back unchanged; "out": only shape, strides and
    dtype count, the buffer starts as fill; "inout": written, and read back as an output.  ``far=``: what the far run gets where it
    differs from the near run's data (a table of real page ids).  On the device: ``near_inputs`` makes the near run's operands,
    ``upload`` writes the far run's and returns the far views by name; after the far run ``finish`` checks the inputs' bits, reads the
    outputs, scans the whole arena and restores the fill."""

    def __init__(self, wrap=32):
        self.layout = Layout(wrap)
        self.near, self.far, self.place, self.role, self.outside = {}, {}, {}, {}, {}

    def put(self, name, t, kind, axis=0, role="in", far=None):
        return self.put_at(name, t, self.layout.like(name, t, kind, axis), role, far)

    def put_at(self, name, t, p, role="in", far=None):
        assert tuple(t.shape) == p.near_shape and t.element_size() == p.esize and role in ("in", "out", "inout"), (name, tuple(t.shape), p.near_shape)
        self.near[name], self.place[name], self.role[name] = t, p, role
        self.far[name] = t if far is None else far
        return p

    def plain(self, name, near, far=None):
        self.outside[name] = (near, near if far is None else far)

    @property
    def outputs(self):
        return [n for n, r in self.role.items() if r != "in"]

    def near_inputs(self, device):
        """The near run's operands on ``device``, with the strides they were recorded with: the inputs' data, and output buffers whose
        every byte holds the fill."""
        out = {name: t[0].to(device) for name, t in self.outside.items()}
        for name, t in self.near.items():
            span = sum((n - 1) * s for n, s in zip(t.shape, t.stride())) + 1
            buf = torch.full((span * t.element_size(),), FILL, dtype=torch.uint8, device=device).view(t.dtype).as_strided(t.shape, t.stride())
            if self.role[name] != "out":
                buf.copy_(t)
            out[name] = buf
        return out

    def upload(self, arena):
        views = {name: t[1].to(arena.device) for name, t in self.outside.items()}
        for name, p in self.place.items():
            if self.role[name] != "out":
                write(arena, p, self.far[name].to(arena.device))
            views[name] = far_view(arena, p, self.near[name].dtype)
        return views

    def finish(self, arena):
        """-> {output name: its live data, read back}.  Asserts that no input changed and that nothing outside the outputs' regions was
        written; leaves the arena all fill."""
        for name, p in self.place.items():
            if self.role[name] == "in":
                got = read(arena, p, self.near[name].dtype)
                assert torch.equal(bits(got), bits(self.far[name].to(arena.device))), f"the far run changed its input {name}"
        outs = {name: read(arena, self.place[name], self.near[name].dtype) for name in self.outputs}
        untouched(arena, np.concatenate([p.regions() for p in self.place.values()]).tolist())
        restore(arena, self.place.values())
        return outs


# --- the two runs of a GPU case ---------------------------------------------------------------------------------------------------------

class Blocks:
    """Every argument and option block ``_capi`` makes while active (``ops`` builds all of them through ``_capi._make``), in order."""

    def __enter__(self):
        from photonic_flash_attention_amd import _capi
        self.made, self._capi, self._make = [], _capi, _capi._make

        def spy(cls, kw):
            a = self._make(cls, kw)
            self.made.append(a)
            return a
        _capi._make = spy
        return self

    def __exit__(self, *exc):
        self._capi._make = self._make

    def of(self, cls_name, n=0):
        """The n-th block of that class, or None"""
        found = [a for a in self.made if type(a).__name__ == cls_name]
        return found[n] if len(found) > n else None


def saw_view(block, field, view, axes="bhs"):
    """(a) of a far case: ``block`` carries ``view``'s pointer in ``field`` and its strides in the ``*_stride_<axis>`` fields."""
    from photonic_flash_attention_amd import ops
    assert getattr(block, field) == view.data_ptr(), f"{field}: the block holds another pointer -- the library saw a copy"
    for name, dim in ops._VIEW_FIELDS[field, axes]:
        assert getattr(block, name) == view.stride(dim), (name, getattr(block, name), view.stride(dim))


@dataclasses.dataclass
class Spec:
    """One GPU case, built on the host.  ``call(t)`` runs the entry point on the tensors ``t`` (by name: the near run's or the far views)
    and returns the further outputs it allocated itself (an LSE); ``seen(blocks, t)`` asserts (a) on the far run's blocks;
    ``describe(blocks)`` names the kernel; ``check(near, extras)`` holds the near run against the existing fp64 bounds; ``family``: what
    the kernel's name must contain, where the far strides change the library's choice."""
    case: FarCase
    call: object
    seen: object
    describe: object
    check: object
    family: str = ""


def two_runs(arena, spec):
    """The near run on ordinary tensors, the far run on views of the arena, and the assertions (a) - (e) of a far case."""
    case, dev = spec.case, arena.device
    assert not case.layout.problems(), case.layout.problems()
    near = case.near_inputs(dev)
    with Blocks() as bn:
        ex_near = spec.call(near)
    torch.cuda.synchronize()
    try:
        far = case.upload(arena)
        with Blocks() as bf:
            ex_far = spec.call(far)
        torch.cuda.synchronize()
        spec.seen(bf, far)                                                                   # (a)
        name_near, name_far = spec.describe(bn), spec.describe(bf)
        print(f"near {name_near}  far {name_far}")
        assert name_near == name_far and spec.family in name_far[0], (name_near, name_far)   # (b)
        got = case.finish(arena)                                                             # (e), and the inputs' bits
    except BaseException:
        arena.fill_(FILL)                                                                    # the next case starts from a clean arena
        raise
    for name, t in got.items():                                                              # (c)
        assert torch.equal(bits(t), bits(near[name])), f"{name}: the far run's bits differ from the near run's"
    assert set(ex_near) == set(ex_far)
    for name in ex_near:
        assert torch.equal(bits(ex_far[name]), bits(ex_near[name])), f"{name}: the far run's bits differ from the near run's"
    spec.check(near, ex_near)                                                                # (d)


# --- the stand-in kernel of the CPU test --------------------------------------------------------------------------------------------------

def standin_copy(arena, src, dst, read_model=None, write_model=None):
    """A NumPy "kernel" over a uint8 array: the slab of every live index of ``src`` copied to the same index of ``dst``, with the whole
    offset computed honestly (None) or under one truncation model on the gather or on the scatter side."""
    assert src.near_shape == dst.near_shape and src.slab_bytes == dst.slab_bytes
    for (_, _, so), (_, _, do) in zip(src.live(), dst.live()):
        s = src.base + truncated(read_model, so, src.esize, src.wrap)
        d = dst.base + truncated(write_model, do, dst.esize, dst.wrap)
        arena[d:d + dst.slab_bytes] = arena[s:s + src.slab_bytes].copy()

"""A paged KV cache for one attention layer, read by ``ops.fa3_decode``, ``ops.fa3_prefill_cache`` and ``ops.fa3_prefill_varlen``
``(..., block_table=...)``.

The cache is a pool of fixed-size pages (``[num_pages, page_size, Hkv, D]`` for K and for V) plus, per sequence slot, a row of a
device block table and a device length.  Which page a sequence's next tokens go to is decided on the host, from a host mirror of
the lengths (the caller says how many tokens it appends, so the host always knows them): nothing here synchronises with the
device.  The device tensors ``block_table`` and ``cache_seqlens`` are allocated once and updated in place, so a captured graph of
``decode`` keeps seeing them; pages a sequence will grow into during replays are assigned ahead with ``reserve``.

A model with sliding-window attention passes ``window=`` to ``decode`` / ``prefill`` / ``prefill_varlen``; the kernels then never read
a key below the 64-key boundary under the lowest visible key, nor its table entry, and ``release_behind_window`` returns the pages
wholly behind the window to the pool while the sequence keeps its logical positions.

Everything except ``decode``, ``prefill`` and ``prefill_varlen`` (the HIP kernels) also runs on CPU tensors, which is how the bookkeeping is tested without a GPU.
``append`` / ``append_varlen`` move the tokens with torch ops from a host-built index, which a captured graph cannot replay.  The
capturable form splits the append in two: ``advance`` (host: pages, lengths, table) and ``write_step`` (device: ``ops.kv_append``, the
HIP copy kernel that places the rows from the device table and lengths).  ``advance`` then ``write_step`` equals ``append_varlen``; a
graph holds ``write_step`` + ``prefill_varlen``, and ``advance`` runs between replays.

With ``copy_on_write=True`` sequences may share pages.  ``fork`` starts a new sequence from an existing one's first keys by sharing
the pages that hold them (parallel sampling, beam search, a cached prefix): it moves no K / V and needs no free page.  Every page has a
reference count; ``free`` and ``release_behind_window`` return a page to the pool only when its last holder lets go.  A slot that
appends into a partly filled tail page it shares takes a fresh page first and the filled rows are copied over by ``ops.page_copy``
(the HIP page-copy kernel): at once in ``append`` / ``append_varlen``, and for ``advance`` from the device tensors ``cow_pairs`` /
``cow_rows`` at the head of ``write_step``, so that a captured step replays through forks.  Full shared pages are never written, so
they are never copied, and ``common_prefix`` names the keys a group of slots shares page for page: the ``shared_prefix=`` of
``decode`` / ``prefill`` / ``prefill_varlen``.

``dtype=torch.float8_e4m3fn`` with ``k_descale=, v_descale=`` (fp32 ``[Hkv]``: one scale per K/V head for the whole pool, since pages may
be shared between sequences) keeps the pools in FP8: half the bytes per key, twice the keys per pool.  The append methods take the
16-bit rows and quantise them (``ops.quantize_kv``'s rule; ``write_step`` runs the quantising HIP append), ``decode`` runs the FP8 decode
kernel, ``gather`` returns the FP8 pages.  Not built for an FP8 cache, and refused with ``ValueError``: ``prefill``, ``prefill_varlen``,
the rotary form of ``write_step``, and ``decode``'s ``window`` / ``tree_mask`` / ``shared_prefix``.

The kernels behind ``prefill`` / ``prefill_varlen`` do read FP8 pages (``ops.fa3_prefill_cache`` / ``ops.fa3_prefill_varlen`` with
``k_descale=, v_descale=``).  The two methods still refuse an FP8 cache because tests pin that refusal and its text; flipping them is
the follow-up that edits those tests.  Until then ``operands(slots)`` hands out what the calls take:
``k, v, kw = cache.operands(slots); ops.fa3_prefill_cache(q, k, v, **kw)`` is the FP8 prefill over this cache's pages.
"""

from __future__ import annotations

from typing import List, Optional, Sequence, Tuple, Union

import torch

from ... import ops

Slots = Union[None, int, slice, range, Sequence[int]]


class PagedCacheFull(RuntimeError):
    """The pool has no free page (or the cache no free slot, or a sequence no table entry) left for the request."""


class PagedKVCache:
    """One layer's K and V page pools, the block table and the per-slot lengths.

    A *slot* is a row of ``block_table`` / ``cache_seqlens``: ``allocate`` hands one out, ``free`` takes it back with its pages.
    A slot that is not allocated has length 0, so a ``decode`` over all slots returns zeros for it and reads none of its entries.

    ``copy_on_write=True`` adds page sharing: ``fork``, per-page reference counts (``page_refcount``), the copy of a shared, partly
    filled tail page in front of the first write into it, and ``common_prefix``.  The copies an ``advance`` calls for wait in the
    device tensors ``cow_pairs`` / ``cow_rows`` (the pending table) for the ``write_step`` behind it.  Ordering contract: every call
    that changes page ownership -- ``append``, ``append_varlen``, ``advance``, ``fork``, ``free``, ``truncate``,
    ``release_behind_window``, ``swap_pages`` -- first resets the pending table to empty (``advance`` then fills in its own entries), so the ``write_step`` of an
    ``advance`` must be enqueued, on the same stream, before the next such call.  With ``copy_on_write=False`` (the default) nothing
    is shared, no extra tensor exists, no extra launch is made, and ``fork`` raises ``ValueError``.
    """

    def __init__(self, num_pages: int, page_size: int, Hkv: int, D: int, dtype: torch.dtype = torch.bfloat16,
                 device: Union[str, torch.device] = "cuda", max_batch: int = 1, max_pages_per_seq: Optional[int] = None,
                 k_descale: Optional[torch.Tensor] = None, v_descale: Optional[torch.Tensor] = None, copy_on_write: bool = False):
        if page_size < 64 or page_size % 64:
            raise ValueError(f"page size {page_size}: must be a multiple of 64 keys (a key tile of the kernel lies inside one page)")
        if num_pages < 1 or Hkv < 1 or D < 1 or max_batch < 1:
            raise ValueError("num_pages, Hkv, D and max_batch must be positive")
        self.num_pages, self.page_size, self.Hkv, self.D = num_pages, page_size, Hkv, D
        self.max_batch = max_batch
        self.max_pages_per_seq = num_pages if max_pages_per_seq is None else max_pages_per_seq
        if self.max_pages_per_seq < 1:
            raise ValueError("max_pages_per_seq must be positive")
        self.device = torch.device(device)
        self._fp8 = dtype == ops.FP8
        self._kd, self._vd = k_descale, v_descale
        if self._fp8:
            if D % 16:
                raise ValueError(f"head dim {D}: an FP8 cache takes a multiple of 16")
            for name, d in (("k_descale", k_descale), ("v_descale", v_descale)):
                if not isinstance(d, torch.Tensor) or d.dtype != torch.float32 or d.shape != (Hkv,) or not d.is_contiguous() \
                        or d.device.type != self.device.type:
                    raise ValueError(f"an FP8 cache needs {name}: a contiguous fp32 [Hkv] = [{Hkv}] tensor on the cache's device (one scale "
                                     "per K/V head: pages may be shared between sequences)")
        elif k_descale is not None or v_descale is not None:
            raise ValueError("k_descale / v_descale go with dtype=torch.float8_e4m3fn only")
        self._k = torch.zeros(num_pages, page_size, Hkv, D, dtype=dtype, device=self.device)
        self._v = torch.zeros_like(self._k)
        self._table = torch.zeros(max_batch, self.max_pages_per_seq, dtype=torch.int32, device=self.device)
        self._lens = torch.zeros(max_batch, dtype=torch.int32, device=self.device)
        # host mirror
        self._host_lens: List[int] = [0] * max_batch
        self._pages: List[List[int]] = [[] for _ in range(max_batch)]
        self._live: List[bool] = [False] * max_batch
        self._free_pages: List[int] = list(range(num_pages - 1, -1, -1))      # popped from the end: lowest id first
        self._ref: List[int] = [0] * num_pages                                # holders per page; never above 1 without copy_on_write
        self._cow = bool(copy_on_write)
        self._copies: List[Tuple[int, int, int, int]] = []                    # (slot, old page, new page, rows) of the last _grow
        self._cow_pairs = self._cow_rows = None
        self._pending = False                                                 # the device pending table holds an entry
        if self._cow:
            self._cow_pairs = torch.full((max_batch, 2), -1, dtype=torch.int32, device=self.device)
            self._cow_rows = torch.full((max_batch,), -1, dtype=torch.int32, device=self.device)

    # --- device tensors (the same storage for the cache's lifetime) ---------------------------------------------------------------
    @property
    def block_table(self) -> torch.Tensor:
        """int32 ``[max_batch, max_pages_per_seq]``; row = slot.  Entries past a sequence's assigned pages are stale and unread."""
        return self._table

    @property
    def cache_seqlens(self) -> torch.Tensor:
        """int32 ``[max_batch]``: tokens held per slot."""
        return self._lens

    @property
    def cow_pairs(self) -> Optional[torch.Tensor]:
        """int32 ``[max_batch, 2]`` (None without ``copy_on_write``): the pending table's ``(old page, new page)``, row = slot, of the
        copies the last ``advance`` calls for; -1 = none.  ``write_step`` hands it to ``ops.page_copy``."""
        return self._cow_pairs

    @property
    def cow_rows(self) -> Optional[torch.Tensor]:
        """int32 ``[max_batch]`` (None without ``copy_on_write``): the filled rows of each pending copy; -1 = none."""
        return self._cow_rows

    @property
    def k_pool(self) -> torch.Tensor:
        """``[num_pages, page_size, Hkv, D]``"""
        return self._k

    @property
    def v_pool(self) -> torch.Tensor:
        return self._v

    # --- host bookkeeping ---------------------------------------------------------------------------------------------------------
    @property
    def free_pages(self) -> int:
        return len(self._free_pages)

    def length(self, slot: int) -> int:
        return self._host_lens[self._check_slot(slot)]

    def pages(self, slot: int) -> Tuple[int, ...]:
        """The pages assigned to the slot, in logical order (those holding tokens first, then the reserved ones); -1 stands for a
        page ``release_behind_window`` gave back."""
        return tuple(self._pages[self._check_slot(slot)])

    def page_refcount(self, page: int) -> int:
        """Slots holding the page (0: it is free).  Above 1 only with ``copy_on_write``."""
        if not 0 <= page < self.num_pages:
            raise ValueError(f"page {page}: the pool has {self.num_pages}")
        return self._ref[page]

    def _check_slot(self, slot: int) -> int:
        if not 0 <= slot < self.max_batch or not self._live[slot]:
            raise ValueError(f"slot {slot} is not allocated")
        return slot

    def _pages_missing(self, slot: int, n_tokens: int) -> int:
        need = -(-n_tokens // self.page_size)
        if need > self.max_pages_per_seq:
            raise PagedCacheFull(f"{n_tokens} tokens need {need} pages, a sequence's table row has {self.max_pages_per_seq}")
        return max(0, need - len(self._pages[slot]))

    def _assign(self, slot: int, count: int) -> None:
        if count == 0:
            return
        first = len(self._pages[slot])
        new = [self._free_pages.pop() for _ in range(count)]
        for pg in new:
            self._ref[pg] = 1
        self._pages[slot].extend(new)
        self._table[slot, first:first + count] = torch.tensor(new, dtype=torch.int32)

    def _let_go(self, pages) -> None:
        """The slot's hold on each page, in the given order; a page goes back to the pool when no slot holds it any more."""
        for pg in pages:
            self._ref[pg] -= 1
            if self._ref[pg] == 0:
                self._free_pages.append(pg)

    def _reset_pending(self) -> None:
        """Empty the pending table (skipped when the host mirror knows it is empty)."""
        self._copies = []
        if self._pending:
            self._cow_pairs.fill_(-1)
            self._cow_rows.fill_(-1)
            self._pending = False

    def _free_slot(self) -> int:
        for slot in range(self.max_batch):
            if not self._live[slot]:
                return slot
        raise PagedCacheFull(f"all {self.max_batch} slots are in use")

    def allocate(self, n_tokens: int = 0) -> int:
        """Take a free slot and assign it pages for ``n_tokens`` tokens (its length stays 0).  -> slot."""
        slot = self._free_slot()
        self._live[slot] = True
        try:
            self.reserve(slot, n_tokens)
        except PagedCacheFull:
            self._live[slot] = False
            raise
        return slot

    def reserve(self, slot: int, n_tokens: int) -> None:
        """Make sure the slot has pages for ``n_tokens`` tokens in all (e.g. before a graph capture whose replays will append)."""
        self._check_slot(slot)
        missing = self._pages_missing(slot, n_tokens)
        if missing > len(self._free_pages):
            raise PagedCacheFull(f"slot {slot} needs {missing} more pages, the pool has {len(self._free_pages)} free")
        self._assign(slot, missing)

    def free(self, slot: int) -> None:
        """Give the slot back and let go of its pages (those not released already): a page returns to the pool unless another
        slot still holds it (``copy_on_write``).  The pages' contents and the table row stay as they are; the slot reads neither
        again.  Resets the pending copy-on-write table first (see the class's ordering contract)."""
        self._check_slot(slot)
        self._reset_pending()
        self._let_go(pg for pg in reversed(self._pages[slot]) if pg >= 0)
        self._pages[slot] = []
        self._host_lens[slot] = 0
        self._live[slot] = False
        self._lens[slot] = 0

    def truncate(self, slot: int, n_tokens: int) -> None:
        """Take the slot back to its first ``n_tokens`` keys (``0 <= n_tokens <= length(slot)``, else ``ValueError``): the other half
        of a speculative step, which appends a drafted tree's rows, verifies them (``decode(tree_mask=)``) and keeps the accepted
        path only -- ``truncate(slot, L)`` to the length before the step, then ``append_varlen`` of the accepted rows in path order.

        Lets go of every page past ``ceil(n_tokens / page_size)``, reserved ones included (``reserve`` again before a capture that
        needs them); a page another slot holds stays alive (``copy_on_write``).  The table row's stale entries stay as they are, as
        after ``free``: nothing reads them.  A partly filled tail page that is still shared is left shared; the next append copies
        it.  Refused with ``ValueError`` when ``n_tokens > 0`` and the page holding key ``n_tokens - 1`` was released behind a
        window: the slot would end in keys that are gone.  Host bookkeeping plus the device length; works on CPU tensors.  Resets the
        pending copy-on-write table first (see the class's ordering contract).

        The window rule, which is the caller's to keep: once ``release_behind_window(slot, W)`` has let go of ``gone`` pages, pass
        ``n_tokens >= gone * page_size + W - 1``, because the next read of Sq new rows at length L starts at key ``L - Sq - W + 1``, which is
        ``n_tokens - W + 1`` right after this call.  A smaller ``n_tokens`` that this method still accepts makes that read name a ``-1``
        table entry, which the kernels clamp into the pool: wrong numbers and no error."""
        self._check_slot(slot)
        n = n_tokens
        if isinstance(n, bool) or not isinstance(n, int) or not 0 <= n <= self._host_lens[slot]:
            raise ValueError(f"n_tokens must be an integer in 0 .. {self._host_lens[slot]}, the slot's length, got {n_tokens!r}")
        pg = self._pages[slot]
        if n > 0 and pg[(n - 1) // self.page_size] < 0:
            raise ValueError(f"slot {slot}: the page holding key {n - 1} was released behind the window")
        self._reset_pending()
        keep = -(-n // self.page_size)
        self._let_go(p for p in reversed(pg[keep:]) if p >= 0)
        del pg[keep:]
        self._host_lens[slot] = n
        self._lens[slot] = n

    def release_behind_window(self, slot: int, window: int) -> int:
        """Return to the pool every page of the slot that lies wholly behind a sliding window of ``window`` keys: logical page p
        with ``(p + 1) * page_size <= max(0, length(slot) - window + 1)``, the lowest key the sequence's newest row sees.  -> the
        number of entries this slot let go in this call (a page another slot still holds stays alive: ``copy_on_write``).

        The slot keeps its length and logical positions: later appends go where they would have gone and take fresh pages.  The
        released table entries are overwritten with -1 and ``pages()`` reports -1 for them.  Afterwards the slot may only be read
        with ``window=`` this value or smaller, by calls whose query rows are the tokens appended since (one decode row, a chunk,
        a ragged step): such a call's lowest visible key is at or above the bound used here, and the kernels read neither a key
        below that key's 64-key boundary nor its table entry.  ``gather`` and ``swap_pages`` refuse a released page.  Host-side
        bookkeeping plus one small table write; works on CPU tensors.  Resets the pending copy-on-write table first (see the class's
        ordering contract).

        Once this has let go of ``gone`` pages, ``truncate`` and ``fork`` of the slot are the caller's to keep at
        ``n_tokens >= gone * page_size + W - 1``: a later read of Sq new rows at length L starts at key ``L - Sq - W + 1``.  Below that
        bound (``truncate`` itself refuses only a tail page that is gone) the next windowed read names a ``-1`` table entry, which the
        kernels clamp into the pool: wrong numbers and no error."""
        self._check_slot(slot)
        if isinstance(window, bool) or not isinstance(window, int) or window < 1:
            raise ValueError(f"window must be an integer >= 1, got {window!r}")
        pg = self._pages[slot]
        behind = min(max(0, self._host_lens[slot] - window + 1) // self.page_size, len(pg))
        gone = [p for p in range(behind) if pg[p] >= 0]
        if not gone:
            return 0
        self._reset_pending()
        self._let_go(pg[p] for p in reversed(gone))
        for p in gone:
            pg[p] = -1
        self._table[slot, gone[0]:behind] = -1           # every entry in front of it went in an earlier call
        return len(gone)

    def _grow(self, slots: List[int], lens: List[int]) -> List[int]:
        """The host half of an append, all or nothing: assign the pages ``lens[i]`` more tokens of ``slots[i]`` need and advance the
        host lengths.  -> each slot's length before.

        Copy-on-write: a slot that gains a token while its tail page is partly filled and held by another slot as well takes a fresh
        page in its place (counted in the all-or-nothing check) and lets go of the old one; ``(slot, old, new, filled rows)`` is
        recorded in ``_copies`` for the caller to run.  Slots are served in order, so of the holders of one tail page the last keeps it."""
        missing = [self._pages_missing(self._check_slot(s), self._host_lens[s] + x) for s, x in zip(slots, lens)]
        cow, let_go = set(), {}
        if self._cow:
            for s, x in zip(slots, lens):
                n = self._host_lens[s]
                if x > 0 and n % self.page_size:
                    pg = self._pages[s][n // self.page_size]
                    if self._ref[pg] - let_go.get(pg, 0) > 1:
                        let_go[pg] = let_go.get(pg, 0) + 1
                        cow.add(s)
        if sum(missing) + len(cow) > len(self._free_pages):
            raise PagedCacheFull(f"the append needs {sum(missing) + len(cow)} more pages, the pool has {len(self._free_pages)} free")
        self._reset_pending()
        starts = []
        for s, m, x in zip(slots, missing, lens):
            if s in cow:
                p, filled = divmod(self._host_lens[s], self.page_size)
                old, new = self._pages[s][p], self._free_pages.pop()
                self._ref[new] = 1
                self._ref[old] -= 1
                self._pages[s][p] = new
                self._table[s, p] = new
                self._copies.append((s, old, new, filled))
            self._assign(s, m)
            starts.append(self._host_lens[s])
            self._host_lens[s] += x
        return starts

    def _copy_pools(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """The pools as ``ops.page_copy`` takes them.  The copy kernel moves 16-byte pieces and does not care what they hold: FP8 pools
        go as a 2-byte view, ``D / 2`` "elements" a row."""
        if self._fp8:
            return self._k.view(torch.float16).transpose(1, 2), self._v.view(torch.float16).transpose(1, 2)
        return self._k.transpose(1, 2), self._v.transpose(1, 2)

    def _copy_now(self) -> None:
        """Run the copies the last ``_grow`` recorded (``ops.page_copy``, one launch) and forget them."""
        if self._copies:
            pairs = torch.tensor([c[1:3] for c in self._copies], dtype=torch.int32).to(self.device, non_blocking=True)
            rows = torch.tensor([c[3] for c in self._copies], dtype=torch.int32).to(self.device, non_blocking=True)
            ops.page_copy(*self._copy_pools(), pairs, rows=rows)
            self._copies = []

    def _check_new(self, k_new: torch.Tensor, v_new: torch.Tensor) -> None:
        if self._fp8:
            if k_new.dtype not in (torch.bfloat16, torch.float16) or v_new.dtype != k_new.dtype:
                raise ValueError("k_new / v_new must be bf16 or fp16: an FP8 cache quantises the rows it is given")
        elif k_new.dtype != self._k.dtype or v_new.dtype != self._k.dtype:
            raise ValueError("k_new / v_new must have the cache's dtype")

    def _put(self, idx: torch.Tensor, k_rows: torch.Tensor, v_rows: torch.Tensor) -> None:
        """Rows ``[n, Hkv, D]`` to rows ``idx`` of the ``[num_pages * page_size]`` token view; an FP8 cache quantises them first
        (``ops.quantize_kv``'s rule) and moves bytes."""
        rows = self.num_pages * self.page_size
        for pool, x, d in ((self._k, k_rows, self._kd), (self._v, v_rows, self._vd)):
            if self._fp8:
                x8 = (x.to(torch.float32) / d[None, :, None]).clamp(-ops.FP8_MAX, ops.FP8_MAX).to(ops.FP8)
                pool.view(torch.uint8).view(rows, self.Hkv, self.D).index_copy_(0, idx, x8.view(torch.uint8))
            else:
                pool.view(rows, self.Hkv, self.D).index_copy_(0, idx, x)

    def _dst_rows(self, slots: List[int], starts: List[int], lens: List[int]) -> List[int]:
        """Row of the ``[num_pages * page_size]`` token view each appended token goes to."""
        return [self._pages[s][j // self.page_size] * self.page_size + j % self.page_size
                for s, at, x in zip(slots, starts, lens) for j in range(at, at + x)]

    def append(self, slots: Union[int, Sequence[int]], k_new: torch.Tensor, v_new: torch.Tensor) -> None:
        """Write ``k_new`` / ``v_new`` ``[n, Hkv, Sq, D]`` at the current end of each of the ``n`` slots and advance their lengths.
        Pages are assigned as needed; if the pool cannot serve all of them nothing is written and ``PagedCacheFull`` is raised.
        With ``copy_on_write`` a shared, partly filled tail page is copied to a fresh page first (``ops.page_copy``), and the pending
        table is reset (see the class's ordering contract)."""
        slots = [slots] if isinstance(slots, int) else list(slots)
        n = len(slots)
        if len(set(slots)) != n:
            raise ValueError("a slot may appear once per append")
        if k_new.dim() != 4 or k_new.shape[:2] != (n, self.Hkv) or k_new.shape[3] != self.D or v_new.shape != k_new.shape:
            raise ValueError(f"k_new / v_new must be [{n}, {self.Hkv}, Sq, {self.D}], got {tuple(k_new.shape)} / {tuple(v_new.shape)}")
        self._check_new(k_new, v_new)
        Sq = k_new.shape[2]
        dst = self._dst_rows(slots, self._grow(slots, [Sq] * n), [Sq] * n)
        self._copy_now()
        if Sq:
            idx = torch.tensor(dst, dtype=torch.int64).to(self.device, non_blocking=True)
            self._put(idx, k_new.permute(0, 2, 1, 3).reshape(n * Sq, self.Hkv, self.D), v_new.permute(0, 2, 1, 3).reshape(n * Sq, self.Hkv, self.D))
        self._lens.copy_(torch.tensor(self._host_lens, dtype=torch.int32), non_blocking=True)

    def append_varlen(self, slots: Union[int, Sequence[int]], k_new: torch.Tensor, v_new: torch.Tensor, lens: Sequence[int]) -> None:
        """``append`` for a different number of tokens per slot: ``k_new`` / ``v_new`` are packed ``[total, Hkv, D]``, slot
        ``slots[i]`` takes the next ``lens[i]`` tokens (a host list, 0 allowed; ``sum(lens) == total``) at its current end.  All or
        nothing: if the pool cannot serve every slot nothing is written and ``PagedCacheFull`` is raised.  Copy-on-write as in
        ``append``."""
        slots = [slots] if isinstance(slots, int) else list(slots)
        lens = [int(x) for x in lens]
        n, total = len(slots), sum(lens)
        if len(set(slots)) != n:
            raise ValueError("a slot may appear once per append")
        if len(lens) != n or any(x < 0 for x in lens):
            raise ValueError(f"lens must hold one non-negative token count per slot, got {lens} for {n} slots")
        if k_new.dim() != 3 or k_new.shape != (total, self.Hkv, self.D) or v_new.shape != k_new.shape:
            raise ValueError(f"k_new / v_new must be [{total}, {self.Hkv}, {self.D}], got {tuple(k_new.shape)} / {tuple(v_new.shape)}")
        self._check_new(k_new, v_new)
        dst = self._dst_rows(slots, self._grow(slots, lens), lens)
        self._copy_now()
        if total:
            idx = torch.tensor(dst, dtype=torch.int64).to(self.device, non_blocking=True)
            self._put(idx, k_new, v_new)
        self._lens.copy_(torch.tensor(self._host_lens, dtype=torch.int32), non_blocking=True)

    def advance(self, slots: Union[int, Sequence[int]], lens: Sequence[int]) -> None:
        """The host half of ``append_varlen``: slot ``slots[i]`` grows by ``lens[i]`` tokens (a host list, 0 allowed).  Assigns the
        pages, updates the host mirror and refreshes the device table and lengths in place; moves no K / V.  All or nothing: if the
        pool cannot serve every slot nothing changes and ``PagedCacheFull`` is raised.  ``write_step`` is the device half:
        ``advance(slots, lens)`` followed by ``write_step(k_new, v_new, lens, slots)`` equals ``append_varlen(slots, k_new, v_new,
        lens)``.  A graph user captures ``write_step`` + ``prefill_varlen`` once and calls ``advance`` between replays.

        With ``copy_on_write`` the copies of shared tail pages this step calls for are written, whole and in place, into ``cow_pairs``
        / ``cow_rows`` (row = slot) for ``write_step`` to run; the table is reset first.  Ordering contract: enqueue this step's
        ``write_step``, on the same stream, before the next call that changes page ownership (``append``, ``append_varlen``,
        ``advance``, ``fork``, ``free``, ``truncate``, ``release_behind_window``, ``swap_pages``): each of them empties the pending
        table."""
        slots = [slots] if isinstance(slots, int) else list(slots)
        lens = [int(x) for x in lens]
        if len(set(slots)) != len(slots):
            raise ValueError("a slot may appear once per append")
        if len(lens) != len(slots) or any(x < 0 for x in lens):
            raise ValueError(f"lens must hold one non-negative token count per slot, got {lens} for {len(slots)} slots")
        self._grow(slots, lens)
        if self._copies:
            pairs, rows = [[-1, -1] for _ in range(self.max_batch)], [-1] * self.max_batch
            for s, old, new, filled in self._copies:
                pairs[s], rows[s] = [old, new], filled
            self._cow_pairs.copy_(torch.tensor(pairs, dtype=torch.int32), non_blocking=True)
            self._cow_rows.copy_(torch.tensor(rows, dtype=torch.int32), non_blocking=True)
            self._pending = True
            self._copies = []
        self._lens.copy_(torch.tensor(self._host_lens, dtype=torch.int32), non_blocking=True)

    def fork(self, slot: int, n_tokens: Optional[int] = None) -> int:
        """Take a free slot whose first ``n_tokens`` keys (default: all, ``0 <= n_tokens <= length(slot)``) are those of ``slot``, by
        sharing the ``ceil(n_tokens / page_size)`` pages that hold them: their counts go up, released ``-1`` entries carry over,
        pages the parent has only reserved are not shared.  Writes the child's table row and length in place; needs no free page and
        moves no K / V -- the first append into a shared, partly filled tail page copies it (``_grow``).  -> the new slot.
        ``PagedCacheFull`` when no slot is free; ``ValueError`` without ``copy_on_write``.  Resets the pending copy-on-write table
        first (see the class's ordering contract).

        The window rule of ``truncate`` holds for the child: when the parent has released ``gone`` pages behind a window W, pass
        ``n_tokens >= gone * page_size + W - 1`` (so never 0), or the child's first read of new rows starts in a released page.  Nothing
        here refuses a smaller value: that read names a ``-1`` entry, which the kernels clamp into the pool -- wrong numbers, no error."""
        if not self._cow:
            raise ValueError("fork needs PagedKVCache(copy_on_write=True)")
        self._check_slot(slot)
        n = self._host_lens[slot] if n_tokens is None else n_tokens
        if isinstance(n, bool) or not isinstance(n, int) or not 0 <= n <= self._host_lens[slot]:
            raise ValueError(f"n_tokens must be an integer in 0 .. {self._host_lens[slot]}, the parent's length, got {n_tokens!r}")
        child = self._free_slot()
        self._reset_pending()
        shared = self._pages[slot][:-(-n // self.page_size)]
        for pg in shared:
            if pg >= 0:
                self._ref[pg] += 1
        self._live[child] = True
        self._pages[child] = list(shared)
        self._host_lens[child] = n
        if shared:
            self._table[child, :len(shared)] = torch.tensor(shared, dtype=torch.int32)
        self._lens[child] = n
        return child

    def common_prefix(self, slots: Sequence[int]) -> int:
        """The largest multiple of ``page_size`` such that every slot in ``slots`` has the same physical pages below it, none of them
        released, and a length at or above it -- what ``decode(q, slots, shared_prefix=...)`` asks of its batch; forks of one parent
        have it.  0 when there is none (``shared_prefix=0`` is refused, so check).  Host only."""
        slots = [self._check_slot(s) for s in slots]
        if not slots:
            raise ValueError("no slots")
        first, p = self._pages[slots[0]], 0
        while all((p + 1) * self.page_size <= self._host_lens[s] for s in slots) and first[p] >= 0 \
                and all(self._pages[s][p] == first[p] for s in slots):
            p += 1
        return p * self.page_size

    def swap_pages(self, slot: int, i: int, j: int) -> None:
        """Exchange the physical pages behind logical pages ``i`` and ``j`` of the slot, moving their contents with them (what a
        compaction does); the sequence reads the same afterwards.  A page another slot holds as well (``copy_on_write``) is refused:
        moving it would have to rewrite the other slots' rows.  Resets the pending copy-on-write table first."""
        pg = self._pages[self._check_slot(slot)]
        if not (0 <= i < len(pg) and 0 <= j < len(pg)):
            raise ValueError(f"slot {slot} has {len(pg)} pages")
        if pg[i] < 0 or pg[j] < 0:
            raise ValueError(f"slot {slot}: page {i if pg[i] < 0 else j} was released behind the window")
        if self._ref[pg[i]] > 1 or self._ref[pg[j]] > 1:
            raise ValueError(f"slot {slot}: page {i if self._ref[pg[i]] > 1 else j} is shared with another slot")
        if i == j:
            return
        self._reset_pending()
        a, b = pg[i], pg[j]
        for pool in (self._k, self._v):
            tmp = pool[a].clone()
            pool[a].copy_(pool[b])
            pool[b].copy_(tmp)
        pg[i], pg[j] = b, a
        self._table[slot, i] = b
        self._table[slot, j] = a

    def gather(self, slot: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """The slot's K and V as contiguous ``[Hkv, len, D]`` tensors of the cache's dtype (tests, debugging)."""
        n = self._host_lens[self._check_slot(slot)]
        if any(p < 0 for p in self._pages[slot][:-(-n // self.page_size)]):
            raise ValueError(f"slot {slot}: its first pages were released behind the window, their keys are gone")
        pg = torch.tensor(self._pages[slot][:-(-n // self.page_size)], dtype=torch.int64).to(self.device)
        out = []
        for pool in (self._k, self._v):
            raw = pool.view(torch.uint8) if self._fp8 else pool            # an FP8 cache: bytes in, the FP8 pages out
            out.append(raw.index_select(0, pg).reshape(-1, self.Hkv, self.D)[:n].permute(1, 0, 2).contiguous().view(pool.dtype))
        return out[0], out[1]

    # --- the kernel ---------------------------------------------------------------------------------------------------------------
    def _rows(self, slots: Slots) -> Tuple[torch.Tensor, torch.Tensor]:
        if slots is None:
            return self._table, self._lens
        if isinstance(slots, int):
            slots = range(slots, slots + 1)
        if isinstance(slots, slice):
            slots = range(*slots.indices(self.max_batch))
        slots = list(slots)
        if not slots:
            raise ValueError("no slots")
        if slots == list(range(slots[0], slots[0] + len(slots))) and 0 <= slots[0] and slots[-1] < self.max_batch:
            return self._table[slots[0]:slots[-1] + 1], self._lens[slots[0]:slots[-1] + 1]     # views: capturable
        idx = torch.tensor(slots, dtype=torch.int64).to(self.device)
        return self._table.index_select(0, idx), self._lens.index_select(0, idx)

    def operands(self, slots: Slots = None) -> Tuple[torch.Tensor, torch.Tensor, dict]:
        """``(k_cache, v_cache, kw)`` as the calls of ``ops`` over a paged cache take them: the pools as ``[num_pages, Hkv, page_size,
        D]``-shaped views and ``kw = dict(cache_seqlens=, block_table=)``, plus ``k_descale=, v_descale=`` for an FP8 cache.  Slots are
        chosen and captured as in ``decode``: None and a run of consecutive slots give views of the cache's own table and lengths (a
        captured call keeps seeing them), any other list a copy of its rows.  ``ops.fa3_prefill_cache(q, k, v, **kw)`` and
        ``ops.fa3_prefill_varlen(q, k, v, cu_seqlens_q=..., max_seqlen_q=..., **kw)`` are then the prefill over this cache's pages,
        FP8 included.  Works on CPU tensors (the calls themselves need the device)."""
        table, lens = self._rows(slots)
        kw = dict(cache_seqlens=lens, block_table=table)
        if self._fp8:
            kw.update(k_descale=self._kd, v_descale=self._vd)
        return self._k.transpose(1, 2), self._v.transpose(1, 2), kw

    def _cu(self, q_lens, cu_seqlens_q, max_seqlen_q, n_slots: int, rows: int, what: str):
        """A ragged step's ``(cu_seqlens_q, max_seqlen_q)``: the caller's device tensor and bound, or the prefix sums of the host
        list ``q_lens`` (a non-blocking copy) with ``max(q_lens)`` unless a bound is given."""
        if (q_lens is None) == (cu_seqlens_q is None):
            raise ValueError("give either q_lens (a host list) or cu_seqlens_q (a device tensor) with max_seqlen_q")
        if cu_seqlens_q is None:
            q_lens = [int(x) for x in q_lens]
            if len(q_lens) != n_slots or any(x < 0 for x in q_lens):
                raise ValueError(f"q_lens must hold one non-negative row count per slot, got {q_lens} for {n_slots} slots")
            cu = [0]
            for x in q_lens:
                cu.append(cu[-1] + x)
            if cu[-1] > rows or cu[-1] < 1:
                raise ValueError(f"q_lens name {cu[-1]} rows, {what} has {rows}")
            cu_seqlens_q = torch.tensor(cu, dtype=torch.int32).to(self.device, non_blocking=True)
            if max_seqlen_q is None:
                max_seqlen_q = max(q_lens)
        elif max_seqlen_q is None:
            raise ValueError("cu_seqlens_q needs max_seqlen_q, the host bound on a sequence's rows (it sizes the grid)")
        return cu_seqlens_q, max_seqlen_q

    def write_step(self, k_new: torch.Tensor, v_new: torch.Tensor, q_lens: Optional[Sequence[int]] = None, slots: Slots = None, *,
                   cu_seqlens_q: Optional[torch.Tensor] = None, max_seqlen_q: Optional[int] = None, q: Optional[torch.Tensor] = None,
                   rotary_cos: Optional[torch.Tensor] = None, rotary_sin: Optional[torch.Tensor] = None, rotary_interleaved: bool = False,
                   pos_offsets: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
        """The device half of an append (``ops.kv_append``, one launch of the HIP copy kernel): write the packed ``k_new`` / ``v_new``
        ``[total, Hkv, D]`` of a ragged step to where the cache's own table and lengths say, sequence i bringing ``q_lens[i]`` rows.
        Call ``advance`` first: the lengths count the step's rows, and row j of sequence i goes to key ``length - q_lens[i] + j``.  Does
        no bookkeeping, so ``advance(slots, lens)`` + ``write_step(k_new, v_new, lens, slots)`` equals ``append_varlen``.  Slots are
        chosen and captured as in ``decode``; a host list ``q_lens``, or a device ``cu_seqlens_q`` (int32 ``[len(slots) + 1]``) plus
        the ``max_seqlen_q`` bound, as in ``prefill_varlen`` -- the form a graph captures, next to ``prefill_varlen``, and replays
        while ``advance`` and in-place updates of ``cu_seqlens_q`` and the inputs happen in between.  Also runs on CPU tensors.

        With ``rotary_cos=, rotary_sin=`` (and ``rotary_interleaved``, ``pos_offsets`` -- int32, one per slot of the call) the launch is
        ``ops.rope_append`` instead: the K rows are rotated at the positions they are written to, and the packed ``q [total, H, D]``, if
        given, is rotated into a fresh buffer that is returned (else None): the tensor ``prefill_varlen`` then takes.

        With ``copy_on_write`` one ``ops.page_copy`` over the pending table (``cow_pairs`` / ``cow_rows``, whatever slots the call
        names) is enqueued in front: the copies the last ``advance`` calls for, or nothing when the table is empty.  It reads the
        device table, so a captured ``write_step`` + attention replays through forks."""
        rotary = rotary_cos is not None or rotary_sin is not None
        if self._fp8 and (rotary or q is not None):
            raise ValueError("write_step: rotary is not fused into the quantising append of an FP8 cache; rotate q and k_new first")
        if not rotary and (q is not None or rotary_interleaved or pos_offsets is not None):
            raise ValueError("q, rotary_interleaved and pos_offsets need rotary_cos and rotary_sin")
        if rotary and (rotary_cos is None or rotary_sin is None):
            raise ValueError("rotary_cos and rotary_sin go together")
        table, lens = self._rows(slots)
        if cu_seqlens_q is None and q_lens is not None and len(q_lens) == table.shape[0] and not any(q_lens):
            return None if q is None else torch.empty_like(q)   # a step without rows, as append_varlen takes one
        cu_seqlens_q, max_seqlen_q = self._cu(q_lens, cu_seqlens_q, max_seqlen_q, table.shape[0], k_new.shape[0], "k_new")
        if self._cow:
            ops.page_copy(*self._copy_pools(), self._cow_pairs, rows=self._cow_rows)
        if rotary:
            return ops.rope_append(k_new, v_new, self._k.transpose(1, 2), self._v.transpose(1, 2), cache_seqlens=lens,
                                   rotary_cos=rotary_cos, rotary_sin=rotary_sin, q=q, rotary_interleaved=rotary_interleaved,
                                   pos_offsets=pos_offsets, cu_seqlens_q=cu_seqlens_q, max_seqlen_q=max_seqlen_q, block_table=table)
        ops.kv_append(k_new, v_new, self._k.transpose(1, 2), self._v.transpose(1, 2), cache_seqlens=lens, cu_seqlens_q=cu_seqlens_q,
                      max_seqlen_q=max_seqlen_q, block_table=table, k_descale=self._kd, v_descale=self._vd)

    def decode(self, q: torch.Tensor, slots: Slots = None, **kw):
        """``ops.fa3_decode`` of ``q [B, H, Sq, D]`` against the sequences in ``slots`` (batch row i reads slot ``slots[i]``; None:
        all ``max_batch`` slots in order).  None and a run of consecutive slots read the cache's own table and lengths, so the
        call can be captured in a graph and replayed while the cache changes; any other list takes a copy of its rows first.
        Keyword arguments (``causal``, ``key_mask`` over ``max_pages_per_seq * page_size`` logical keys, ``out_dtype``,
        ``window`` -- the sliding window, required once ``release_behind_window`` has given pages back --, ``tree_mask`` -- int64
        ``[B, Sq]`` words that verify a drafted token tree, ``ops.tree_mask_from_parents``; ``truncate`` then takes the rejected rows
        back --, ``sinks`` -- fp32 ``[H]`` attention sinks, one per query head --, ...) pass through.  -> ``(o, lse)``."""
        table, lens = self._rows(slots)
        if self._fp8:                                                      # the cache's own scales; the refused keywords raise in ops
            kw = dict(kw, k_descale=self._kd, v_descale=self._vd)
        return ops.fa3_decode(q, self._k.transpose(1, 2), self._v.transpose(1, 2), cache_seqlens=lens, block_table=table, **kw)

    def prefill(self, q: torch.Tensor, slots: Slots = None, **kw):
        """``ops.fa3_prefill_cache`` of ``q [B, H, Sq, D]`` (any Sq: a prompt chunk, the suffix behind shared prefix pages, a
        speculative step) against the sequences in ``slots``, which are chosen and captured as in ``decode``.  ``append`` the rows'
        own K / V first: the lengths count them, and ``causal`` (the default) is bottom-right aligned.  Keyword arguments
        (``causal``, ``out_dtype``, ``return_lse``, ``out``, ``window``, ``sinks``, ...) pass through.  -> ``(o, lse)``."""
        if self._fp8:
            raise ValueError("prefill over an FP8 cache is not built: run the dense forward on the prompt's 16-bit K / V and append them")
        table, lens = self._rows(slots)
        return ops.fa3_prefill_cache(q, self._k.transpose(1, 2), self._v.transpose(1, 2), cache_seqlens=lens, block_table=table, **kw)

    def prefill_varlen(self, q: torch.Tensor, q_lens: Optional[Sequence[int]] = None, slots: Slots = None, *,
                       cu_seqlens_q: Optional[torch.Tensor] = None, max_seqlen_q: Optional[int] = None, **kw):
        """``ops.fa3_prefill_varlen`` of the packed ``q [total_q, H, D]`` against the sequences in ``slots`` (chosen and captured as
        in ``decode``): sequence i brings ``q_lens[i]`` rows, one step of continuous batching in one launch.  ``append_varlen`` the
        rows' own K / V first.  A host list ``q_lens`` becomes a device ``cu_seqlens_q`` by a non-blocking copy, with
        ``max_seqlen_q = max(q_lens)`` unless given; a caller that captures graphs passes its own device ``cu_seqlens_q`` (int32
        ``[len(slots) + 1]``, updated in place between replays) and the ``max_seqlen_q`` bound instead.  Keyword arguments
        (``causal``, ``out_dtype``, ``return_lse``, ``out``, ``window``, ``sinks``, ...) pass through.  -> ``(o [total_q, H, D], lse [H, total_q])``."""
        if self._fp8:
            raise ValueError("prefill_varlen over an FP8 cache is not built: run the dense forward on the 16-bit K / V and append them")
        table, lens = self._rows(slots)
        cu_seqlens_q, max_seqlen_q = self._cu(q_lens, cu_seqlens_q, max_seqlen_q, table.shape[0], q.shape[0], "q")
        return ops.fa3_prefill_varlen(q, self._k.transpose(1, 2), self._v.transpose(1, 2), cu_seqlens_q=cu_seqlens_q,
                                      max_seqlen_q=max_seqlen_q, cache_seqlens=lens, block_table=table, **kw)

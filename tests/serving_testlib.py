"""Serving traces: a long random session on one ``PagedKVCache`` against a dense model of what the cache should hold.  Plain functions
and classes; pytest collects nothing from here.  tests/test_serving_testlib.py runs the traces on CPU tensors with a stand-in attention
and with caches and stand-ins that are wrong in one way each; tests/test_hip_serving_trace.py runs them through the HIP kernels.

  ``Seq`` / the model       per live slot the appended K and V rows as dense ``[n, Hkv, D]`` tensors of the 16-bit dtype, the number of
                            leading pages released behind a window (``gone``) and the number of table entries the slot holds (``cap``).
                            No pages, no table, no sharing: a fork copies the rows.
  ``Session``               the seeded generator (``random.Random(seed)`` for every choice, a CPU ``torch.Generator`` for the data), the
                            driver that applies each operation to the cache and to the model, the poison rule and the checks.  The
                            attention functions come in as ``calls``: ``decode(cache, q, slots, **kw)``, ``prefill(cache, q, slots,
                            **kw)`` and ``prefill_varlen(cache, q, q_lens, slots, **kw)`` -- ``GPU_CALLS`` are the cache's own methods.

The operations are the cache's public methods only: ``new`` (``allocate`` and a prompt of 1 .. 200 rows, in one piece or in chunks),
``step`` (a random subset of the live slots in random order gains ``GAINS`` rows each, through ``advance`` + ``write_step`` or through
``append_varlen``, and the rows are read back by an attention call), ``fork``, ``free``, ``truncate``, ``release`` (windowed sessions),
``swap`` (two pages of one slot that are neither shared nor released), ``reserve`` and ``spec`` (non-windowed 16-bit sessions: append a
drafted tree of 2 .. 8 nodes, ``decode(tree_mask=)``, ``truncate`` to the length before, ``append_varlen`` one root-to-leaf path).  An
operation that is impossible when drawn (no live slot, no free slot, no two swappable pages) is redrawn and counted in ``redraws``.

The contracts the generator keeps are those of the docstrings: ``write_step`` directly behind its ``advance``; a windowed slot is read
with ``window=W`` by the rows appended since.  And the window rule of ``truncate`` / ``fork``: once ``release_behind_window(slot, W)`` has
let go of ``gone`` pages, ``n_tokens >= gone * page_size + W - 1`` -- the next read of Sq new rows at length L starts at key
``L - Sq - W + 1 = n_tokens - W + 1``, which must not lie in a released page.  ``assert_read_range_is_named`` checks that on every read.

The poison rule: the pools start as NaN (an FP8 pool as the byte 0x7f) and after every operation every page whose reference count is 0
is refilled with NaN, and so are the rows behind the new end of a truncated slot's tail page when nobody else holds it.  A read
through a stale entry, a released entry or a freed page comes back non-finite, which ``check_out`` refuses.

The checks, after every operation, from the DEVICE tensors:
  1  ``cache_seqlens[slot]`` is the model's length for a live slot and 0 for the others;
  2  every key of every live slot from its first unreleased page on is bit-equal to the model's rows -- the page ``block_table`` names,
     the row the layout says, the pools read directly; an FP8 cache holds the bytes of ``ops.quantize_kv`` of the model's rows;
  3  ``page_refcount(p)`` is the number of live slots whose table row names p, ``free_pages`` the number of pages nobody names, the
     released entries are -1 and ``pages(slot)`` is the table row;
  4  a ``PagedCacheFull`` leaves ``pages()``, ``length()``, ``free_pages``, the table and the lengths as they were;
  5  every read is within ``check_out`` / ``check_lse`` of ``kvcache_testlib.reference`` over the model's dense rows (``with_sink`` for
     sinks, ``folded_reference`` for the tree step; an FP8 session's reference runs over ``dequantize_kv`` of the quantised rows).
A failed check raises ``AssertionError`` whose text starts with ``check N``."""

from __future__ import annotations

import collections
import random

import torch

from kvcache_testlib import EPS, FP8, INF, NAN, NANB, check_lse, check_out, folded_reference, reference, with_sink
from photonic_flash_attention_amd import ops
from photonic_flash_attention_amd.integration.pytorch import PagedCacheFull, PagedKVCache

PROMPTS = (1, 37, 64, 65, 100, 128, 200)                   # both sides of a page of 64 and of 128
GAINS = (0, 1, 1, 1, 3, 17, 70)
WEIGHTS = dict(new=10, step=40, fork=10, free=7, truncate=8, release=8, swap=3, reserve=4, spec=5)
GPU_CALLS = dict(decode=PagedKVCache.decode, prefill=PagedKVCache.prefill, prefill_varlen=PagedKVCache.prefill_varlen)


def ceil_div(a, b):
    return -(-a // b)


class Seq:
    """One live slot of the model: ``k`` / ``v`` the appended rows ``[n, Hkv, D]`` (CPU, 16-bit), ``ek`` / ``ev`` the bits the cache
    must hold for them (on the cache's device: int16, or the bytes of an FP8 cache), ``rk`` / ``rv`` the values the cache stands for
    (on the cache's device: the rows, or fp64 ``dequantize_kv`` of the bytes)."""

    def __init__(self, parts, gone=0, cap=0):
        self.k, self.v, self.ek, self.ev, self.rk, self.rv = parts
        self.gone, self.cap = gone, cap

    def __len__(self):
        return self.k.shape[0]

    def first(self, n, gone, cap):
        return Seq([t[:n].clone() for t in (self.k, self.v, self.ek, self.ev, self.rk, self.rv)], gone, cap)

    def extend(self, parts):
        self.k, self.v, self.ek, self.ev, self.rk, self.rv = (torch.cat([a, b]) for a, b in zip(
            (self.k, self.v, self.ek, self.ev, self.rk, self.rv), parts))


class Session:
    """One trace: ``Session(cache, calls, seed, H=...)``, then ``run(n_ops)``.  mode: "plain" (every step read with ``prefill_varlen``,
    sinks on about half of the reads; a step of one row each also with ``decode``; stepped slots behind a common prefix also with
    ``decode(shared_prefix=)``), "window" (needs ``window=W``; every read takes it, through ``prefill_varlen``, ``decode`` and ``prefill``
    in turn) or "fp8" (``decode`` of the last 1 .. 4 rows of what each slot gained).  skip: check numbers left out (the CPU tests of the
    mutants use it to show what a later check sees).  Counts: ``counts`` (operations done, by kind; ``refused_full``; ``pending_copies``,
    the copies that went through the device pending table; ``releases``, those that let go of a page), ``reads`` (by call), ``draws`` /
    ``redraws``, ``worst_ratio`` (error over ``check_out``'s bound) and ``worst_lse``."""

    def __init__(self, cache, calls, seed, *, H, mode="plain", window=None, weights=None, gains=GAINS, skip=()):
        assert mode in ("plain", "window", "fp8") and (mode == "window") == (window is not None)
        self.cache, self.calls, self.H, self.mode, self.W, self.gains, self.skip = cache, calls, H, mode, window, gains, set(skip)
        self.rng = random.Random(seed)
        self.gen = torch.Generator().manual_seed(seed)
        self.fp8 = cache.k_pool.dtype == FP8
        assert self.fp8 == (mode == "fp8")
        self.dtype = torch.bfloat16 if self.fp8 else cache.k_pool.dtype                       # of the appended rows and of q
        self.dev, self.page, self.NP = cache.device, cache.page_size, cache.num_pages
        w = dict(WEIGHTS if weights is None else weights)
        if mode != "window":
            w.pop("release", None)
        if mode != "plain":
            w.pop("spec", None)
        self.kinds, self.weights = list(w), [w[k] for k in w]
        self.model = {}
        self.counts, self.reads = collections.Counter(), collections.Counter()
        self.draws = self.redraws = self.n_ops = self.n_reads = 0
        self.worst_ratio = self.worst_lse = 0.0
        self.log = []
        self.step_hows = ("device", "varlen")
        self.poison()

    # --- data ----------------------------------------------------------------------------------------------------------------------
    def rows(self, n):
        """n new K and V rows ``[n, Hkv, D]`` of the 16-bit dtype on the CPU."""
        c = self.cache
        return tuple(torch.randn(n, c.Hkv, c.D, generator=self.gen).to(self.dtype) for _ in range(2))

    def queries(self, B, Sq):
        """q as a ``[B, H, Sq, D]`` view of a ``[B, Sq, H, D]`` buffer on the cache's device."""
        return torch.randn(B, Sq, self.H, self.cache.D, generator=self.gen).to(self.dtype).to(self.dev).permute(0, 2, 1, 3)

    def parts(self, k, v):
        """The six tensors of ``Seq`` for rows k, v."""
        if not self.fp8:
            kd, vd = k.to(self.dev), v.to(self.dev)
            return k, v, kd.view(torch.int16), vd.view(torch.int16), kd, vd
        c = self.cache
        out = [k, v]
        scales = [c.operands()[2][n].cpu() for n in ("k_descale", "v_descale")]
        q8 = [ops.quantize_kv(x.permute(1, 0, 2)[None].float(), d) for x, d in zip((k, v), scales)]               # [1, Hkv, n, D]
        out += [x[0].permute(1, 0, 2).contiguous().view(torch.uint8).to(self.dev) for x in q8]
        out += [ops.dequantize_kv(x, d, torch.float64)[0].permute(1, 0, 2).contiguous().to(self.dev) for x, d in zip(q8, scales)]
        return tuple(out)

    # --- the poison rule -------------------------------------------------------------------------------------------------------------
    def _raw(self, pool):
        return pool.view(torch.uint8) if self.fp8 else pool

    def poison(self):
        c = self.cache
        free = [p for p in range(self.NP) if c.page_refcount(p) == 0]
        if free:
            idx = torch.tensor(free, dtype=torch.int64).to(self.dev)
            for pool in (c.k_pool, c.v_pool):
                self._raw(pool).index_fill_(0, idx, NANB if self.fp8 else NAN)

    def poison_tail(self, slot):
        """The rows behind the end of the slot's tail page, when no other slot holds the page: a call must never read them."""
        c, n = self.cache, len(self.model[slot])
        if n % self.page:
            pg = c.pages(slot)[n // self.page]
            if pg >= 0 and c.page_refcount(pg) == 1:
                for pool in (c.k_pool, c.v_pool):
                    self._raw(pool)[pg, n % self.page:] = NANB if self.fp8 else NAN

    # --- checks 1 - 4 ----------------------------------------------------------------------------------------------------------------
    def after(self, what):
        """What follows every operation: the poison rule, then checks 1, 2, 3."""
        self.poison()
        self.log.append(what)
        c, m = self.cache, self.model
        table, lens = c.block_table.cpu(), c.cache_seqlens.cpu().tolist()
        tag = f"after op {self.n_ops} ({what})"
        if 1 not in self.skip:
            want = [len(m[s]) if s in m else 0 for s in range(c.max_batch)]
            assert lens == want, f"check 1 (device lengths) {tag}: cache_seqlens {lens}, the model has {want}"
        if 2 not in self.skip:
            flat = [self._raw(pool).view(self.NP * self.page, c.Hkv, c.D) for pool in (c.k_pool, c.v_pool)]
            for s, seq in m.items():
                lo, n = seq.gone * self.page, len(seq)
                if n <= lo:
                    continue
                j = torch.arange(lo, n)
                pg = table[s, j // self.page].long()
                assert bool(((pg >= 0) & (pg < self.NP)).all()), f"check 2 (contents) {tag}: slot {s}'s table row names no page for a key"
                idx = (pg * self.page + j % self.page).to(self.dev)
                for name, pool, want in (("K", flat[0], seq.ek), ("V", flat[1], seq.ev)):
                    got = pool.index_select(0, idx)
                    got = got if self.fp8 else got.view(torch.int16)
                    if not torch.equal(got, want[lo:]):
                        bad = int((got != want[lo:]).flatten(1).any(1).nonzero()[0]) + lo
                        raise AssertionError(f"check 2 (contents) {tag}: slot {s}, {name} differs from the model's rows, first at key {bad} of {n}")
        if 3 not in self.skip:
            named = collections.Counter()
            for s, seq in m.items():
                row = table[s, :seq.cap].tolist()
                assert tuple(row) == c.pages(s), f"check 3 (ownership) {tag}: slot {s}'s table row {row}, pages() {c.pages(s)}"
                assert all(e == -1 for e in row[:seq.gone]) and all(0 <= e < self.NP for e in row[seq.gone:]), \
                    f"check 3 (ownership) {tag}: slot {s}'s table row {row} with {seq.gone} released pages"
                named.update(row[seq.gone:])
            counts = [c.page_refcount(p) for p in range(self.NP)]
            assert counts == [named[p] for p in range(self.NP)], \
                f"check 3 (ownership) {tag}: reference counts {counts}, live table rows name {[named[p] for p in range(self.NP)]}"
            assert c.free_pages == self.NP - len(named), f"check 3 (ownership) {tag}: {c.free_pages} free pages, {self.NP - len(named)} unnamed"

    def _snapshot(self):
        c = self.cache
        host = [(c.pages(s), c.length(s)) if s in self.model else None for s in range(c.max_batch)]
        return host, c.free_pages, c.block_table.clone(), c.cache_seqlens.clone()

    def guarded(self, what, fn):
        """``fn()`` -> (True, its result), or (False, None) after a ``PagedCacheFull`` that left everything as it was (check 4)."""
        snap = self._snapshot()
        try:
            return True, fn()
        except PagedCacheFull:
            now = self._snapshot()
            same = snap[:2] == now[:2] and torch.equal(snap[2], now[2]) and torch.equal(snap[3], now[3])
            assert same or 4 in self.skip, f"check 4 (refused-full) at op {self.n_ops} ({what}): the refusal changed the cache"
            self.counts["refused_full"] += 1
            self.after(what + " refused")
            return False, None

    # --- check 5: the reads -------------------------------------------------------------------------------------------------------------
    def assert_read_range_is_named(self, slot, Sq):
        """The generator's own promise: no released entry in the range a read of the slot's last Sq rows may touch."""
        seq = self.model[slot]
        lo = max(0, len(seq) - Sq - self.W + 1) if self.W is not None else 0
        assert lo >= seq.gone * self.page, f"the generator drew a read of slot {slot} from key {lo} with {seq.gone} pages released"

    def reference_of(self, slot, q1, sinks=None, words=None):
        """fp64 ``(o [1,H,Sq,D], lse [1,H,Sq], pnorm [1,H,Sq,1])`` of ``q1 [1,H,Sq,D]`` over the model's rows of the slot."""
        seq = self.model[slot]
        k, v = seq.rk.permute(1, 0, 2)[None], seq.rv.permute(1, 0, 2)[None]
        lens = torch.tensor([len(seq)], dtype=torch.int32, device=self.dev)
        if words is None:
            ref = reference(q1, k, v, seqlens=lens, window=self.W)
        else:
            ref = folded_reference(dict(q=q1, B=1, Sq=q1.shape[2], Smax=len(seq), k=k, v=v, lens=lens), words)
        return ref if sinks is None else with_sink(ref, sinks)

    def check_read(self, name, o, lse, refs, slots):
        """``o [rows..., D]`` / ``lse [rows...]`` against ``refs`` (o, lse, pnorm of matching shapes)."""
        self.reads[name] += 1
        if 5 in self.skip:
            return
        vmax = max(float(self.model[s].rv.abs().max()) for s in slots)
        what = f"{name} at op {self.n_ops}"
        try:
            assert o.dtype == self.dtype and o.shape == refs[0].shape and lse.shape == refs[1].shape, (o.dtype, o.shape, lse.shape)
            check_out(o, refs[0], refs[2], vmax, self.dtype, what)
            check_lse(o, lse, refs[1], what)
        except AssertionError as e:
            raise AssertionError(f"check 5 (read) {what}, slots {list(slots)}: {e}") from None
        eps = EPS[self.dtype]
        err = (o.double() - refs[0]).abs()
        self.worst_ratio = max(self.worst_ratio, float((err / (eps * refs[0].abs() + 3 * eps * vmax * refs[2] + 2e-6)).max()))
        fin = torch.isfinite(refs[1])
        if bool(fin.any()):
            self.worst_lse = max(self.worst_lse, float((lse.double() - refs[1])[fin].abs().max()))

    def draw_sinks(self):
        """fp32 ``[H]`` sinks on the device on about half of the calls, in the range of the LSEs; head 0 has none (-inf)."""
        if self.rng.random() < 0.5:
            return None
        s = torch.rand(self.H, generator=self.gen) * 6.0
        s[0] = -INF
        return s.to(self.dev)

    def read_uniform(self, call, slots, Sq, **kw):
        """``decode`` / ``prefill`` (``call``) of the last Sq rows of each slot."""
        for s in slots:
            self.assert_read_range_is_named(s, Sq)
        q = self.queries(len(slots), Sq)
        opt = {n: x for n, x in kw.items() if x is not None}
        if self.W is not None:
            opt["window"] = self.W
        o, lse = self.calls[call](self.cache, q, list(slots), return_lse=True, **opt)
        refs = [self.reference_of(s, q[b:b + 1], kw.get("sinks"), None if kw.get("tree_mask") is None else kw["tree_mask"][b:b + 1])
                for b, s in enumerate(slots)]
        name = call + "".join(f"+{n}" for n in ("shared_prefix", "tree_mask") if n in opt)
        self.check_read(name, o, lse, [torch.cat([r[i] for r in refs]) for i in range(3)], slots)
        return o, lse

    def read_varlen(self, slots, gains, sinks=None):
        """``prefill_varlen`` of each slot's last ``gains[i]`` rows, packed."""
        for s, x in zip(slots, gains):
            if x:
                self.assert_read_range_is_named(s, x)
        total = sum(gains)
        q = self.queries(1, total)[0].permute(1, 0, 2)                                   # [total, H, D]
        opt = {} if sinks is None else dict(sinks=sinks)
        if self.W is not None:
            opt["window"] = self.W
        o, lse = self.calls["prefill_varlen"](self.cache, q, list(gains), list(slots), return_lse=True, **opt)
        self.check_varlen("prefill_varlen", q, o, lse, slots, gains, sinks)

    def check_varlen(self, name, q, o, lse, slots, gains, sinks=None):
        """A packed result ``o [total, H, D]``, ``lse [H, total]`` of the rows ``q [total, H, D]`` against fp64, sequence by sequence."""
        refs, at = [], 0
        for s, x in zip(slots, gains):
            if x:
                r = self.reference_of(s, q[at:at + x].permute(1, 0, 2)[None], sinks)
                refs.append((r[0][0].permute(1, 0, 2), r[1][0].t(), r[2][0].permute(1, 0, 2)))
            at += x
        refs = [torch.cat([r[i] for r in refs]) for i in range(3)]
        self.check_read(name, o[:at], lse[:, :at].t(), refs, [s for s, x in zip(slots, gains) if x])

    def read_step(self, slots, gains):
        """The attention read of exactly the rows a step appended (an FP8 session: of the last 1 .. 4 of each slot's)."""
        self.n_reads += 1
        by_gain = collections.defaultdict(list)
        for s, x in zip(slots, gains):
            by_gain[min(x, 4) if self.fp8 else x].append(s)
        by_gain.pop(0, None)
        if not by_gain:
            return
        if self.mode == "fp8":
            for x, group in by_gain.items():
                self.read_uniform("decode", group, x)
        elif self.mode == "window":
            turn = self.n_reads % 3
            if turn == 0:
                self.read_varlen(slots, gains)
            else:
                for x, group in by_gain.items():
                    self.read_uniform("decode" if turn == 1 and x <= 64 else "prefill", group, x)
        else:
            sinks = self.draw_sinks()
            self.read_varlen(slots, gains, sinks)
            if set(by_gain) == {1} and 0 not in gains:
                self.read_uniform("decode", slots, 1, sinks=sinks)
            for x, group in by_gain.items():
                if x <= 64:
                    self.read_shared_prefix(group, x, sinks)

    def read_shared_prefix(self, group, x, sinks):
        """``decode(shared_prefix=P)`` over the first set of the group's slots, grown greedily, that shares ``P >= page_size`` keys page
        for page with every one of the x new rows behind them."""
        def prefix(slots):
            P = self.cache.common_prefix(slots)
            return P if P >= self.page and all(len(self.model[s]) - x >= P for s in slots) else 0

        for i, a in enumerate(group):
            chosen = [a]
            for b in group[i + 1:]:
                if prefix(chosen + [b]):
                    chosen.append(b)
            if len(chosen) >= 2:
                self.read_uniform("decode", chosen, x, shared_prefix=prefix(chosen), sinks=sinks)
                return

    # --- the operations ------------------------------------------------------------------------------------------------------------------
    def write(self, slots, gains, k, v, how, step=False):
        """The step's rows into the cache (how: "device" = ``advance`` + ``write_step``, "varlen" = ``append_varlen``, "append" = the
        uniform ``append`` of one slot) and into the model.  -> False when the cache refused (full)."""
        c = self.cache
        kd, vd = k.to(self.dev), v.to(self.dev)
        what = f"{how} {dict(zip(slots, gains))}"
        if how == "device":
            ok, _ = self.guarded(what, lambda: c.advance(slots, gains))
            if ok:
                self.counts["pending_copies"] += int((c.cow_pairs >= 0).any(dim=1).sum()) if c.cow_pairs is not None and sum(gains) else 0
                self.write_step(slots, gains, kd, vd, step)
        elif how == "varlen":
            ok, _ = self.guarded(what, lambda: c.append_varlen(slots, kd, vd, gains))
        else:
            ok, _ = self.guarded(what, lambda: c.append(slots[0], kd.permute(1, 0, 2)[None], vd.permute(1, 0, 2)[None]))
        if not ok:
            return False
        at = 0
        for s, x in zip(slots, gains):
            seq = self.model[s]
            seq.extend(self.parts(k[at:at + x], v[at:at + x]))
            seq.cap = max(seq.cap, ceil_div(len(seq), self.page))
            at += x
        self.after(what)
        return True

    def write_step(self, slots, gains, kd, vd, step):
        """The device half behind an ``advance``; step: it is a ``step`` operation's (a session with a captured graph replays it then)."""
        self.cache.write_step(kd, vd, gains, slots)

    def op_new(self):
        c = self.cache
        if len(self.model) == c.max_batch:
            return None
        L = self.rng.choice(PROMPTS)
        ahead = L if self.rng.random() < 0.5 else 0
        # the model does not know the slot yet: the snapshot of check 4 covers the live slots, and a refused allocate leaves none
        ok, slot = self.guarded(f"allocate({ahead})", lambda: c.allocate(ahead))
        if not ok:
            return "refused"
        assert slot not in self.model
        empty = self.rows(0)
        self.model[slot] = Seq(self.parts(*empty), 0, ceil_div(ahead, self.page))
        self.after(f"allocate({ahead}) -> {slot}")
        pieces = [L]
        if L > 1 and self.rng.random() < 0.5:
            cut = sorted(self.rng.sample(range(1, L), min(self.rng.randint(1, 2), L - 1)))
            pieces = [b - a for a, b in zip([0] + cut, cut + [L])]
        for x in pieces:
            how = self.rng.choice(("device", "varlen", "append"))
            if not self.write([slot], [x], *self.rows(x), how):
                return "refused"
            self.read_step([slot], [x])
        return "done"

    def op_step(self):
        live = sorted(self.model)
        if not live:
            return None
        slots = self.rng.sample(live, self.rng.randint(1, len(live)))
        gains = [self.rng.choice(self.gains) for _ in slots]
        how = self.rng.choice(self.step_hows)
        if not self.write(slots, gains, *self.rows(sum(gains)), how, step=True):
            return "refused"
        self.read_step(slots, gains)
        return "done"

    def _cut(self, slot, with_all):
        """A length to fork or truncate the slot at: None (all), 0, the last page boundary, len - 1 or uniform -- of those the window
        rule allows (module docstring).  -> (True, n) or (False, None)."""
        seq = self.model[slot]
        n = len(seq)
        cands = [None, 0, n // self.page * self.page, n - 1, self.rng.randint(0, n)]
        if not with_all:
            cands[0] = n
        floor = seq.gone * self.page + self.W - 1 if seq.gone else 0
        cands = [x for x in cands if x is None or floor <= x <= n]
        return (True, self.rng.choice(cands)) if cands else (False, None)

    def op_fork(self):
        c = self.cache
        if not self.model or len(self.model) == c.max_batch:
            return None
        slot = self.rng.choice(sorted(self.model))
        ok, n = self._cut(slot, True)
        if not ok:
            return None
        child = c.fork(slot) if n is None else c.fork(slot, n)
        seq = self.model[slot]
        n = len(seq) if n is None else n
        pages = ceil_div(n, self.page)
        assert child not in self.model
        self.model[child] = seq.first(n, min(seq.gone, pages), pages)
        self.after(f"fork({slot}, {n}) -> {child}")
        return "done"

    def op_free(self):
        if not self.model:
            return None
        slot = self.rng.choice(sorted(self.model))
        self.cache.free(slot)
        del self.model[slot]
        self.after(f"free({slot})")
        return "done"

    def op_truncate(self):
        if not self.model:
            return None
        slot = self.rng.choice(sorted(self.model))
        ok, n = self._cut(slot, False)
        if not ok:
            return None
        self.truncate(slot, n)
        return "done"

    def truncate(self, slot, n):
        self.cache.truncate(slot, n)
        seq = self.model[slot]
        pages = ceil_div(n, self.page)
        self.model[slot] = seq.first(n, min(seq.gone, pages), pages)
        self.poison_tail(slot)
        self.after(f"truncate({slot}, {n})")

    def op_release(self):
        if not self.model:
            return None
        slot = self.rng.choice(sorted(self.model))
        seq = self.model[slot]
        let_go = self.cache.release_behind_window(slot, self.W)
        behind = min(max(0, len(seq) - self.W + 1) // self.page, seq.cap)
        assert let_go == max(0, behind - seq.gone), f"check 3 (ownership): release_behind_window let go of {let_go} entries"
        seq.gone = max(seq.gone, behind)
        self.counts["releases"] += let_go > 0
        self.after(f"release_behind_window({slot}, {self.W}) -> {let_go}")
        return "done"

    def op_swap(self):
        c = self.cache
        able = {}
        for s in sorted(self.model):
            mine = [i for i, p in enumerate(c.pages(s)) if p >= 0 and c.page_refcount(p) == 1]
            if len(mine) >= 2:
                able[s] = mine
        if not able:
            return None
        slot = self.rng.choice(sorted(able))
        i, j = self.rng.sample(able[slot], 2)
        c.swap_pages(slot, i, j)
        self.after(f"swap_pages({slot}, {i}, {j})")
        return "done"

    def op_reserve(self):
        if not self.model:
            return None
        slot = self.rng.choice(sorted(self.model))
        seq = self.model[slot]
        n = len(seq) + self.rng.choice((1, self.page, 2 * self.page, 3 * self.page, 7 * self.page))
        ok, _ = self.guarded(f"reserve({slot}, {n})", lambda: self.cache.reserve(slot, n))
        if not ok:
            return "refused"
        seq.cap = max(seq.cap, ceil_div(n, self.page))
        self.after(f"reserve({slot}, {n})")
        return "done"

    def op_spec(self):
        """The documented speculative step: a drafted tree's rows, ``decode(tree_mask=)``, ``truncate`` to the length before,
        ``append_varlen`` of one root-to-leaf path."""
        if not self.model:
            return None
        slot = self.rng.choice(sorted(self.model))
        L, Sq = len(self.model[slot]), self.rng.randint(2, 8)
        parents = [-1] + [self.rng.randint(-1, i - 1) for i in range(1, Sq)]
        k, v = self.rows(Sq)
        if not self.write([slot], [Sq], k, v, self.rng.choice(("device", "varlen"))):
            return "refused"
        words = ops.tree_mask_from_parents(torch.tensor([parents]))[0].to(self.dev)
        self.n_reads += 1
        self.read_uniform("decode", [slot], Sq, tree_mask=words)
        self.truncate(slot, L)
        path, node = [], self.rng.randrange(Sq)
        while node >= 0:
            path.append(node)
            node = parents[node]
        path.reverse()
        if not self.write([slot], [len(path)], k[path], v[path], "varlen"):
            return "refused"
        return "done"

    def run(self, n_ops):
        """n_ops operations, each drawn by weight and redrawn while impossible."""
        done = 0
        while done < n_ops:
            kind = self.rng.choices(self.kinds, self.weights)[0]
            self.draws += 1
            self.n_ops = done
            res = getattr(self, "op_" + kind)()
            if res is None:
                self.redraws += 1
                continue
            done += 1
            if res == "done":
                self.counts[kind] += 1
        self.n_ops = done
        assert 4 * self.redraws <= self.draws, f"{self.redraws} of {self.draws} draws were redrawn"
        return self

    def summary(self):
        ops_done = ", ".join(f"{k} {self.counts[k]}" for k in self.kinds)
        extra = ", ".join(f"{k} {self.counts[k]}" for k in ("refused_full", "pending_copies", "releases"))
        reads = ", ".join(f"{k} {n}" for k, n in sorted(self.reads.items()))
        return (f"{ops_done}; {extra}; redraws {self.redraws}/{self.draws}; reads: {reads}; worst err/bound {self.worst_ratio:.3f}, "
                f"worst LSE err {self.worst_lse:.2e}")

"""CPU tests of tests/serving_testlib.py: the serving traces on CPU tensors, where ``write_step``, ``page_copy`` and ``append_varlen``
run their plain-torch models and the attention is a stand-in -- it reads the pools through the table and the lengths it is handed, runs
the fp64 reference and rounds.  The honest cache with the honest stand-in passes every check at page sizes 64 and 128, with and
without a window, and over an FP8 cache; eight mutants, each wrong in one way, are each caught by the fixed seeds, and every test names
the check that catches its mutant (``check N`` of the library's docstring).

Shapes: H 4 / Hkv 2 / D 16, otherwise the sizes of the GPU traces (6 slots, 8 table entries a slot, 24 pages), so that a trace of 120
operations with its checks takes a second or two."""

from __future__ import annotations

import pytest
import torch

from kvcache_testlib import FP8, folded_reference, reference, window_lo, with_sink
from photonic_flash_attention_amd import ops
from photonic_flash_attention_amd.integration.pytorch import PagedKVCache
from serving_testlib import Session

H, HKV, D = 4, 2, 16
N_OPS = 120
W = {64: 40, 128: 96}                                       # shorter than a page


def make_cache(page, dtype=torch.bfloat16, cls=PagedKVCache, **kw):
    if dtype == FP8:
        kw.update(k_descale=torch.tensor([0.006, 0.02]), v_descale=torch.tensor([0.017, 0.0055]))
    return cls(num_pages=24, page_size=page, Hkv=HKV, D=D, dtype=dtype, device="cpu", max_batch=6, max_pages_per_seq=8,
               copy_on_write=True, **kw)


# --- the stand-in attention ----------------------------------------------------------------------------------------------------------

def standin(page_bound=True, lens_before=False):
    """``calls`` for a ``Session`` on CPU tensors.  Each call takes the pools, the table rows and the lengths from ``cache.operands``,
    gathers every sequence's keys page by page through the table (an id clamped into the pool, as the kernels clamp it), zeroes what
    the kernels promise not to read -- keys at and past len_b, and under a window keys below floor64(lo_b); table entries below
    ``lo_b // page_size`` and at or past ``ceil(len_b / page_size)`` are not even looked at -- and runs the fp64 reference (the tree rule
    and the sinks through ``folded_reference`` / ``with_sink``), rounded to q's dtype.  ``shared_prefix`` is the same attention.
    The mutants: page_bound=False reads every page from 0 and zeroes nothing below the window; lens_before=True takes each length
    from before the step (``len_b - Sq_b``)."""
    def uniform(cache, q, slots=None, *, return_lse=False, causal=True, window=None, sinks=None, tree_mask=None, shared_prefix=None):
        kp, vp, kw = cache.operands(slots)
        table, lens = kw["block_table"], kw["cache_seqlens"].tolist()
        B, Sq = q.shape[0], q.shape[2]
        assert causal and table.shape[0] == B
        if lens_before:
            lens = [max(0, n - Sq) for n in lens]
        NP, Hkv, page, Dk = kp.shape
        Smax = table.shape[1] * page
        dense = []
        for pool, scale in ((kp, kw.get("k_descale")), (vp, kw.get("v_descale"))):
            out = torch.zeros(B, Hkv, Smax, Dk, dtype=torch.float64)
            for b, (n, lo) in enumerate(zip(lens, window_lo(lens, Sq, window))):
                for p in range(lo // page if page_bound else 0, -(-n // page)):
                    x = pool[int(table[b, p].clamp(0, NP - 1))]
                    out[b, :, p * page:(p + 1) * page] = x.double() if scale is None else ops.dequantize_kv(x[None], scale, torch.float64)[0]
                out[b, :, n:] = 0
                if page_bound:
                    out[b, :, :lo // 64 * 64] = 0
            dense.append(out)
        sl = torch.tensor(lens, dtype=torch.int32)
        if tree_mask is None:
            ref = reference(q, *dense, seqlens=sl, window=window)
        else:
            ref = folded_reference(dict(q=q, B=B, Sq=Sq, Smax=Smax, k=dense[0], v=dense[1], lens=sl), tree_mask)
        if sinks is not None:
            ref = with_sink(ref, sinks)
        return ref[0].to(q.dtype), ref[1].float()

    def varlen(cache, q, q_lens, slots=None, *, return_lse=False, **kw):
        slots = list(range(cache.max_batch)) if slots is None else slots
        o = torch.empty_like(q)
        lse = torch.empty(q.shape[1], q.shape[0])
        at = 0
        for s, x in zip(slots, q_lens):
            if x:
                ob, lb = uniform(cache, q[at:at + x].permute(1, 0, 2)[None], [s], **kw)
                o[at:at + x], lse[:, at:at + x] = ob[0].permute(1, 0, 2), lb[0]
            at += x
        return o, lse

    return dict(decode=uniform, prefill=uniform, prefill_varlen=varlen)


def trace(seed, page=64, mode="plain", cls=PagedKVCache, calls=None, n_ops=N_OPS, **kw):
    cache = make_cache(page, {"plain": torch.bfloat16, "window": torch.float16, "fp8": FP8}[mode], cls)
    window = W[page] if mode == "window" else None
    return Session(cache, calls or standin(), seed, H=H, mode=mode, window=window, **kw).run(n_ops)


# --- the honest run --------------------------------------------------------------------------------------------------------------------

# two fixed seeds per configuration, chosen so that the honest trace of N_OPS operations holds the events asserted below
SEEDS = {(64, "plain"): (2, 4), (128, "plain"): (2, 12), (64, "window"): (1, 4), (128, "window"): (2, 3), (64, "fp8"): (8, 11)}


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("page,mode", list(SEEDS))
def test_the_honest_cache_passes_every_check(page, mode, which):
    s = trace(SEEDS[page, mode][which], page, mode)
    print(s.summary())
    c = s.counts
    assert c["step"] >= 20 and c["fork"] >= 5 and c["truncate"] >= 4 and c["free"] >= 3 and s.reads and s.n_ops == N_OPS
    assert 4 * s.redraws <= s.draws
    if mode == "window":
        assert c["releases"] >= 2 and set(s.reads) == {"decode", "prefill", "prefill_varlen"}
    if mode == "plain":
        assert c["spec"] >= 2 and s.reads["decode+tree_mask"] == c["spec"]
    if mode == "fp8":
        assert set(s.reads) == {"decode"}


def test_a_trace_is_a_function_of_its_seed():
    a, b, c = trace(2), trace(2), trace(4)
    assert a.log == b.log and a.log != c.log and a.counts == b.counts


# --- the mutants: each wrong in one way, each caught, each by the check the test names ------------------------------------------------
# Each runs the seeds of the honest run (which pass above) and must be caught on every one of them.

def caught(check, page=64, mode="plain", **kw):
    for seed in SEEDS[page, mode]:
        with pytest.raises(AssertionError, match=check):
            trace(seed, page, mode, **kw)


def test_mutant_1_fork_does_not_raise_the_reference_counts():
    class Mutant(PagedKVCache):
        def fork(self, slot, n_tokens=None):
            before = list(self._ref)
            child = super().fork(slot, n_tokens)
            self._ref[:] = before
            return child
    for page in (64, 128):
        caught(r"check 3 \(ownership\)", page=page, cls=Mutant)


def test_mutant_2_no_copy_on_write_of_a_shared_tail():
    """The slot writes into the page it shares: the other holder's rows change (check 2)."""
    class Mutant(PagedKVCache):
        def _grow(self, slots, lens):
            self._cow = False
            try:
                return super()._grow(slots, lens)
            finally:
                self._cow = True
    caught(r"check 2 \(contents\)", cls=Mutant)


def test_mutant_3_a_stale_pending_copy_replays_at_a_later_write_step():
    """``_reset_pending`` does nothing, so the copy of an earlier ``advance`` runs again in front of a later ``write_step`` and overwrites
    rows its destination page has gained since, or a page that went to another slot (check 2)."""
    class Mutant(PagedKVCache):
        def _reset_pending(self):
            self._copies = []
    caught(r"check 2 \(contents\)", cls=Mutant)


def test_mutant_4_the_page_copy_moves_one_row_less(monkeypatch):
    model = ops._page_copy_model
    monkeypatch.setattr(ops, "_page_copy_model", lambda kp, vp, pairs, rows: model(
        kp, vp, pairs, [kp.shape[2] - 1] * len(pairs) if rows is None else [r - 1 for r in rows]))
    for page in (64, 128):
        caught(r"check 2 \(contents\)", page=page)


def test_mutant_5_truncate_leaves_the_device_length():
    """Only check 1 can see it: the next append copies the host lengths over, and a read follows an append."""
    class Mutant(PagedKVCache):
        def truncate(self, slot, n_tokens):
            before = self._lens[slot].clone()
            super().truncate(slot, n_tokens)
            self._lens[slot] = before
    caught(r"check 1 \(device lengths\)", cls=Mutant)


def test_mutant_6_free_leaves_the_device_length():
    class Mutant(PagedKVCache):
        def free(self, slot):
            before = self._lens[slot].clone()
            super().free(slot)
            self._lens[slot] = before
    caught(r"check 1 \(device lengths\)", cls=Mutant)


def test_mutant_7_release_returns_the_pages_but_leaves_the_table_entries():
    """Check 3 sees the entries.  Without check 3 the honest stand-in passes -- it keeps the kernels' promise and never looks at an entry
    below ``lo_b // page_size`` -- and the stand-in that ignores the window's lower page bound reads the poison in the returned pages."""
    class Mutant(PagedKVCache):
        def release_behind_window(self, slot, window):
            before = self._table[slot].clone()
            let_go = super().release_behind_window(slot, window)
            self._table[slot] = before
            return let_go
    for page in (64, 128):
        for seed in SEEDS[page, "window"]:
            with pytest.raises(AssertionError, match=r"check 3 \(ownership\)"):
                trace(seed, page, "window", Mutant)
            s = trace(seed, page, "window", Mutant, skip=(3,))
            assert s.counts["releases"] >= 2
            with pytest.raises(AssertionError, match=r"check 5 \(read\).*non-finite"):
                trace(seed, page, "window", Mutant, calls=standin(page_bound=False), skip=(3,))


def test_mutant_8_a_standin_that_takes_the_lengths_from_before_the_step():
    for page, mode in ((64, "plain"), (128, "window"), (64, "fp8")):
        caught(r"check 5 \(read\)", page=page, mode=mode, calls=standin(lens_before=True))


def test_a_refused_full_is_checked_and_counted():
    """Check 4 on a cache whose refusal is not clean: ``reserve`` takes a page before it raises."""
    class Mutant(PagedKVCache):
        def reserve(self, slot, n_tokens):
            try:
                super().reserve(slot, n_tokens)
            except Exception:
                if self._free_pages:
                    self._assign(slot, 1)
                raise
    assert sum(trace(seed).counts["refused_full"] for seed in SEEDS[64, "plain"]) >= 1
    caught(r"check 4 \(refused-full\)", cls=Mutant)

"""GPU tests: serving traces (tests/serving_testlib.py) through the HIP kernels -- long random sessions on one ``PagedKVCache`` in which
prompts come in by chunks, sequences fork, grow, get truncated after a speculative step and are freed, pages go back to the pool behind
a window and are handed to somebody else, and a captured step is replayed while all of that happens around it.  After every operation
the device table, lengths and pools are compared with a dense model of what the cache should hold, bit for bit, and every attention
read with the fp64 reference over the model's rows under ``kvcache_testlib``'s bounds.  The pools start as NaN and every page nobody
holds is refilled with NaN after every operation, so a stale table entry, a length the device did not get, a pending copy that
replays late or a reference count off by one gives a non-finite read or a content mismatch, where the kernels' clamps alone would
give finite, plausible numbers.

All traces: ``copy_on_write=True``, 6 slots, 8 table entries a slot, 24 pages, H 8 / Hkv 2 -- the smallest sizes at which sharing, a full
pool and page reuse all occur -- and two fixed seeds of 175 operations each, chosen on the CPU (the choices do not depend on the
data, the head dim or the attention function) so that the honest trace holds the events ``assert_conditions`` asks for.  Those are
conditions on the test, not measurements.

  plain      bf16, D 128, page 64: all operations, the speculative step included; every step read with ``prefill_varlen`` (sinks on about
             half of the reads), one-row steps also with ``decode``, stepped slots behind a common prefix also with
             ``decode(shared_prefix=)``
  window     fp16, D 64, page 128, W 96 (shorter than a page: a window regularly straddles a page edge, and the 64-key boundary lies
             inside a page); ``release_behind_window`` among the operations; every read takes ``window=W``, through
             ``prefill_varlen``, ``decode`` and ``prefill`` in turn
  fp8        e4m3fn pools, bf16 rows and queries, D 128, page 64, per-head descales under which some rows saturate; reads are ``decode``
             of the last 1 .. 4 rows of what a slot gained (the class refuses the other calls over an FP8 cache)
  captured   the plain trace with one graph: ``write_step(cu_seqlens_q=, max_seqlen_q=70)`` + ``prefill_varlen`` over all slots, a single
             chain on one stream, captured once on an empty step and replayed for every ``step`` of the trace through static input
             buffers while forks, frees, truncates and swaps run between replays; each replay is compared bit for bit with the eager
             calls on the same state, and with fp64
  mutant     the plain trace on a cache that never empties its pending table: the content check must fail, through the kernels too

Measured on one MI355X (``profiles/serving_trace.md``): 0.4 - 1.9 s a trace (the first one carries the library's load), the file's ten tests in 7 s."""

from __future__ import annotations

import time

import pytest
import torch

from kvcache_testlib import FP8, capture, device
from photonic_flash_attention_amd.integration.pytorch import PagedKVCache
from serving_testlib import GPU_CALLS, Session

pytestmark = pytest.mark.gpu

H, HKV = 8, 2
N_OPS = 175
MAX_STEP = 70                                                # the largest gain of a step: the graph's max_seqlen_q


def make_cache(page, D, dtype, cls=PagedKVCache):
    kw = {}
    if dtype == FP8:                                         # |x| / descale passes 448 from 2.7 (K head 0) and 2.5 (V head 1) standard deviations on
        kw = dict(k_descale=torch.tensor([0.006, 0.02], device=device()), v_descale=torch.tensor([0.017, 0.0055], device=device()))
    return cls(num_pages=24, page_size=page, Hkv=HKV, D=D, dtype=dtype, device=device(), max_batch=6, max_pages_per_seq=8,
               copy_on_write=True, **kw)


def assert_conditions(s, mode):
    c = s.counts
    print(s.summary())
    assert c["pending_copies"] >= 3 and c["fork"] >= 8 and c["truncate"] >= 8 and c["free"] >= 5 and c["swap"] >= 2 and c["refused_full"] >= 1, c
    assert 4 * s.redraws <= s.draws and s.n_ops == N_OPS
    if mode == "window":
        assert c["releases"] >= 4 and set(s.reads) == {"decode", "prefill", "prefill_varlen"}, (c, s.reads)
    if mode == "plain":
        assert c["spec"] >= 3 and s.reads["decode+shared_prefix"] >= 2 and s.reads["decode+tree_mask"] >= 3 and s.reads["decode"] >= 1, (c, s.reads)
    if mode == "fp8":
        assert set(s.reads) == {"decode"}


def run(session, mode):
    t = time.perf_counter()
    session.run(N_OPS)
    torch.cuda.synchronize()
    print(f"wall {time.perf_counter() - t:.1f} s")
    assert_conditions(session, mode)


@pytest.mark.parametrize("seed", [15, 24])
def test_plain_trace(seed):
    run(Session(make_cache(64, 128, torch.bfloat16), GPU_CALLS, seed, H=H), "plain")


@pytest.mark.parametrize("seed", [8, 22])
def test_window_trace(seed):
    run(Session(make_cache(128, 64, torch.float16), GPU_CALLS, seed, H=H, mode="window", window=96), "window")


@pytest.mark.parametrize("seed", [8, 22])
def test_fp8_trace(seed):
    s = Session(make_cache(64, 128, FP8), GPU_CALLS, seed, H=H, mode="fp8")
    run(s, "fp8")
    sat = sum(int(((seq.ek & 0x7f) == 0x7e).sum()) for seq in s.model.values())
    assert sat > 0 or not s.model, "no element of the live rows saturated: the descales are too large"


class StalePending(PagedKVCache):
    """Wrong in one way: the pending table is never emptied, so ``pfa_page_copy`` runs an earlier step's copy again in front of a later
    ``pfa_kv_append``.  Every page id stays valid; only contents go wrong."""

    def _reset_pending(self):
        self._copies = []


@pytest.mark.parametrize("seed", [15, 24])
def test_the_trace_sees_a_stale_pending_copy_through_the_kernels(seed):
    """The device half of the harness is not blind: the mutant of tests/test_serving_testlib.py that only the device path shows is
    caught here by the content check, as on the CPU."""
    with pytest.raises(AssertionError, match=r"check 2 \(contents\)"):
        Session(make_cache(64, 128, torch.bfloat16, StalePending), GPU_CALLS, seed, H=H).run(N_OPS)


class CapturedSession(Session):
    """The plain session whose every ``step`` goes through one captured graph: ``advance`` on the host, then a replay of
    ``write_step`` + ``prefill_varlen`` over all slots in slot order from static buffers."""

    def __init__(self, cache, seed):
        super().__init__(cache, GPU_CALLS, seed, H=H)
        self.step_hows = ("device",)
        rows = cache.max_batch * MAX_STEP
        self.k_s = torch.zeros(rows, HKV, cache.D, dtype=self.dtype, device=self.dev)
        self.v_s = torch.zeros_like(self.k_s)
        self.q_s = torch.zeros(rows, H, cache.D, dtype=self.dtype, device=self.dev)
        self.cu = torch.zeros(cache.max_batch + 1, dtype=torch.int32, device=self.dev)           # no rows while warming up and capturing
        self.graph, (self.o_g, self.lse_g) = capture(self.step)
        torch.cuda.synchronize()
        self.replayed = None
        self.replays = 0

    def step(self):
        self.cache.write_step(self.k_s, self.v_s, cu_seqlens_q=self.cu, max_seqlen_q=MAX_STEP)
        return self.cache.prefill_varlen(self.q_s, cu_seqlens_q=self.cu, max_seqlen_q=MAX_STEP, return_lse=True)

    def write_step(self, slots, gains, kd, vd, step):
        if not step:
            return super().write_step(slots, gains, kd, vd, step)
        B = self.cache.max_batch
        per_slot, at = {}, 0
        for s, x in zip(slots, gains):
            per_slot[s] = (at, x)
            at += x
        order = [per_slot.get(s, (0, 0)) for s in range(B)]
        idx = torch.tensor([a + i for a, x in order for i in range(x)], dtype=torch.int64).to(self.dev)
        all_gains = [x for _, x in order]
        total = sum(all_gains)
        self.k_s.zero_(), self.v_s.zero_()
        self.k_s[:total], self.v_s[:total] = kd.index_select(0, idx), vd.index_select(0, idx)
        self.q_s[:total] = self.queries(1, total)[0].permute(1, 0, 2) if total else 0
        cu = [0]
        for x in all_gains:
            cu.append(cu[-1] + x)
        self.cu.copy_(torch.tensor(cu, dtype=torch.int32))
        self.graph.replay()
        torch.cuda.synchronize()
        self.replays += 1
        self.replayed = (all_gains, total, self.o_g[:total].clone(), self.lse_g[:, :total].clone())

    def read_step(self, slots, gains):
        if self.replayed is not None:
            (all_gains, total, o_g, lse_g), self.replayed = self.replayed, None
            if total:
                self.check_varlen("captured", self.q_s, o_g, lse_g, list(range(self.cache.max_batch)), all_gains)
                o_e, lse_e = self.step()                                           # the eager calls on the same state: the writes are idempotent
                torch.cuda.synchronize()
                assert torch.equal(o_e[:total], o_g) and torch.equal(lse_e[:, :total], lse_g), f"op {self.n_ops}: the replay is not the eager step"
                self.after("the eager step behind the replay")
        super().read_step(slots, gains)


@pytest.mark.parametrize("seed", [15, 24])
def test_captured_trace(seed):
    s = CapturedSession(make_cache(64, 128, torch.bfloat16), seed)
    run(s, "plain")
    assert s.replays == s.counts["step"] >= 30 and s.reads["captured"] >= 25, (s.replays, s.counts, s.reads)

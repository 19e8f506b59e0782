"""CPU-side tests (no GPU) of attention sinks over the KV cache (``pfa_fa3_sinks`` and the ``*_sink`` entry points, ABI v9 additive):
a NULL block agreeing with the sink-less sibling, the block's rules in their documented order with
the sibling's errors behind them, the describe names, plan and workspace equal to the sink-less call's, ``ops``' refusals on CPU
tensors, the signatures -- and the reference helper of tests/test_hip_attn_sinks.py against an independent formulation, with the
condition that the sinks those tests choose matter."""

from __future__ import annotations

import ctypes as C
import inspect

import pytest
import torch

from capi_testlib import ALIGN, FLAGS, NULL, SIZE, decode_args, decode_paged, lib, name_of, prefill_varlen_args, ref, sinks  # noqa: F401
from kvcache_testlib import INF, reference
from photonic_flash_attention_amd import _capi, ops
from test_hip_attn_sinks import CASES, assert_sinks_matter, choose_sinks, with_sink


def _dargs(**over):
    """A valid contiguous block of the decode / prefill calls: B 2, H 8, Hkv 2, Sq 4, Smax 4096, D 128, with a workspace."""
    return decode_args(over, Sq=4)


def _paged(**over):
    return decode_paged(over, Sq=4)


def _vargs(**over):
    """A valid block of the ragged call: B 5, H 8, Hkv 2, 640 packed rows, Smax 4096, D 128."""
    return prefill_varlen_args(over)


# blocks good and bad, for every family: the sibling's verdict must come through
BAD = [dict(), dict(q=0), dict(B=0), dict(D=96), dict(dtype_out=1), dict(k_stride_s=257), dict(o=0x800008), dict(flags=1), dict(reserved0=1),
       dict(page_size=64), dict(causal=0), dict(dtype_out=2), dict(D=64), dict(H=7), dict(softmax_scale=0.0)]
EXTS = [None, dict(), dict(window=128), dict(window=5000), dict(window=-1), dict(flags=1), dict(size=8)]


def _families(lib):
    """(name, make, sibling check, sink check, sibling describe, sink describe, nsplit?) of the three calls that take an extension."""
    return [("decode", _dargs, lib.pfa_fa3_decode_check_ex, lib.pfa_fa3_decode_sink_check, lib.pfa_fa3_decode_describe_ex,
             lib.pfa_fa3_decode_sink_describe, True),
            ("prefill", lambda **kw: _dargs(**{"Sq": 300, **kw}), lib.pfa_fa3_prefill_check_ex, lib.pfa_fa3_prefill_sink_check,
             lib.pfa_fa3_prefill_describe_ex, lib.pfa_fa3_prefill_sink_describe, False),
            ("varlen", _vargs, lib.pfa_fa3_prefill_varlen_check_ex, lib.pfa_fa3_prefill_varlen_sink_check, lib.pfa_fa3_prefill_varlen_describe_ex,
             lib.pfa_fa3_prefill_varlen_sink_describe, False)]


def test_a_null_block_is_the_sibling_call(lib):
    for name, make, chk, schk, desc, sdesc, ns in _families(lib):
        for over in BAD + [dict(Smax=1024), dict(Smax=65536)]:
            for mk in ([make] if name == "varlen" else [make, _paged if name == "decode" else lambda **kw: _paged(**{"Sq": 300, **kw})]):
                a = mk(**over)
                for e in EXTS:
                    ext = None if e is None else _capi.make_cache_ext(**e)
                    want = chk(C.byref(a), ref(ext))
                    assert schk(C.byref(a), ref(ext), None) == want, (name, over, e)
                    assert name_of(sdesc, a, ref(ext), None, nsplit=ns) == name_of(desc, a, ref(ext), nsplit=ns), (name, over, e)
                    if name == "decode":
                        assert lib.pfa_fa3_decode_sink_workspace_bytes(C.byref(a), ref(ext), None) == \
                            lib.pfa_fa3_decode_workspace_bytes_ex(C.byref(a), ref(ext))
        assert schk(None, None, None) == NULL
    for over in BAD + [dict(Sq=256, Smax=8192), dict(Sq=300)]:
        a = _dargs(**{"Sq": 256, **over})
        for ks in (0, 1, 3, 8, 9, -1):
            assert lib.pfa_fa3_prefill_split_sink_check(C.byref(a), ks, None) == lib.pfa_fa3_prefill_split_check(C.byref(a), ks)
            assert name_of(lib.pfa_fa3_prefill_split_sink_describe, a, ks, None, nsplit=True) == \
                name_of(lib.pfa_fa3_prefill_split_describe, a, ks, nsplit=True)
            assert lib.pfa_fa3_prefill_split_sink_workspace_bytes(C.byref(a), ks, None) == lib.pfa_fa3_prefill_split_workspace_bytes(C.byref(a), ks)


def test_block_rules_in_their_documented_order_then_the_siblings(lib):
    # size, flags, NULL pointer, alignment: each reported in front of the ones behind it, and all of them in front of the sibling's
    wrong = [(dict(size=8, flags=1, sinks=0), SIZE), (dict(flags=1, sinks=0), FLAGS), (dict(sinks=0), NULL), (dict(sinks=0xA002), ALIGN)]
    for name, make, chk, schk, _, sdesc, ns in _families(lib):
        for a in (make(), make(B=0), make(q=0)):
            for kw, want in wrong:
                s = sinks(**kw)
                assert schk(C.byref(a), None, C.byref(s)) == want, (name, kw)
                assert schk(C.byref(a), C.byref(_capi.make_cache_ext(flags=1)), C.byref(s)) == want, (name, kw)
                assert name_of(sdesc, a, None, C.byref(s), nsplit=ns)[0] == want
        # behind a good block the sibling's errors come through, for the argument block and for the extension
        good = sinks()
        for over in BAD:
            a = make(**over)
            for e in EXTS:
                ext = None if e is None else _capi.make_cache_ext(**e)
                assert schk(C.byref(a), ref(ext), C.byref(good)) == chk(C.byref(a), ref(ext)), (name, over, e)
        assert schk(None, None, C.byref(good)) == NULL
    a = _dargs(Sq=256)
    for kw, want in wrong:
        s = sinks(**kw)
        for ks in (0, 3, 9):
            assert lib.pfa_fa3_prefill_split_sink_check(C.byref(a), ks, C.byref(s)) == want
    good = sinks()
    for over in BAD + [dict(workspace=0), dict(workspace=0x4000004), dict(o_stride_s=4 * 8 * 128 + 4, dtype_out=0)]:
        a = _dargs(**{"Sq": 256, **over})
        for ks in (0, 1, 3, 9, -1):
            assert lib.pfa_fa3_prefill_split_sink_check(C.byref(a), ks, C.byref(good)) == lib.pfa_fa3_prefill_split_check(C.byref(a), ks), (over, ks)
    # the workspace queries leave out the pointer's rules and answer 0 where another fails
    a = _dargs(Smax=65536)
    full = lib.pfa_fa3_decode_workspace_bytes_ex(C.byref(a), None)
    assert full > 0
    assert lib.pfa_fa3_decode_sink_workspace_bytes(C.byref(a), None, C.byref(sinks(sinks=0))) == full
    assert lib.pfa_fa3_decode_sink_workspace_bytes(C.byref(a), None, C.byref(sinks(flags=1))) == 0
    assert lib.pfa_fa3_decode_sink_workspace_bytes(C.byref(a), None, C.byref(sinks(size=12))) == 0
    a = _dargs(Sq=256, Smax=8192)
    assert lib.pfa_fa3_prefill_split_sink_workspace_bytes(C.byref(a), 3, C.byref(sinks(sinks=0))) == \
        lib.pfa_fa3_prefill_split_workspace_bytes(C.byref(a), 3) > 0
    assert lib.pfa_fa3_prefill_split_sink_workspace_bytes(C.byref(a), 3, C.byref(sinks(flags=1))) == 0


def test_describe_names_plan_and_workspace_are_the_sink_less_calls(lib):
    s = sinks()
    win = _capi.make_cache_ext(window=128)
    wide = _capi.make_cache_ext(window=2048)
    want = [
        ("decode", False, None, "fa3_decode_bf16_d128_o16_sink+combine"),
        ("decode", True, None, "fa3_decode_bf16_d128_o16_sink+combine_paged"),
        ("decode", False, win, "fa3_decode_bf16_d128_o16_win_sink"),
        ("decode", True, win, "fa3_decode_bf16_d128_o16_win_sink_paged"),
        ("decode", True, wide, "fa3_decode_bf16_d128_o16_win_sink+combine_paged"),
        ("prefill", False, None, "fa3_prefill_bf16_d128_o16_causal_sink"),
        ("prefill", True, win, "fa3_prefill_bf16_d128_o16_causal_win_sink_paged"),
        ("varlen", False, None, "fa3_prefill_bf16_d128_o16_causal_sink_varlen"),
        ("varlen", False, win, "fa3_prefill_bf16_d128_o16_causal_win_sink_varlen"),
    ]
    fam = {f[0]: f for f in _families(lib)}
    for name, paged, ext, text in want:
        _, make, _, _, desc, sdesc, ns = fam[name]
        a = make() if not paged else (_paged() if name == "decode" else _paged(Sq=300))
        got, plain = name_of(sdesc, a, ref(ext), C.byref(s), nsplit=ns), name_of(desc, a, ref(ext), nsplit=ns)
        assert got[1] == text and got[1].replace("_sink", "") == plain[1]
        assert got[0] == plain[0] > 0 and got[2] == plain[2]          # workgroups and split count
        if name == "decode":
            assert lib.pfa_fa3_decode_sink_workspace_bytes(C.byref(a), ref(ext), C.byref(s)) == \
                lib.pfa_fa3_decode_workspace_bytes_ex(C.byref(a), ref(ext))
    a = _vargs(block_table=0x8000, block_table_stride_b=32, page_size=128, num_pages=100, k_stride_b=128 * 2 * 128, v_stride_b=128 * 2 * 128)
    assert name_of(lib.pfa_fa3_prefill_varlen_sink_describe, a, None, C.byref(s))[1] == "fa3_prefill_bf16_d128_o16_causal_sink_varlen_paged"
    for mk in (_dargs, _paged):
        a = mk(Sq=256, Smax=8192, dtype_out=2)
        for ks in (0, 1, 3, 8):
            got = name_of(lib.pfa_fa3_prefill_split_sink_describe, a, ks, C.byref(s), nsplit=True)
            plain = name_of(lib.pfa_fa3_prefill_split_describe, a, ks, nsplit=True)
            assert got[0] == plain[0] > 0 and got[2] == plain[2] and got[1].replace("_sink", "") == plain[1]
            tail = "_paged" if mk is _paged else ""
            assert got[1] == ("fa3_prefill_bf16_d128_o32_causal_sink" + (f"_split{got[2]}+merge" if got[2] > 1 else "") + tail)
            assert lib.pfa_fa3_prefill_split_sink_workspace_bytes(C.byref(a), ks, C.byref(s)) == lib.pfa_fa3_prefill_split_workspace_bytes(C.byref(a), ks)
            assert lib.pfa_fa3_prefill_split_plan(C.byref(a), ks) == got[2]


def test_ops_refuse_bad_sinks_on_cpu_tensors_before_anything_else():
    q = torch.zeros(2, 8, 3, 64, dtype=torch.bfloat16)
    k = torch.zeros(2, 2, 128, 64, dtype=torch.bfloat16)
    qv = torch.zeros(6, 8, 64, dtype=torch.bfloat16)
    cu = torch.tensor([0, 3, 6], dtype=torch.int32)
    calls = [("decode", lambda **kw: ops.fa3_decode(q, kw.pop("k", k), kw.pop("v", k), **kw)),
             ("prefill", lambda **kw: ops.fa3_prefill_cache(q, kw.pop("k", k), kw.pop("v", k), **kw)),
             ("varlen", lambda **kw: ops.fa3_prefill_varlen(qv, kw.pop("k", k), kw.pop("v", k), cu_seqlens_q=cu, max_seqlen_q=3, **kw))]
    k8 = k.to(torch.float8_e4m3fn)
    ones = torch.ones(2)
    for name, call in calls:
        for bad, text in ((torch.zeros(8, dtype=torch.bfloat16), "sinks must be an fp32"), (torch.zeros(8, dtype=torch.float64), "sinks must be an fp32"),
                          ([0.0] * 8, "sinks must be an fp32"), (torch.zeros(4), r"sinks must be \[H\] = \[8\]"),
                          (torch.zeros(1, 8), r"sinks must be \[H\]"), (torch.zeros(16)[::2], "sinks must be contiguous"),
                          (torch.zeros(8, device="meta"), "sinks must live on the operands' device")):
            with pytest.raises(ValueError, match=text):
                call(sinks=bad)
        with pytest.raises(ValueError, match=r"sinks is not supported with an FP8 \(torch.float8_e4m3fn\) KV cache"):
            call(k=k8, v=k8, k_descale=ones, v_descale=ones, sinks=torch.zeros(8))
    with pytest.raises(ValueError, match="sinks is not supported with tree_mask"):
        ops.fa3_decode(q, k, k, tree_mask=torch.zeros(2, 3, dtype=torch.int64), sinks=torch.zeros(8))
    with pytest.raises(ValueError, match="sinks must be an fp32"):       # ... also on the way through shared_prefix
        ops.fa3_decode(q, k, k, cache_seqlens=torch.tensor([100, 100], dtype=torch.int32), shared_prefix=64, sinks=torch.zeros(8).half())


def test_sinks_is_the_last_keyword_and_the_others_stay():
    for fn in (ops.fa3_decode, ops.fa3_prefill_cache, ops.fa3_prefill_varlen):
        params = list(inspect.signature(fn).parameters.values())
        assert params[-1].name == "sinks" and params[-1].default is None and params[-1].kind is inspect.Parameter.KEYWORD_ONLY
        assert params[-2].name == "v_descale" and params[-3].name == "k_descale"
    assert "sinks" not in inspect.signature(ops.rope_append).parameters
    assert "sinks" not in inspect.signature(ops.kv_append).parameters


# --- the reference helper of the GPU tests, against the formulation that appends a key ----------------------------------------------------

def _appended_key_reference(q, k, v, sinks, *, seqlens, causal=True, window=None, key_mask=None):
    """Plain fp64 softmax over the visible keys and one more key of score sinks[h] with a zero value row -> (o, lse, ||p_row||_2 over
    the real keys)."""
    B, H, Sq, D = q.shape
    Hkv, Smax = k.shape[1], k.shape[2]
    g = H // Hkv
    o = torch.zeros(B, H, Sq, D, dtype=torch.float64)
    lse = torch.zeros(B, H, Sq, dtype=torch.float64)
    pn = torch.zeros(B, H, Sq, 1, dtype=torch.float64)
    for b in range(B):
        n = int(seqlens[b])
        for h in range(H):
            for i in range(Sq):
                top = n - Sq + i if causal else n - 1
                vis = [j for j in range(min(n, top + 1)) if (window is None or j > top - window) and (key_mask is None or bool(key_mask[b, j]))]
                x = torch.cat([(k[b, h // g, vis].double() @ q[b, h, i].double()) * D ** -0.5, sinks[h:h + 1].double()])
                vals = torch.cat([v[b, h // g, vis].double(), torch.zeros(1, D, dtype=torch.float64)])
                if bool(torch.isneginf(x).all()):
                    lse[b, h, i] = -INF
                    continue
                p = torch.softmax(x, dim=0)
                o[b, h, i] = p @ vals
                lse[b, h, i] = torch.logsumexp(x, dim=0)
                pn[b, h, i, 0] = p[:-1].norm()
    return o, lse, pn


@pytest.mark.parametrize("Sq,lens,window,H,Hkv", [(1, (0, 37, 96), None, 4, 4), (5, (0, 3, 96), None, 8, 2), (5, (96, 50, 4), 16, 8, 2),
                                                  (1, (96, 0, 20), 16, 4, 1)])
def test_with_sink_is_the_softmax_with_one_more_key(Sq, lens, window, H, Hkv):
    g = torch.Generator().manual_seed(17 + Sq + H)
    q = torch.randn(3, H, Sq, 64, generator=g).bfloat16()
    k = torch.randn(3, Hkv, 96, 64, generator=g).bfloat16()
    v = torch.randn(3, Hkv, 96, 64, generator=g).bfloat16()
    km = torch.rand(3, 96, generator=g) > 0.2
    L = torch.tensor(lens)
    ref = reference(q, k, v, seqlens=L, window=window, key_mask=km)
    sinks = choose_sinks(ref[1])
    assert bool(torch.isneginf(sinks[0])) and bool(torch.isfinite(sinks[1:]).all())
    got = with_sink(ref, sinks)
    want = _appended_key_reference(q, k, v, sinks, seqlens=L, window=window, key_mask=km)
    for a, b, what in zip(got, want, ("o", "lse", "pnorm")):
        fin = torch.isfinite(b)
        assert torch.equal(torch.isfinite(a), fin), what
        assert torch.equal(a[~fin], b[~fin]), what
        assert float((a - b)[fin].abs().max()) <= 1e-12, (what, float((a - b)[fin].abs().max()))
    dead = torch.isneginf(ref[1])
    assert bool(dead.any()) and bool((got[0][dead] == 0).all())
    assert torch.equal(got[1][dead], sinks.double().view(1, -1, 1).expand_as(dead)[dead])          # LSE = sink, -inf where the sink is


def test_the_sinks_the_gpu_tests_choose_matter():
    n = 0
    for name, c, out32 in CASES():
        frac = assert_sinks_matter(c["ref"], c["sinks"], c["dtype"], c["vmax"], out32)
        assert bool(torch.isneginf(c["sinks"][0])) and bool(torch.isfinite(c["sinks"][1:]).all()), name
        print(f"{name}: {frac:.3f} of the rows have a sink share in [0.2, 0.8]")
        n += 1
    assert n > 60

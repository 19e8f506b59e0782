"""CPU-side tests (no GPU) of the FP8 (e4m3fn) KV cache: ``pfa_fa3_kv_quant`` and the ``pfa_fa3_decode_q8*`` / ``pfa_kv_append_q8*`` entry
points (ABI v9 additive) -- every field rule in its documented order, names, split counts and
workspace sizes equal to the 16-bit call's -- then ``ops``' refusals, ``quantize_kv`` / ``dequantize_kv``, the plain-torch model of the
quantising append (placement, saturation, NaN) and ``PagedKVCache`` in FP8 on CPU tensors."""

from __future__ import annotations

import ctypes as C
import os

import pytest
import torch

from capi_testlib import ALIGN, DTYPE, FLAGS, HEAD_DIM, NULL, SHAPE, SIZE, STRIDE, decode_args, decode_paged, lib, quant, ref  # noqa: F401
from conftest import REPO
from photonic_flash_attention_amd import _capi, ops

FP8 = torch.float8_e4m3fn
KD, VD = 0x7000, 0x7400


def _dargs(**over):
    """A valid contiguous block of the decode over one-byte caches: B 2, H 8, Hkv 2, Sq 5, Smax 1024, D 128, with a workspace."""
    return decode_args(over, Sq=5, Smax=1024)


def _paged(**over):
    return decode_paged(over, Sq=5, Smax=1024)


def _aargs(**over):
    """A valid block of the append: B 2, Hkv 2, 3 rows each, D 64, into [B, Smax 256, Hkv, D] one-byte caches."""
    d, hkv, sq, smax = over.get("D", 64), over.get("Hkv", 2), 3, 256
    base = dict(k_new=0x1000, v_new=0x2000, k_cache=0x1000000, v_cache=0x2000000, cache_seqlens=0x5000, B=2, Hkv=hkv, total_new=2 * sq,
                max_seqlen_q=sq, Smax=smax, D=d, dtype=0, kn_stride_b=sq * hkv * d, kn_stride_s=hkv * d, kn_stride_h=d,
                vn_stride_b=sq * hkv * d, vn_stride_s=hkv * d, vn_stride_h=d, k_stride_b=smax * hkv * d, k_stride_h=d, k_stride_s=hkv * d,
                v_stride_b=smax * hkv * d, v_stride_h=d, v_stride_s=hkv * d)
    base.update(over)
    return _capi.make_kv_append_args(**base)


def test_the_fp8_dtype_value_the_abi_history_entry_and_the_quant_block_defaults():
    header = open(os.path.join(REPO, "include", "pfa_hip.h")).read()
    assert "PFA_DTYPE_FP8_E4M3 = 3" in header
    assert "pfa_fa3_decode_q8*" in header.split("Reference seam")[0]            # the ABI history names it
    assert _capi.PFA_DTYPE_FP8_E4M3 == 3
    assert _capi.make_kv_quant().size == 40 and _capi.make_kv_quant().kv_dtype == 3


def _quant_rules(chk, make, ok_over=None):
    """The rules of pfa_fa3_kv_quant and of one-byte caches, each alone and in their order, for ``chk(a, quant)`` over blocks ``make``."""
    ok = make()
    assert chk(ok, quant()) == 0
    assert chk(ok, quant(descale_stride_b=2)) == 0 and chk(ok, quant(descale_stride_b=64)) == 0
    # each rule alone
    assert chk(None, quant()) == NULL
    short = make()
    short.size -= 8
    assert chk(short, quant()) == SIZE
    assert chk(ok, None) == NULL
    wrong = quant()
    for size in (32, 48):
        wrong.size = size
        assert chk(ok, wrong) == SIZE
    assert chk(ok, quant(flags=1)) == FLAGS
    assert chk(ok, quant(reserved=1)) == FLAGS
    for dt in (0, 1, 2, 4, -1):
        assert chk(ok, quant(kv_dtype=dt)) == DTYPE
    assert chk(ok, quant(k_descale=0)) == NULL and chk(ok, quant(v_descale=0)) == NULL
    assert chk(ok, quant(k_descale=KD + 2)) == ALIGN and chk(ok, quant(v_descale=VD + 1)) == ALIGN
    assert chk(ok, quant(descale_stride_b=1)) == STRIDE and chk(ok, quant(descale_stride_b=-2)) == STRIDE
    for f in ("k_stride_b", "k_stride_h", "k_stride_s", "v_stride_b", "v_stride_h", "v_stride_s"):
        a = make()
        setattr(a, f, getattr(a, f) + 8)                                         # a multiple of 8 passes the 16-bit rule, not this one
        assert chk(a, quant()) == STRIDE, f
    assert chk(make(k_stride_s=-256), quant()) == STRIDE and chk(make(v_stride_s=-256), quant()) == STRIDE
    assert chk(make(k_cache=0x1000008), quant()) == ALIGN and chk(make(v_cache=0x2000004), quant()) == ALIGN
    # the order: each rule wins over all that follow it
    bad = make(k_stride_s=264, k_cache=0x1000008)
    every = dict(flags=1, kv_dtype=0, k_descale=0, v_descale=VD + 2, descale_stride_b=1)
    q = quant(**every)
    q.size = 8
    assert chk(bad, q) == SIZE
    assert chk(bad, quant(**every)) == FLAGS
    del every["flags"]
    assert chk(bad, quant(**every)) == DTYPE
    del every["kv_dtype"]
    assert chk(bad, quant(**every)) == NULL
    del every["k_descale"]
    assert chk(bad, quant(**every)) == ALIGN
    del every["v_descale"]
    assert chk(bad, quant(**every)) == STRIDE                                   # descale_stride_b
    assert chk(bad, quant()) == STRIDE                                          # the cache stride in front of the cache base
    assert chk(make(k_cache=0x1000008), quant()) == ALIGN
    # the block's own size comes first of all; its other rules behind the quant block's
    short = make(k_stride_s=264)
    short.size -= 8
    assert chk(short, quant(flags=1)) == SIZE
    return ok


def test_decode_q8_field_rules_in_their_order(lib):
    for make in (_dargs, _paged):
        def chk(a, q, ext=None):
            return lib.pfa_fa3_decode_q8_check(ref(a), ref(ext), ref(q))
        ok = _quant_rules(chk, make)
        # a window does not combine; window = 0 and a NULL extension are the plain call
        assert chk(ok, quant(), _capi.make_cache_ext(window=4)) == FLAGS
        assert chk(ok, quant(), _capi.make_cache_ext(window=0)) == 0
        assert chk(make(k_cache=0x1000008), quant(), _capi.make_cache_ext(window=4)) == ALIGN      # the cache base in front of the window
        assert chk(make(D=96), quant(), _capi.make_cache_ext(window=4)) == FLAGS                   # ... which is in front of the old rules
        # then the unchanged rules of pfa_fa3_decode_ex: the same status for every block the quant rules pass
        for over in (dict(q=0), dict(B=0), dict(D=96), dict(dtype_out=1), dict(dtype_in=2), dict(o=0x800008), dict(flags=1), dict(reserved0=1),
                     dict(Sq=65), dict(workspace=0), dict(workspace_bytes=16), dict(softmax_scale=0.0), dict(q_stride_s=4), dict(o_stride_s=6),
                     dict(H=7), dict(key_mask=0x6000, key_mask_stride_b=1024), dict(causal=0), dict(dtype_out=2)):
            a = make(**over)
            assert chk(a, quant()) == lib.pfa_fa3_decode_check_ex(C.byref(a), None), over
        bad_ext = _capi.make_cache_ext(window=-1)
        assert chk(ok, quant(), bad_ext) == lib.pfa_fa3_decode_check_ex(C.byref(ok), C.byref(bad_ext)) == SHAPE
        assert chk(ok, quant(), _capi.make_cache_ext(flags=1)) == FLAGS
        # dtype_in stays q's dtype: FP8 is refused there
        assert chk(make(dtype_in=3), quant()) == DTYPE
        # describe and the launch entry refuse the same way (nothing is launched: the status comes first)
        with pytest.raises(_capi.PfaError) as e:
            _capi.describe_decode_q8(ok, None, quant(kv_dtype=1))
        assert e.value.status == DTYPE
        assert lib.pfa_fa3_decode_q8(C.byref(ok), None, C.byref(quant(k_descale=0)), None) == NULL
        assert lib.pfa_fa3_decode_q8(C.byref(ok), None, None, None) == NULL


def test_append_q8_field_rules_in_their_order(lib):
    def chk(a, q):
        return lib.pfa_kv_append_q8_check(ref(a), ref(q))
    ok = _quant_rules(chk, _aargs)
    pg = dict(k_stride_b=64 * 2 * 64, v_stride_b=64 * 2 * 64, block_table=0x8000, block_table_stride_b=4, page_size=64, num_pages=9)
    assert chk(_aargs(**pg), quant()) == 0
    assert chk(_aargs(cu_seqlens_q=0x6000, kn_stride_b=0, vn_stride_b=0), quant()) == 0
    for d in (16, 48, 256):
        assert chk(_aargs(D=d), quant()) == 0
    for d in (8, 24, 72):                                                        # fine for the 16-bit append, not for 16-element items
        a = _aargs(D=d, k_stride_b=256 * 2 * 80, v_stride_b=256 * 2 * 80, k_stride_h=80, v_stride_h=80, k_stride_s=160, v_stride_s=160)
        assert lib.pfa_kv_append_check(C.byref(a)) == 0 and chk(a, quant()) == HEAD_DIM, d
    assert chk(_aargs(D=272), quant()) == HEAD_DIM                              # past 256: the 16-bit append's own rule
    for over in (dict(k_new=0), dict(cache_seqlens=0), dict(B=0), dict(dtype=2), dict(dtype=3), dict(kn_stride_s=4), dict(k_new=0x1008),
                 dict(flags=1), dict(reserved1=1), dict(page_size=64), dict(total_new=5), dict(max_seqlen_q=0)):
        a = _aargs(**over)
        assert chk(a, quant()) == lib.pfa_kv_append_check(C.byref(a)) != 0, over
    assert lib.pfa_kv_append_q8(C.byref(ok), C.byref(quant(v_descale=0)), None) == NULL
    assert lib.pfa_kv_append_q8(C.byref(ok), None, None) == NULL


@pytest.mark.parametrize("smax, want_ns", [(128, 1), (1024, 4)])
def test_names_splits_and_workspace_are_the_16_bit_calls(lib, smax, want_ns):
    for make in (_dargs, _paged):
        for over in (dict(), dict(D=64, dtype_in=1, dtype_out=1), dict(dtype_out=2), dict(causal=0), dict(Sq=1),
                     dict(B=8, H=32, Hkv=8, Sq=1)):
            a = make(Smax=smax, **over)
            name0, items0, ns0 = _capi.describe_decode_ex(a, None)
            ws0 = lib.pfa_fa3_decode_workspace_bytes_ex(C.byref(a), None)
            if "B" not in over:
                assert ns0 == want_ns and (ws0 > 0) == (want_ns > 1)
            for q in (quant(), quant(descale_stride_b=a.Hkv), quant(k_descale=0x123450)):
                for ext in (None, _capi.make_cache_ext()):
                    name, items, ns = _capi.describe_decode_q8(a, ext, q)
                    assert (items, ns) == (items0, ns0)
                    head, plus, tail = name0.partition("+combine") if "+combine" in name0 else name0.partition("_paged")
                    assert name == head + "_kv8" + plus + tail and "_kv8" not in name0
                    assert lib.pfa_fa3_decode_q8_workspace_bytes(C.byref(a), ref(ext), C.byref(q)) == ws0
            # the workspace query takes no pointers and skips the pointer and stride rules; what the other rules refuse is 0
            assert lib.pfa_fa3_decode_q8_workspace_bytes(C.byref(a), None, C.byref(quant(k_descale=0, v_descale=0))) == ws0
            assert lib.pfa_fa3_decode_q8_workspace_bytes(C.byref(a), None, C.byref(quant(kv_dtype=0))) == 0
            assert lib.pfa_fa3_decode_q8_workspace_bytes(C.byref(a), None, None) == 0
            assert lib.pfa_fa3_decode_q8_workspace_bytes(C.byref(a), C.byref(_capi.make_cache_ext(window=8)), C.byref(quant())) == 0
    assert _capi.describe_decode_q8(_dargs(Smax=128), None, quant())[0] == "fa3_decode_bf16_d128_o16_kv8"
    assert _capi.describe_decode_q8(_dargs(), None, quant())[0] == "fa3_decode_bf16_d128_o16_kv8+combine"
    assert _capi.describe_decode_q8(_paged(D=64, dtype_in=1, dtype_out=2), None, quant())[0] == "fa3_decode_fp16_d64_o32_kv8+combine_paged"
    assert _capi.describe_decode_q8(_paged(Smax=128), None, quant())[0] == "fa3_decode_bf16_d128_o16_kv8_paged"


# --- ops: refusals ------------------------------------------------------------------------------------------------------------------

def _operands(B=2, H=8, Hkv=2, Sq=4, Smax=512, D=128):
    q = torch.zeros(B, H, Sq, D, dtype=torch.bfloat16)
    k8 = torch.zeros(B, Hkv, Smax, D, dtype=FP8)
    return q, k8, k8.clone(), torch.ones(Hkv), torch.ones(Hkv)


def test_fa3_decode_refuses_what_an_fp8_cache_does_not_take():
    q, k8, v8, kd, vd = _operands()
    lens = torch.tensor([100, 100], dtype=torch.int32)

    def call(**kw):
        return ops.fa3_decode(q, k8, v8, **{"k_descale": kd, "v_descale": vd, **kw})

    for kw, name in ((dict(window=16), "window"), (dict(tree_mask=torch.ones(2, 4, dtype=torch.int64)), "tree_mask"),
                     (dict(shared_prefix=64, cache_seqlens=lens), "shared_prefix"),
                     (dict(rotary_cos=torch.zeros(8, 64), rotary_sin=torch.zeros(8, 64)), "rotary_cos / rotary_sin")):
        with pytest.raises(ValueError, match=f"{name} is not supported with an FP8"):
            call(**kw)
    # the descales: required with FP8 caches, refused without them
    for kw in (dict(k_descale=None), dict(v_descale=None), dict(k_descale=None, v_descale=None)):
        with pytest.raises(ValueError, match="caches need k_descale and v_descale"):
            call(**kw)
    kb = torch.zeros(2, 2, 512, 128, dtype=torch.bfloat16)
    for kw in (dict(k_descale=kd), dict(v_descale=vd), dict(k_descale=kd, v_descale=vd)):
        with pytest.raises(ValueError, match="go with torch.float8_e4m3fn caches only"):
            ops.fa3_decode(q, kb, kb.clone(), **kw)
    with pytest.raises(ValueError, match="must both be torch.float8_e4m3fn"):
        ops.fa3_decode(q, k8, kb, k_descale=kd, v_descale=vd)
    for bad in (torch.ones(3), torch.ones(2, 3), torch.ones(2, dtype=torch.float64), torch.ones(2, 4)[:, ::2], [1.0, 1.0], torch.ones(1, 2)):
        with pytest.raises(ValueError, match="k_descale must be a contiguous fp32 tensor"):
            call(k_descale=bad)
    with pytest.raises(ValueError, match="must have one shape"):
        call(v_descale=torch.ones(2, 2))
    with pytest.raises(ValueError, match="v_descale must live on the operands' device"):
        call(v_descale=torch.ones(2, device="meta"))
    with pytest.raises(ValueError, match="q must be bf16 or fp16"):
        ops.fa3_decode(q.float(), k8, v8, k_descale=kd, v_descale=vd)
    # good arguments: the next refusal is the usual one (the decode has no CPU path)
    for kw in (dict(), dict(k_descale=torch.ones(2, 2), v_descale=torch.ones(2, 2)), dict(causal=False, out_dtype=torch.float32),
               dict(cache_seqlens=lens, return_lse=True)):
        with pytest.raises(ValueError, match="device tensors"):
            call(**kw)


def test_kv_append_refusals_with_an_fp8_cache():
    _, k8, v8, kd, vd = _operands()
    kn = torch.zeros(2, 2, 3, 128, dtype=torch.bfloat16)
    lens = torch.tensor([10, 10], dtype=torch.int32)
    with pytest.raises(ValueError, match="caches need k_descale and v_descale"):
        ops.kv_append(kn, kn, k8, v8, cache_seqlens=lens)
    with pytest.raises(ValueError, match="go with torch.float8_e4m3fn caches only"):
        ops.kv_append(kn, kn, k8.to(torch.bfloat16), v8.to(torch.bfloat16), cache_seqlens=lens, k_descale=kd, v_descale=vd)
    with pytest.raises(ValueError, match="k_new, v_new must share dtype bf16 or fp16"):
        ops.kv_append(kn.to(FP8), kn.to(FP8), k8, v8, cache_seqlens=lens, k_descale=kd, v_descale=vd)
    with pytest.raises(ValueError, match="multiple of 16"):
        ops.kv_append(kn[..., :24], kn[..., :24], k8[..., :24], v8[..., :24], cache_seqlens=lens, k_descale=kd, v_descale=vd)


# --- quantize_kv / dequantize_kv and the model of the quantising append ----------------------------------------------------------------

def test_quantize_saturates_keeps_nan_and_rounds_to_nearest_even():
    x = torch.tensor([500.0, -1000.0, 448.0, -448.0, 464.0, 449.0, float("nan"), 0.0, -0.0, 17.0, 19.0, 2.0 ** -9, 2.0 ** -10, 1.5 * 2.0 ** -10,
                      float("inf"), -float("inf")]).reshape(1, 1, -1, 1)
    one = torch.ones(1)
    assert bool(torch.isnan(x.to(FP8).float()[0, 0, :2, 0]).all())               # the plain cast does not saturate: the clamp matters
    q = ops.quantize_kv(x, one)
    assert q.dtype == FP8 and q.shape == x.shape
    #            500  -1000   448  -448   464   449   nan   0    -0    17 (tie -> 16)  19 (tie -> 20)  2^-9  2^-10 (tie -> 0)  1.5 * 2^-10
    want = [0x7e, 0xfe, 0x7e, 0xfe, 0x7e, 0x7e, None, 0x00, 0x80, 0x58, 0x5a, 0x01, 0x00, 0x01, 0x7e, 0xfe]
    got = q.view(torch.uint8)[0, 0, :, 0].tolist()
    for i, (g, w) in enumerate(zip(got, want)):
        assert (g & 0x7f) == 0x7f if w is None else g == w, (i, hex(g))
    # the descale divides first: 448 * d saturates exactly at the edge, per head and per (batch, head)
    d = torch.tensor([0.37, 3.0])
    y = torch.tensor([[448 * 0.37, 500.0], [-4000.0, 1344.0]]).reshape(1, 2, 2, 1).repeat(3, 1, 1, 1)
    assert ops.quantize_kv(y, d).view(torch.uint8)[0, :, :, 0].tolist() == [[0x7e, 0x7e], [0xfe, 0x7e]]
    d2 = torch.tensor([[1.0, 1.0], [2.0, 0.5], [4.0, 1e-3]])
    z = torch.full((3, 2, 1, 1), 3.0)
    assert ops.quantize_kv(z, d2).float().flatten().tolist() == [3.0, 3.0, 1.5, 6.0, 0.75, 448.0]
    for dt in (torch.bfloat16, torch.float16):                                   # 16-bit sources go through fp32
        s = torch.randn(2, 2, 5, 16, generator=torch.Generator().manual_seed(1)).to(dt)
        assert torch.equal(ops.quantize_kv(s, d).view(torch.uint8), (s.float() / d[None, :, None, None]).clamp(-448, 448).to(FP8).view(torch.uint8))
    with pytest.raises(ValueError, match="descale"):
        ops.quantize_kv(z, torch.ones(3))
    with pytest.raises(ValueError, match="descale"):
        ops.quantize_kv(z, torch.ones(2, dtype=torch.float64))


def test_dequantize_is_exact_for_every_code():
    codes = torch.arange(256, dtype=torch.uint8).reshape(1, 1, 16, 16)
    x8 = codes.view(FP8)
    one = torch.ones(1)
    v64 = ops.dequantize_kv(x8, one, torch.float64)
    fin = ~torch.isnan(v64)
    assert int(fin.sum()) == 254 and not bool(fin.flatten()[0x7f]) and not bool(fin.flatten()[0xff])
    assert float(v64[fin].max()) == 448.0 and float(v64[fin].abs()[v64[fin] != 0].min()) == 2.0 ** -9
    for dt in (torch.bfloat16, torch.float16, torch.float32):                    # every e4m3 value is a value of the three
        assert torch.equal(ops.dequantize_kv(x8, one, dt).double()[fin], v64[fin])
        assert torch.equal(ops.quantize_kv(ops.dequantize_kv(x8, one, dt), one).view(torch.uint8)[fin], codes[fin])
    d = torch.tensor([0.3])
    assert torch.equal(ops.dequantize_kv(x8, d, torch.float64)[fin], v64[fin] * float(d.double()))
    assert torch.equal(ops.dequantize_kv(x8, d, torch.float32)[fin], x8.float()[fin] * d)
    with pytest.raises(ValueError, match="float8_e4m3fn"):
        ops.dequantize_kv(codes, one)


def _rows(shape, seed, dt=torch.bfloat16):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g) * 3.0
    x.view(-1)[::7] *= 200.0                                                     # values far beyond +-448 * descale
    x.view(-1)[5::31] = float("nan")
    return x.to(dt)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("paged", [False, True])
@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("per_batch", [False, True])
def test_the_append_model_places_like_the_16_bit_model_and_quantises(dt, paged, ragged, per_batch):
    B, Hkv, D, Smax, page = 4, 2, 32, 256, 64
    kd = torch.tensor([[0.37, 1.0], [2.5, 0.011], [1.0, 1.0], [0.6, 0.7]]) if per_batch else torch.tensor([0.37, 2.5])
    vd = kd * 1.3
    lens = torch.tensor([66, 2, 256, 0], dtype=torch.int32)                     # sequence 1 has fewer keys than rows: rows in front of key 0
    if ragged:
        cu, msq = torch.tensor([0, 5, 9, 12, 12], dtype=torch.int32), 5
        kn, vn = _rows((14, Hkv, D), 1, dt), _rows((14, Hkv, D), 2, dt)
        kw = dict(cu_seqlens_q=cu, max_seqlen_q=msq)
    else:
        kn, vn = _rows((B, Hkv, 5, D), 1, dt), _rows((B, Hkv, 5, D), 2, dt)
        kw = {}
    if paged:
        # sequence 0's rows 61 .. 65 straddle its pages 0 and 1, and page 1 has an id outside the pool: those rows are dropped
        table = torch.tensor([[3, 99, 1, 0], [2, 9, 9, 9], [4, 5, -1, 6], [8, 8, 8, 8]], dtype=torch.int32)
        shape = (10, Hkv, page, D)
        kw["block_table"] = table
    else:
        shape = (B, Hkv, Smax, D)
    # the 16-bit model on the dequantisable values: where it writes, and the FP8 model writes the quantised rows there
    k16, v16 = torch.full(shape, 7.0, dtype=dt), torch.full(shape, 7.0, dtype=dt)
    mark_k, mark_v = torch.ones_like(kn), torch.ones_like(vn) * 2
    ops.kv_append(mark_k, mark_v, k16, v16, cache_seqlens=lens, **kw)
    k8 = torch.full(shape, 0x7f, dtype=torch.uint8).view(FP8)                   # a NaN-patterned destination
    v8 = torch.full(shape, 0x7f, dtype=torch.uint8).view(FP8)
    ops.kv_append(kn, vn, k8, v8, cache_seqlens=lens, k_descale=kd, v_descale=vd, **kw)
    written = k16 == 1
    assert torch.equal(written, v16 == 2) and 0 < int(written.sum()) < written.numel()
    assert bool((k8.view(torch.uint8)[~written] == 0x7f).all()) and bool((v8.view(torch.uint8)[~written] == 0x7f).all())
    # value by value: scatter the expected bytes with the 16-bit model of a byte-exact carrier (every byte is an fp16 value)
    for new, d, got in ((kn, kd, k8), (vn, vd, v8)):
        if ragged:
            seq = torch.zeros(new.shape[0], dtype=torch.int64)
            for b in range(B):
                seq[int(cu[b]):int(cu[b + 1])] = b
            dd = (d[seq] if per_batch else d[None].expand(new.shape[0], Hkv))[..., None]
        else:
            dd = (d if per_batch else d[None].expand(B, Hkv))[..., None, None]
        want = (new.float() / dd).clamp(-448, 448).to(FP8).view(torch.uint8)
        carrier = torch.full(shape, 0x7f, dtype=torch.float16)
        ops.kv_append(want.to(torch.float16), want.to(torch.float16), carrier, carrier.clone(), cache_seqlens=lens, **kw)
        assert torch.equal(got.view(torch.uint8), carrier.to(torch.uint8))
        vals = got.float()[written]
        assert bool(torch.isnan(vals).any()) and float(vals[~torch.isnan(vals)].abs().max()) == 448.0        # NaN kept, the rest saturated


# --- PagedKVCache in FP8 on CPU tensors -------------------------------------------------------------------------------------------------

def _cache(**kw):
    from photonic_flash_attention_amd.integration.pytorch import PagedKVCache
    base = dict(num_pages=12, page_size=64, Hkv=2, D=64, dtype=FP8, device="cpu", max_batch=3, max_pages_per_seq=8,
                k_descale=torch.tensor([0.5, 0.031]), v_descale=torch.tensor([1.0, 0.7]))
    base.update(kw)
    return PagedKVCache(**base)


def _tok(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(1, 2, n, 64, generator=g).to(torch.bfloat16), torch.randn(1, 2, n, 64, generator=g).to(torch.bfloat16)


def _bytes(x):
    return x.view(torch.uint8)


def test_paged_cache_in_fp8_appends_gathers_forks_and_copies():
    c = _cache(copy_on_write=True)
    kd, vd = c._kd, c._vd
    assert c.k_pool.dtype == FP8 and c.k_pool.element_size() == 1
    s = c.allocate()
    k, v = _tok(70, 1)
    c.append(s, k, v)
    gk, gv = c.gather(s)
    assert gk.dtype == FP8 and gk.shape == (2, 70, 64)
    assert torch.equal(_bytes(gk), _bytes(ops.quantize_kv(k, kd)[0])) and torch.equal(_bytes(gv), _bytes(ops.quantize_kv(v, vd)[0]))
    # fork, then both write into the shared tail page: the child's append copies it through the 2-byte view
    child = c.fork(s)
    tail = c.pages(s)[1]
    assert c.pages(child) == c.pages(s) and c.page_refcount(tail) == 2
    ck, cv = _tok(3, 2)
    c.append(child, ck, cv)
    assert c.pages(child)[1] != tail and c.page_refcount(tail) == 1
    assert torch.equal(_bytes(c.gather(child)[0]), _bytes(ops.quantize_kv(torch.cat([k, ck], dim=2), kd)[0]))
    assert torch.equal(_bytes(c.gather(child)[1]), _bytes(ops.quantize_kv(torch.cat([v, cv], dim=2), vd)[0]))
    assert torch.equal(_bytes(c.gather(s)[0]), _bytes(gk))                       # the parent reads what it read
    # advance + write_step (the capturable form) through a fork's pending copy, packed rows
    c2 = c.fork(s)
    pk, pv = _tok(2, 3)
    c.advance([s, c2], [2, 1])
    c.write_step(torch.cat([pk[0], pk[0, :, :1]], dim=1).transpose(0, 1).contiguous(),
                 torch.cat([pv[0], pv[0, :, :1]], dim=1).transpose(0, 1).contiguous(), [2, 1], [s, c2])
    assert torch.equal(_bytes(c.gather(s)[0]), _bytes(ops.quantize_kv(torch.cat([k, pk], dim=2), kd)[0]))
    assert torch.equal(_bytes(c.gather(c2)[1]), _bytes(ops.quantize_kv(torch.cat([v, pv[:, :, :1]], dim=2), vd)[0]))
    # append_varlen, truncate, free
    c.truncate(child, 64)
    nk, nv = _tok(4, 4)
    c.append_varlen([child], nk[0].transpose(0, 1).contiguous(), nv[0].transpose(0, 1).contiguous(), [4])
    assert torch.equal(_bytes(c.gather(child)[0]), _bytes(ops.quantize_kv(torch.cat([k[:, :, :64], nk], dim=2), kd)[0]))
    for slot in (s, child, c2):
        c.free(slot)
    assert c.free_pages == 12


def test_paged_cache_in_fp8_refusals(monkeypatch):
    from photonic_flash_attention_amd.integration.pytorch import PagedKVCache, paged_cache
    kw = dict(num_pages=4, page_size=64, Hkv=2, D=64, device="cpu")
    for bad in (dict(), dict(k_descale=torch.ones(2)), dict(k_descale=torch.ones(2), v_descale=torch.ones(3)),
                dict(k_descale=torch.ones(1, 2), v_descale=torch.ones(1, 2)),           # per-sequence scales cannot coexist with shared pages
                dict(k_descale=torch.ones(2, dtype=torch.float64), v_descale=torch.ones(2))):
        with pytest.raises(ValueError, match="an FP8 cache needs"):
            PagedKVCache(dtype=FP8, **kw, **bad)
    with pytest.raises(ValueError, match="go with dtype=torch.float8_e4m3fn only"):
        PagedKVCache(dtype=torch.bfloat16, k_descale=torch.ones(2), v_descale=torch.ones(2), **kw)
    with pytest.raises(ValueError, match="multiple of 16"):
        PagedKVCache(dtype=FP8, k_descale=torch.ones(2), v_descale=torch.ones(2), **dict(kw, D=24))
    c = _cache()
    s = c.allocate()
    k, v = _tok(5, 1)
    with pytest.raises(ValueError, match="must be bf16 or fp16"):
        c.append(s, k.to(FP8), v.to(FP8))
    with pytest.raises(ValueError, match="must be bf16 or fp16"):
        c.append_varlen([s], k[0].transpose(0, 1).float(), v[0].transpose(0, 1).float(), [5])
    with pytest.raises(ValueError, match="prefill over an FP8 cache is not built"):
        c.prefill(torch.zeros(3, 8, 4, 64, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="prefill_varlen over an FP8 cache is not built"):
        c.prefill_varlen(torch.zeros(4, 8, 64, dtype=torch.bfloat16), [4, 0, 0])
    c.advance([s], [5])
    rows = k[0].transpose(0, 1).contiguous()
    with pytest.raises(ValueError, match="rotary is not fused into the quantising append"):
        c.write_step(rows, rows, [5], [s], rotary_cos=torch.zeros(8, 32), rotary_sin=torch.zeros(8, 32))
    with pytest.raises(ValueError, match="rotary is not fused into the quantising append"):
        c.write_step(rows, rows, [5], [s], q=torch.zeros(5, 8, 64, dtype=torch.bfloat16))
    # decode hands the cache's own scales to ops.fa3_decode, whose refusals stand
    seen = []
    monkeypatch.setattr(paged_cache.ops, "fa3_decode", lambda q, k, v, **kw: seen.append((k, kw)) or ("o", None))
    c.decode(torch.zeros(3, 8, 1, 64, dtype=torch.bfloat16), causal=False)
    assert seen[0][0].dtype == FP8 and seen[0][1]["k_descale"] is c._kd and seen[0][1]["v_descale"] is c._vd and seen[0][1]["causal"] is False
    monkeypatch.undo()
    with pytest.raises(ValueError, match="window is not supported with an FP8"):
        c.decode(torch.zeros(3, 8, 1, 64, dtype=torch.bfloat16), window=8)


def test_a_16_bit_paged_cache_is_what_it_was():
    from photonic_flash_attention_amd.integration.pytorch import PagedKVCache
    c = PagedKVCache(num_pages=4, page_size=64, Hkv=2, D=64, dtype=torch.bfloat16, device="cpu", copy_on_write=True, max_batch=2)
    s = c.allocate()
    k, v = _tok(70, 1)
    c.append(s, k, v)
    assert c.k_pool.dtype == torch.bfloat16 and torch.equal(c.gather(s)[0], k[0]) and torch.equal(c.gather(s)[1], v[0])
    child = c.fork(s)
    c.append(child, *_tok(1, 2))
    assert torch.equal(c.gather(child)[0][:, :70], k[0]) and c.pages(child)[1] != c.pages(s)[1]

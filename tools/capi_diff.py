#!/usr/bin/env python3
"""Do two builds of libpfa_hip.so validate, name and plan the calls over a KV cache alike?

    python tools/capi_diff.py OLD.so NEW.so [--cases 24000] [--seed 0]

Host code only: it calls the `*_check*`, `*_describe*` and `*_workspace_bytes*` exports of the decode, the prefill, the ragged prefill and
the split prefill (plain, `_ex`, `_tree`, `_q8`, `_sink`) and `pfa_fa3_prefill_split_plan`, never an export that launches, so it needs no
GPU; the pointers it passes are made-up addresses that validation compares and never follows.  A case is one argument block with one
choice of the optional blocks (ext, tree, quant, sinks: NULL, valid, or valid with one field spoilt), given to every such export of its
family in both libraries; the argument block is a valid one or a valid one with one field spoilt.  Compared: the status or count each
export returns, the whole name buffer (pre-filled, so a byte written behind the name shows) and nsplit.  The first part crosses every
spoilt argument block with every variant of every block, the rest is drawn from a fixed seed.  Exit status 1 on any difference."""
import argparse
import ctypes as C
import importlib.util
import os
import random
import sys

_spec = importlib.util.spec_from_file_location(
    "_pfa_capi", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "photonic_flash_attention_amd", "_capi.py"))
capi = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(capi)

LAUNCHING = ("pfa_fa3_decode", "pfa_fa3_prefill", "pfa_fa3_prefill_varlen", "pfa_fa3_prefill_split")
PTR = 0x7F0000100000           # made-up device addresses, 1 MiB apart, never followed


def is_query(name):
    return name == "pfa_fa3_prefill_split_plan" or any(s in name for s in ("_check", "_describe", "_workspace_bytes"))


def load(path):
    lib = C.CDLL(os.path.abspath(path))
    for name, (restype, argtypes) in capi._PROTOTYPES.items():
        if name.startswith(LAUNCHING) and is_query(name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
    lib.pfa_abi_version.restype = C.c_int
    return lib


# ---- valid blocks ------------------------------------------------------------------------------------------------------------------
def base_args(rng, varlen):
    """A valid argument block of the family: pfa_fa3_decode_args (decode, prefill, split) or pfa_fa3_prefill_varlen_args."""
    Hkv = rng.choice((1, 2, 8))
    H = Hkv * rng.choice((1, 4))
    D = rng.choice((64, 128))
    B = rng.choice((1, 2, 5))
    Sq = rng.choice((1, 1, 3, 16, 64, 65, 256, 300, 2048))
    paged = rng.random() < 0.4
    page = rng.choice((64, 128, 256))
    Smax = rng.choice((64, 192, 1024, 4096, 32768, 131072))
    if paged:
        Smax = (Smax + page - 1) // page * page
    dt = rng.choice((capi.PFA_DTYPE_BF16, capi.PFA_DTYPE_FP16))
    kw = dict(q=PTR, k_cache=2 * PTR, v_cache=3 * PTR, o=4 * PTR, lse=rng.choice((0, 5 * PTR)), cache_seqlens=rng.choice((0, 6 * PTR)),
              q_stride_s=H * D, q_stride_h=D, o_stride_s=H * D, o_stride_h=D,
              k_stride_b=(page if paged else Smax) * Hkv * D, k_stride_s=Hkv * D, k_stride_h=D,
              v_stride_b=(page if paged else Smax) * Hkv * D, v_stride_s=Hkv * D, v_stride_h=D,
              B=B, H=H, Hkv=Hkv, Smax=Smax, D=D, dtype_in=dt, dtype_out=rng.choice((dt, capi.PFA_DTYPE_FP32)), causal=rng.choice((0, 1, 1)),
              softmax_scale=D ** -0.5, device_id=0)
    if paged:
        kw.update(block_table=7 * PTR, block_table_stride_b=Smax // page + rng.choice((0, 3)), page_size=page, num_pages=rng.choice((1, 4096)))
    if varlen:
        kw.update(cu_seqlens_q=8 * PTR, max_seqlen_q=Sq, total_q=Sq * B + rng.choice((0, 7)))
        return capi._make(capi.PfaFa3PrefillVarlenArgs, kw)
    kw.update(Sq=Sq, q_stride_b=Sq * H * D, o_stride_b=Sq * H * D, workspace=9 * PTR, workspace_bytes=1 << 40)
    return capi._make(capi.PfaFa3DecodeArgs, kw)


def put(**kw):
    def f(a):
        for k, v in kw.items():
            if hasattr(a, k):
                setattr(a, k, v(a) if callable(v) else v)
    return f


# one field of a valid argument block spoilt (a field the block does not have leaves it valid)
ARG_MUTATIONS = [put()] + [put(**{k: v}) for k, v in (
    ("size", 8), ("flags", 1), ("reserved0", 1), ("q", 0), ("k_cache", 0), ("o", 0), ("q", PTR + 8), ("v_cache", 3 * PTR + 4), ("lse", 5 * PTR + 2),
    ("cache_seqlens", 6 * PTR + 1), ("dtype_in", capi.PFA_DTYPE_FP32), ("dtype_in", capi.PFA_DTYPE_FP8_E4M3), ("dtype_out", 7),
    ("dtype_out", lambda a: 1 - a.dtype_in), ("D", 96), ("D", 0), ("D", 256), ("Sq", 0), ("Sq", 1), ("Sq", 64), ("Sq", 65), ("max_seqlen_q", 0),
    ("max_seqlen_q", 1), ("max_seqlen_q", 64), ("max_seqlen_q", 65), ("max_seqlen_q", lambda a: a.total_q + 1), ("total_q", 0), ("cu_seqlens_q", 0),
    ("cu_seqlens_q", 8 * PTR + 2), ("H", lambda a: a.Hkv * 3 + 1), ("Hkv", 0), ("B", 0), ("B", 1 << 20), ("Smax", 0), ("Smax", lambda a: a.Smax + 32),
    ("key_mask", 10 * PTR), ("key_mask", 10 * PTR + 1), ("softmax_scale", 0.0), ("softmax_scale", float("inf")), ("softmax_scale", float("nan")),
    ("q_stride_s", lambda a: a.q_stride_s + 4), ("k_stride_s", lambda a: a.k_stride_s + 8), ("v_stride_h", lambda a: a.v_stride_h + 4),
    ("k_stride_s", -128), ("v_stride_s", 1 << 27), ("o_stride_s", lambda a: a.o_stride_s + 4), ("o_stride_h", lambda a: a.o_stride_h + 2),
    ("o_stride_b", lambda a: a.o_stride_b + 4), ("k_stride_b", lambda a: a.k_stride_b + 8), ("causal", 0), ("causal", 1), ("causal", 2),
    ("block_table", 0), ("block_table", 7 * PTR + 2), ("page_size", 0), ("page_size", 32), ("page_size", 64), ("page_size", 96), ("num_pages", 0),
    ("num_pages", 5), ("block_table_stride_b", 0), ("block_table_stride_b", 1), ("block_table", 7 * PTR),
    ("workspace", 0), ("workspace", 9 * PTR + 8), ("workspace_bytes", 0), ("workspace_bytes", 4096), ("workspace_bytes", lambda a: 1 << 20),
    ("device_id", 3),
)] + [None]                  # (the last one: the NULL argument block, see mutate())
NULL_ARGS = len(ARG_MUTATIONS) - 1


def mutate(a, i):
    if i == NULL_ARGS:
        return None
    ARG_MUTATIONS[i](a)
    return a


def block_variants(cls, valid, spoilt):
    """None, the valid blocks, and the first valid block with one field spoilt."""
    out = [None] + [capi._make(cls, kw) for kw in valid]
    for k, v in spoilt:
        kw = dict(valid[0])
        kw[k] = v
        out.append(capi._make(cls, kw))
    return out


def ext_variants(Smax):
    return block_variants(capi.PfaFa3CacheExt, [dict(window=w) for w in (0, 1, 17, 64, 1000, Smax - 1, Smax, Smax + 5, 2**31 - 1)],
                          [("size", 12), ("size", 0), ("flags", 1), ("reserved", 1), ("window", -1), ("window", -(2**31))])


TREE = block_variants(capi.PfaFa3TreeMask, [dict(words=11 * PTR, stride_b=64), dict(words=11 * PTR, stride_b=4096)],
                      [("size", 8), ("flags", 2), ("words", 0), ("words", 11 * PTR + 4), ("stride_b", 0), ("stride_b", 2), ("stride_b", -1)])
QUANT = block_variants(capi.PfaFa3KvQuant,
                       [dict(kv_dtype=capi.PFA_DTYPE_FP8_E4M3, k_descale=12 * PTR, v_descale=13 * PTR, descale_stride_b=s) for s in (0, 8, 1024)],
                       [("size", 16), ("flags", 1), ("reserved", 1), ("kv_dtype", capi.PFA_DTYPE_BF16), ("k_descale", 0), ("v_descale", 0),
                        ("k_descale", 12 * PTR + 2), ("v_descale", 13 * PTR + 1), ("descale_stride_b", 1), ("descale_stride_b", -8)])
SINKS = block_variants(capi.PfaFa3Sinks, [dict(sinks=14 * PTR)], [("size", 8), ("size", 24), ("flags", 1), ("sinks", 0), ("sinks", 14 * PTR + 2)])
KEY_SPLITS = list(range(-1, 10))
BUFS = ((128, False), (128, False), (128, False), (24, False), (1, False), (0, False), (128, True))       # (n, NULL buffer)


# ---- one case ----------------------------------------------------------------------------------------------------------------------
def ref(x):
    return None if x is None else C.byref(x)


def describe(fn, lead, n, null_buf, nsplit):
    buf = C.create_string_buffer(b"\xa5" * 160, 160)
    ns = C.c_int32(-777)
    r = fn(*lead, None if null_buf else buf, n, *([C.byref(ns)] if nsplit else []))
    return (r, buf.raw, ns.value)


def run_case(lib, family, a, ext, tree, quant, sinks, ks, n, null_buf):
    """Every query export of the family on these blocks -> the list of what they returned."""
    A, E, T, Q, S = ref(a), ref(ext), ref(tree), ref(quant), ref(sinks)
    out = []
    if family == "decode":
        p = "pfa_fa3_decode"
        for sfx, lead in (("", (A,)), ("_ex", (A, E)), ("_tree", (A, E, T)), ("_q8", (A, E, Q)), ("_sink", (A, E, S))):
            stem = p + sfx.replace("_ex", "")
            tail = "_ex" if sfx == "_ex" else ""
            out.append(getattr(lib, f"{stem}_workspace_bytes{tail}")(*lead))
            out.append(getattr(lib, f"{stem}_check{tail}")(*lead))
            out.append(describe(getattr(lib, f"{stem}_describe{tail}"), lead, n, null_buf, True))
    elif family in ("prefill", "varlen"):
        p = "pfa_fa3_prefill" if family == "prefill" else "pfa_fa3_prefill_varlen"
        for sfx, lead in (("", (A,)), ("_ex", (A, E)), ("_q8", (A, E, Q)), ("_sink", (A, E, S))):
            stem = p + sfx.replace("_ex", "")
            tail = "_ex" if sfx == "_ex" else ""
            out.append(getattr(lib, f"{stem}_check{tail}")(*lead))
            out.append(describe(getattr(lib, f"{stem}_describe{tail}"), lead, n, null_buf, False))
    else:
        out.append(lib.pfa_fa3_prefill_split_plan(A, ks))
        for stem, lead in (("pfa_fa3_prefill_split", (A, ks)), ("pfa_fa3_prefill_split_sink", (A, ks, S))):
            out.append(getattr(lib, stem + "_workspace_bytes")(*lead))
            out.append(getattr(lib, stem + "_check")(*lead))
            out.append(describe(getattr(lib, stem + "_describe"), lead, n, null_buf, True))
    return out


def cases(rng, total):
    """(family, argument block, ext, tree, quant, sinks, key_splits, n, NULL buffer), `total` of them."""
    count = 0
    # every spoilt argument block against every variant of each block in turn, the other blocks NULL or valid
    for family in ("decode", "prefill", "varlen", "split"):
        for i in range(len(ARG_MUTATIONS)):
            probe = base_args(random.Random(i), family == "varlen")
            exts = ext_variants(probe.Smax)
            axes = [(0, exts), (1, TREE if family == "decode" else [None]), (2, QUANT), (3, SINKS)]
            if family == "split":
                axes = [(3, SINKS), (4, KEY_SPLITS)]
            for axis, variants in axes:
                for v in variants:
                    for others_valid in (False, True):
                        a = mutate(base_args(random.Random(i), family == "varlen"), i)
                        blocks = [exts[2], TREE[1], QUANT[1], SINKS[1], 0] if others_valid else [None, None, None, None, 0]
                        if others_valid and axis != 1:
                            blocks[1] = None              # a tree refuses the window of exts[2]: keep it for its own axis
                        blocks[axis] = v
                        yield (family, a, *blocks, 128, False)
                        count += 1
    # ... and the rest at random
    while count < total:
        family = rng.choice(("decode", "decode", "prefill", "varlen", "split"))
        a = base_args(rng, family == "varlen")
        Smax = a.Smax
        muts = rng.choice((0, 0, 1, 1, 1, 2))
        for _ in range(muts):
            a = mutate(a, rng.randrange(len(ARG_MUTATIONS))) if a is not None else None
        n, null_buf = rng.choice(BUFS)
        yield (family, a, rng.choice(ext_variants(Smax)) if rng.random() < 0.7 else None, rng.choice(TREE) if rng.random() < 0.4 else None,
               rng.choice(QUANT) if rng.random() < 0.8 else None, rng.choice(SINKS) if rng.random() < 0.8 else None, rng.choice(KEY_SPLITS), n,
               null_buf)
        count += 1


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--cases", type=int, default=24000)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    old, new = load(args.old), load(args.new)
    print(f"ABI version: {old.pfa_abi_version()} / {new.pfa_abi_version()}")
    rng = random.Random(args.seed)
    n_cases = n_calls = n_diff = n_ok = 0
    per_family, statuses, names = {}, {}, set()
    for case in cases(rng, args.cases):
        r_old, r_new = run_case(old, *case), run_case(new, *case)
        n_cases += 1
        n_calls += len(r_old)
        per_family[case[0]] = per_family.get(case[0], 0) + 1
        for r in r_old:
            st = r[0] if isinstance(r, tuple) else r
            n_ok += st > 0
            if st < 0:
                statuses[st] = statuses.get(st, 0) + 1
            if isinstance(r, tuple) and st > 0 and case[7] == 128 and not case[8]:
                names.add(r[1].split(b"\0")[0])
        if r_old != r_new:
            n_diff += 1
            if n_diff <= 20:
                at = next(i for i, (x, y) in enumerate(zip(r_old, r_new)) if x != y)
                fields = None if case[1] is None else {k: getattr(case[1], k) for k, _ in case[1]._fields_}
                print(f"DIFFERENT {case[0]} export #{at}: {r_old[at]!r} / {r_new[at]!r}\n    args {fields}\n    blocks "
                      f"{[None if b is None or isinstance(b, int) else {k: getattr(b, k) for k, _ in b._fields_} for b in case[2:6]]} key_splits {case[6]}")
    print(f"{n_cases} cases ({', '.join(f'{k} {v}' for k, v in sorted(per_family.items()))}), {n_calls} calls per library, "
          f"{n_ok} of them answered with a count above 0 under {len(names)} distinct kernel names, error statuses "
          f"{dict(sorted(statuses.items(), reverse=True))} (old library); {n_diff} cases differ")
    return 1 if n_diff or old.pfa_abi_version() != new.pfa_abi_version() else 0


if __name__ == "__main__":
    sys.exit(main())

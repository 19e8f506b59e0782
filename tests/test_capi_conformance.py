"""The one ABI conformance test (no GPU): every header under ``include/`` against the ctypes module that binds it (``HEADERS``:
``pfa_hip.h`` and ``_capi``, and the side headers with ``_capi_sinks``, ``_capi_rotary`` and ``_capi_qk_norm``) and the built library.

Every ``typedef struct pfa_*`` of a header has a mirror class in its module and every mirror a struct, with the same field names in the
same order and -- by one C program per header that ``gcc`` compiles -- the same ``sizeof`` and, per field, the same ``offsetof`` and
size.  Every function a header declares has a row in its module's ``_PROTOTYPES`` with the header's return and parameter types (a side
header's may name ``_capi``'s structs), every row is declared, no two headers share an export, and every symbol resolves.  The sizes
are pinned as literals too, so that a change made to both sides at once still shows, and the ABI version and the side headers' flag
values are pinned here and nowhere else.  The comparisons are plain functions over the tables, and three mutants show that they bite."""

from __future__ import annotations

import ctypes as C
import os
import re
import subprocess

import pytest

from capi_testlib import lib  # noqa: F401  (the fixture)
from conftest import REPO
from photonic_flash_attention_amd import _capi, _capi_qk_norm, _capi_rotary, _capi_sinks

INCLUDE = os.path.join(REPO, "include")

# every header with the module that binds it, and what a full reading of it finds: (structs, fields, prototypes)
HEADERS = {"pfa_hip.h": (_capi, (14, 402, 88)), "pfa_hip_train_sinks.h": (_capi_sinks, (1, 19, 10)),
           "pfa_hip_rotary.h": (_capi_rotary, (1, 36, 3)), "pfa_hip_qk_norm.h": (_capi_qk_norm, (2, 92, 7))}

# sizeof of every argument and option block, as ABI v9 shipped them
SIZES = dict(pfa_fa3_args=288, pfa_fa3_bwd_args=400, pfa_fa3_decode_args=256, pfa_fa3_prefill_varlen_args=224, pfa_fa3_cache_ext=16,
             pfa_fa3_tree_mask=24, pfa_kv_append_args=216, pfa_rope_append_args=328, pfa_attn_merge_args=624, pfa_page_copy_args=128,
             pfa_fa3_varlen_args=184, pfa_fa3_varlen_bwd_args=288, pfa_fa3_kv_quant=40, pfa_fa3_sinks=16,
             pfa_fa3_sink_grad_args=120, pfa_rotary_args=240, pfa_qk_norm_args=264, pfa_qk_norm_bwd_args=360)
# the flag bits of the side headers, as their #define lines spell them and as the bindings must have them
FLAG_DEFINES = {"pfa_hip_rotary.h": (_capi_rotary, {"PFA_ROTARY_INTERLEAVED": 1, "PFA_ROTARY_CONJUGATE": 2}),
                "pfa_hip_qk_norm.h": (_capi_qk_norm, {"PFA_QKNORM_INTERLEAVED": 1, "PFA_QKNORM_UNIT_OFFSET": 2})}

SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "size_t": C.c_size_t, "char*": C.c_char_p,
           "void*": C.c_void_p, "float*": C.c_void_p, "int32_t*": C.POINTER(C.c_int32), "double*": C.POINTER(C.c_double)}


# --- the header -----------------------------------------------------------------------------------------------------------------------

def parse_header(text):
    """-> ({struct: [field names in order]}, {function: (return type, [parameter types], as C spells them without ``const``)})."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", "", text, flags=re.S)
    structs = {}
    for name, body in re.findall(r"typedef\s+struct\s+(pfa_\w+)\s*\{(.*?)\}\s*\1\s*;", text, flags=re.S):
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            names = re.fullmatch(r".*?[\s*]((?:\w+(?:\[\w+\])?\s*,\s*)*\w+(?:\[\w+\])?)", decl, flags=re.S).group(1)
            fields += [n.split("[")[0].strip() for n in names.split(",")]             # ``int64_t a, b, c;`` and ``void* p[N];``
        structs[name] = fields
    protos = {}
    for ret, name, params in re.findall(r"^((?:const\s+)?\w+\s*\*?)\s*(pfa_\w+)\s*\(([^)]*)\)\s*;", text, flags=re.M):
        plist = [] if params.strip() == "void" else [re.fullmatch(r"(.*?[\s*])\w+", p.strip(), flags=re.S).group(1) for p in params.split(",")]
        protos[name] = tuple(re.sub(r"\bconst\b|\s+", "", t) for t in [ret] + plist)
    return structs, {k: (v[0], list(v[1:])) for k, v in protos.items()}


def c_layout(header_file, structs, workdir):
    """-> {struct: (sizeof, [(field, offsetof, sizeof the field)])} from one C program over the header."""
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{header_file}"', "int main(void) {"]
    for s, fields in structs.items():
        lines.append(f'  printf("{s} %zu\\n", sizeof({s}));')
        lines += [f'  printf("{s}.{f} %zu %zu\\n", offsetof({s}, {f}), sizeof((({s}*)0)->{f}));' for f in fields]
    src, exe = os.path.join(workdir, "layout.c"), os.path.join(workdir, "layout")
    with open(src, "w") as f:
        f.write("\n".join(lines + ["  return 0;", "}", ""]))
    subprocess.run(["gcc", "-I", INCLUDE, src, "-o", exe], check=True)
    out = {}
    for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines():
        key, *nums = line.split()
        s, _, f = key.partition(".")
        if f:
            out[s][1].append((f, int(nums[0]), int(nums[1])))
        else:
            out[s] = (int(nums[0]), [])
    return out


# --- the comparisons: plain functions over the tables, [] when all is well ------------------------------------------------------------------

def snake(cls_name):
    return re.sub(r"(?<!^)(?=[A-Z])", "_", cls_name).lower()


def mirrors_of(module):
    """{C struct name: mirror class} of every ``ctypes.Structure`` a module defines."""
    return {snake(n): t for n, t in vars(module).items()
            if isinstance(t, type) and issubclass(t, C.Structure) and t.__module__ == module.__name__}      # not what it imports


def struct_mismatches(structs, layout, mirrors, sizes):
    bad = [f"{s}: a struct of the header without a mirror" for s in structs if s not in mirrors]
    bad += [f"{s}: a mirror without a struct in the header" for s in mirrors if s not in structs]
    bad += [f"{s}: no pinned size" for s in structs if s not in sizes] + [f"{s}: a pinned size of no struct" for s in sizes if s not in structs]
    for s in (s for s in structs if s in mirrors):
        t = mirrors[s]
        names = [f for f, _ in t._fields_]
        if names != structs[s]:
            bad.append(f"{s}: field names {[(a, b) for a, b in zip(names, structs[s]) if a != b] or (names, structs[s])} (mirror, header)")
            continue
        size, fields = layout[s]
        if not size == C.sizeof(t) == sizes.get(s):
            bad.append(f"{s}: sizeof {size} in C, {C.sizeof(t)} in the mirror, {sizes.get(s)} pinned")
        for f, off, fsize in fields:
            d = getattr(t, f)
            if (off, fsize) != (d.offset, d.size):
                bad.append(f"{s}.{f}: offset {off} size {fsize} in C, offset {d.offset} size {d.size} in the mirror")
    return bad


def ctype_of(c_type, mirrors):
    """The ctypes type the binding gives a C parameter or return type: a pointer to a struct is a pointer to its mirror."""
    if c_type.endswith("*") and c_type[:-1] in mirrors:
        return C.POINTER(mirrors[c_type[:-1]])
    return SCALARS[c_type]


def prototype_mismatches(protos, table, mirrors):
    bad = [f"{n}: declared, no row in the table" for n in protos if n not in table]
    bad += [f"{n}: a row of the table, not declared" for n in table if n not in protos]
    for n in (n for n in protos if n in table):
        (ret, params), (restype, argtypes) = protos[n], table[n]
        if ctype_of(ret, mirrors) is not restype:
            bad.append(f"{n}: returns {ret}, the table has {restype}")
        want = [ctype_of(p, mirrors) for p in params]
        if argtypes is None:
            if params:
                bad.append(f"{n}: argtypes None for ({', '.join(params)}); only (void) may be left untyped")
        elif list(argtypes) != want:
            bad.append(f"{n}: takes ({', '.join(params)}) = {[t.__name__ for t in want]}, the table has {[t.__name__ for t in argtypes]}")
    return bad


# --- the tests ------------------------------------------------------------------------------------------------------------------------

def read_header(header_file, workdir):
    """(structs, prototypes, C layout) of one header."""
    structs, protos = parse_header(open(os.path.join(INCLUDE, header_file)).read())
    return structs, protos, c_layout(header_file, structs, workdir)


@pytest.fixture(scope="module")
def headers(tmp_path_factory):
    """{header file: (structs, prototypes, C layout)} of every header: each parsed and compiled once."""
    return {h: read_header(h, str(tmp_path_factory.mktemp("layout"))) for h in HEADERS}


@pytest.fixture(scope="module")
def header(headers):
    return headers["pfa_hip.h"]


def sizes_of(structs):
    return {s: n for s, n in SIZES.items() if s in structs}


def test_the_header_is_read_in_full(headers):
    for h, (structs, protos, layout) in headers.items():
        assert (len(structs), sum(len(f) for f in structs.values()), len(protos)) == HEADERS[h][1], h
        assert set(layout) == set(structs) and all(len(layout[s][1]) == len(structs[s]) for s in structs), h
    structs, protos, _ = headers["pfa_hip.h"]
    assert structs["pfa_fa3_cache_ext"] == ["size", "flags", "window", "reserved"]
    assert protos["pfa_abi_version"] == ("int", []) and protos["pfa_status_string"] == ("char*", ["int"])
    assert protos["pfa_fa3_prefill_split_sink_describe"] == ("int", ["pfa_fa3_decode_args*", "int32_t", "pfa_fa3_sinks*", "char*", "size_t",
                                                                     "int32_t*"])
    assert list(headers["pfa_hip_train_sinks.h"][0]) == ["pfa_fa3_sink_grad_args"]
    assert list(headers["pfa_hip_rotary.h"][0]) == ["pfa_rotary_args"]
    assert sorted(headers["pfa_hip_rotary.h"][1]) == ["pfa_rotary", "pfa_rotary_check", "pfa_rotary_describe"]
    assert list(headers["pfa_hip_qk_norm.h"][0]) == ["pfa_qk_norm_args", "pfa_qk_norm_bwd_args"]
    assert sorted(headers["pfa_hip_qk_norm.h"][1]) == ["pfa_qk_norm", "pfa_qk_norm_bwd", "pfa_qk_norm_bwd_check", "pfa_qk_norm_bwd_describe",
                                                       "pfa_qk_norm_bwd_workspace_bytes", "pfa_qk_norm_check", "pfa_qk_norm_describe"]


def test_every_struct_matches_its_mirror_and_its_pinned_size(headers):
    for h, (structs, _, layout) in headers.items():
        assert struct_mismatches(structs, layout, mirrors_of(HEADERS[h][0]), sizes_of(structs)) == [], h
    assert set(SIZES) == {s for structs, _, _ in headers.values() for s in structs}


def test_every_prototype_matches_the_header_and_resolves(headers, lib):
    seen = set()
    for h, (_, protos, _) in headers.items():
        module = HEADERS[h][0]
        assert prototype_mismatches(protos, module._PROTOTYPES, dict(mirrors_of(_capi), **mirrors_of(module))) == [], h
        assert set(module.EXPORTS) == set(protos) and not seen & set(protos), h         # no two headers share an export
        seen |= set(protos)
        for name in protos:
            assert getattr(lib, name) is not None


def test_abi_version(lib):
    assert lib.pfa_abi_version() == _capi.PFA_ABI_VERSION == 9
    assert re.search(r"^#define PFA_ABI_VERSION 9$", open(os.path.join(INCLUDE, "pfa_hip.h")).read(), flags=re.M)
    for h, (module, flags) in FLAG_DEFINES.items():
        text = open(os.path.join(INCLUDE, h)).read()
        for name, value in flags.items():
            assert re.search(rf"^#define {name}\s+{value}u$", text, flags=re.M) and getattr(module, name) == value, name


# --- mutants: each hands a checker a spoilt table and expects the mismatch by name --------------------------------------------------------

def _mutant(cls, fields):
    return type(cls.__name__, (C.Structure,), {"_fields_": fields})


def test_mutant_two_fields_swapped_is_named(header):
    structs, _, layout = header
    f = list(_capi.PfaFa3BwdArgs._fields_)
    i, j = [n for n, _ in f].index("dq"), [n for n, _ in f].index("dk")            # same type: sizes and offsets stay, only the order tells
    f[i], f[j] = f[j], f[i]
    mirrors = dict(mirrors_of(_capi), pfa_fa3_bwd_args=_mutant(_capi.PfaFa3BwdArgs, f))
    bad = struct_mismatches(structs, layout, mirrors, sizes_of(structs))
    assert len(bad) == 1 and bad[0].startswith("pfa_fa3_bwd_args: field names") and "('dk', 'dq')" in bad[0]


def test_mutant_one_int32_widened_is_named(header):
    structs, _, layout = header
    f = [(n, C.c_int64 if n == "page_size" else t) for n, t in _capi.PfaFa3DecodeArgs._fields_]
    mirrors = dict(mirrors_of(_capi), pfa_fa3_decode_args=_mutant(_capi.PfaFa3DecodeArgs, f))
    bad = struct_mismatches(structs, layout, mirrors, sizes_of(structs))
    assert any(b.startswith("pfa_fa3_decode_args.page_size: offset 248 size 4 in C, offset 248 size 8") for b in bad), bad
    assert any(b.startswith("pfa_fa3_decode_args: sizeof 256 in C, 264 in the mirror") for b in bad), bad
    assert all(b.startswith("pfa_fa3_decode_args") for b in bad)


def test_mutant_one_argument_dropped_is_named(header):
    _, protos, _ = header
    restype, argtypes = _capi._PROTOTYPES["pfa_fa3_decode_tree"]
    table = dict(_capi._PROTOTYPES, pfa_fa3_decode_tree=(restype, argtypes[:-1]))
    bad = prototype_mismatches(protos, table, mirrors_of(_capi))
    assert len(bad) == 1 and bad[0].startswith("pfa_fa3_decode_tree: takes (pfa_fa3_decode_args*, pfa_fa3_cache_ext*, pfa_fa3_tree_mask*, void*)")

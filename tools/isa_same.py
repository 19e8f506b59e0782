#!/usr/bin/env python3
"""Are the kernels of two builds of one translation unit the same code?  Compares, function by function, the instruction text and the
kernel descriptor directives of two -save-temps device assemblies (`make asm ASM_SRC=...` leaves one in /tmp/pfa_asm; keep the one of
the commit to compare against under another name).

    python tools/isa_same.py OLD.s NEW.s

Prints one line per kernel of OLD: `same` (instruction for instruction, same register counts, LDS, scratch and kernarg size),
`DIFFERENT` with the first differing line, or `missing`; then the kernels only NEW has.  Exit status 1 if any differs or is missing.
Comments, debug labels and the order of functions in the file (with it the function index in `.LBB<function>_<block>` labels) are
ignored; nothing else is.  A kernel of OLD is matched with the kernel of
NEW that has its name and its template arguments, followed by nothing or by trailing `false` (`Lb0E`) / `void` arguments only: a template
that gained defaulted parameters keeps its old instantiations under longer mangled names."""
import re
import sys


def functions(path):
    """name -> (instruction lines, descriptor directives) of every .amdhsa_kernel in the file."""
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^(\w+):\s*; @\1\n(.*?)^\.Lfunc_end\d+:", text, flags=re.S | re.M):
        # (a local label carries the index of its function in the file, .LBB<function>_<block>: the order of functions is not compared)
        body = [re.sub(r"\.(LBB|LJTI)\d+_", r".\1_", re.sub(r"\s*;.*$", "", ln)).strip() for ln in m.group(2).splitlines()]
        out[m.group(1)] = [[ln.replace(m.group(1), "SELF") for ln in body if ln and not ln.startswith((".loc", ".file", ".cfi", ";"))], []]
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\w+)\n(.*?)^\s*\.end_amdhsa_kernel", text, flags=re.S | re.M):
        if m.group(1) in out:
            out[m.group(1)][1] = [ln.strip() for ln in m.group(2).splitlines() if ln.strip()]
    return out


def template_args(mangled):
    """The mangled name up to the end of its last template argument (a kernel returns void: the argument list closes in front of the
    first `EEv`), without demangling: binutils' c++filt does not know __bf16."""
    at = mangled.find("EEv")
    return mangled if at < 0 else mangled[:at]


def main():
    old, new = functions(sys.argv[1]), functions(sys.argv[2])
    sigs = {n: template_args(n) for n in new}
    bad, used = 0, set()
    for old_name, (ins, desc) in old.items():
        args = template_args(old_name)
        name = next((n for n, a2 in sigs.items() if a2.startswith(args) and re.fullmatch(r"(Lb0E)*v?", a2[len(args):])), None)
        if name is None:
            print(f"missing    {old_name}")
            bad += 1
            continue
        used.add(name)
        ins2, desc2 = new[name]
        if ins == ins2 and desc == desc2:
            print(f"same       {name}  ({len(ins)} lines)")
            continue
        bad += 1
        a, b = (ins, ins2) if ins != ins2 else (desc, desc2)
        at = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
        print(f"DIFFERENT  {name}: line {at}: {a[at] if at < len(a) else '<end>'!r} / {b[at] if at < len(b) else '<end>'!r}")
    for name in new:
        if name not in used:
            print(f"new        {name}")
    print(f"{len(old) - bad} of {len(old)} kernels unchanged")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Build code objects of the persistent forward for tools/p4_ab.py (build container, no GPU):

    git show HEAD~1:photonic_flash_attention_amd/csrc/gen_fa3_fwd_p4.py > /tmp/gen_parent.py
    python3 tools/p4_variants.py new= parent=@/tmp/gen_parent.py stamp3=P4_STAMP=3 "pstamp3=@/tmp/gen_parent.py P4_STAMP=3"

writes photonic_flash_attention_amd/csrc/build/variants/<name>.s and <name>.hsaco (git-ignored).  A spec is `name=` followed by
blank-separated tokens: none = this tree's generator; `@PATH` = the generator FILE at PATH instead (an experiment is an edited copy of
the generator, A/B'd against the one in the tree -- the generator itself has one schedule and no experiment knobs); `P4_STAMP=3` = the
stamped diagnostic build (kernel totals; p4_ab.py --stamp reads them, never time it).  The generator honours P4_STAMP only with
P4_DEV=1, which this script sets; the product `make` never does."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "photonic_flash_attention_amd", "csrc")
OUT = os.path.join(CSRC, "build", "variants")
LLVM = os.environ.get("LLVM", "/opt/rocm/lib/llvm/bin")
os.makedirs(OUT, exist_ok=True)
procs = []
for spec in sys.argv[1:]:
    name, _, tokens = spec.partition("=")
    gen = os.path.join(CSRC, "gen_fa3_fwd_p4.py")
    env = {k: v for k, v in os.environ.items() if not k.startswith("P4_")}
    env["P4_DEV"] = "1"
    for tok in tokens.split():
        if tok.startswith("@"):
            gen = os.path.abspath(tok[1:])
        elif tok.startswith("P4_STAMP="):
            env["P4_STAMP"] = tok.partition("=")[2]
        else:
            sys.exit(f"{spec!r}: {tok!r} is neither @PATH (a generator file) nor P4_STAMP=3")
    s = os.path.join(OUT, name + ".s")
    with open(s, "w") as f:
        subprocess.run([sys.executable, gen], env=env, stdout=f, check=True, cwd=CSRC)
    procs.append((name, subprocess.Popen(
        f"{LLVM}/clang -x assembler -target amdgcn-amd-amdhsa -mcpu=gfx950 -c {s} -o {OUT}/{name}.o && "
        f"{LLVM}/ld.lld -shared {OUT}/{name}.o -o {OUT}/{name}.hsaco && rm -f {OUT}/{name}.o", shell=True)))
for name, p in procs:
    rc = p.wait()
    print(f"{name}: {'ok' if rc == 0 else 'FAILED'} -> {OUT}/{name}.hsaco")
    if rc:
        sys.exit(1)

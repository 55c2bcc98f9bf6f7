"""Compare the instruction streams of the kernels of two gfx950 code objects, kernel by kernel (no GPU needed).

A template flag added to a kernel must leave the existing instantiations as they were: build the parent commit and the change
(`python __graft_entry__.py` leaves lib/build_libscaml_hip/scaml_gfx950.hsaco), keep both code objects, and run

  python tools/dev_isa_diff.py OLD.hsaco NEW.hsaco [--only SUBSTRING] [--rename OLD_TEXT=NEW_TEXT ...]

Every kernel of OLD whose name contains SUBSTRING is disassembled in both (its name in NEW after the --rename substitutions, for
a template parameter list that grew) and the two listings are compared without addresses, comments and the pc-relative offsets of
globals (they move with the size of the code object).  Prints one line per kernel
and exits 1 if any differs or is missing.
"""
import argparse
import difflib
import os
import re
import subprocess
import sys

OBJDUMP = next((p for p in ("/opt/rocm/lib/llvm/bin/llvm-objdump", "/opt/rocm/llvm/bin/llvm-objdump") if os.path.exists(p)), "llvm-objdump")


def kernels(path):
    out = subprocess.run([OBJDUMP, "-t", path], check=True, capture_output=True, text=True).stdout
    return sorted({ln.split()[-1] for ln in out.splitlines() if " F .text" in ln})


def listing(path, sym):
    out = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", f"--disassemble-symbols={sym}", path], check=True, capture_output=True,
                         text=True).stdout
    rows = []
    for ln in out.splitlines():
        ln = re.sub(r"\s*//.*", "", ln).strip()
        if ln and not ln.endswith(">:") and "file format" not in ln and not ln.startswith("Disassembly"):
            # (the pc-relative distance to a global moves with the size of the code object: not an instruction change)
            rows.append(re.sub(r"^(s_addc?_u32 s\d+, s\d+, )0x[0-9a-f]+$", r"\1<pc-relative>", ln))
    return rows


ap = argparse.ArgumentParser()
ap.add_argument("old")
ap.add_argument("new")
ap.add_argument("--only", default="")
ap.add_argument("--rename", action="append", default=[])
args = ap.parse_args()
new_names = set(kernels(args.new))
bad = 0
for sym in kernels(args.old):
    if args.only not in sym:
        continue
    to = sym
    for r in args.rename:
        a, b = r.split("=", 1)
        to = to.replace(a, b)
    if to not in new_names:
        print(f"MISSING  {sym} -> {to}")
        bad += 1
        continue
    a, b = listing(args.old, sym), listing(args.new, to)
    d = sum(1 for ln in difflib.unified_diff(a, b, lineterm="", n=0) if ln[:1] in "+-" and ln[:3] not in ("+++", "---"))
    print(f"{'same' if d == 0 else 'DIFFERS'}  {len(a):6d} {len(b):6d} instructions, {d:5d} changed lines  {sym}")
    bad += d != 0
sys.exit(1 if bad else 0)

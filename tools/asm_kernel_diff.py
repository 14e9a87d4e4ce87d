#!/usr/bin/env python3
"""Per-kernel text comparison of two device assembly listings of the library.

    hipcc <build()'s flags> --cuda-device-only -S -o a.s 4dcapture-fpv_amd/csrc/fdcap.hip      (once per tree)
    python tools/asm_kernel_diff.py a.s b.s [--show KERNEL] [--pair A_KERNEL=B_KERNEL ...]

Every kernel (.amdhsa_kernel name) present in either file gets one of
    identical    the same instruction text (comments, debug directives and label numbers aside)
    registers    the same instructions on other register numbers
    differs      other instructions; the instruction counts of both sides are given
    only in A/B
A generic text diff: it looks for no particular instruction.  --show prints the unified diff of one kernel (demangled name
prefix or mangled name).  --pair compares kernel A_KERNEL of a.s with kernel B_KERNEL of b.s (demangled names, as printed) -- for a
kernel whose signature or template parameter list changed between the two trees, so that its symbol did: e.g.
--pair 'fdc::nn_stream4_kernel<1, 1>=fdc::nn_stream4_kernel<1, 1, false>'."""
import argparse
import difflib
import re
import subprocess
import sys


def kernels(path):
    """mangled name -> its instruction and label lines, from the kernel's label to its .amdhsa_kernel block"""
    out, name, lines = {}, None, None
    start = re.compile(r"^(\w+):\s*; @\1")
    for ln in open(path):
        m = start.match(ln)
        if m:
            name, lines = m.group(1), []
            continue
        if name is None:
            continue
        if ln.lstrip().startswith(".amdhsa_kernel"):
            if ln.split()[1] == name:
                out[name] = lines
            name = None
            continue
        if ln.startswith(".Lfunc_end"):                              # a device function, not a kernel
            name = None
            continue
        ln = ln.split(";")[0].strip()
        if not ln or (ln.startswith(".") and not ln.endswith(":")):  # comments, directives
            continue
        ln = re.sub(r"\.LBB\d+_", ".LBB_", ln)                       # (the function's ordinal in the file)
        lines.append(re.sub(r"\s+", " ", ln))
    return out


def no_regs(lines):
    return [re.sub(r"\b[vsa]\[\d+:\d+\]|\b[vsa]\d+\b", "R", ln) for ln in lines]


def n_instr(lines):
    return sum(1 for ln in lines if not ln.endswith(":") and not ln.startswith("."))


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return {n: re.sub(r"^void ", "", d.replace("(anonymous namespace)::", "").split("(")[0]) or n for n, d in zip(names, out)}
    except Exception:
        return {n: n for n in names}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--show", default=None)
    ap.add_argument("--pair", action="append", default=[], metavar="A_KERNEL=B_KERNEL")
    args = ap.parse_args()
    ka, kb = kernels(args.a), kernels(args.b)
    if args.pair:                                                   # file B's kernel takes file A's symbol
        da, db = demangle(sorted(ka)), demangle(sorted(kb))
        for pr in args.pair:
            na, nb = pr.split("=", 1)
            ma, mb = [n for n in ka if da[n] == na], [n for n in kb if db.get(n) == nb]
            if len(ma) != 1 or len(mb) != 1:
                sys.exit(f"--pair {pr}: {len(ma)} kernels of that name in A, {len(mb)} in B")
            kb[ma[0]] = kb.pop(mb[0])
            print(f"paired     {na}  =  {nb}")
    names = sorted(set(ka) | set(kb))
    dm = demangle(names)
    if args.show:
        for n in names:
            if n == args.show or dm[n].startswith(args.show):
                for l in difflib.unified_diff(ka.get(n, []), kb.get(n, []), "A " + dm[n], "B " + dm[n], lineterm="", n=2):
                    print(l)
        return 0
    count = {"identical": 0, "registers": 0, "differs": 0, "only": 0}
    for n in names:
        if n not in ka or n not in kb:
            print(f"only in {'A' if n in ka else 'B'}  {dm[n]}")
            count["only"] += 1
        elif ka[n] == kb[n]:
            count["identical"] += 1
        elif no_regs(ka[n]) == no_regs(kb[n]):
            print(f"registers  {dm[n]}  ({n_instr(ka[n])} instructions)")
            count["registers"] += 1
        else:
            print(f"differs    {dm[n]}  ({n_instr(ka[n])} -> {n_instr(kb[n])} instructions)")
            count["differs"] += 1
    print(f"{len(ka)} kernels in A, {len(kb)} in B: {count['identical']} identical, {count['registers']} differ in register numbers only, "
          f"{count['differs']} differ in instructions, {count['only']} on one side only")
    return 0


if __name__ == "__main__":
    sys.exit(main())

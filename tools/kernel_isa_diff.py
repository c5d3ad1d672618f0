#!/usr/bin/env python3
"""kernel_isa_diff.py <parent csrc> <new csrc> [-DCLIPX_ABLATE] -- do two builds hold the same machine code, kernel by kernel?

Compiles every .hip of both directories to device assembly with the Makefile's flags, cuts the text per kernel symbol and compares,
for every kernel, its instruction text and its .amdhsa_* descriptor block (registers, LDS, scratch).  A refactor that moves kernels
between files, or deletes code that was never compiled, must come out "identical" for every kernel present in both.

Only what depends on a kernel's position in its file is normalised: the function number inside .LBB<n>_<m> / .LJTI<n>_<m> /
.Lfunc_end<n> labels, and comments.  The tool knows nothing about individual instructions.

  --rename 'OLD=NEW'   a demangled-name substring that changed on purpose (template arguments), applied to the parent's names;
                       may be given more than once
  --symbol 'KERNEL:OLD=NEW'  a device symbol that kernels whose demangled name contains KERNEL refer to under a new (mangled) name
  --ignore-signature   match kernels by their name and template arguments only (a parameter was added to or taken from a kernel)
  --hunks              for a kernel whose code differs, list every differing stretch (difflib opcodes: where, how many lines each
                       side) instead of the first differing line only
  --vector-view        compare what the vector units, the LDS and the memory pipes are given, in order: scalar ALU / scalar memory
                       instructions, branches, lane spills of scalar registers (v_writelane / v_readlane) and labels are
                       dropped (s_waitcnt, s_barrier, s_nop, s_setprio, s_sleep stay) and scalar register numbers are blanked.
                       For a change that costs a kernel scalar registers on purpose (one more kernel argument): the scalar
                       numbering moves everywhere, the question is whether anything else did
  --cache DIR          keep the .s files there and reuse one when it is newer than every source of its directory
  -j N                 compilers in parallel (default 8)
Exit status 0: every common kernel identical.  1: some kernel differs.
"""
import argparse
import concurrent.futures
import difflib
import os
import re
import subprocess
import sys
import tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", "-Wno-unused-result", "-Wno-unused-value"]
LABEL = re.compile(r"\.(LBB|LJTI|Lfunc_end|Lfunc_begin)\d+")


def compile_dir(src, out, defines, jobs):
    os.makedirs(out, exist_ok=True)
    files = sorted(f for f in os.listdir(src) if f.endswith(".hip"))
    newest = max(os.path.getmtime(os.path.join(src, f)) for f in os.listdir(src) if f.endswith((".hip", ".h")))

    def one(f):
        s = os.path.join(out, f[:-4] + ".s")
        if not (os.path.exists(s) and os.path.getmtime(s) > newest):
            r = subprocess.run([HIPCC, *FLAGS, *defines, os.path.join(src, f), "-o", s], stderr=subprocess.PIPE, text=True)
            if r.returncode != 0:
                sys.exit(f"{os.path.join(src, f)} does not compile:\n{r.stderr}")
        return f, s

    with concurrent.futures.ThreadPoolExecutor(jobs) as ex:
        return dict(ex.map(one, files))


def demangle(names):
    if not names:
        return {}
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
    return dict(zip(names, r.stdout.splitlines()))


def cut(path):
    """{kernel symbol: (code lines, descriptor lines)}, [device objects] of one assembly file"""
    lines = open(path).read().splitlines()
    kernels, objects = {}, []
    start = {}
    for i, ln in enumerate(lines):
        m = re.match(r"\s*\.type\s+(\S+),@(function|object)", ln)
        if m and m.group(2) == "function":
            start[m.group(1)] = i + 1  # the line "<symbol>:"
        elif m and not m.group(1).startswith("__hip_cuid"):
            objects.append(m.group(1))
    for i, ln in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if not m:
            continue
        sym = m.group(1)
        end = next(j for j in range(i, len(lines)) if lines[j].strip() == ".end_amdhsa_kernel")
        desc = [l.strip() for l in lines[i + 1:end]]
        # code: from the symbol's label to the .section directive in front of its descriptor
        first = start[sym] + 1
        last = max(j for j in range(first, i) if lines[j].strip().startswith(".section"))
        code = []
        for l in lines[first:last]:
            l = l.split(";", 1)[0].rstrip()
            if l.strip():
                code.append(LABEL.sub(lambda m: "." + m.group(1), l).replace(sym, "@self"))
        kernels[sym] = (code, desc)
    return kernels, objects


SREG = re.compile(r"\bs(\d+|\[\d+:\d+\])")
KEPT_SCALAR = ("s_waitcnt", "s_barrier", "s_nop", "s_setprio", "s_sleep")


def vector_view(code):
    out = []
    for ln in code:
        m = ln.split()[0]
        if ln.strip().endswith(":") or m in ("v_writelane_b32", "v_readlane_b32") or (m.startswith("s_") and m not in KEPT_SCALAR):
            continue
        out.append(SREG.sub("s#", ln.strip()))
    return out


def collect(asm):
    kernels, objects, where = {}, [], {}
    for f, s in asm.items():
        k, o = cut(s)
        for sym, v in k.items():
            kernels[sym] = v
            where[sym] = f
        objects += o
    return kernels, objects, where


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("-D", dest="defines", action="append", default=[])
    ap.add_argument("--rename", action="append", default=[])
    ap.add_argument("--symbol", action="append", default=[])
    ap.add_argument("--ignore-signature", action="store_true")
    ap.add_argument("--hunks", action="store_true")
    ap.add_argument("--vector-view", action="store_true")
    ap.add_argument("--cache")
    ap.add_argument("-j", type=int, default=8)
    a = ap.parse_args()
    defines = ["-D" + d for d in a.defines]
    tmp = a.cache or tempfile.mkdtemp(prefix="kernel_isa_diff_")
    tag = "_".join(a.defines) or "product"
    sides = []
    for side, src in (("parent", a.parent), ("new", a.new)):
        asm = compile_dir(src, os.path.join(tmp, side + "_" + tag), defines, a.j)
        k, o, w = collect(asm)
        d = demangle(list(k))
        if a.ignore_signature:
            d = {s: (n[:n.index("(")] if "(" in n else n) for s, n in d.items()}
        sides.append(({d[s]: (v, w[s]) for s, v in k.items()}, sorted(demangle(o).values())))
    (pk, po), (nk, no) = sides
    renamed = []
    for r in a.rename:
        old, new = r.split("=", 1)
        for name in [n for n in pk if old in n]:
            pk[name.replace(old, new)] = pk.pop(name)
            renamed.append((name, name.replace(old, new)))

    for r in a.symbol:
        kern, pair = r.split(":", 1)
        old, new = pair.split("=", 1)
        for name in [n for n in pk if kern in n]:
            (code, desc), f = pk[name]
            pk[name] = (([l.replace(old, new) for l in code], desc), f)
            renamed.append((f"{old} in {name}", new))

    print(f"kernel_isa_diff: flags {' '.join(FLAGS + defines)}")
    print(f"kernels: parent {len(pk)}, new {len(nk)}, in both {len(pk.keys() & nk.keys())}")
    differ = 0
    for name in sorted(pk.keys() & nk.keys()):
        (pc, pd), pf = pk[name]
        (nc, nd), nf = nk[name]
        if a.vector_view:
            pc, nc = vector_view(pc), vector_view(nc)
        if pc == nc and pd == nd:
            continue
        differ += 1
        what = " and ".join(w for w, bad in (("code", pc != nc), ("descriptor", pd != nd)) if bad)
        print(f"DIFFERS ({what}): {name}   [{pf} -> {nf}]")
        if pc != nc and a.hunks:
            print(f"    {len(pc)} -> {len(nc)} lines")
            for tag, i1, i2, j1, j2 in difflib.SequenceMatcher(None, pc, nc, autojunk=False).get_opcodes():
                if tag != "equal":
                    print(f"    {tag}: parent lines {i1}..{i2} ({i2 - i1}) -> new lines {j1}..{j2} ({j2 - j1})")
        elif pc != nc:
            at = next((i for i, (x, y) in enumerate(zip(pc, nc)) if x != y), min(len(pc), len(nc)))
            print(f"    {len(pc)} -> {len(nc)} lines, first difference at line {at}:")
            print(f"    - {pc[at] if at < len(pc) else '<end>'}\n    + {nc[at] if at < len(nc) else '<end>'}")
        for x, y in zip(pd, nd):
            if x != y:
                print(f"    - {x}\n    + {y}")
    print(f"identical in code and descriptor: {len(pk.keys() & nk.keys()) - differ}; differing: {differ}")
    for old, new in renamed:
        print(f"renamed: {old} -> {new}")
    moved = {}
    for name in pk.keys() & nk.keys():
        if pk[name][1] != nk[name][1]:
            moved.setdefault((pk[name][1], nk[name][1]), []).append(name)
    for (pf, nf), names in sorted(moved.items()):
        print(f"moved: {len(names)} kernels {pf} -> {nf}")
    for name in sorted(pk.keys() - nk.keys()):
        print(f"only in parent: {name}   [{pk[name][1]}]")
    for name in sorted(nk.keys() - pk.keys()):
        print(f"only in new: {name}   [{nk[name][1]}]")
    for o in sorted(set(po) - set(no)):
        print(f"device object only in parent: {o}")
    for o in sorted(set(no) - set(po)):
        print(f"device object only in new: {o}")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())

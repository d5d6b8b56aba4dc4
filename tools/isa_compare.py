#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds, function by function.

    tools/isa_compare.py PARENT_DIR BRANCH_DIR [--rename old=new ...]

Each directory holds the `.s` files of one side, made with the flags of aquery2_amd/csrc/Makefile plus
`--offload-device-only -S` (one file per .hip; the two sides need not cut their sources into the same files).

Every function is cut from its label to `.Lfunc_end`, comments and directives are dropped, local labels (`.LBB<n>_<m>`) lose the
function number, mangled names are demangled and stripped of their namespaces -- so a kernel may move to another file, and a type
it takes to another namespace, and still compare equal.  Functions are matched by name across ALL files of a side:

  * a kernel must occur exactly once per side; its instructions and its `.amdhsa_next_free_vgpr`, `.amdhsa_next_free_sgpr`,
    `.amdhsa_group_segment_fixed_size`, `.amdhsa_private_segment_fixed_size` and `.amdhsa_accum_offset` are compared;
  * a device function that was not inlined (the `__noinline__` store helpers) may occur once per file; all its copies, on both
    sides, must be equal.  `--rename old=new` names a helper that the change renames on purpose.

Prints `kernels compared K, functions compared F, differing D` and exits non-zero when anything differs or a function is
missing on one side.  Needs c++filt (or llvm-cxxfilt) on the PATH.
"""
import argparse
import collections
import glob
import os
import re
import shutil
import subprocess
import sys

RESOURCES = ("next_free_vgpr", "next_free_sgpr", "group_segment_fixed_size", "private_segment_fixed_size", "accum_offset")
MANGLED = re.compile(r"\b_Z\w+")


def demangler(symbols):
    tool = shutil.which("c++filt") or shutil.which("llvm-cxxfilt") or "/opt/rocm/llvm/bin/llvm-cxxfilt"
    symbols = sorted(symbols)
    out = subprocess.run([tool], input="\n".join(symbols) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    table = {}
    for sym, name in zip(symbols, out):
        name = name.replace("(anonymous namespace)::", "")
        table[sym] = re.sub(r"\b[A-Za-z_]\w*::", "", name)
    return table


def cut_functions(path):
    """-> [(mangled name, is_kernel, body lines, resources)] of one .s file"""
    funcs, name, body, res, kernel, in_desc = [], None, None, None, False, False
    for raw in open(path, errors="replace"):
        line = raw.split(";", 1)[0].strip()
        if name is None:
            m = re.match(r"\.type\s+(\S+),@function", line)
            if m:
                name, body, res, kernel, in_desc = m.group(1), [], {}, False, False
            continue
        if re.match(r"\.Lfunc_end\d+:", line):
            funcs.append((name, kernel, body, res))
            name = None
        elif line.startswith(".amdhsa_kernel"):
            kernel = in_desc = True
        elif line.startswith(".end_amdhsa_kernel"):
            in_desc = False
        elif in_desc:
            m = re.match(r"\.amdhsa_(\w+)\s+(.*)", line)
            if m and m.group(1) in RESOURCES:
                res[m.group(1)] = m.group(2)
        elif not line or line == name + ":" or (line.startswith(".") and not line.endswith(":")):
            continue                                    # blank, the function's own label, a directive
        else:
            body.append(re.sub(r"\.L([A-Za-z_]+)\d+_", r".L\1_", line))
    return funcs


def load_side(directory, renames):
    files = sorted(glob.glob(os.path.join(directory, "*.s")))
    if not files:
        sys.exit("no .s files in " + directory)
    raw = [(os.path.basename(f), fn) for f in files for fn in cut_functions(f)]
    symbols = {fn[0] for _, fn in raw}
    for _, fn in raw:
        for line in fn[2]:
            symbols.update(MANGLED.findall(line))
    names = demangler(symbols)

    def pretty(sym):
        n = names.get(sym, sym)
        for old, new in renames:
            n = re.sub(r"\b%s\b" % re.escape(old), new, n)
        return n

    side = collections.defaultdict(list)              # name -> [(file, is_kernel, text)]
    for fname, (sym, kernel, body, res) in raw:
        text = "\n".join(MANGLED.sub(lambda m: pretty(m.group(0)), l) for l in body)
        if kernel:
            text += "\n" + " ".join("%s=%s" % (k, res.get(k, "?")) for k in RESOURCES)
        side[pretty(sym)].append((fname, kernel, text))
    return side


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent_dir")
    ap.add_argument("branch_dir")
    ap.add_argument("--rename", action="append", default=[], metavar="old=new")
    ap.add_argument("-v", "--verbose", action="store_true", help="list every function with the files it was found in")
    args = ap.parse_args()
    renames = [tuple(r.split("=", 1)) for r in args.rename]
    a, b = load_side(args.parent_dir, renames), load_side(args.branch_dir, renames)
    kernels = functions = differing = 0
    for name in sorted(set(a) | set(b)):
        ca, cb = a.get(name, []), b.get(name, [])
        is_kernel = any(k for _, k, _ in ca + cb)
        functions += 1
        kernels += is_kernel
        problem = None
        if not ca or not cb:
            problem = "only in " + (args.parent_dir if ca else args.branch_dir)
        elif is_kernel and (len(ca) != 1 or len(cb) != 1):
            problem = "kernel occurs %d / %d times" % (len(ca), len(cb))
        elif len({t for _, _, t in ca + cb}) != 1:
            problem = "code differs"
        if args.verbose or problem:
            print("%-9s %s  [%s | %s]%s" % ("kernel" if is_kernel else "function", name, " ".join(f for f, _, _ in ca), " ".join(f for f, _, _ in cb),
                                           "  <-- " + problem if problem else ""))
        differing += problem is not None
    print("kernels compared %d, functions compared %d, differing %d" % (kernels, functions, differing))
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Do two source trees compile to the same kernels?

  python tools/isa_compare.py TREE_A TREE_B [--groups 0,4,13] [--asm-dir DIR]

TREE_A / TREE_B: a checkout (its lodestar_amd/csrc and include are used) or a csrc directory
(include is taken from ../../include).  lb_kgroup.hip of each is compiled to gfx950 assembly once
per kernel group (tools/gen_kdecls.py GROUPS) with the flags of lodestar_amd/build.py plus
--cuda-device-only -S, at most 16 compiles at a time, and the two texts are compared:

  * functions (kernels and out-of-line device functions) by name: the instructions, the labels
    renumbered per function, the kernel descriptor and the resource `.set` lines; comments dropped;
  * data objects (constant tables, LDS) as a set of (name, section, size, contents): the order in
    which the compiler emits them is free;
  * a function or object that has no namesake on the other side is paired with the one whose
    demangled name is equal once template arguments are left out; the pair is printed as renamed
    and its new name stands in for the old one in every body before the comparison.

One line per group, one per function or object that differs; exit status 1 on any difference.
The text is only diffed: nothing here looks for a particular instruction.  --asm-dir keeps the
assembly (DIR/a, DIR/b) and reuses a file newer than every source of its tree.
"""
import argparse
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_kdecls  # noqa: E402
from lodestar_amd import build as B  # noqa: E402

CXXFILT = "c++filt"  # (binutils; only run when a name has no namesake on the other side)


def tree_dirs(path):
    """(csrc, include) of a checkout or of a csrc directory"""
    sub = os.path.join(path, "lodestar_amd", "csrc")
    if os.path.isdir(sub):
        return sub, os.path.join(path, "include")
    return path, os.path.normpath(os.path.join(path, "..", "..", "include"))


def compile_groups(csrc, inc, groups, outdir):
    """outdir/kgroup<g>.s for every group; returns {g: path}"""
    os.makedirs(outdir, exist_ok=True)
    srcs = [os.path.join(csrc, f) for f in os.listdir(csrc)] + [os.path.join(inc, "lodestar_bls.h")]
    newest = max(os.path.getmtime(s) for s in srcs)
    out = {g: os.path.join(outdir, f"kgroup{g}.s") for g in groups}
    pend = [g for g in groups if not (os.path.exists(out[g]) and os.path.getmtime(out[g]) > newest)]
    running, failed = [], []
    while pend or running:
        while pend and len(running) < B._jobs():
            g = pend.pop(0)
            cmd = [B.HIPCC, *B.LIB_FLAGS, "-I" + inc, "-I" + csrc, f"-DLB_KGROUP={g}", "--cuda-device-only", "-S",
                   os.path.join(csrc, "lb_kgroup.hip"), "-o", out[g] + ".tmp"]
            running.append((subprocess.Popen(cmd, stderr=subprocess.DEVNULL), g))
        time.sleep(0.2)
        for r in list(running):
            rc = r[0].poll()
            if rc is not None:
                running.remove(r)
                if rc != 0:
                    failed.append(r[1])
                else:
                    os.replace(out[r[1]] + ".tmp", out[r[1]])
    if failed:
        sys.exit(f"{csrc}: groups {sorted(failed)} did not compile")
    return out


LABEL = re.compile(r"\.L(BB|JTI|func_end|func_begin|tmp)\d+(_\d+)?")


def parse(path):
    """({function: [lines]}, {object: (section, [lines])}) of one assembly file"""
    funcs, objs = {}, {}
    kind = {}
    cur = body = None
    section = ""
    for raw in open(path):
        line = raw.split(";", 1)[0].rstrip()
        s = line.strip()
        if not s:
            continue
        if s == ".amdgpu_metadata":  # the descriptors above already say what the notes repeat
            break
        m = re.match(r"\.type\s+([^,\s]+),@(function|object)", s)
        if m:
            kind[m.group(1)] = m.group(2)
            continue
        if s.startswith(".section") or s in (".text", ".data", ".bss"):
            if cur is None or kind.get(cur) == "object":
                section = s.split(",")[0]
            if cur is None:
                continue
        if s.startswith(".amdgpu_lds"):
            name = s.split()[1].rstrip(",")
            objs[name] = ("lds", [s])
            continue
        if cur is None:
            if s.endswith(":") and kind.get(s[:-1]) in ("function", "object") and not s.startswith("__hip_cuid_"):
                cur, body = s[:-1], []
            elif s.startswith(".set "):
                owner = s[5:].split(",")[0].rsplit(".", 1)[0]
                owner = owner[2:] if owner.startswith(".L") else owner
                if owner in funcs:
                    funcs[owner].append(s)
            continue
        if kind[cur] == "function" and re.match(r"\.Lfunc_end\d+:", s):
            funcs[cur] = body
            cur = None
        elif kind[cur] == "object" and s.startswith(".size") and s[5:].split(",")[0].strip() == cur:
            objs[cur] = (section, body + [s])
            cur = None
        else:
            body.append(s)
    return funcs, objs


def renumber(lines):
    """the labels of one function, numbered in order of first appearance"""
    seen = {}
    return [LABEL.sub(lambda m: seen.setdefault(m.group(0), f".L{m.group(1)}#{len(seen)}"), s) for s in lines]


def base_names(names):
    """{name: demangled name without template arguments}"""
    names = sorted(names)
    if not names:
        return {}
    dem = subprocess.run([CXXFILT], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    out = {}
    for n, d in zip(names, dem):
        prev = None
        while prev != d:
            prev, d = d, re.sub(r"<[^<>]*>", "", d)
        i = d.find("(")  # a template function's demangled name starts with its return type
        out[n] = d[:i].split()[-1] + d[i:] if i > 0 else d
    return out


def renames(a, b):
    """{name in a: name in b} for the names only one side has, paired by base name"""
    only_a, only_b = set(a) - set(b), set(b) - set(a)
    ba, bb = base_names(only_a), base_names(only_b)
    out = {}
    for n, d in ba.items():
        ma = [x for x in ba if ba[x] == d]
        mb = [x for x in bb if bb[x] == d]
        if len(ma) == 1 and len(mb) == 1:
            out[n] = mb[0]
    return out


def rename_in(lines, ren):
    if not ren:
        return lines
    rx = re.compile("|".join(sorted(map(re.escape, ren), key=len, reverse=True)))
    return [rx.sub(lambda m: ren[m.group(0)], s) for s in lines]


def first_diff(x, y):
    for i, (p, q) in enumerate(zip(x, y)):
        if p != q:
            return f"line {i} of {len(x)} / {len(y)}: `{p}` | `{q}`"
    return f"{len(x)} lines | {len(y)} lines"


def compare_group(g, fa, fb):
    """prints the group's lines; True if identical"""
    (funcs_a, objs_a), (funcs_b, objs_b) = parse(fa), parse(fb)
    ren = renames({**funcs_a, **objs_a}, {**funcs_b, **objs_b})
    funcs_a = {ren.get(n, n): rename_in(v, ren) for n, v in funcs_a.items()}
    objs_a = {ren.get(n, n): (sec, rename_in(v, ren)) for n, (sec, v) in objs_a.items()}
    lines = [f"  renamed, compared under the new name: {o} -> {n}" for o, n in sorted(ren.items())]
    bad = 0
    for n in sorted(set(funcs_a) | set(funcs_b)):
        what = "kernel" if ".amdhsa_kernel " + n in (funcs_a.get(n) or funcs_b.get(n)) else "function"
        if n not in funcs_a or n not in funcs_b:
            lines.append(f"  {what} {n}: only in {'A' if n in funcs_a else 'B'}")
        elif renumber(funcs_a[n]) != renumber(funcs_b[n]):
            lines.append(f"  {what} {n}: differs, {first_diff(renumber(funcs_a[n]), renumber(funcs_b[n]))}")
        else:
            continue
        bad += 1
    for n in sorted(set(objs_a) | set(objs_b)):
        if n not in objs_a or n not in objs_b:
            lines.append(f"  object {n}: only in {'A' if n in objs_a else 'B'}")
        elif objs_a[n] != objs_b[n]:
            lines.append(f"  object {n}: differs, {first_diff(objs_a[n][1], objs_b[n][1])}")
        else:
            continue
        bad += 1
    nk = sum(1 for v in funcs_b.values() if any(s.startswith(".amdhsa_kernel ") for s in v))
    ni = sum(len(v) for v in funcs_b.values())
    print(f"group {g}: {nk} kernels, {len(funcs_b)} functions, {ni} lines, {len(objs_b)} data objects: "
          + ("identical" if not bad else f"{bad} DIFFER"))
    for s in lines:
        print(s)
    return not bad


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("tree_a")
    ap.add_argument("tree_b")
    ap.add_argument("--groups", default="", help="comma-separated kernel groups (default: all)")
    ap.add_argument("--asm-dir", default="", help="keep the assembly here and reuse what is up to date")
    a = ap.parse_args()
    groups = [int(g) for g in a.groups.split(",") if g] or list(range(gen_kdecls.N_GROUPS))
    if a.asm_dir:
        asm = a.asm_dir
    else:
        import tempfile
        tmp = tempfile.TemporaryDirectory()
        asm = tmp.name
    files = [compile_groups(*tree_dirs(t), groups, os.path.join(asm, side)) for t, side in ((a.tree_a, "a"), (a.tree_b, "b"))]
    same = [compare_group(g, files[0][g], files[1][g]) for g in groups]
    print(f"{sum(same)} of {len(groups)} groups identical")
    sys.exit(0 if all(same) else 1)


if __name__ == "__main__":
    main()

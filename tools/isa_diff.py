#!/usr/bin/env python3
"""Per-kernel comparison of two `make asm` outputs:  tools/isa_diff.py [--rename RE=REPL ...] [--table] OLD NEW  (two .s files or two directories)

A kernel is its instruction body, its .amdhsa_* descriptor, its `.set <kernel>.*` resource symbols and its entry in the
amdhsa.kernels metadata.  Comment lines and trailing comments are dropped, local labels (.LBB3_12, .Lfunc_end3, ...) are
renumbered in order of appearance inside the kernel, and the per-build __hip_cuid_<hash> symbol is masked, so that two
builds of the same code compare equal wherever the kernel sits in the file.  Whatever belongs to no kernel (device
variables, target lines) is compared as `<file scope>`.  Exit status 1 when anything differs or a kernel is missing.

Given two directories, the kernels of every .s inside each are pooled and compared by name: a kernel that moved to another
file is `same` when nothing of it changed.  The pooled `<file scope>` lines are compared as sorted sets and reported, but
the exit status then rests on the kernels alone: device variables and target lines regroup with the files.

--rename RE=REPL (repeatable): for kernels that were renamed.  Applied (re.sub) to the demangled name, without `void` and
the parameter list, of every kernel only OLD has; one that then reads like a kernel only NEW has is compared with it, under
the new name, its own mangled name replaced by the new one in its lines.  Needs c++filt.
    --rename 'shade_refract_kernel<=shade_kernel<trt::ShadeRefract, '
--table: a Markdown row per kernel that differs or was renamed — instructions, VGPRs, SGPRs, scratch, waves per SIMD, LDS — with the
demangled name; waves per SIMD are what the VGPRs allow on gfx950 (512 per lane and SIMD in granules of 8, at most 8 waves)."""
import glob
import os
import re
import subprocess
import sys

LABEL = re.compile(r"\.L[A-Za-z_]*\d+(?:_\d+)?(?:\$\w+)?")
FIELDS = (("vgpr", ".amdhsa_next_free_vgpr"), ("sgpr", ".amdhsa_next_free_sgpr"),
          ("scratch", ".amdhsa_private_segment_fixed_size"), ("lds", ".amdhsa_group_segment_fixed_size"))
COLUMNS = ("insts", "vgpr", "sgpr", "scratch", "waves", "lds")   # of --table


def kernels(path):
    """{kernel: normalised lines}, with the lines outside every kernel under '<file scope>'."""
    out, cur, in_meta = {"<file scope>": []}, None, False
    lines = [re.sub(r"__hip_cuid_\w+", "__hip_cuid", ln.split(";")[0].rstrip()) for ln in open(path)]
    names = [m.group(1) for ln in lines if (m := re.match(r"\s*\.amdhsa_kernel (\S+)", ln))]
    for ln in filter(str.strip, lines):
        if m := re.match(r"(\S+):$", ln):
            if m.group(1) in names:
                cur = m.group(1)
                out[cur] = []
        if ln.startswith("amdhsa.kernels:"):
            in_meta, cur = True, None
        elif in_meta and ln.startswith("  - "):       # next kernel's metadata entry: owner known at its .name
            cur = "<meta>"
            out[cur] = []
        elif in_meta and not ln.startswith("  "):
            in_meta, cur = False, None
        if m := re.match(r"\s*\.set (\S+?)\.\w+,", ln):   # resource symbols follow .Lfunc_end
            out[m.group(1) if m.group(1) in names else "<file scope>"].append(ln)
            continue
        out[cur or "<file scope>"].append(ln)
        if in_meta and (m := re.match(r"    \.name:\s+(\S+)", ln)) and cur == "<meta>":
            cur = m.group(1)
            out[cur] += out.pop("<meta>")
        if re.match(r"\.Lfunc_end\d+:", ln):
            cur = None
    for k, body in out.items():
        ids = {}
        out[k] = [LABEL.sub(lambda m: ".L%d" % ids.setdefault(m.group(0), len(ids)), ln) for ln in body]
    return out


def pooled(path):
    """kernels() of a file, or of every .s of a directory pooled (file scope: the distinct lines, sorted)."""
    if not os.path.isdir(path):
        return kernels(path)
    out, scope = {}, set()
    for f in sorted(glob.glob(os.path.join(path, "*.s"))):
        k = kernels(f)
        scope.update(k.pop("<file scope>"))
        dup = set(k) & set(out)
        if dup:
            sys.exit("%s: %s is in another file of %s too" % (f, sorted(dup)[0], path))
        out.update(k)
    out["<file scope>"] = sorted(scope)
    return out


def figures(body):
    f = {n: next((int(ln.split()[1]) for ln in body if ln.split()[0] == key), None) for n, key in FIELDS}
    f["insts"] = sum(1 for ln in body if re.match(r"\t[a-z]\w+", ln))   # instructions: tab, mnemonic (directives start with '.')
    f["waves"] = min(8, 512 // (-(-f["vgpr"] // 8) * 8)) if f["vgpr"] else None
    return f


def demangled(names):
    """{mangled: 'trt::kernel<...>'}: no `void`, no parameter list."""
    text = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.splitlines()
    return {n: re.sub(r"\(.*$", "", re.sub(r"^void ", "", d)) for n, d in zip(names, text)}


def pair_renamed(old, new, renames):
    """Moves every kernel only `old` has to the name of the kernel only `new` has that --rename maps it to; the new names."""
    moved = set()
    only_old, only_new = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    if not only_old or not only_new:
        return moved
    names = demangled(only_old + only_new)
    target = {names[k]: k for k in only_new}
    for k in only_old:
        key = names[k]
        for pattern, repl in renames:
            key = re.sub(pattern, repl, key)
        if key in target:
            old[target[key]] = [ln.replace(k, target[key]) for ln in old.pop(k)]
            moved.add(target[key])
    return moved


def main():
    args, renames, table = sys.argv[1:], [], False
    while args and args[0].startswith("--"):
        if args[0] == "--table":
            table, args = True, args[1:]
        elif args[0] == "--rename" and len(args) > 1 and "=" in args[1]:
            renames.append(args[1].split("=", 1))
            args = args[2:]
        else:
            sys.exit(__doc__)
    if len(args) != 2:
        sys.exit(__doc__)
    old, new = pooled(args[0]), pooled(args[1])
    moved = pair_renamed(old, new, renames) if renames else set()
    if os.path.isdir(args[0]) and os.path.isdir(args[1]) and old["<file scope>"] != new["<file scope>"]:
        print("differs  <file scope> (not counted: the files regrouped)")
        old.pop("<file scope>"), new.pop("<file scope>")
    n_same = n_kernels = 0
    rows = []
    for k in sorted(set(old) | set(new)):
        n_kernels += k != "<file scope>"
        if k not in old or k not in new:
            print("%-8s %s" % ("only old" if k in old else "only new", k))
        elif old[k] == new[k]:
            print("same     %s" % k)
            n_same += k != "<file scope>"
            if k in moved:
                rows.append((k, ["%s" % figures(new[k])[n] for n in COLUMNS]))
        else:
            fo, fn = figures(old[k]), figures(new[k])
            delta = ("%s %s%s" % (n, fo[n], "" if fn[n] == fo[n] else " -> %s (%+d)" % (fn[n], fn[n] - fo[n])) for n in fo)
            print("differs  %s\n         %s" % (k, "  ".join(delta)))
            rows.append((k, ["%s" % fo[n] if fn[n] == fo[n] else "%s -> %s" % (fo[n], fn[n]) for n in COLUMNS]))
    print("%d kernels: %d same, %d not" % (n_kernels, n_same, n_kernels - n_same))
    if table and rows:
        names = demangled([k for k, _ in rows])
        print("| kernel | instructions | VGPRs | SGPRs | scratch B/lane | waves/SIMD | LDS B/block |\n|---|---|---|---|---|---|---|")
        for k, cells in sorted(rows, key=lambda r: names[r[0]]):
            print("| `%s` | %s |" % (names[k].replace("trt::", ""), " | ".join(cells)))
    sys.exit(0 if old == new else 1)


if __name__ == "__main__":
    main()

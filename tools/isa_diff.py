#!/usr/bin/env python3
"""Per-kernel comparison of two `make asm` outputs:  tools/isa_diff.py OLD.s NEW.s  |  tools/isa_diff.py OLD_DIR NEW_DIR

A kernel is its instruction body, its .amdhsa_* descriptor, its `.set <kernel>.*` resource symbols and its entry in the
amdhsa.kernels metadata.  Comment lines and trailing comments are dropped, local labels (.LBB3_12, .Lfunc_end3, ...) are
renumbered in order of appearance inside the kernel, and the per-build __hip_cuid_<hash> symbol is masked, so that two
builds of the same code compare equal wherever the kernel sits in the file.  Whatever belongs to no kernel (device
variables, target lines) is compared as `<file scope>`.  Exit status 1 when anything differs or a kernel is missing.

Given two directories, the kernels of every .s inside each are pooled and compared by name: a kernel that moved to another
file is `same` when nothing of it changed.  The pooled `<file scope>` lines are compared as sorted sets and reported, but
the exit status then rests on the kernels alone: device variables and target lines regroup with the files."""
import glob
import os
import re
import sys

LABEL = re.compile(r"\.L[A-Za-z_]*\d+(?:_\d+)?(?:\$\w+)?")
FIELDS = (("vgpr", ".amdhsa_next_free_vgpr"), ("sgpr", ".amdhsa_next_free_sgpr"),
          ("scratch", ".amdhsa_private_segment_fixed_size"), ("lds", ".amdhsa_group_segment_fixed_size"))


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
    return f


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    old, new = pooled(sys.argv[1]), pooled(sys.argv[2])
    if os.path.isdir(sys.argv[1]) and os.path.isdir(sys.argv[2]) and old["<file scope>"] != new["<file scope>"]:
        print("differs  <file scope> (not counted: the files regrouped)")
        old.pop("<file scope>"), new.pop("<file scope>")
    n_same = n_kernels = 0
    for k in sorted(set(old) | set(new)):
        n_kernels += k != "<file scope>"
        if k not in old or k not in new:
            print("%-8s %s" % ("only old" if k in old else "only new", k))
        elif old[k] == new[k]:
            print("same     %s" % k)
            n_same += k != "<file scope>"
        else:
            fo, fn = figures(old[k]), figures(new[k])
            delta = ("%s %s%s" % (n, fo[n], "" if fn[n] == fo[n] else " -> %s (%+d)" % (fn[n], fn[n] - fo[n])) for n in fo)
            print("differs  %s\n         %s" % (k, "  ".join(delta)))
    print("%d kernels: %d same, %d not" % (n_kernels, n_same, n_kernels - n_same))
    sys.exit(0 if old == new else 1)


if __name__ == "__main__":
    main()

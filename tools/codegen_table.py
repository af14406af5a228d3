#!/usr/bin/env python3
"""Table of the generated code of every kernel in device assembly files, for a
before / after comparison of a refactor:

    make -C tlslite-ng_amd/csrc asm          # in each tree
    python tools/codegen_table.py PARENT/asm/tls12-hip-amdgcn-*.s ... > before.tsv
    python tools/codegen_table.py --compare before.tsv after.tsv

Per kernel (its name and template arguments, without the parameter list): the number of instruction lines between its label and the end of
its function, `.amdhsa_next_free_vgpr`, and from the metadata notes
`.vgpr_spill_count` and `.private_segment_fixed_size`.  Plain text processing:
a line of the body counts as an instruction when it is neither empty, a
comment, a directive nor a label.  The count is a size, not a speed.
"""
import re
import subprocess
import sys

FIELDS = ("instructions", "next_free_vgpr", "vgpr_spill_count", "private_segment_fixed_size")


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
        return dict(zip(names, out.splitlines()))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def scan(path):
    """{mangled kernel name: {field: value}} of one .s file."""
    lines = open(path).read().splitlines()
    rows, kernels = {}, set()
    for ln in lines:
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if m:
            kernels.add(m.group(1))
    cur, desc = None, None
    for ln in lines:
        s = ln.split(";")[0].strip()
        if cur is None and s.endswith(":") and s[:-1] in kernels and s[:-1] not in rows:
            cur = s[:-1]
            rows[cur] = dict.fromkeys(FIELDS, 0)
            continue
        if cur is not None:
            if s.startswith(".Lfunc_end"):
                cur = None
            elif s and s[0] not in ".;" and not s.endswith(":"):
                rows[cur]["instructions"] += 1
        m = re.match(r"\.amdhsa_kernel\s+(\S+)", s)
        if m:
            desc = m.group(1)
        elif s == ".end_amdhsa_kernel":
            desc = None
        elif desc:
            m = re.match(r"\.amdhsa_next_free_vgpr\s+(\d+)", s)
            if m:
                rows[desc]["next_free_vgpr"] = int(m.group(1))
    meta = {}   # the metadata notes: one map per kernel, its own keys indented by four
    for ln in lines + ["  - ."]:
        if ln.startswith("  - ."):
            if meta.get("name") in rows:
                rows[meta["name"]].update({k: int(v) for k, v in meta.items() if k != "name"})
            meta = {}
        m = re.match(r"(?:    |  - )\.(name|vgpr_spill_count|private_segment_fixed_size):\s+(\S+)", ln)
        if m:
            meta[m.group(1)] = m.group(2)
    return rows


def short(demangled):
    """A kernel's name and template arguments: no return type, namespace or parameter list."""
    name = demangled.replace("tg::(anonymous namespace)::", "")
    return re.sub(r"^void ", "", re.sub(r"\(.*\)$", "", name))


def table(paths):
    rows = {}
    for p in paths:
        rows.update(scan(p))
    names = demangle(sorted(rows))
    print("\t".join(("kernel",) + FIELDS))
    for n in sorted(rows, key=lambda n: short(names[n])):
        print("\t".join([short(names[n])] + [str(rows[n][f]) for f in FIELDS]))


def load(path):
    out = {}
    for ln in open(path).read().splitlines()[1:]:
        c = ln.split("\t")
        out[c[0]] = dict(zip(FIELDS, map(int, c[1:])))
    return out


def compare(before, after):
    a, b = load(before), load(after)
    ok = set(a) == set(b)
    for n in sorted(set(a) - set(b)):
        print("MISSING\t" + n)
    for n in sorted(set(b) - set(a)):
        print("ADDED\t" + n)
    print("kernel\tinstr before\tinstr after\tchange %\tvgpr before\tvgpr after\tspill\tprivate")
    for n in sorted(set(a) & set(b)):
        x, y = a[n], b[n]
        pct = 100.0 * (y["instructions"] - x["instructions"]) / max(x["instructions"], 1)
        print("%s\t%d\t%d\t%+.2f\t%d\t%d\t%d\t%d" % (n, x["instructions"], y["instructions"], pct, x["next_free_vgpr"],
                                                    y["next_free_vgpr"], y["vgpr_spill_count"],
                                                    y["private_segment_fixed_size"]))
        ok = ok and y["vgpr_spill_count"] == 0 and y["private_segment_fixed_size"] == 0
    return 0 if ok else 1


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    table(sys.argv[1:])

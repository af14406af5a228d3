"""Every kernel of a built libtlsgpu.so with its register, spill, private-segment
and LDS figures, one per line, sorted (the method of tests/test_kernel_metadata.py).
usage: kernel_list.py LIB > list.txt"""
import os, re, shutil, subprocess, sys, tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
FIELDS = ("vgpr_count", "sgpr_count", "vgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")


def tool(name):
    p = os.path.join(LLVM, name)
    return p if os.path.exists(p) else shutil.which(name)


def main(lib):
    d = tempfile.mkdtemp()
    fb = os.path.join(d, "fb.bin")
    subprocess.run([tool("llvm-objcopy"), "--dump-section=.hip_fatbin=" + fb, lib, os.path.join(d, "j.so")], check=True)
    blob = open(fb, "rb").read()
    starts = [m.start() for m in re.finditer(re.escape(b"__CLANG_OFFLOAD_BUNDLE__"), blob)]
    rows = []
    for n, a in enumerate(starts):
        part, co = os.path.join(d, "b%d.bin" % n), os.path.join(d, "k%d.co" % n)
        open(part, "wb").write(blob[a:starts[n + 1] if n + 1 < len(starts) else len(blob)])
        subprocess.run([tool("clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                        "--input=" + part, "--output=" + co, "--unbundle"], check=True)
        if not os.path.getsize(co):
            continue   # a translation unit without kernels
        notes = subprocess.run([tool("llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
        cur = None
        for line in notes.splitlines():
            m = re.match(r"\s+\.(name|%s):\s+(\S+)" % "|".join(FIELDS), line)
            if not m:
                continue
            k, v = m.groups()
            if k == "name":
                cur = {"name": v}
                rows.append(cur)
            elif cur is not None:
                cur[k] = v
    rows = [r for r in rows if "vgpr_count" in r]   # kernels, not their arguments
    for r in sorted(rows, key=lambda r: r["name"]):
        print(r["name"], *("%s=%s" % (f, r.get(f)) for f in FIELDS))
    shutil.rmtree(d)


main(sys.argv[1])

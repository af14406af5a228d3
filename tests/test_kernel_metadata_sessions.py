"""CPU check of the built library's code-object metadata for the many-session
record framing: its prep and finish kernels (records.hip) and EVERY kernel of
the counter-mode rank pass's code object (sessions.hip: the rank kernels and
the rocPRIM sort and scan kernels instantiated there) spill no VGPRs and have
no private segment, so calling them on many streams allocates no per-queue
scratch (test_kernel_metadata.py has the reason).  The rank pass calls
rocPRIM's merge sort, not its radix sort, for this: the radix sort's Onesweep
kernels, which it runs above 2^20 items, have a private segment."""
import os
import re
import subprocess

import pytest

from test_kernel_metadata import LIB, _tool, kernels  # noqa: F401  (module-scoped fixture)

# mangled-name fragments (anonymous namespace inside tg)
FRAMING_KERNELS = {
    "seal_prep_sessions": "18seal_prep_sessions",
    "open_prep_sessions": "18open_prep_sessions",
    "open_finish_sessions": "20open_finish_sessions",
}
RANK_KERNELS = ("9rank_keys", "12rank_scatter", "12rank_advance")


@pytest.mark.parametrize("label", sorted(FRAMING_KERNELS))
def test_session_framing_kernel_has_no_private_segment(kernels, label):  # noqa: F811
    frag = FRAMING_KERNELS[label]
    found = [v for k, v in kernels.items() if frag in k and not k.endswith(".kd")]
    assert len(found) == 1, (label, len(found))
    meta = found[0]
    assert meta["vgpr_spill_count"] == 0, (label, meta)
    assert meta["private_segment_fixed_size"] == 0, (label, meta)


@pytest.fixture(scope="module")
def rank_object(tmp_path_factory):
    """{kernel name: metadata} of the one code object that holds the rank
    kernels (the library has one offload bundle per object file)."""
    tools = [_tool(n) for n in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")]
    if not all(tools) or not os.path.exists(LIB):
        pytest.skip("ROCm LLVM tools or the built library not present")
    objcopy, bundler, readelf = tools
    d = tmp_path_factory.mktemp("meta_sessions")
    fb = str(d / "fb.bin")
    subprocess.run([objcopy, "--dump-section=.hip_fatbin=" + fb, LIB, str(d / "j.so")], check=True)
    blob = open(fb, "rb").read()
    starts = [m.start() for m in re.finditer(re.escape(b"__CLANG_OFFLOAD_BUNDLE__"), blob)]
    hits = []
    for n, a in enumerate(starts):
        part, co = str(d / ("b%d.bin" % n)), str(d / ("k%d.co" % n))
        open(part, "wb").write(blob[a:starts[n + 1] if n + 1 < len(starts) else len(blob)])
        subprocess.run([bundler, "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + part,
                        "--output=" + co, "--unbundle"], check=True)
        notes = subprocess.run([readelf, "--notes", co], check=True, capture_output=True, text=True).stdout
        out, cur = {}, None
        for line in notes.splitlines():
            m = re.match(r"\s+\.(name|vgpr_count|vgpr_spill_count|private_segment_fixed_size):\s+(\S+)", line)
            if not m:
                continue
            k, v = m.groups()
            if k == "name":
                cur = out.setdefault(v, {})
            elif cur is not None:
                cur[k] = int(v)
        if any("9rank_keys" in k for k in out):
            hits.append(out)
    assert len(hits) == 1, len(hits)
    return hits[0]


def test_every_kernel_of_the_rank_pass_has_no_private_segment(rank_object):
    names = sorted(rank_object)
    for frag in RANK_KERNELS:
        assert sum(frag in k for k in names) == 1, frag
    # rocPRIM's block sort, merge levels and scan are in the same object
    assert any("merge_sort" in k for k in names) and any("scan" in k for k in names), names
    assert not any("onesweep" in k for k in names), [k for k in names if "onesweep" in k]
    assert len(names) >= 8
    for k in names:
        meta = rank_object[k]
        assert meta["vgpr_spill_count"] == 0, (k, meta)
        assert meta["private_segment_fixed_size"] == 0, (k, meta)

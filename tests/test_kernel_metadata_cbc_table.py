"""CPU check of the built library's code-object metadata for the many-session
AES-CBC + HMAC record kernels (csrc/aes_cbc_table.hip): every instantiation --
seal and open, AES-128 / AES-256, SHA-1 / SHA-256 / SHA-384, MAC-then-encrypt
and encrypt-then-MAC -- is there exactly once, spills no VGPRs and has no
private segment.  A lane of these kernels holds its own session's schedule in
44 / 60 VGPRs during the cipher pass; they run on callers' streams, where a
private segment would bring back the per-queue scratch allocation
(test_kernel_metadata.py has the reason)."""
import pytest

from test_kernel_metadata import kernels  # noqa: F401  (module-scoped fixture)

# cbctab_{seal,open}<NR, H, ETM> in tg's anonymous namespace
ALL = {"cbctab_%s<%d, %s, %s>" % (d, nr, h, "etm" if etm else "mte"):
       ("11cbctab_%sILi%dENS0_%d%sELb%dEE" % (d, nr, len(h), h, etm),)
       for d in ("seal", "open") for nr in (10, 14) for h in ("Sha1", "Sha256", "Sha384") for etm in (0, 1)}


def test_every_instantiation_is_listed(kernels):  # noqa: F811
    assert len(ALL) == 24
    assert len([k for k in kernels if "cbctab_" in k and not k.endswith(".kd")]) == 24


@pytest.mark.parametrize("label", sorted(ALL))
def test_cbc_table_kernel_has_no_private_segment(kernels, label):  # noqa: F811
    frags = ALL[label]
    found = [v for k, v in kernels.items() if all(f in k for f in frags) and not k.endswith(".kd")]
    assert len(found) == 1, (label, len(found))
    meta = found[0]
    assert meta["vgpr_spill_count"] == 0, (label, meta)
    assert meta["private_segment_fixed_size"] == 0, (label, meta)

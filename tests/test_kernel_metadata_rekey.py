"""CPU check of the built library's code-object metadata for the in-place
rekey (tg_key_replace_device / tg_sessions_rekey): every new kernel -- the
fused front kernel in each (hash, key length, layout) instantiation, the
slot-indexed forms of the three table derive kernels and the guarded forms of
the single key's chain -- is there exactly once, spills no VGPRs and has no
private segment.  These kernels run on callers' streams between record
batches; a private segment would bring back the per-queue scratch allocation
(test_kernel_metadata.py has the reason)."""
import pytest

from test_kernel_metadata import kernels  # noqa: F401  (module-scoped fixture)

# rekey_kernel<H, NK, LAYOUT>: NK 4 / 8 with layouts 0 (single AES-GCM key),
# 1 (AES-GCM table), 2 (AES-CCM); NK 0 = ChaCha20-Poly1305, layout 3
FRONT = {"rekey_kernel<%s, %d, %d>" % (h, nk, lay): ("12rekey_kernelI", "%d%sELi%dELi%dEE" % (len(h), h, nk, lay))
         for h in ("NoHash", "Sha256", "Sha384")
         for nk, lay in ((4, 0), (4, 1), (4, 2), (8, 0), (8, 1), (8, 2), (0, 3))}
# mangled-name fragments (anonymous namespace inside tg); ILb1E = the slot /
# guarded instantiation, beside the creation-time ILb0E one
DERIVE = {"table_hpow_kernel<slot>": ("17table_hpow_kernelILb1EE",),
          "kt_planes_kernel<slot>": ("16kt_planes_kernelILb1EE",),
          "kt_rot_kernel<slot>": ("13kt_rot_kernelILb1EE",),
          "ghash_table_kernel<guard>": ("18ghash_table_kernelILb1EE",),
          "hpow_kernel<guard>": ("N_111hpow_kernelILb1EE",),
          "ghash64_table_kernel<guard>": ("20ghash64_table_kernelILb1EE",),
          "ghash8_table_kernel<guard>": ("19ghash8_table_kernelILb1EE",),
          "bs_mask_kernel<guard>": ("14bs_mask_kernelILb1EE",),
          # the creation-time instantiations are still there, once each
          "table_hpow_kernel": ("17table_hpow_kernelILb0EE",),
          "kt_planes_kernel": ("16kt_planes_kernelILb0EE",),
          "kt_rot_kernel": ("13kt_rot_kernelILb0EE",),
          "bs_mask_kernel": ("14bs_mask_kernelILb0EE",)}
ALL = dict(FRONT, **DERIVE)


def test_every_instantiation_is_listed():
    assert len(FRONT) == 21 and len(ALL) == 33


@pytest.mark.parametrize("label", sorted(ALL))
def test_rekey_kernel_has_no_private_segment(kernels, label):  # noqa: F811
    frags = ALL[label]
    found = [v for k, v in kernels.items() if all(f in k for f in frags) and not k.endswith(".kd")]
    assert len(found) == 1, (label, len(found))
    meta = found[0]
    assert meta["vgpr_spill_count"] == 0, (label, meta)
    assert meta["private_segment_fixed_size"] == 0, (label, meta)

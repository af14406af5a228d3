"""CPU check of the built library's code-object metadata for the TLS 1.0 / 1.1
key setup (tls10.hip): the template pack kernel, the PRF kernel and the fused
CBC row install for AES-128 and AES-256 are there exactly once, spill no VGPRs
and have no private segment, and nothing else of theirs is built.  These
kernels run on callers' streams between record batches
(test_kernel_metadata_tls12.py has the reason).  The PRF kernel holds four HMAC
midstates, two A(i), a hash state, sixteen message words and two 20-word
output windows; the installs hold the key block's two windows, 28 and 30 words
for AES-256 -- this is the check that they still fit, and that MD5's constants
and shift amounts stayed immediates rather than a table in scratch."""
import pytest

from test_kernel_metadata import kernels  # noqa: F401  (module-scoped fixture)

ALL = {"tls10_pack_kernel": "17tls10_pack_kernelE",
       "tls10_prf_kernel": "16tls10_prf_kernelE",
       "tls11_cbcrow_install_kernel<4>": "27tls11_cbcrow_install_kernelILi4EE",
       "tls11_cbcrow_install_kernel<8>": "27tls11_cbcrow_install_kernelILi8EE"}


def test_every_kernel_is_listed(kernels):  # noqa: F811
    names = [k for k in kernels if not k.endswith(".kd")]
    for frag, count in (("tls10_", 2), ("tls11_", 2), ("17tls10_pack_kernelE", 1), ("16tls10_prf_kernelE", 1),
                        ("27tls11_cbcrow_install_kernelI", 2)):
        assert len([k for k in names if frag in k]) == count, frag
    # MD5 is instantiated nowhere else: no TLS 1.2 kernel and no CBC row kernel takes it
    assert [k for k in names if "3Md5" in k] == []


@pytest.mark.parametrize("label", sorted(ALL))
def test_tls10_kernel_has_no_private_segment(kernels, label):  # noqa: F811
    found = [v for k, v in kernels.items() if ALL[label] in k and not k.endswith(".kd")]
    assert len(found) == 1, (label, len(found))
    meta = found[0]
    assert meta["vgpr_spill_count"] == 0, (label, meta)
    assert meta["private_segment_fixed_size"] == 0, (label, meta)

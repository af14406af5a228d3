"""CPU check of the built library's code-object metadata for the TLS 1.2 key
setup (tls12.hip): the template pack kernel, the PRF kernel for both hashes,
the CBC row kernel and the two fused install kernels in every instantiation
are there exactly once, spill no VGPRs and have no private segment.  These
kernels run on callers' streams between record batches; a private segment
would bring back the per-queue scratch allocation (test_kernel_metadata.py has
the reason).  The PRF's registers hold two HMAC midstates, A(i), a hash state
and sixteen message words -- with SHA-384 all of them 64-bit -- and the installs
add the key block's window, so this is the check that they still fit."""
import pytest

from test_kernel_metadata import kernels  # noqa: F401  (module-scoped fixture)

HASHES = ("Sha256", "Sha384")
MACS = ("Sha1", "Sha256", "Sha384")


def _t(name):
    """Itanium fragment of a type of the anonymous namespace inside tg."""
    return "NS0_%d%sE" % (len(name), name)


# the (PRF hash, handle) pairs a TLS 1.2 suite can produce: the SHA-384 PRF goes
# with AES-256-GCM (single key or table) and AES-256-CBC + HMAC-SHA384 alone
AEAD_PAIRS = [("Sha256", nk, lay) for nk, lay in ((4, 0), (4, 1), (4, 2), (8, 0), (8, 1), (8, 2), (0, 3))] + [
    ("Sha384", 8, 0), ("Sha384", 8, 1)]
CBC_PAIRS = [("Sha256", 4, "Sha1"), ("Sha256", 4, "Sha256"), ("Sha256", 8, "Sha1"), ("Sha256", 8, "Sha256"),
             ("Sha384", 8, "Sha384")]

ALL = {"prf_pack_kernel": ("15prf_pack_kernelE",)}
for h in HASHES:
    ALL["tls12_prf_kernel<%s>" % h] = ("16tls12_prf_kernelI%sEE" % _t(h),)
# tls12_install_kernel<H, NK, LAYOUT>: (NK, LAYOUT) as rekey_kernel's
for h, nk, lay in AEAD_PAIRS:
    ALL["tls12_install_kernel<%s, %d, %d>" % (h, nk, lay)] = (
        "20tls12_install_kernelI%sLi%dELi%dEE" % (_t(h), nk, lay),)
# tls12_cbcrow_install_kernel<PRF hash, NK, MAC>; a MAC equal to the PRF hash
# mangles as a substitution
for h, nk, mac in CBC_PAIRS:
    ALL["tls12_cbcrow_install_kernel<%s, %d, %s>" % (h, nk, mac)] = (
        "27tls12_cbcrow_install_kernelI%sLi%dE%sEE" % (_t(h), nk, "S2_" if mac == h else _t(mac)),)
for nk in (4, 8):
    for mac in MACS:
        ALL["cbcrows_kernel<%d, %s>" % (nk, mac)] = ("14cbcrows_kernelILi%dE%sEE" % (nk, _t(mac)),)


def test_every_instantiation_is_listed(kernels):  # noqa: F811
    assert len(ALL) == 1 + 2 + 9 + 5 + 6
    # and nothing else is built: a pair no suite uses is an argument error, not a kernel
    names = [k for k in kernels if not k.endswith(".kd")]
    for frag, count in (("20tls12_install_kernelI", 9), ("27tls12_cbcrow_install_kernelI", 5),
                        ("14cbcrows_kernelI", 6), ("16tls12_prf_kernelI", 2), ("15prf_pack_kernelE", 1)):
        assert len([k for k in names if frag in k]) == count, frag


@pytest.mark.parametrize("label", sorted(ALL))
def test_tls12_kernel_has_no_private_segment(kernels, label):  # noqa: F811
    frags = ALL[label]
    found = [v for k, v in kernels.items() if all(f in k for f in frags) and not k.endswith(".kd")]
    assert len(found) == 1, (label, len(found))
    meta = found[0]
    assert meta["vgpr_spill_count"] == 0, (label, meta)
    assert meta["private_segment_fixed_size"] == 0, (label, meta)

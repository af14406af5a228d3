"""CPU check of the built library's code-object metadata for the TLS 1.3 key
schedule (tls13.hip): the Extract, Expand-Label-rows, Finished, handshake-stage
and application-stage kernels are there exactly once per hash, spill no VGPRs
and have no private segment, and nothing else with the tls13_ prefix is built.
These kernels run on callers' streams between record batches; a private
segment would bring back the per-queue scratch allocation
(test_kernel_metadata.py has the reason).  The application stage holds two
HMAC midstates, a hash state, sixteen message words and four digests at once --
with SHA-384 all of them 64-bit -- so this is the check that they still fit."""
import pytest

from test_kernel_metadata import kernels  # noqa: F401  (module-scoped fixture)

HASHES = ("Sha256", "Sha384")
NAMES = ("tls13_extract_kernel", "tls13_expand_rows_kernel", "tls13_finished_kernel", "tls13_handshake_kernel",
         "tls13_application_kernel")


def _frag(name, h):
    """Itanium fragment of name<tg::(anonymous namespace)::h>."""
    return "%d%sINS0_%d%sEEE" % (len(name), name, len(h), h)


ALL = dict(("%s<%s>" % (name, h), _frag(name, h)) for name in NAMES for h in HASHES)


def test_every_instantiation_is_listed(kernels):  # noqa: F811
    assert len(ALL) == 10
    built = sorted(k for k in kernels if "tls13_" in k and not k.endswith(".kd"))
    assert len(built) == len(ALL), built
    for label, frag in ALL.items():
        assert len([k for k in built if frag in k]) == 1, label


@pytest.mark.parametrize("label", sorted(ALL))
def test_tls13_kernel_has_no_private_segment(kernels, label):  # noqa: F811
    found = [v for k, v in kernels.items() if ALL[label] in k and not k.endswith(".kd")]
    assert len(found) == 1, (label, len(found))
    meta = found[0]
    assert meta["vgpr_spill_count"] == 0, (label, meta)
    assert meta["private_segment_fixed_size"] == 0, (label, meta)

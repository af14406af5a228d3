"""Register budget of the ChaCha20-Poly1305 lane kernels from the built
library's code-object metadata (the reader of test_kernel_metadata.py).

The tile loop holds the state, the keystream, a record's first-round words,
Poly1305 and both forms of the tile's addressing at 4 waves per SIMD: at most
128 VGPRs.  The single-key kernels with the LDS-DMA tile (the headline's) must
fit without a spill or a private segment; the key-table kernels, which hold
the key per lane as well, may spill no more than they did before the
wave-relative addressing went in.
"""
import pytest

from test_kernel_metadata import kernels  # noqa: F401  (the module-scoped fixture)

# chacha_kernel<OPEN, MULTIKEY, 4, DMA> by mangled-name fragment
SINGLE_DMA = {
    "seal": "13chacha_kernelILb0ELb0ELi4ELb1EE",
    "open": "13chacha_kernelILb1ELb0ELi4ELb1EE",
}

# vgpr_spill_count of the key-table instantiations at commit daa7e2b (the
# parent of this change), read from its gfx950 build with
# -Rpass-analysis=kernel-resource-usage and the same metadata notes:
# LDS-DMA tile 0 (seal) / 3 (open), register-staged tile 7 / 21.
MULTIKEY_PARENT_SPILLS = {
    "13chacha_kernelILb0ELb1ELi4ELb1EE": 0,
    "13chacha_kernelILb1ELb1ELi4ELb1EE": 3,
    "13chacha_kernelILb0ELb1ELi4ELb0EE": 7,
    "13chacha_kernelILb1ELb1ELi4ELb0EE": 21,
}


def _one(kernels, frag):  # noqa: F811
    found = [v for k, v in kernels.items() if frag in k]
    assert len(found) == 1, (frag, len(found))
    return found[0]


@pytest.mark.parametrize("role", sorted(SINGLE_DMA))
def test_single_key_dma_kernel_fits(kernels, role):  # noqa: F811
    meta = _one(kernels, SINGLE_DMA[role])
    assert meta["vgpr_spill_count"] == 0, (role, meta)
    assert meta["private_segment_fixed_size"] == 0, (role, meta)
    assert meta["vgpr_count"] <= 128, (role, meta)


@pytest.mark.parametrize("frag", sorted(MULTIKEY_PARENT_SPILLS))
def test_key_table_kernel_spills_no_more_than_before(kernels, frag):  # noqa: F811
    meta = _one(kernels, frag)
    assert meta["vgpr_spill_count"] <= MULTIKEY_PARENT_SPILLS[frag], (frag, meta)
    assert meta["vgpr_count"] <= 128, (frag, meta)

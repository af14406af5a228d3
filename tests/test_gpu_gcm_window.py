"""The single-key AES-GCM hybrid kernel's 256-counter window paths on the GPU
(gcm_variant 15: aes_bs8.h win_rounds on the bitsliced waves, aes_round.h
win_consts on the T-table waves), bit-exact against the oracle.

Record lengths sit on the window edges -- block k has counter k + 2, so a
window ends at block 254 + 256 m -- and cover every residue mod 8 (every lane
offset rho of an octet), the headline's 1 024 / 1 025-block shapes and a
partial last block; three records run past counter 2^16, where the bitsliced
waves fall back to full rounds.  The records are shuffled, so the eight records
of an octet job mix lengths: some lanes finish or cross a window while others
do not.  hy_t 16 runs T-table waves only, hy_t -1 bitsliced waves only (16 of
them: one B buffer per wave, the crossing batches in full rounds); the default
split keeps two buffers per bitsliced wave."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    return t


@pytest.fixture(scope="module")
def tg(torch):
    import tlsgpu
    return tlsgpu


BLOCKS = ([0, 1, 8, 63, 64, 65] + list(range(253, 263)) + list(range(509, 513)) +
          list(range(1021, 1027)))
BYTES = [16 * 254 - 1, 16 * 254 + 1, 16 * 1024 + 5]
LONG = [16 * 65533, 16 * 65534, 16 * 65535 + 5]   # last counters 65 535 / 65 536 / 65 537


def edge_lens(seed):
    lens = [16 * b for b in BLOCKS] * 3 + BYTES * 2 + LONG
    np.random.default_rng(seed).shuffle(lens)
    assert len(lens) <= 120
    return [int(x) for x in lens]


OPTS = [{}, {"hy_t": 16}, {"hy_t": -1}]


CASES = [(o, k, a) for o in OPTS for k in (16, 32) for a in (16, 1)] + [({"hy_threads": 768}, 16, 16)]


@pytest.mark.parametrize("opts,klen,align", CASES, ids=lambda v: "-".join(
    "%s%d" % kv for kv in sorted(v.items())) or "default" if isinstance(v, dict) else str(v))
def test_window_edges_vs_oracle(torch, tg, oracle_mod, opts, klen, align):
    from batchpack import HostBatch, run_seal_open
    seed = 1000 * klen + 10 * align + len(opts) + sum(opts.values())
    lens = edge_lens(seed)
    hb = HostBatch(lens, payload_seed=seed, align=align, aad_mode="tls13")
    key = np.random.default_rng(seed).bytes(klen)
    obj = tg.HipAESGCM(bytearray(key))
    tamper = tuple(sorted({2, lens.index(LONG[1]), lens.index(16 * 255), lens.index(BYTES[2])}))
    with tg.options(gcm_variant=15, **opts):
        run_seal_open(torch, tg, oracle_mod, hb, "aesgcm", np.frombuffer(key, np.uint8), obj,
                      tamper=tamper)


@pytest.mark.parametrize("opts", OPTS, ids=["default", "hy_t16", "hy_t-1"])
def test_uniform_16k_batch_vs_oracle(torch, tg, oracle_mod, opts):
    """Twenty full 16 KiB records (not a multiple of 8: the last octet job is
    half empty), every lane in step through the same four windows."""
    from batchpack import HostBatch, run_seal_open
    hb = HostBatch([16384] * 20, payload_seed=77, align=16, aad_mode="tls13")
    key = np.random.default_rng(78).bytes(16)
    obj = tg.HipAESGCM(bytearray(key))
    with tg.options(gcm_variant=15, **opts):
        run_seal_open(torch, tg, oracle_mod, hb, "aesgcm", np.frombuffer(key, np.uint8), obj,
                      tamper=(0, 19))

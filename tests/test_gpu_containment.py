"""GPU: the AEAD batch kernels write a record's own bytes and nothing else.

Every kernel behind tg_seal_batch / tg_open_batch is forced in turn on a
guarded batch (tests/guarded.py): canary-filled buffers, 48-byte canary gaps
between the extents, input and output address residues chosen independently,
a status array longer than the batch.  Whole buffers are compared with the
image the C oracle gives, so a store outside ``len + T`` bytes (seal) or
``len`` bytes (open), on accepted and on rejected records, fails the test
with the record and the offset it landed at.  The record lengths
(guarded.LENS) are the smallest at which a store path changes.
"""
import zlib

import numpy as np
import pytest

import guarded as G

pytestmark = pytest.mark.gpu

NKEYS = 7


class Case(object):
    """One kernel path: algorithm, key length, tag length, key count, record
    count (None: the length list as it is) and the options that force it."""

    def __init__(self, alg, klen, opts, n=None, nkeys=1, modes=("aligned", "skewed")):
        self.alg, self.klen, self.opts, self.n, self.nkeys, self.modes = alg, klen, dict(opts), n, nkeys, modes
        self.tag = 8 if alg == "aesccm8" else 16
        name = {"aesgcm": "gcm%d", "chacha": "chacha%d", "aesccm": "ccm%d", "aesccm8": "ccm8_%d"}[alg] % (8 * klen)
        if alg == "chacha":
            name = "chacha"
        parts = [name] + (["table"] if nkeys > 1 else []) + \
            ["%s=%d" % kv for kv in sorted(self.opts.items())] + (["n%d" % n] if n else [])
        self.id = "-".join(parts if (self.opts or n) else parts + ["default"])

    def seed(self, mode):
        return zlib.crc32(("%s/%s" % (self.id, mode)).encode())

    def layout(self, mode):
        seed = self.seed(mode)
        return G.GuardedLayout(G.case_lens(seed, self.n), self.tag, mode, seed=seed + 1, key_count=self.nkeys)


def _cases():
    c = []
    both = ("aligned", "skewed", "in0_out5")
    for klen in (16, 32):          # single-key AES-GCM
        for w in (1, 4, 16):
            c.append(Case("aesgcm", klen, {"gcm_variant": 6, "waves_per_record": w}))
        for v in (16, 14, 15):
            c.append(Case("aesgcm", klen, {"gcm_variant": v}, modes=both if (v, klen) == (15, 16) else both[:2]))
        for o in ({"hy_t": 16}, {"hy_t": -1}, {"hy_threads": 768}):
            c.append(Case("aesgcm", klen, dict(o, gcm_variant=15)))
        for v in (16, 14, 15):
            c.append(Case("aesgcm", klen, {"gcm_variant": v}, n=G.PLANNED_N))
        c.append(Case("aesgcm", klen, {}))
    for w in (1, 4, 16):           # single-key ChaCha20-Poly1305
        c.append(Case("chacha", 32, {"chacha_variant": 3, "waves_per_record": w}))
    for v in (4, 5, 6):
        c.append(Case("chacha", 32, {"chacha_variant": v}))
    for v in (4, 5, 6):
        c.append(Case("chacha", 32, {"chacha_variant": v}, n=G.PLANNED_N))
    c.append(Case("chacha", 32, {}, modes=both))
    for alg in ("aesccm", "aesccm8"):   # AES-CCM and CCM_8
        for klen in (16, 32):
            for v in (1, 2, 3, 4, 5, 8):
                c.append(Case(alg, klen, {"ccm_variant": v}, modes=both if (v, klen) == (4, 16) else both[:2]))
            c.append(Case(alg, klen, {"ccm_variant": 4, "ccm_hy_t": -1}))
    for klen in (16, 32):          # key tables, AES-GCM
        for v in (1, 5, 6, 14):
            c.append(Case("aesgcm", klen, {"gcm_table_variant": v}, nkeys=NKEYS))
        for lpr in (8, 16, 32, 64, -1):
            c.append(Case("aesgcm", klen, {"gcm_table_variant": 0, "kt_split": 1000, "kt_lpr": lpr}, nkeys=NKEYS,
                          modes=both if (lpr, klen) == (32, 16) else both[:2]))
        for o in ({"kt_hybrid": -1}, {"kt_t": 1}, {"kt_t": 11}, {"kt_overlap": -1}):
            c.append(Case("aesgcm", klen, dict(o, kt_lpr=32), nkeys=NKEYS))
        c.append(Case("aesgcm", klen, {}, n=G.PLANNED_N, nkeys=NKEYS))
    c.append(Case("chacha", 32, {}, nkeys=NKEYS))
    c.append(Case("chacha", 32, {"chacha_variant": 4}, nkeys=NKEYS))
    for alg, klen in (("aesccm", 16), ("aesccm8", 32)):
        for v in (2, 3):
            c.append(Case(alg, klen, {"ccm_variant": v}, nkeys=NKEYS))
    return c


CASES = _cases()
assert len(set(c.id for c in CASES)) == len(CASES)


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


def _key_object(tg, case, keys):
    if case.nkeys > 1:
        name = {"aesgcm": "aesgcm", "chacha": "chacha20-poly1305", "aesccm": "aesccm", "aesccm8": "aesccm_8"}
        return tg.KeyTable(name[case.alg], keys)
    if case.alg == "aesgcm":
        return tg.HipAESGCM(bytearray(keys[0]))
    if case.alg == "chacha":
        return tg.HipCHACHA20_POLY1305(bytearray(keys[0]))
    return tg.HipAESCCM(bytearray(keys[0]), tag_length=case.tag)


@pytest.mark.parametrize("case,mode", [pytest.param(c, m, id="%s-%s" % (c.id, m)) for c in CASES for m in c.modes])
def test_batch_writes_only_its_extents(torch, tg, oracle_mod, case, mode):
    lay = case.layout(mode)
    rng = np.random.default_rng(case.seed(mode) + 2)
    keys = [rng.bytes(case.klen) for _ in range(case.nkeys)]
    karr = np.frombuffer(b"".join(keys), np.uint8)
    if case.nkeys > 1:
        karr = karr.reshape(case.nkeys, case.klen)
    reject = G.make_reject(lay, case.seed(mode) + 3)
    G.check_reject_coverage(lay, reject)
    with tg.options(**case.opts):
        G.run_guarded(torch, tg, oracle_mod, lay, case.alg, karr, _key_object(tg, case, keys), reject)

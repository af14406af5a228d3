"""GPU: rekeying live key handles in place (tg_key_replace_device,
tg_sessions_rekey; KeyTable.replace, Sessions.key_update / install) against
handles built fresh from the same keys, the reference RecordLayer's KeyUpdate
wire bytes (tests/golden/keyupdate.json) and the key-derivation and framing
oracles.  Everything is bit-exact."""
import functools
import hashlib

import numpy as np
import pytest

from batchpack import HostBatch
from test_gpu_session_records import Batch, _i32, _i64
from vectors import detbytes, load

pytestmark = pytest.mark.gpu

CASES = load("keyupdate.json")
BAD_MAC = 1


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


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _rows(torch, rows):
    return _dev(torch, np.frombuffer(b"".join(rows), np.uint8).reshape(len(rows), len(rows[0])).copy())


def _seal(torch, tg, hb, key):
    d = hb.to_device(torch)
    tg.seal_batch(key, hb.batch_kwargs(d))
    torch.cuda.synchronize()
    return d["out"].cpu().numpy()


# ---- 1. a replaced table seals like a fresh one -------------------------------------

NKEYS = 300                                  # not a multiple of the power kernel's four keys per block
BOUNDARY = [0, 1, 15, 16, 17, 1000, 1535, 1536, 2047, 2048, 16384]
SKIPPED = {40: NKEYS, 200: 2 ** 32 - 1}      # list position -> out-of-range slot
ALGS = {"aesgcm16": ("aesgcm", 16, 16), "aesgcm32": ("aesgcm", 32, 16), "aesccm16": ("aesccm", 16, 16),
        "aesccm_8-32": ("aesccm_8", 32, 8), "chacha": ("chacha20-poly1305", 32, 16)}
GCM_OPTIONS = [dict(gcm_table_variant=1), dict(gcm_table_variant=5), dict(gcm_table_variant=6),
               dict(gcm_table_variant=14), dict(kt_split=1, kt_hybrid=0), dict(kt_split=1, kt_hybrid=-1),
               dict(kt_split=1, kt_lpr=-1)]


@functools.lru_cache(maxsize=None)
def _replace_case(name):
    """Host side of test 1 for one algorithm (built once): the old and new
    keys, the slot list and a ragged batch that uses every key."""
    alg, klen, tag = ALGS[name]
    rng = np.random.default_rng(300 + klen + tag + len(alg))
    old = [rng.bytes(klen) for _ in range(NKEYS)]
    picked = [0, NKEYS - 1] + [int(x) for x in rng.permutation(np.arange(1, NKEYS - 1))[:268]]
    slots = [picked[j] for j in rng.permutation(270)]           # 270 distinct slots: two blocks of lanes
    for pos, bad in sorted(SKIPPED.items()):
        slots.insert(pos, bad)
    new = [rng.bytes(klen) for _ in slots]                      # the skipped slots' rows are never used
    final = list(old)
    for s, k in zip(slots, new):
        if s < NKEYS:
            final[s] = k
    assert len(slots) == 272 and sum(a != b for a, b in zip(old, final)) == 270
    # 320 records, so that each of the 300 keys seals at least one
    lens = BOUNDARY + [int(x) for x in rng.integers(0, 3000, 320 - len(BOUNDARY))]
    hb = HostBatch(lens, payload_seed=klen + tag, key_count=NKEYS, tag=tag)
    hb.key_idx = np.concatenate([rng.permutation(NKEYS), rng.integers(0, NKEYS, 20)]).astype(np.uint32)
    assert set(hb.key_idx.tolist()) == set(range(NKEYS))
    return old, slots, new, final, hb


def _replaced_equals_fresh(torch, tg, name, options):
    alg, klen, tag = ALGS[name]
    old, slots, new, final, hb = _replace_case(name)
    table = tg.KeyTable(alg, old)
    table.replace(slots, new)
    with tg.options(**options):
        got = _seal(torch, tg, hb, table)
        want = _seal(torch, tg, hb, tg.KeyTable(alg, final))
        before = _seal(torch, tg, hb, tg.KeyTable(alg, old))
    assert np.array_equal(got, want), (name, options)
    assert not np.array_equal(got, before)


@pytest.mark.parametrize("options", [{}] + GCM_OPTIONS, ids=lambda o: "-".join("%s%d" % kv for kv in o.items()) or "auto")
@pytest.mark.parametrize("name", ["aesgcm16", "aesgcm32"])
def test_replaced_gcm_table_seals_like_a_fresh_one(torch, tg, name, options):
    _replaced_equals_fresh(torch, tg, name, options)


@pytest.mark.parametrize("name", ["aesccm16", "aesccm_8-32", "chacha"])
def test_replaced_table_seals_like_a_fresh_one(torch, tg, name):
    _replaced_equals_fresh(torch, tg, name, {})


@pytest.mark.parametrize("name", sorted(ALGS))
def test_replace_one_slot_and_null_slot_list(torch, tg, name):
    alg, klen, tag = ALGS[name]
    old, _, new, _, hb = _replace_case(name)
    # n = 1, the table's last entry
    table = tg.KeyTable(alg, old)
    table.replace([NKEYS - 1], new[:1])
    assert np.array_equal(_seal(torch, tg, hb, table), _seal(torch, tg, hb, tg.KeyTable(alg, old[:-1] + new[:1])))
    # slot = NULL: rows 0 .. n-1, n = 7 (a partial block of the power kernel)
    table = tg.KeyTable(alg, old)
    table.replace(None, _rows(torch, new[:7]))
    assert np.array_equal(_seal(torch, tg, hb, table), _seal(torch, tg, hb, tg.KeyTable(alg, new[:7] + old[7:])))
    # under the split path too when the table is AES-GCM (planes and rotated keys)
    if alg == "aesgcm":
        with tg.options(kt_split=1):
            assert np.array_equal(_seal(torch, tg, hb, table),
                                  _seal(torch, tg, hb, tg.KeyTable(alg, new[:7] + old[7:])))


# ---- 2. the single-key handle ----------------------------------------------------------

@pytest.mark.parametrize("klen", [16, 32])
def test_single_key_handle_is_rebuilt_in_full(torch, tg, klen):
    rng = np.random.default_rng(klen)
    old, new = rng.bytes(klen), rng.bytes(klen)
    key = tg.KeyTable("aesgcm", [old])                 # nkeys == 1: the single-key GcmKeyDev handle
    fresh_old, fresh_new = tg.HipAESGCM(bytearray(old)), tg.HipAESGCM(bytearray(new))
    small = HostBatch(BOUNDARY + [int(x) for x in rng.integers(0, 5000, 40)], payload_seed=klen)   # wave path
    n, L = 32768, 80                                   # above 24 576 records: the large-batch kernel
    inp = torch.randint(0, 256, (n * L,), dtype=torch.uint8, device="cuda")
    nonce = torch.randint(0, 256, (n * 12,), dtype=torch.uint8, device="cuda")
    aad = torch.randint(0, 256, (5,), dtype=torch.uint8, device="cuda")

    def large(k):
        out = torch.zeros(n * (L + 16), dtype=torch.uint8, device="cuda")
        tg.seal_batch(k, tg.make_batch(n, inp, out, nonce, aad=aad, fixed_len=L, in_stride=L, out_stride=L + 16,
                                       fixed_aad_len=5))
        torch.cuda.synchronize()
        return out

    # a slot list that names another entry than 0: the handle stays as it is
    key.replace([1], [new])
    assert np.array_equal(_seal(torch, tg, small, key), _seal(torch, tg, small, fresh_old))
    assert torch.equal(large(key), large(fresh_old))
    key.replace([0], [new])
    assert np.array_equal(_seal(torch, tg, small, key), _seal(torch, tg, small, fresh_new))
    assert torch.equal(large(key), large(fresh_new))
    for variant in (14, 16):                           # the bitsliced planes and the T-table lane kernel
        with tg.options(gcm_variant=variant):
            assert np.array_equal(_seal(torch, tg, small, key), _seal(torch, tg, small, fresh_new)), variant
    key.replace(None, [old])                           # slot NULL: entry 0
    assert np.array_equal(_seal(torch, tg, small, key), _seal(torch, tg, small, fresh_old))


# ---- 3. stream order -------------------------------------------------------------------

@pytest.mark.parametrize("name", ["aesgcm16", "chacha"])
def test_replace_is_ordered_on_the_stream(torch, tg, name):
    alg, klen, tag = ALGS[name]
    old, slots, new, final, hb = _replace_case(name)
    want_a = _seal(torch, tg, hb, tg.KeyTable(alg, old))
    want_b = _seal(torch, tg, hb, tg.KeyTable(alg, final))
    table = tg.KeyTable(alg, old)
    da, db = hb.to_device(torch), hb.to_device(torch)
    d_slots, d_new = _dev(torch, _i32(slots)), _rows(torch, new)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):                         # three enqueues, no host sync in between
        tg.seal_batch(table, hb.batch_kwargs(da))
        table.replace(d_slots, d_new)
        tg.seal_batch(table, hb.batch_kwargs(db))
    s.synchronize()
    assert np.array_equal(da["out"].cpu().numpy(), want_a)
    assert np.array_equal(db["out"].cpu().numpy(), want_b)


# ---- 4. KeyUpdate against the reference -------------------------------------------------

def _phase_batch(torch, c, phase):
    recs = phase["records"]
    datas = [bytes(detbytes("kurec-%d-%d" % (r["index"], r["len"]), r["len"])) for r in recs]
    return datas, Batch(torch, "tls13", c["alg"], [r["conn"] for r in recs], [r["ctype"] for r in recs], datas,
                        [r["pad"] for r in recs])


def _sessions(torch, tg, c):
    s = tg.Sessions.from_traffic_secrets(c["suite"], _rows(torch, [bytes.fromhex(x) for x in c["initial_secrets"]]))
    s.seq().copy_(_dev(torch, _i64(c["starts"])))
    return s


def _state(s):
    return ([bytes(r).hex() for r in s.secrets.cpu().numpy()], [bytes(r).hex() for r in s.ivs.cpu().numpy()],
            [int(x) & (2 ** 64 - 1) for x in s.seq().cpu().numpy()])


@pytest.mark.parametrize("ci", range(len(CASES)), ids=[c["alg"] for c in CASES])
def test_key_update_matches_reference_wire_bytes(torch, tg, ci):
    c = CASES[ci]
    tx, rx = _sessions(torch, tg, c), _sessions(torch, tg, c)
    assert tx.hashlen == c["hashlen"] and tx.cipher_suite == c["suite"]
    sent = []
    for p, phase in enumerate(c["phases"]):
        datas, b = _phase_batch(torch, c, phase)
        wires, _, _ = b.seal(tg, tx.table, tx.ivs, seq_next=tx.seq())
        for r, w in zip(phase["records"], wires):
            assert len(w) == r["wire_len"], (p, r["index"])
            assert hashlib.sha256(w).hexdigest() == r["wire_sha256"], (p, r["index"])
            if "wire" in r:
                assert w.hex() == r["wire"], (p, r["index"])
        opened, _, _ = b.open(tg, rx.table, rx.ivs, wires, seq_next=rx.seq())
        for r, d, o in zip(phase["records"], datas, opened):
            assert o == (0, r["ctype"], d), (p, r["index"])
        want = ([a["secret"] for a in phase["after"]], [a["iv"] for a in phase["after"]],
                [a["seqnum"] for a in phase["after"]])
        assert _state(tx) == want, p                   # the untouched sessions too
        assert _state(rx) == want, p
        sent.append((b, wires))
        if p < len(c["updates"]):
            tx.key_update(c["updates"][p])
            rx.key_update(_dev(torch, _i32(c["updates"][p])))
    # a phase-0 record of connection 1 after that connection's update: the old key is gone
    stale = _sessions(torch, tg, c)
    stale.key_update(c["updates"][0])
    b0, wires0 = sent[0]
    opened, _, _ = b0.open(tg, stale.table, stale.ivs, wires0, seq_next=stale.seq())
    conns = [r["conn"] for r in c["phases"][0]["records"]]
    assert 1 in conns and 2 in conns
    for conn, r, o in zip(conns, c["phases"][0]["records"], opened):
        if conn in c["updates"][0]:
            assert o[0] == BAD_MAC, r["index"]
        else:
            assert o[0] == 0, r["index"]


# ---- 5. INSTALL ---------------------------------------------------------------------------

@pytest.mark.parametrize("ci", range(len(CASES)), ids=[c["alg"] for c in CASES])
def test_install_equals_sessions_built_from_the_new_secrets(torch, tg, ci):
    c = CASES[ci]
    h = c["hashlen"]
    live = _sessions(torch, tg, c)
    live.seq().copy_(_dev(torch, _i64([7, 8, 2 ** 40, 10])))
    secrets = [bytes.fromhex(x) for x in c["initial_secrets"]]
    new = [bytes(detbytes("install-%s-%d" % (c["alg"], j), h)) for j in range(2)]
    live.install([3, 1], _rows(torch, new))
    secrets[3], secrets[1] = new
    fresh = tg.Sessions.from_traffic_secrets(c["suite"], _rows(torch, secrets))
    torch.cuda.synchronize()
    assert live.seq().cpu().tolist() == [7, 0, 2 ** 40, 0]    # counters of the installed slots only
    assert torch.equal(live.ivs, fresh.ivs) and torch.equal(live.secrets, fresh.secrets)
    fresh.seq().copy_(live.seq())
    datas, b = _phase_batch(torch, c, c["phases"][0])
    w_live, _, _ = b.seal(tg, live.table, live.ivs, seq_next=live.seq())
    w_fresh, _, _ = b.seal(tg, fresh.table, fresh.ivs, seq_next=fresh.seq())
    assert w_live == w_fresh and all(w_live)
    # a Sessions without a secrets table takes an install as well (no key_update afterwards)
    bare = tg.Sessions(tg.KeyTable.from_device(fresh.table.alg, torch.zeros(4 * fresh.table.keylen, dtype=torch.uint8,
                                                                            device="cuda"), 4, fresh.table.keylen),
                       torch.zeros((4, 12), dtype=torch.uint8, device="cuda"), cipher_suite=c["suite"])
    bare.install(None, _rows(torch, secrets))
    torch.cuda.synchronize()
    assert torch.equal(bare.ivs, fresh.ivs) and bare.secrets is None
    bare.seq().copy_(_dev(torch, _i64([7, 0, 2 ** 40, 0])))
    w_bare, _, _ = b.seal(tg, bare.table, bare.ivs, seq_next=bare.seq())
    assert w_bare == w_live
    with pytest.raises(ValueError, match="without traffic secrets"):
        bare.key_update([0])


# ---- 6. both hashes, three generations ----------------------------------------------------

@pytest.mark.parametrize("suite,alg,hashlen", [(0x1301, "aes128gcm", 32), (0x1302, "aes256gcm", 48)])
def test_three_generations_against_the_oracle(torch, tg, suite, alg, hashlen):
    from oracle import keysetup as K
    from oracle import records as R
    nsess = 70
    rng = np.random.default_rng(suite)
    secrets = [bytes(detbytes("gen-secret-%x-%d" % (suite, s), hashlen)) for s in range(nsess)]
    chosen = sorted(int(x) for x in rng.permutation(nsess)[:33])
    slots = [int(x) for x in rng.permutation(chosen)]
    slots.insert(5, nsess)                              # skipped: nothing of theirs is touched
    slots.insert(20, 2 ** 32 - 1)
    tx = tg.Sessions.from_traffic_secrets(suite, _rows(torch, secrets))
    d_slots = _dev(torch, _i32(slots))
    seq = [0] * nsess
    for gen in range(3):
        tx.seq().add_(gen + 3)                          # counters in use before each update
        seq = [q + gen + 3 for q in seq]
        tx.key_update(d_slots)
        for s in chosen:
            secrets[s] = K.key_update(suite, secrets[s])
            seq[s] = 0
    torch.cuda.synchronize()
    host = [K.traffic_keys(suite, s) for s in secrets]
    got_sec, got_iv, got_seq = _state(tx)
    assert got_sec == [s.hex() for s in secrets]
    assert got_iv == [iv.hex() for _, iv in host]
    assert got_seq == seq and set(seq) == {0, 12}
    sessions = [int(x) for x in rng.permutation(nsess)]
    lens = [int(x) for x in rng.choice([0, 1, 16, 17, 100, 1000, 5000], nsess)]
    datas = [rng.bytes(L) for L in lens]
    pads = [int(x) for x in rng.integers(0, 40, nsess)]
    b = Batch(torch, "tls13", alg, sessions, [23] * nsess, datas, pads)
    wires, _, _ = b.seal(tg, tx.table, tx.ivs, seq_next=tx.seq())
    for i, s in enumerate(sessions):
        key, iv = host[s]
        assert wires[i] == R.seal_record("tls13", alg, key, iv, seq[s], 23, datas[i], pads[i]), (i, s)


@pytest.mark.parametrize("suite,alg,hashlen", [(0x1301, "aes128gcm", 32), (0x1302, "aes256gcm", 48)])
def test_one_session_on_the_single_key_handle(torch, tg, suite, alg, hashlen):
    """nsessions == 1: the handle is the single-key GcmKeyDev, rebuilt through
    the derivation (update, update, install) with all of its tables."""
    from oracle import keysetup as K
    from oracle import records as R
    secret = bytes(detbytes("one-secret-%x" % suite, hashlen))
    other = bytes(detbytes("one-install-%x" % suite, hashlen))
    tx = tg.Sessions.from_traffic_secrets(suite, _rows(torch, [secret]))
    assert tx.table.nkeys == 1
    rng = np.random.default_rng(suite + 1)
    lens = [0, 1, 17, 1000, 16384] + [int(x) for x in rng.integers(0, 4000, 19)]
    datas = [rng.bytes(L) for L in lens]
    b = Batch(torch, "tls13", alg, [0] * len(lens), [23] * len(lens), datas, [0] * len(lens))
    steps = [lambda: tx.key_update([7]),                # another entry than 0: nothing changes
             lambda: tx.key_update([0]), lambda: tx.key_update(None),
             lambda: tx.install([0], _rows(torch, [other]))]
    expect = [secret, K.key_update(suite, secret), K.key_update(suite, K.key_update(suite, secret)), other]
    seq = 0
    for step, want in zip(steps, expect):
        if step is not steps[0]:
            seq = 0
        step()
        key, iv = K.traffic_keys(suite, want)
        assert _state(tx) == ([want.hex()], [iv.hex()], [seq])
        wires, _, _ = b.seal(tg, tx.table, tx.ivs, seq_next=tx.seq())
        for i, d in enumerate(datas):
            assert wires[i] == R.seal_record("tls13", alg, key, iv, seq + i, 23, d, 0), i
        seq += len(lens)


# ---- 7. refusals that need a live handle ----------------------------------------------------

def test_refusals_launch_nothing(torch, tg):
    c = CASES[0]
    s = _sessions(torch, tg, c)
    before = _state(s)
    with pytest.raises(tg.TlsGpuError, match="above the key handle's nkeys"):
        s.key_update([0, 1, 2, 3, 4])
    with pytest.raises(tg.TlsGpuError, match="above the key handle's nkeys"):
        s.table.replace([0, 1, 2, 3, 4], [bytes(16)] * 5)
    import ctypes
    from tlsgpu import _lib
    r = _lib.TgRekey()
    r.n, r.mode, r.hashlen, r.nsessions = 1, _lib.TG_REKEY_UPDATE, 32, 3
    r.secrets, r.iv_table = s.secrets.data_ptr(), s.ivs.data_ptr()
    assert _lib.load().tg_sessions_rekey(s.table._dkey.handle, ctypes.byref(r), None) == _lib.TG_EINVAL
    assert b"nsessions (3) must equal" in _lib.load().tg_last_error()
    s.key_update([])                                    # n == 0: TG_OK, nothing launched
    s.table.replace(None, torch.zeros(16, dtype=torch.uint8, device="cuda")[:0])
    torch.cuda.synchronize()
    assert _state(s) == before

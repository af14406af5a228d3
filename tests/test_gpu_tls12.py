"""GPU: TLS 1.2 key setup on the device -- tg_tls12_prf, the CBC rows built
from device memory, and the fused installs into live tables -- against the
reference's outputs (tests/golden/tls12_keys.json) and its wire bytes for the
TLS 1.2 connections of cbc_sessions.json and sessions.json, whose keys the
device now derives from the fixtures' master secrets and randoms.  Where a
fixture has keys but no wire bytes, the expected record comes from the framing
oracle (oracle/records.py) or the CBC model (tests/cbc_model.py) under the
fixture's key; both are held to the reference's wire bytes by their own tests.

No test provokes a fault: every out-of-range slot is a documented skip."""
import functools
import hashlib

import numpy as np
import pytest

import cbc_model
import guarded
import tls12_model as m
from test_cbc_sessions_oracle import record_data, wire_matches
from test_gpu_cbc_sessions import SBatch
from test_gpu_session_records import Batch, _host_rank, _i64, _table_alg
from vectors import detbytes, load

pytestmark = pytest.mark.gpu

KEYS = load("tls12_keys.json")
CBC_CASES = [c for c in load("cbc_sessions.json") if c["version"] == [3, 3]]
CBC_IDS = ["%s-%s" % (c["suite"], "etm" if c["etm"] else "mte") for c in CBC_CASES]
AEAD_CASES = [c for c in load("sessions.json") if c["version"] == "tls12"]
PENDING = dict((c["suite"], c) for c in KEYS["pending"])
CANARY = 0xC7
TLS12 = 0x0303


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


def _rows(torch, rows, odd=False):
    """Byte strings of one length as an n x len device tensor; ``odd``: at an
    address 1 past a 256-byte boundary, so nothing in it is 4-byte aligned."""
    n, w = len(rows), len(rows[0])
    host = np.frombuffer(b"".join(rows), np.uint8).copy()
    if not odd:
        return torch.from_numpy(host.reshape(n, w)).cuda()
    flat = torch.zeros(n * w + 1, dtype=torch.uint8, device="cuda")
    assert flat.data_ptr() % 4 == 0
    view = flat[1:].view(n, w)
    view.copy_(torch.from_numpy(host.reshape(n, w)))
    return view


def _inputs(torch, triples, odd=False):
    """(master secrets, client randoms, server randoms) device tensors."""
    return tuple(_rows(torch, [t[k] for t in triples], odd) for k in range(3))


# ---- 1. tg_tls12_prf -----------------------------------------------------------
PRF_ENTRIES = [("prf", c) for c in KEYS["prf"]] + [("calc_key", c) for c in KEYS["calc_key"]]
VARIANTS = 7   # row r carries the fixture's inputs when r % 7 == 0, else a variant of them


@functools.lru_cache(maxsize=None)
def _prf_row(ei, v):
    """(secret, seed, expected output) of variant v of entry ei; the label is
    shared.  Variant 0 is the fixture's own row; the others are held by the
    host model, which reproduces every fixture row (test_tls12_model.py)."""
    kind, c = PRF_ENTRIES[ei]
    secret, label, seed = m.prf_inputs(c) if kind == "prf" else m.calc_key_inputs(c)
    if v == 0:
        return secret, seed, bytes.fromhex(c["out"])
    secret = bytes(detbytes("k12-var-secret-%d-%d" % (ei, v), len(secret)))
    seed = bytes(detbytes("k12-var-seed-%d-%d" % (ei, v), len(seed)))
    return secret, seed, m.prf(c["hashlen"], secret, label, seed, c["outlen"])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_prf_matches_every_fixture_entry(torch, tg, n):
    for ei, (kind, c) in enumerate(PRF_ENTRIES):
        label = (m.prf_inputs(c) if kind == "prf" else m.calc_key_inputs(c))[1]
        rows = [_prf_row(ei, r % VARIANTS) for r in range(n)]
        outlen, guard = c["outlen"], 64
        secrets = _rows(torch, [r[0] for r in rows], odd=True)
        seeds = _rows(torch, [r[1] for r in rows], odd=True) if len(rows[0][1]) else None
        flat = torch.full((guard + 1 + n * outlen + guard,), CANARY, dtype=torch.uint8, device="cuda")
        out = flat[guard + 1:guard + 1 + n * outlen].view(n, outlen)
        assert out.data_ptr() % 4 == 1
        got = tg.keysetup.tls12_prf(secrets, label, seeds, outlen, c["hashlen"], out=out)
        torch.cuda.synchronize()
        assert got is out
        host = flat.cpu().numpy()
        want = b"".join(r[2] for r in rows)
        assert host[guard + 1:guard + 1 + n * outlen].tobytes() == want, (kind, c["hashlen"], c.get("label"), c["outlen"])
        assert (host[:guard + 1] == CANARY).all() and (host[guard + 1 + n * outlen:] == CANARY).all(), (kind, ei)


# ---- 2. the key block, both sides ---------------------------------------------
@pytest.mark.parametrize("case", KEYS["pending"], ids=[c["suite"] for c in KEYS["pending"]])
def test_key_block_reproduces_both_sides(torch, tg, case):
    n = len(case["conns"])
    ms, cr, sr = _inputs(torch, [m.pending_inputs(case["suite"], c) for c in range(n)])
    cut = tg.keysetup.tls12_key_block(case["suite_id"], ms, cr, sr)
    torch.cuda.synchronize()
    cmac, smac, ckey, skey, civ, siv = [t.cpu().numpy() for t in cut]
    aead = tg.keysetup.TLS12_SUITES[case["suite_id"]][3] is None
    for c, conn in enumerate(case["conns"]):
        assert ckey[c].tobytes().hex() == conn["client"]["key"] and skey[c].tobytes().hex() == conn["server"]["key"]
        assert cmac[c].tobytes().hex() == conn["client"]["mac_key"]
        assert smac[c].tobytes().hex() == conn["server"]["mac_key"]
        if aead:
            assert civ[c].tobytes().hex() == conn["client"]["iv"] and siv[c].tobytes().hex() == conn["server"]["iv"]


# ---- 3. CBC sessions from master secrets: the reference's wire bytes -----------
@pytest.mark.parametrize("case", CBC_CASES, ids=CBC_IDS)
def test_cbc_sessions_from_master_secrets(torch, tg, case):
    recs, mac, etm = case["records"], case["mac"], case["etm"]
    n = len(recs)
    ms, cr, sr = _inputs(torch, [m.cbc_sessions_inputs(case, c) for c in range(5)], odd=True)
    suite = m.CBC_SUITE_IDS[case["suite"]]
    send = tg.CbcSessions.from_master_secrets(suite, ms, cr, sr, "client", TLS12, etm)
    recv = tg.CbcSessions(send.table, TLS12, etm)
    assert len(send) == 5 and guarded.download(send.seq(), np.uint64).tolist() == [0] * 5
    starts = guarded.upload(torch, np.array(case["starts"], np.uint64)).view(torch.int64)
    send.seq().copy_(starts)
    recv.seq().copy_(starts)
    datas = [record_data(i, r) for i, r in enumerate(recs)]
    b = SBatch(torch, mac, etm, datas, aligned=False)
    b.inputs([r["conn"] for r in recs], [r["ctype"] for r in recs], [bytes.fromhex(r["iv"]) for r in recs])
    send.seal(b.session, n, b.data, b.d_off, b.d_len, b.ctype, b.iv, b.wire, b.w_off, b.w_len)
    recv.open(b.session, n, b.wire, b.w_off, b.w_len, b.out, b.o_off, b.o_len, b.o_ct, b.st)
    torch.cuda.synchronize()
    wires, _, _ = b.wires()
    for i, (r, w) in enumerate(zip(recs, wires)):
        assert wire_matches(r, w), (i, r["conn"], r["len"])
    opened, _ = b.opened()
    for i, (r, d) in enumerate(zip(recs, datas)):
        assert opened[i] == (0, r["ctype"], r["len"], d), (i, opened[i][:3])
    send.table.close()


# ---- 4. AEAD sessions from master secrets: 4-byte and 12-byte IV rows ----------
@pytest.mark.parametrize("case", AEAD_CASES, ids=[c["alg"] for c in AEAD_CASES])
def test_aead_sessions_from_master_secrets(torch, tg, case):
    recs = case["records"]
    ms, cr, sr = _inputs(torch, [m.sessions_inputs(case, c) for c in range(5)], odd=True)
    suite = m.SESSIONS_SUITE_IDS[case["alg"]]
    s = tg.Sessions.from_master_secrets(suite, ms, cr, sr, "client")
    torch.cuda.synchronize()
    assert s.version == TLS12 and s.ivs.shape == (5, len(case["ivs"][0]) // 2)
    assert [bytes(r).hex() for r in s.ivs.cpu().numpy()] == case["ivs"]
    assert guarded.download(s.seq(), np.uint64).tolist() == [0] * 5
    sessions = [r["conn"] for r in recs]
    datas = [bytes(detbytes("srec-%d-%d" % (i, r["len"]), r["len"])) for i, r in enumerate(recs)]
    b = Batch(torch, "tls12", case["alg"], sessions, [r["ctype"] for r in recs], datas, [0] * len(recs), False)
    nxt = torch.from_numpy(_i64(case["starts"])).cuda()
    wires, _, _ = b.seal(tg, s.table, s.ivs, seq_next=nxt)
    for r, w in zip(recs, wires):
        assert len(w) == r["wire_len"] and hashlib.sha256(w).hexdigest() == r["wire_sha256"], case["alg"]
    nxt2 = torch.from_numpy(_i64(case["starts"])).cuda()
    opened, _, _ = b.open(tg, s.table, s.ivs, wires, seq_next=nxt2)
    for r, d, o in zip(recs, datas, opened):
        assert o == (0, r["ctype"], d)


# ---- probes: one short record per listed session, explicit numbers --------------
class AeadProbe(object):
    def __init__(self, torch, alg, sessions, seqs):
        self.torch, self.alg, self.sessions, self.seqs = torch, alg, list(sessions), list(seqs)
        self.n = n = len(self.sessions)
        self.datas = [bytes(detbytes("k12-probe-%d" % i, 33 + i % 9)) for i in range(n)]
        self.ctypes = [(23, 22, 21)[i % 3] for i in range(n)]
        host = np.zeros(64 * n, np.uint8)
        for i, d in enumerate(self.datas):
            host[64 * i:64 * i + len(d)] = np.frombuffer(d, np.uint8)
        up = lambda a: guarded.upload(torch, a)   # noqa: E731
        self.data, self.d_off = up(host), up(np.arange(n, dtype=np.uint64) * 64)
        self.w_off = up(np.arange(n, dtype=np.uint64) * 128 + 3)
        self.d_len = up(np.array([len(d) for d in self.datas], np.uint32))
        self.ctype = up(np.array(self.ctypes, np.uint8))
        self.session = up(np.array(self.sessions, np.uint32))
        self.seq = up(np.array(self.seqs, np.uint64)).view(torch.int64)

    def seal(self, tg, table, ivs, stream=None):
        """Enqueues the seal; -> (wire, wire_len) device tensors, not synchronised."""
        t = self.torch
        wire = t.zeros(128 * self.n + 16, dtype=t.uint8, device="cuda")
        w_len = t.full((self.n,), -1, dtype=t.int32, device="cuda")
        tg.seal_session_records(table, TLS12, ivs, self.session, self.n, self.data, self.d_off, self.d_len,
                                self.ctype, wire, self.w_off, w_len, seq=self.seq, stream=stream)
        return wire, w_len

    @staticmethod
    def host(result):
        wire, w_len = result
        wh, wl = wire.cpu().numpy(), w_len.cpu().numpy()
        return [wh[128 * i + 3:128 * i + 3 + max(int(k), 0)].tobytes() for i, k in enumerate(wl)]

    def want(self, i, key, iv):
        from oracle import records as R
        return R.seal_record("tls12", self.alg, key, iv, self.seqs[i], self.ctypes[i], self.datas[i])


class CbcProbe(object):
    def __init__(self, torch, mac, etm, sessions, seqs):
        self.torch, self.mac, self.etm = torch, mac, etm
        self.sessions, self.seqs = list(sessions), list(seqs)
        self.n = n = len(self.sessions)
        self.datas = [bytes(detbytes("k12-cprobe-%d" % i, 33 + i % 9)) for i in range(n)]
        self.ctypes = [(23, 22, 21)[i % 3] for i in range(n)]
        self.ivs = [bytes(detbytes("k12-cprobe-iv-%d" % i, 16)) for i in range(n)]
        host = np.zeros(64 * n, np.uint8)
        for i, d in enumerate(self.datas):
            host[64 * i:64 * i + len(d)] = np.frombuffer(d, np.uint8)
        up = lambda a: guarded.upload(torch, a)   # noqa: E731
        self.data, self.d_off = up(host), up(np.arange(n, dtype=np.uint64) * 64)
        self.w_off = up(np.arange(n, dtype=np.uint64) * 192 + 3)
        self.d_len = up(np.array([len(d) for d in self.datas], np.uint32))
        self.ctype = up(np.array(self.ctypes, np.uint8))
        self.session = up(np.array(self.sessions, np.uint32))
        self.seq = up(np.array(self.seqs, np.uint64)).view(torch.int64)
        self.iv = up(np.frombuffer(b"".join(self.ivs), np.uint8))

    def seal(self, tg, table, stream=None):
        t = self.torch
        wire = t.zeros(192 * self.n + 16, dtype=t.uint8, device="cuda")
        w_len = t.full((self.n,), -1, dtype=t.int32, device="cuda")
        tg.cbc.seal_session_records(table, TLS12, self.etm, self.session, self.n, self.data, self.d_off,
                                    self.d_len, self.ctype, self.iv, wire, self.w_off, w_len, seq=self.seq,
                                    stream=stream)
        return wire, w_len

    @staticmethod
    def host(result):
        wire, w_len = result
        wh, wl = wire.cpu().numpy(), w_len.cpu().numpy()
        return [wh[192 * i + 3:192 * i + 3 + max(int(k), 0)].tobytes() for i, k in enumerate(wl)]

    def open(self, tg, table, result):
        """Opens the sealed records again; -> [(status, ctype, plaintext)]."""
        t = self.torch
        wire, w_len = result
        out = t.full((192 * self.n,), CANARY, dtype=t.uint8, device="cuda")
        o_off = guarded.upload(t, np.arange(self.n, dtype=np.uint64) * 192)
        o_len = t.full((self.n,), -1, dtype=t.int32, device="cuda")
        o_ct = t.full((self.n,), 255, dtype=t.uint8, device="cuda")
        st = t.full((self.n,), 255, dtype=t.uint8, device="cuda")
        tg.cbc.open_session_records(table, TLS12, self.etm, self.session, self.n, wire, self.w_off, w_len, out,
                                    o_off, o_len, o_ct, st, seq=self.seq)
        oh = out.cpu().numpy()
        return [(int(a), int(c), oh[192 * i:192 * i + max(int(k), 0)].tobytes())
                for i, (a, c, k) in enumerate(zip(st.cpu().numpy(), o_ct.cpu().numpy(), o_len.cpu().numpy()))]

    def want(self, i, enc_key, mac_key):
        return cbc_model.seal_record(enc_key, mac_key, self.mac, TLS12, self.etm, self.seqs[i], self.ctypes[i],
                                     self.datas[i], self.ivs[i])


# ---- 5. rows built from device memory ------------------------------------------
@pytest.mark.parametrize("etm", [0, 1], ids=["mte", "etm"])
@pytest.mark.parametrize("keylen", [16, 32])
@pytest.mark.parametrize("mac", ["sha1", "sha256", "sha384"])
def test_cbc_rows_from_device_match_host_rows(torch, tg, keylen, mac, etm):
    """A device-built and a host-built table do the same in both directions:
    seal reads a row's ek and midstates, open its dk (the inverse schedule)."""
    n, maclen = 67, tg.cbc.MAC_LENGTH[mac]
    enc = [bytes(detbytes("k12-rows-enc-%d" % j, keylen)) for j in range(n)]
    mk = [bytes(detbytes("k12-rows-mac-%d" % j, maclen)) for j in range(n)]
    host_table = tg.CbcKey.table(enc, mk, mac)
    dev_table = tg.CbcKey.table_from_device(_rows(torch, enc, odd=True), _rows(torch, mk, odd=True), mac)
    assert dev_table.nkeys == n and dev_table._keylen() == keylen
    p = CbcProbe(torch, mac, etm, range(n), [5 + 3 * j for j in range(n)])
    sealed = p.seal(tg, host_table)
    a, b = p.host(sealed), p.host(p.seal(tg, dev_table))
    assert a == b and a[0] == p.want(0, enc[0], mk[0]) and a[n - 1] == p.want(n - 1, enc[n - 1], mk[n - 1])
    plain = [(0, p.ctypes[i], p.datas[i]) for i in range(n)]
    assert p.open(tg, dev_table, sealed) == plain and p.open(tg, host_table, sealed) == plain
    # in place: scattered distinct slots, one of them out of range (skipped), a MAC key of another length
    slots = [66, 0, 31, n + 4]
    enc2 = [bytes(detbytes("k12-rows-enc2-%d" % j, keylen)) for j in range(4)]
    mk2 = [bytes(detbytes("k12-rows-mac2-%d" % j, 13)) for j in range(4)]
    dev_table.replace_device(slots, _rows(torch, enc2, odd=True), _rows(torch, mk2, odd=True))
    host_table.replace(slots, enc2, mk2)
    sealed = p.seal(tg, host_table)
    a, b = p.host(sealed), p.host(p.seal(tg, dev_table))
    assert a == b
    for j, s in enumerate(slots[:3]):
        assert b[s] == p.want(s, enc2[j], mk2[j])
    assert b[1] == p.want(1, enc[1], mk[1])
    assert p.open(tg, dev_table, sealed) == plain
    # the documented argument errors that need a live handle
    one_e, one_m = _rows(torch, enc2[:1]), _rows(torch, mk2[:1])
    lib, h = dev_table._lib, dev_table.handle
    assert lib.tg_cbc_key_replace_device(h, None, one_e.data_ptr(), one_m.data_ptr(), 13, n + 1, None) == -22
    assert b"rows for a table of" in lib.tg_last_error()
    block = 128 if mac == "sha384" else 64
    for bad in (0, block + 1):
        assert lib.tg_cbc_key_replace_device(h, None, one_e.data_ptr(), one_m.data_ptr(), bad, 1, None) == -22
        assert b"mac key length must be 1..%d" % block in lib.tg_last_error()
    assert p.open(tg, dev_table, sealed) == plain   # and they changed nothing
    host_table.close()
    dev_table.close()


# ---- 6. install into a live table ------------------------------------------------
NS = 65
SLOTS = [64, 0, 33, 7, 12]          # the fixture's connections 0..4
OUT_OF_RANGE = NS + 5


def _guarded(torch, shape, dtype, guard):
    """A canary-filled flat tensor and its middle viewed as ``shape``."""
    count = int(np.prod(shape))
    flat = torch.full((guard + count + guard,), CANARY if dtype == torch.uint8 else -0x3839, dtype=dtype,
                      device="cuda")
    return flat, flat[guard:guard + count].view(*shape)


def _guards_intact(flat, guard, fill):
    h = flat.cpu().numpy()
    return bool((h[:guard] == fill).all() and (h[-guard:] == fill).all())


def _aead_install_case(kind):
    """(suite id, oracle alg name, key length, IV length, [(ms, cr, sr)], [(key, iv)])"""
    if kind in ("gcm-table", "chacha"):
        case = AEAD_CASES[0 if kind == "gcm-table" else 1]
        assert case["alg"] == ("aes256gcm" if kind == "gcm-table" else "chacha20-poly1305")
        ins = [m.sessions_inputs(case, c) for c in range(5)]
        keys = [(bytes.fromhex(k), bytes.fromhex(v)) for k, v in zip(case["keys"], case["ivs"])]
        return m.SESSIONS_SUITE_IDS[case["alg"]], case["alg"], 32, len(keys[0][1]), ins, keys, case
    name = {"ccm": "TLS_RSA_WITH_AES_128_CCM_8", "gcm-single": "TLS_RSA_WITH_AES_128_GCM_SHA256"}[kind]
    case = PENDING[name]
    ins = [m.pending_inputs(name, c) for c in range(3)]
    keys = [(bytes.fromhex(c["client"]["key"]), bytes.fromhex(c["client"]["iv"])) for c in case["conns"]]
    return case["suite_id"], "aes128ccm_8" if kind == "ccm" else "aes128gcm", 16, 4, ins, keys, None


@pytest.mark.parametrize("kind", ["gcm-table", "chacha", "ccm"])
def test_aead_install_in_place(torch, tg, kind):
    suite, alg, keylen, ivlen, ins, keys, case = _aead_install_case(kind)
    old_keys = [bytes(detbytes("k12-old-key-%s-%d" % (kind, s), keylen)) for s in range(NS)]
    old_ivs = [bytes(detbytes("k12-old-iv-%s-%d" % (kind, s), ivlen)) for s in range(NS)]
    table = tg.KeyTable(_table_alg(alg), old_keys)
    iv_flat, ivs = _guarded(torch, (NS, ivlen), torch.uint8, 64)
    ivs.copy_(_rows(torch, old_ivs))
    seq_flat, seq = _guarded(torch, (NS,), torch.int64, 8)
    seq.copy_(torch.arange(100, 100 + NS, dtype=torch.int64, device="cuda"))
    s = tg.Sessions(table, ivs, TLS12, seq_next=seq, cipher_suite=suite)
    p = AeadProbe(torch, alg, range(NS), [1000 + 7 * j for j in range(NS)])
    before = p.host(p.seal(tg, table, ivs))
    assert before[5] == p.want(5, old_keys[5], old_ivs[5])

    slots = SLOTS[:len(ins)] + [OUT_OF_RANGE]
    rows = ins + [(bytes(detbytes("k12-skip-ms", 48)), bytes(detbytes("k12-skip-cr", 32)),
                   bytes(detbytes("k12-skip-sr", 32)))]
    ms, cr, sr = _inputs(torch, rows, odd=True)
    s.install_tls12(slots, ms, cr, sr, "client")
    after = p.host(p.seal(tg, table, ivs))
    torch.cuda.synchronize()
    seq_host, iv_host = guarded.download(seq, np.uint64).tolist(), ivs.cpu().numpy()
    for slot in range(NS):
        if slot in slots:
            key, iv = keys[slots.index(slot)]
            assert after[slot] == p.want(slot, key, iv), (kind, slot)
            assert seq_host[slot] == 0 and iv_host[slot].tobytes() == iv, (kind, slot)
        else:
            assert after[slot] == before[slot], (kind, slot)
            assert seq_host[slot] == 100 + slot and iv_host[slot].tobytes() == old_ivs[slot], (kind, slot)
    assert _guards_intact(iv_flat, 64, CANARY) and _guards_intact(seq_flat, 8, -0x3839)

    if case is not None:   # the reference's own wire bytes through the installed slots
        recs = case["records"]
        sessions = [SLOTS[r["conn"]] for r in recs]
        want_seq, _ = _host_rank([r["conn"] for r in recs], case["starts"])
        datas = [bytes(detbytes("srec-%d-%d" % (i, r["len"]), r["len"])) for i, r in enumerate(recs)]
        b = Batch(torch, "tls12", case["alg"], sessions, [r["ctype"] for r in recs], datas, [0] * len(recs), True)
        wires, _, _ = b.seal(tg, table, ivs, seq=torch.from_numpy(_i64(want_seq)).cuda())
        for r, w in zip(recs, wires):
            assert len(w) == r["wire_len"] and hashlib.sha256(w).hexdigest() == r["wire_sha256"], kind

    # the documented argument errors that need a live handle
    with pytest.raises(tg.TlsGpuError, match="above the key handle's nkeys"):
        big = _inputs(torch, [rows[0]] * (NS + 1))
        s.install_tls12(None, big[0], big[1], big[2], "client")
    r = tg.keysetup.tls12_install_args(1, 32, "client", NS + 1, None, ms[:1], cr[:1], sr[:1], ivlen, ivs, None)
    import ctypes
    lib, handle = table._dkey._lib, table._dkey.handle
    assert lib.tg_sessions_install_tls12(handle, ctypes.byref(r), None) == -22
    assert b"must equal the key handle's nkeys" in lib.tg_last_error()
    if kind != "gcm-table":   # the SHA-384 PRF goes with AES-256-GCM alone
        r = tg.keysetup.tls12_install_args(1, 48, "client", NS, None, ms[:1], cr[:1], sr[:1], ivlen, ivs, None)
        assert lib.tg_sessions_install_tls12(handle, ctypes.byref(r), None) == -22
        assert b"no TLS 1.2 suite pairs" in lib.tg_last_error()
    # TLS 1.2 sessions have no traffic secret: the TLS 1.3 calls refuse them
    with pytest.raises(ValueError, match="TLS 1.3"):
        s.key_update([0])
    with pytest.raises(ValueError, match="TLS 1.3"):
        s.install([0], ms[:1])
    with pytest.raises(ValueError, match="neither TLS13_SUITES nor TLS12_SUITES"):
        tg.Sessions(table, ivs, TLS12, seq_next=seq, cipher_suite=0x0005)
    assert p.host(p.seal(tg, table, ivs)) == after


def test_single_key_gcm_handle_install(torch, tg):
    suite, alg, keylen, ivlen, ins, keys, _ = _aead_install_case("gcm-single")
    old_key, old_iv = bytes(detbytes("k12-single-old", 16)), bytes(detbytes("k12-single-old-iv", 4))
    table = tg.KeyTable("aesgcm", [old_key])
    assert table.nkeys == 1
    iv_flat, ivs = _guarded(torch, (1, 4), torch.uint8, 64)
    ivs.copy_(_rows(torch, [old_iv]))
    seq_flat, seq = _guarded(torch, (1,), torch.int64, 8)
    seq.fill_(9)
    s = tg.Sessions(table, ivs, TLS12, seq_next=seq, cipher_suite=suite)
    p = AeadProbe(torch, alg, [0] * 6, [0, 1, 2, 2 ** 32 - 1, 2 ** 32, 77])
    before = p.host(p.seal(tg, table, ivs))
    assert before[3] == p.want(3, old_key, old_iv)
    ms, cr, sr = _inputs(torch, ins[:1], odd=True)
    # slot 1 does not exist: nothing changes, not even the chain behind the key
    s.install_tls12([1], ms, cr, sr, "client")
    same = p.host(p.seal(tg, table, ivs))
    torch.cuda.synchronize()
    assert same == before and int(seq.item()) == 9 and ivs.cpu().numpy().tobytes() == old_iv
    s.install_tls12([0], ms, cr, sr, "client")
    after = p.host(p.seal(tg, table, ivs))
    torch.cuda.synchronize()
    for i in range(p.n):
        assert after[i] == p.want(i, *keys[0]), i
    assert int(seq.item()) == 0 and ivs.cpu().numpy().tobytes() == keys[0][1]
    assert _guards_intact(iv_flat, 64, CANARY) and _guards_intact(seq_flat, 8, -0x3839)


@pytest.mark.parametrize("case", [CBC_CASES[0], CBC_CASES[3], CBC_CASES[4]],
                         ids=[CBC_IDS[0], CBC_IDS[3], CBC_IDS[4]])
def test_cbc_install_in_place(torch, tg, case):
    mac, etm = case["mac"], case["etm"]
    suite = m.CBC_SUITE_IDS[case["suite"]]
    keylen, maclen = tg.keysetup.TLS12_SUITES[suite][1], tg.keysetup.TLS12_SUITES[suite][4]
    old_enc = [bytes(detbytes("k12-cold-enc-%d" % s, keylen)) for s in range(NS)]
    old_mac = [bytes(detbytes("k12-cold-mac-%d" % s, maclen)) for s in range(NS)]
    table = tg.CbcKey.table(old_enc, old_mac, mac)
    seq_flat, seq = _guarded(torch, (NS,), torch.int64, 8)
    seq.copy_(torch.arange(100, 100 + NS, dtype=torch.int64, device="cuda"))
    s = tg.CbcSessions(table, TLS12, etm, seq_next=seq, cipher_suite=suite)
    p = CbcProbe(torch, mac, etm, range(NS), [1000 + 7 * j for j in range(NS)])
    before = p.host(p.seal(tg, table))
    assert before[5] == p.want(5, old_enc[5], old_mac[5])

    slots = SLOTS + [OUT_OF_RANGE]
    rows = [m.cbc_sessions_inputs(case, c) for c in range(5)] + [
        (bytes(detbytes("k12-skip-ms", 48)), bytes(detbytes("k12-skip-cr", 32)), bytes(detbytes("k12-skip-sr", 32)))]
    ms, cr, sr = _inputs(torch, rows, odd=True)
    s.install(slots, ms, cr, sr, "client")
    after = p.host(p.seal(tg, table))
    torch.cuda.synchronize()
    seq_host = guarded.download(seq, np.uint64).tolist()
    for slot in range(NS):
        if slot in SLOTS:
            c = SLOTS.index(slot)
            assert after[slot] == p.want(slot, bytes.fromhex(case["enc_keys"][c]), bytes.fromhex(case["mac_keys"][c]))
            assert seq_host[slot] == 0, slot
        else:
            assert after[slot] == before[slot] and seq_host[slot] == 100 + slot, slot
    assert _guards_intact(seq_flat, 8, -0x3839)

    # the reference's own wire bytes through the installed slots (explicit numbers)
    recs = case["records"]
    datas = [record_data(i, r) for i, r in enumerate(recs)]
    b = SBatch(torch, mac, etm, datas, aligned=True)
    b.inputs([SLOTS[r["conn"]] for r in recs], [r["ctype"] for r in recs], [bytes.fromhex(r["iv"]) for r in recs],
             seq=[r["seq"] for r in recs])
    tg.cbc.seal_session_records(table, TLS12, etm, b.session, b.n, b.data, b.d_off, b.d_len, b.ctype, b.iv, b.wire,
                                b.w_off, b.w_len, seq=b.seq)
    torch.cuda.synchronize()
    wires, _, _ = b.wires()
    for i, (r, w) in enumerate(zip(recs, wires)):
        assert wire_matches(r, w), (i, r["conn"], r["len"])
    with pytest.raises(tg.TlsGpuError, match="above the key handle's nkeys"):
        big = _inputs(torch, [rows[0]] * (NS + 1))
        s.install(None, big[0], big[1], big[2], "client")
    import ctypes
    hashlen = tg.keysetup.TLS12_SUITES[suite][5]
    r = tg.keysetup.tls12_install_args(1, hashlen, "client", NS + 1, None, ms[:1], cr[:1], sr[:1])
    assert table._lib.tg_cbc_sessions_install_tls12(table.handle, ctypes.byref(r), None) == -22
    assert b"must equal the key handle's nkeys" in table._lib.tg_last_error()
    # a PRF hash that no suite pairs with this table's key length and MAC
    r = tg.keysetup.tls12_install_args(1, 80 - hashlen, "client", NS, None, ms[:1], cr[:1], sr[:1])
    assert table._lib.tg_cbc_sessions_install_tls12(table.handle, ctypes.byref(r), None) == -22
    assert b"no TLS 1.2 suite pairs" in table._lib.tg_last_error()
    assert p.host(p.seal(tg, table)) == after
    table.close()


# ---- 7. stream ordering: batch, install, batch, no sync in between ----------------
def test_install_is_ordered_on_its_stream(torch, tg):
    suite, alg, keylen, ivlen, ins, keys, _ = _aead_install_case("gcm-table")
    old_keys = [bytes(detbytes("k12-ord-key-%d" % s, keylen)) for s in range(NS)]
    old_ivs = [bytes(detbytes("k12-ord-iv-%d" % s, ivlen)) for s in range(NS)]
    table = tg.KeyTable("aesgcm", old_keys)
    ivs = _rows(torch, old_ivs)
    s = tg.Sessions(table, ivs, TLS12, cipher_suite=suite)
    p = AeadProbe(torch, alg, range(NS), [3 * j for j in range(NS)])
    ms, cr, sr = _inputs(torch, ins)
    slots = guarded.upload(torch, np.array(SLOTS, np.uint32))
    ccase = CBC_CASES[2]
    csuite = m.CBC_SUITE_IDS[ccase["suite"]]
    c_enc = [bytes(detbytes("k12-ord-enc-%d" % j, 32)) for j in range(NS)]
    c_mac = [bytes(detbytes("k12-ord-mac-%d" % j, 32)) for j in range(NS)]
    ctable = tg.CbcKey.table(c_enc, c_mac, ccase["mac"])
    cs = tg.CbcSessions(ctable, TLS12, ccase["etm"], cipher_suite=csuite)
    cp = CbcProbe(torch, ccase["mac"], ccase["etm"], range(NS), [3 * j for j in range(NS)])
    cms, ccr, csr = _inputs(torch, [m.cbc_sessions_inputs(ccase, c) for c in range(5)])
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        first = p.seal(tg, table, ivs, stream=st)
        s.install_tls12(slots, ms, cr, sr, "client", stream=st)
        second = p.seal(tg, table, ivs, stream=st)
        cfirst = cp.seal(tg, ctable, stream=st)
        cs.install(slots, cms, ccr, csr, "client", stream=st)
        csecond = cp.seal(tg, ctable, stream=st)
    st.synchronize()
    first, second, cfirst, csecond = p.host(first), p.host(second), cp.host(cfirst), cp.host(csecond)
    for slot in range(NS):
        assert first[slot] == p.want(slot, old_keys[slot], old_ivs[slot]), slot
        assert cfirst[slot] == cp.want(slot, c_enc[slot], c_mac[slot]), slot
        if slot in SLOTS:
            c = SLOTS.index(slot)
            assert second[slot] == p.want(slot, *keys[c]), slot
            assert csecond[slot] == cp.want(slot, bytes.fromhex(ccase["enc_keys"][c]),
                                            bytes.fromhex(ccase["mac_keys"][c])), slot
        else:
            assert second[slot] == first[slot] and csecond[slot] == cfirst[slot], slot
    ctable.close()


# ---- 8. the server's write keys -----------------------------------------------------
@pytest.mark.parametrize("name,alg", [("TLS_RSA_WITH_AES_128_GCM_SHA256", "aes128gcm"),
                                      ("TLS_RSA_WITH_AES_256_GCM_SHA384", "aes256gcm"),
                                      ("TLS_RSA_WITH_AES_128_CCM_8", "aes128ccm_8"),
                                      ("TLS_ECDHE_RSA_WITH_CHACHA20_POLY1305_SHA256", "chacha20-poly1305"),
                                      ("TLS_ECDHE_RSA_WITH_CHACHA20_POLY1305_draft_00", "chacha20-poly1305")])
def test_server_side_aead(torch, tg, name, alg):
    case = PENDING[name]
    n = len(case["conns"])
    ms, cr, sr = _inputs(torch, [m.pending_inputs(name, c) for c in range(n)], odd=True)
    for side in ("server", "client"):
        s = tg.Sessions.from_master_secrets(case["suite_id"], ms, cr, sr, side)
        p = AeadProbe(torch, alg, [2, 0, 1, 1, 2], [0, 1, 2 ** 32 - 1, 2 ** 32, 5])
        got = p.host(p.seal(tg, s.table, s.ivs))
        for i, c in enumerate(p.sessions):
            key, iv = bytes.fromhex(case["conns"][c][side]["key"]), bytes.fromhex(case["conns"][c][side]["iv"])
            assert got[i] == p.want(i, key, iv), (name, side, i)


@pytest.mark.parametrize("name", ["TLS_RSA_WITH_AES_128_CBC_SHA", "TLS_RSA_WITH_AES_256_CBC_SHA256",
                                  "TLS_ECDHE_RSA_WITH_AES_256_CBC_SHA384"])
def test_server_side_cbc(torch, tg, name):
    case = PENDING[name]
    n = len(case["conns"])
    mac = tg.keysetup.TLS12_SUITES[case["suite_id"]][3]
    ms, cr, sr = _inputs(torch, [m.pending_inputs(name, c) for c in range(n)], odd=True)
    for side in ("server", "client"):
        for etm in (0, 1):
            s = tg.CbcSessions.from_master_secrets(case["suite_id"], ms, cr, sr, side, TLS12, etm)
            p = CbcProbe(torch, mac, etm, [2, 0, 1, 1, 2], [0, 1, 2 ** 32 - 1, 2 ** 32, 5])
            got = p.host(p.seal(tg, s.table))
            for i, c in enumerate(p.sessions):
                keys = case["conns"][c][side]
                assert got[i] == p.want(i, bytes.fromhex(keys["key"]), bytes.fromhex(keys["mac_key"])), (side, etm, i)
            s.table.close()


# ---- 9. creation on a stream that is not the current one ----------------------------
def test_from_master_secrets_on_another_stream(torch, tg):
    name = "TLS_RSA_WITH_AES_256_GCM_SHA384"
    case = PENDING[name]
    cname = "TLS_ECDHE_RSA_WITH_AES_256_CBC_SHA384"
    ccase = PENDING[cname]
    ms, cr, sr = _inputs(torch, [m.pending_inputs(name, c) for c in range(3)])
    cms, ccr, csr = _inputs(torch, [m.pending_inputs(cname, c) for c in range(3)])
    p = AeadProbe(torch, "aes256gcm", [2, 0, 1], [0, 1, 2])
    cp = CbcProbe(torch, "sha384", 0, [2, 0, 1], [0, 1, 2])
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    assert torch.cuda.current_stream() != st
    s = tg.Sessions.from_master_secrets(case["suite_id"], ms, cr, sr, "server", stream=st)
    cs = tg.CbcSessions.from_master_secrets(ccase["suite_id"], cms, ccr, csr, "server", TLS12, 0, stream=st)
    cut = tg.keysetup.tls12_key_block(case["suite_id"], ms, cr, sr, stream=st)
    with torch.cuda.stream(st):
        got, cgot = p.seal(tg, s.table, s.ivs, stream=st), cp.seal(tg, cs.table, stream=st)
    st.synchronize()
    got, cgot = p.host(got), cp.host(cgot)
    for i, c in enumerate(p.sessions):
        k = case["conns"][c]["server"]
        assert got[i] == p.want(i, bytes.fromhex(k["key"]), bytes.fromhex(k["iv"])), i
        ck = ccase["conns"][c]["server"]
        assert cgot[i] == cp.want(i, bytes.fromhex(ck["key"]), bytes.fromhex(ck["mac_key"])), i
        assert cut[3][c].cpu().numpy().tobytes().hex() == k["key"]
    assert guarded.download(s.seq(), np.uint64).tolist() == [0] * 3
    assert guarded.download(cs.seq(), np.uint64).tolist() == [0] * 3
    cs.table.close()

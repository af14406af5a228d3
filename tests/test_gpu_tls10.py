"""GPU: TLS 1.0 / 1.1 key setup on the device -- tg_tls10_prf (P_MD5 xor
P_SHA1) and the fused install of its key block into live CBC tables -- against
the reference's outputs (tests/golden/tls10_keys.json) and its wire bytes for
the TLS 1.1 connections of cbc_sessions.json, whose keys the device now derives
from the fixture's master secrets and randoms.  Where a fixture has keys but no
wire bytes, the expected record comes from the CBC model (tests/cbc_model.py)
under the fixture's key; the model is held to the reference's wire bytes by its
own tests.  Everything is bit-exact.

No test provokes a fault: every out-of-range slot is a documented skip."""
import ctypes
import functools

import numpy as np
import pytest

import cbc_model
import guarded
import tls10_model as m
import tls12_model
from test_cbc_sessions_oracle import record_data, wire_matches
from test_gpu_cbc_sessions import SBatch, _zeros_then_canary
from test_gpu_tls12 import (CANARY, NS, OUT_OF_RANGE, SLOTS, CbcProbe, _guarded, _guards_intact, _inputs, _rows)
from vectors import detbytes, load

pytestmark = pytest.mark.gpu

KEYS = load("tls10_keys.json")
CASES = [c for c in load("cbc_sessions.json") if c["version"] == [3, 2]]
IDS = ["%s-%s" % (c["suite"], "etm" if c["etm"] else "mte") for c in CASES]
PENDING = dict((c["suite"], c) for c in KEYS["pending"])
TLS11 = 0x0302
BAD_MAC = 1
AES128_SHA, AES256_SHA, AES128_SHA256 = 0x002f, 0x0035, 0x003c


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


class Probe11(CbcProbe):
    """CbcProbe with TLS 1.1 in the record header and the MAC input."""

    def seal(self, tg, table, stream=None):
        t = self.torch
        wire = t.zeros(192 * self.n + 16, dtype=t.uint8, device="cuda")
        w_len = t.full((self.n,), -1, dtype=t.int32, device="cuda")
        tg.cbc.seal_session_records(table, TLS11, self.etm, self.session, self.n, self.data, self.d_off,
                                    self.d_len, self.ctype, self.iv, wire, self.w_off, w_len, seq=self.seq,
                                    stream=stream)
        return wire, w_len

    def want(self, i, enc_key, mac_key):
        return cbc_model.seal_record(enc_key, mac_key, self.mac, TLS11, self.etm, self.seqs[i], self.ctypes[i],
                                     self.datas[i], self.ivs[i])


# ---- 1. tg_tls10_prf -----------------------------------------------------------
PRF_ENTRIES = [("prf", c) for c in KEYS["prf"]] + [("calc_key", c) for c in KEYS["calc_key"]]
VARIANTS = 7   # row r carries the fixture's inputs when r % 7 == 0, else a variant of them


def _entry_inputs(kind, c):
    return m.prf_inputs(c) if kind == "prf" else m.calc_key_inputs(c)


@functools.lru_cache(maxsize=None)
def _prf_row(ei, v):
    """(secret, seed, expected output) of variant v of entry ei; the label is
    shared.  Variant 0 is the fixture's own row; the others are held by the
    host model, which reproduces every fixture row (test_tls10_model.py)."""
    kind, c = PRF_ENTRIES[ei]
    secret, label, seed = _entry_inputs(kind, c)
    if v == 0:
        return secret, seed, bytes.fromhex(c["out"])
    secret = bytes(detbytes("k10-var-secret-%d-%d" % (ei, v), len(secret)))
    seed = bytes(detbytes("k10-var-seed-%d-%d" % (ei, v), len(seed)))
    return secret, seed, m.prf(secret, label, seed, c["outlen"])


@pytest.mark.parametrize("odd", [True, False], ids=["odd", "aligned"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_prf_matches_every_fixture_entry(torch, tg, n, odd):
    for ei, (kind, c) in enumerate(PRF_ENTRIES):
        label = _entry_inputs(kind, c)[1]
        rows = [_prf_row(ei, r % VARIANTS) for r in range(n)]
        outlen, guard = c["outlen"], 64
        lead = 1 if odd else 0
        secrets = _rows(torch, [r[0] for r in rows], odd=odd)
        seeds = _rows(torch, [r[1] for r in rows], odd=odd) if len(rows[0][1]) else None
        flat = torch.full((guard + lead + n * outlen + guard,), CANARY, dtype=torch.uint8, device="cuda")
        out = flat[guard + lead:guard + lead + n * outlen].view(n, outlen)
        assert out.data_ptr() % 4 == lead
        got = tg.keysetup.tls10_prf(secrets, label, seeds, outlen, out=out)
        torch.cuda.synchronize()
        assert got is out
        host = flat.cpu().numpy()
        want = b"".join(r[2] for r in rows)
        what = (kind, ei, c.get("label"), c.get("secretlen"), c.get("labellen"), c.get("seedlen"), outlen)
        assert host[guard + lead:guard + lead + n * outlen].tobytes() == want, what
        assert (host[:guard + lead] == CANARY).all() and (host[guard + lead + n * outlen:] == CANARY).all(), what


# ---- 2. the key block, both sides ---------------------------------------------
@pytest.mark.parametrize("case", KEYS["pending"], ids=[c["suite"] for c in KEYS["pending"]])
def test_key_block_reproduces_both_sides(torch, tg, case):
    n = len(case["conns"])
    ms, cr, sr = _inputs(torch, [m.pending_inputs(case["suite"], c) for c in range(n)])
    cut = tg.keysetup.tls11_key_block(case["suite_id"], ms, cr, sr)
    torch.cuda.synchronize()
    assert len(cut) == 4
    cmac, smac, ckey, skey = [t.cpu().numpy() for t in cut]
    for c, conn in enumerate(case["conns"]):
        assert ckey[c].tobytes().hex() == conn["client"]["key"] and skey[c].tobytes().hex() == conn["server"]["key"]
        assert cmac[c].tobytes().hex() == conn["client"]["mac_key"]
        assert smac[c].tobytes().hex() == conn["server"]["mac_key"]


# ---- 3. CBC sessions from master secrets: the reference's wire bytes -----------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_cbc_sessions_from_master_secrets(torch, tg, case):
    recs, mac, etm = case["records"], case["mac"], case["etm"]
    n = len(recs)
    ms, cr, sr = _inputs(torch, [tls12_model.cbc_sessions_inputs(case, c) for c in range(5)], odd=True)
    suite = m.SUITE_IDS[case["suite"]]
    send = tg.CbcSessions.from_master_secrets(suite, ms, cr, sr, "client", version=TLS11, etm=etm)
    recv = tg.CbcSessions(send.table, TLS11, etm)
    assert send.version == TLS11 and len(send) == 5
    assert guarded.download(send.seq(), np.uint64).tolist() == [0] * 5
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
        assert r["recv"] == "ok" and opened[i] == (0, r["ctype"], r["len"], d), (i, opened[i][:3])
    # the reference's TLSBadRecordMAC for another session's keys, and for the
    # right session with the neighbour's number: explicit numbers, same wire
    cross = [i for i, r in enumerate(recs) if "cross" in r]
    assert len(cross) >= 3
    for how in ("other_keys", "neighbour_number"):
        b.reset_out()
        session, seq = [r["conn"] for r in recs], [r["seq"] for r in recs]
        for i in cross:
            assert recs[i]["cross"][how] == "TLSBadRecordMAC"
            if how == "other_keys":
                session[i] = recs[i]["cross"]["other_conn"]
            else:
                seq[i] = recs[i]["cross"]["other_seq"]
        b.inputs(session, [r["ctype"] for r in recs], [bytes.fromhex(r["iv"]) for r in recs], seq=seq)
        tg.cbc.open_session_records(send.table, TLS11, etm, b.session, b.n, b.wire, b.w_off, b.w_len, b.out,
                                    b.o_off, b.o_len, b.o_ct, b.st, seq=b.seq)
        torch.cuda.synchronize()
        opened, oh = b.opened()
        for i, (r, d) in enumerate(zip(recs, datas)):
            if i in cross:
                assert opened[i] == (BAD_MAC, r["ctype"], 0, b""), (how, i, opened[i][:3])
                assert _zeros_then_canary(b.room(oh, i)), (how, i)
            else:
                assert opened[i] == (0, r["ctype"], r["len"], d), (how, i, opened[i][:3])
    send.table.close()


# ---- 4. install into a live table ------------------------------------------------
SKIP_ROW = (bytes(detbytes("k10-skip-ms", 48)), bytes(detbytes("k10-skip-cr", 32)), bytes(detbytes("k10-skip-sr", 32)))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_install_in_place(torch, tg, case):
    etm = case["etm"]
    old_enc = [bytes(detbytes("k10-old-enc-%d" % s, 16)) for s in range(NS)]
    old_mac = [bytes(detbytes("k10-old-mac-%d" % s, 20)) for s in range(NS)]
    table = tg.CbcKey.table(old_enc, old_mac, "sha1")
    seq_flat, seq = _guarded(torch, (NS,), torch.int64, 8)
    seq.copy_(torch.arange(100, 100 + NS, dtype=torch.int64, device="cuda"))
    s = tg.CbcSessions(table, TLS11, etm, seq_next=seq, cipher_suite=AES128_SHA)
    p = Probe11(torch, "sha1", etm, range(NS), [1000 + 7 * j for j in range(NS)])
    before = p.host(p.seal(tg, table))
    assert before[5] == p.want(5, old_enc[5], old_mac[5])

    slots = SLOTS + [OUT_OF_RANGE]
    rows = [tls12_model.cbc_sessions_inputs(case, c) for c in range(5)] + [SKIP_ROW]
    flats, views = [], []
    for k, width in enumerate((48, 32, 32)):   # guard bytes around every input
        flat, view = _guarded(torch, (len(rows), width), torch.uint8, 64)
        view.copy_(_rows(torch, [r[k] for r in rows]))
        flats.append((flat, flat.cpu().numpy().copy()))
        views.append(view)
    s.install(slots, views[0], views[1], views[2], "client")
    after = p.host(p.seal(tg, table))
    torch.cuda.synchronize()
    seq_host = guarded.download(seq, np.uint64).tolist()
    # the named rows seal like a host-built table of the fixture's keys
    enc, mk = list(old_enc), list(old_mac)
    for c, slot in enumerate(SLOTS):
        enc[slot], mk[slot] = bytes.fromhex(case["enc_keys"][c]), bytes.fromhex(case["mac_keys"][c])
    host_table = tg.CbcKey.table(enc, mk, "sha1")
    assert after == p.host(p.seal(tg, host_table))
    for slot in range(NS):
        if slot in SLOTS:
            assert after[slot] == p.want(slot, enc[slot], mk[slot]) and after[slot] != before[slot], slot
            assert seq_host[slot] == 0, slot
        else:
            assert after[slot] == before[slot] and seq_host[slot] == 100 + slot, slot
    assert _guards_intact(seq_flat, 8, -0x3839)
    for flat, was in flats:   # inputs and their guards: nothing written
        assert np.array_equal(flat.cpu().numpy(), was)
    # the rebuilt rows decrypt too (dk, the inverse schedule)
    plain = [(0, p.ctypes[i], p.datas[i]) for i in range(NS)]
    t = torch
    wire, w_len = p.seal(tg, host_table)
    out = t.full((192 * NS,), CANARY, dtype=t.uint8, device="cuda")
    o_off = guarded.upload(t, np.arange(NS, dtype=np.uint64) * 192)
    o_len = t.full((NS,), -1, dtype=t.int32, device="cuda")
    o_ct = t.full((NS,), 255, dtype=t.uint8, device="cuda")
    st = t.full((NS,), 255, dtype=t.uint8, device="cuda")
    tg.cbc.open_session_records(table, TLS11, etm, p.session, NS, wire, p.w_off, w_len, out, o_off, o_len, o_ct, st,
                                seq=p.seq)
    oh = out.cpu().numpy()
    got = [(int(a), int(c), oh[192 * i:192 * i + max(int(k), 0)].tobytes())
           for i, (a, c, k) in enumerate(zip(st.cpu().numpy(), o_ct.cpu().numpy(), o_len.cpu().numpy()))]
    assert got == plain

    # the documented argument errors that need a live handle
    ms, cr, sr = _inputs(torch, rows)
    with pytest.raises(tg.TlsGpuError, match="above the key handle's nkeys"):
        big = _inputs(torch, [rows[0]] * (NS + 1))
        s.install(None, big[0], big[1], big[2], "client")
    r = tg.keysetup.tls12_install_args(1, 32, "client", NS + 1, None, ms[:1], cr[:1], sr[:1])
    assert table._lib.tg_cbc_sessions_install_tls11(table.handle, ctypes.byref(r), None) == -22
    assert b"must equal the key handle's nkeys" in table._lib.tg_last_error()
    # n == 0 is fine and changes nothing
    r = tg.keysetup.tls12_install_args(0, 0, "server", NS, None, ms[:0], cr[:0], sr[:0])
    r.master_secrets, r.client_random, r.server_random = ms.data_ptr(), cr.data_ptr(), sr.data_ptr()
    assert table._lib.tg_cbc_sessions_install_tls11(table.handle, ctypes.byref(r), None) == 0
    assert p.host(p.seal(tg, table)) == after
    table.close()
    host_table.close()


# ---- 5. the server's write keys, AES-128 and AES-256 --------------------------------
@pytest.mark.parametrize("name", ["TLS_RSA_WITH_AES_128_CBC_SHA", "TLS_RSA_WITH_AES_256_CBC_SHA"])
def test_server_side(torch, tg, name):
    case = PENDING[name]
    n = len(case["conns"])
    ms, cr, sr = _inputs(torch, [m.pending_inputs(name, c) for c in range(n)], odd=True)
    for side in ("server", "client"):
        keys = [(bytes.fromhex(c[side]["key"]), bytes.fromhex(c[side]["mac_key"])) for c in case["conns"]]
        host_table = tg.CbcKey.table([k[0] for k in keys], [k[1] for k in keys], "sha1")
        for etm in (0, 1):
            s = tg.CbcSessions.from_master_secrets(case["suite_id"], ms, cr, sr, side, version=TLS11, etm=etm)
            p = Probe11(torch, "sha1", etm, [2, 0, 1, 1, 2], [0, 1, 2 ** 32 - 1, 2 ** 32, 5])
            got = p.host(p.seal(tg, s.table))
            assert got == p.host(p.seal(tg, host_table)), (side, etm)
            for i, c in enumerate(p.sessions):
                assert got[i] == p.want(i, *keys[c]), (side, etm, i)
            s.table.close()
        host_table.close()


# ---- 6. stream ordering: batch, install, batch, no sync in between ----------------
def test_install_is_ordered_on_its_stream(torch, tg):
    case = CASES[0]
    enc = [bytes(detbytes("k10-ord-enc-%d" % j, 16)) for j in range(NS)]
    mk = [bytes(detbytes("k10-ord-mac-%d" % j, 20)) for j in range(NS)]
    table = tg.CbcKey.table(enc, mk, "sha1")
    s = tg.CbcSessions(table, TLS11, case["etm"], cipher_suite=AES128_SHA)
    p = Probe11(torch, "sha1", case["etm"], range(NS), [3 * j for j in range(NS)])
    ms, cr, sr = _inputs(torch, [tls12_model.cbc_sessions_inputs(case, c) for c in range(5)])
    slots = guarded.upload(torch, np.array(SLOTS, np.uint32))
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        first = p.seal(tg, table, stream=st)
        s.install(slots, ms, cr, sr, "client", stream=st)
        second = p.seal(tg, table, stream=st)
    st.synchronize()
    first, second = p.host(first), p.host(second)
    for slot in range(NS):
        assert first[slot] == p.want(slot, enc[slot], mk[slot]), slot
        if slot in SLOTS:
            c = SLOTS.index(slot)
            assert second[slot] == p.want(slot, bytes.fromhex(case["enc_keys"][c]),
                                          bytes.fromhex(case["mac_keys"][c])), slot
        else:
            assert second[slot] == first[slot], slot
    table.close()


# ---- 7. refusals ---------------------------------------------------------------------
def test_refusals(torch, tg):
    name = "TLS_RSA_WITH_AES_128_CBC_SHA"
    ms, cr, sr = _inputs(torch, [m.pending_inputs(name, c) for c in range(3)])
    # a SHA-256-MAC suite has no TLS 1.1 form
    with pytest.raises(ValueError, match="0x003c"):
        tg.CbcSessions.from_master_secrets(AES128_SHA256, ms, cr, sr, "client", version=TLS11)
    with pytest.raises(ValueError, match="0x003c"):
        tg.keysetup.tls11_key_block(AES128_SHA256, ms, cr, sr)
    for mac, maclen, keylen in (("sha256", 32, 16), ("sha384", 48, 32)):
        enc = [bytes(detbytes("k10-ref-enc-%s-%d" % (mac, j), keylen)) for j in range(3)]
        mk = [bytes(detbytes("k10-ref-mac-%s-%d" % (mac, j), maclen)) for j in range(3)]
        table = tg.CbcKey.table(enc, mk, mac)
        p = CbcProbe(torch, mac, 0, [0, 1, 2], [0, 1, 2])
        before = p.host(p.seal(tg, table))
        # a TLS 1.1 object of a SHA-256-MAC suite refuses in Python
        with pytest.raises(ValueError, match="0x003c"):
            tg.CbcSessions(table, TLS11, 0, cipher_suite=AES128_SHA256).install(None, ms, cr, sr, "client")
        # the C call refuses the handle whatever the struct says, and says why
        r = tg.keysetup.tls12_install_args(3, 32, "client", 3, None, ms, cr, sr)
        assert table._lib.tg_cbc_sessions_install_tls11(table.handle, ctypes.byref(r), None) == -22
        err = table._lib.tg_last_error()
        assert b"HMAC-SHA1 only" in err and (b"HMAC-%s" % mac.upper().encode()) in err, err
        assert p.host(p.seal(tg, table)) == before
        table.close()
    # a TLS 1.1 object without a suite still cannot install
    table = tg.CbcKey.table([bytes(16)], [bytes(20)], "sha1")
    with pytest.raises(ValueError):
        tg.CbcSessions(table, TLS11, 0).install(None, ms[:1], cr[:1], sr[:1], "client")
    table.close()

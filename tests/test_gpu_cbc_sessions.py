"""GPU: AES-CBC + HMAC records of many sessions in one batch
(tg_cbc_seal_session_records / tg_cbc_open_session_records, key tables,
tg_cbc_key_replace, tlsgpu.CbcSessions) against the reference RecordLayer's
many-connection fixtures (tests/golden/cbc_sessions.json), the CPU model
(tests/cbc_model.py, held against the same fixtures by
test_cbc_sessions_oracle.py) and the single-connection calls.

Every buffer is canary-filled with the extents placed by tests/guarded.py, and
the gaps are checked after every call.  Malformed records are malformed in
content only; the offsets of a SKIPPED record (session out of range) may point
anywhere, and one test makes them do so."""
import ctypes
import json
import os

import numpy as np
import pytest

import cbc_model
import guarded
from conftest import ROOT
from test_cbc_sessions_oracle import record_data, wire_matches
from vectors import detbytes

pytestmark = pytest.mark.gpu

CASES = json.load(open(os.path.join(ROOT, "tests", "golden", "cbc_sessions.json")))
IDS = ["%s-%d.%d-%s" % (c["suite"], c["version"][0], c["version"][1], "etm" if c["etm"] else "mte")
       for c in CASES]
CANARY_D, CANARY_W, CANARY_O = guarded.CANARY_IN, guarded.CANARY_SEALED, guarded.CANARY_BACK
BAD_MAC, BAD_SESSION = 1, 8
CTYPES = (23, 22, 21)


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


def _leads(aligned, n):
    """Address residues of (fragment, wire, plaintext out) extents: all on the
    vector path (wire + 5 at 0 mod 16), or running through the residues."""
    i = np.arange(n)
    if aligned:
        return np.zeros(n, np.int64), np.full(n, 11, np.int64), np.zeros(n, np.int64)
    return (7 * i + 3) % 16, (5 * i + 4) % 16, (3 * i + 1) % 16


class SBatch(object):
    """Device buffers of one many-session batch: fragments in, wire, fragments
    out, in canary-guarded layouts."""

    def __init__(self, torch, mac, etm, datas, aligned=True):
        self.torch, self.n, self.datas = torch, len(datas), datas
        n = self.n
        self.lens = [len(x) for x in datas]
        self.wlens = [cbc_model.wire_len(mac, etm, k) for k in self.lens]
        self.rooms = [w - 21 for w in self.wlens]
        dl, wl, ol = _leads(aligned, n)
        self.data_off, dsz = guarded._place(self.lens, dl, 48, 256)
        self.wire_off, wsz = guarded._place(self.wlens, wl, 48, 256)
        self.out_off, osz = guarded._place(self.rooms, ol, 48, 256)
        self.data_host = np.full(dsz, CANARY_D, np.uint8)
        for o, x in zip(self.data_off, datas):
            self.data_host[int(o):int(o) + len(x)] = np.frombuffer(bytes(x), np.uint8)
        self.up = lambda a: guarded.upload(torch, a)
        self.data = self.up(self.data_host)
        self.d_off, self.w_off, self.o_off = self.up(self.data_off), self.up(self.wire_off), self.up(self.out_off)
        self.d_len = self.up(np.array(self.lens, np.uint32))
        self.wire = torch.full((wsz,), CANARY_W, dtype=torch.uint8, device="cuda")
        self.w_len = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        self.reset_out(osz)

    def reset_out(self, osz=None):
        t = self.torch
        self.out = t.full((osz or self.out.numel(),), CANARY_O, dtype=t.uint8, device="cuda")
        self.o_len = t.full((self.n,), -1, dtype=t.int32, device="cuda")
        self.o_ct = t.full((self.n,), 255, dtype=t.uint8, device="cuda")
        self.st = t.full((self.n,), 255, dtype=t.uint8, device="cuda")

    def inputs(self, session, ctypes_, ivs, seq=None):
        self.session_host = np.array(session, np.uint32)
        self.session = self.up(self.session_host)
        self.ctype = self.up(np.array(ctypes_, np.uint8))
        self.iv_host = np.frombuffer(b"".join(ivs), np.uint8).copy()
        self.iv = self.up(self.iv_host)
        self.seq_host = None if seq is None else np.array(seq, np.uint64)
        self.seq = None if seq is None else self.up(self.seq_host)

    def wires(self):
        wh, wl = self.wire.cpu().numpy(), self.w_len.cpu().numpy()
        return [wh[int(o):int(o) + max(int(k), 0)].tobytes() for o, k in zip(self.wire_off, wl)], wh, wl

    def set_wires(self, wires):
        """Replace the wire records (same extents or shorter) for an open."""
        wh = np.full(self.wire.numel(), CANARY_W, np.uint8)
        for o, w, room in zip(self.wire_off, wires, self.wlens):
            assert len(w) <= room
            wh[int(o):int(o) + len(w)] = np.frombuffer(w, np.uint8)
        self.wire = self.up(wh)
        self.w_len = self.up(np.array([len(w) for w in wires], np.uint32))

    def opened(self):
        oh = self.out.cpu().numpy()
        res = [(int(s), int(c), int(k), oh[int(o):int(o) + max(int(k), 0)].tobytes()) for s, c, k, o in
               zip(self.st.cpu().numpy(), self.o_ct.cpu().numpy(), self.o_len.cpu().numpy(), self.out_off)]
        return res, oh

    def room(self, oh, i):
        return oh[int(self.out_off[i]):int(self.out_off[i]) + self.rooms[i]]

    def check_gaps(self, what, buf, offs, sizes, canary, untouched=()):
        """Every byte outside the extents -- and every byte of the extents of
        the records in ``untouched`` -- is still canary."""
        mask = np.ones(len(buf), bool)
        for i, (o, s) in enumerate(zip(offs, sizes)):
            if i not in untouched:
                mask[int(o):int(o) + int(s)] = False
        bad = np.flatnonzero(buf[mask] != canary)
        if len(bad):
            pos = int(np.flatnonzero(mask)[bad[0]])
            i = int(np.argmin([min(abs(pos - int(o)), abs(pos - int(o) - int(s))) for o, s in zip(offs, sizes)]))
            raise guarded.ContainmentError(what, record=i, rel=pos - int(offs[i]), extent=int(sizes[i]),
                                           expected=canary, got=buf[pos], offset=pos)

    def check_inputs_unchanged(self):
        assert np.array_equal(self.data.cpu().numpy(), self.data_host)
        assert np.array_equal(self.iv.cpu().numpy(), self.iv_host)
        assert np.array_equal(guarded.download(self.session, np.uint32), self.session_host)
        assert np.array_equal(guarded.download(self.d_off, np.uint64), self.data_off)
        assert np.array_equal(guarded.download(self.w_off, np.uint64), self.wire_off)
        if self.seq is not None:
            assert np.array_equal(guarded.download(self.seq, np.uint64), self.seq_host)


def _seal(tg, key, version, etm, b, seq_next=None, seq_out=None, stream=None):
    tg.cbc.seal_session_records(key, version, etm, b.session, b.n, b.data, b.d_off, b.d_len, b.ctype, b.iv,
                                b.wire, b.w_off, b.w_len, seq=b.seq, seq_next=seq_next, seq_out=seq_out,
                                stream=stream)


def _open(tg, key, version, etm, b, seq_next=None, seq_out=None, stream=None):
    tg.cbc.open_session_records(key, version, etm, b.session, b.n, b.wire, b.w_off, b.w_len, b.out, b.o_off,
                                b.o_len, b.o_ct, b.st, seq=b.seq, seq_next=seq_next, seq_out=seq_out,
                                stream=stream)


def _zeros_then_canary(room):
    """A rejected record's extent: a zeroed prefix, then bytes nobody wrote."""
    k = int(np.count_nonzero(room == 0)) if len(room) and room[0] == 0 else 0
    return bool((room[:k] == 0).all() and (room[k:] == CANARY_O).all())


def _i64(torch, values):
    return guarded.upload(torch, np.array(values, np.uint64)).view(torch.int64)


# ---- fixture replay ----------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "odd"])
def test_fixture_replay(torch, tg, case, aligned):
    recs, mac, etm = case["records"], case["mac"], case["etm"]
    version = case["version"][0] << 8 | case["version"][1]
    n = len(recs)
    table = tg.CbcKey.table([bytes.fromhex(k) for k in case["enc_keys"]],
                            [bytes.fromhex(k) for k in case["mac_keys"]], mac)
    assert table.nkeys == 5
    datas = [record_data(i, r) for i, r in enumerate(recs)]
    b = SBatch(torch, mac, etm, datas, aligned)
    b.inputs([r["conn"] for r in recs], [r["ctype"] for r in recs], [bytes.fromhex(r["iv"]) for r in recs])
    counts = [sum(1 for r in recs if r["conn"] == c) for c in range(5)]
    want_next = [s + k for s, k in zip(case["starts"], counts)]

    send = tg.CbcSessions(table, version, etm, seq_next=_i64(torch, case["starts"]))
    recv = tg.CbcSessions(table, version, etm, seq_next=_i64(torch, case["starts"]))
    seq_out = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    send.seal(b.session, n, b.data, b.d_off, b.d_len, b.ctype, b.iv, b.wire, b.w_off, b.w_len, seq_out=seq_out)
    recv.open(b.session, n, b.wire, b.w_off, b.w_len, b.out, b.o_off, b.o_len, b.o_ct, b.st)
    torch.cuda.synchronize()
    assert guarded.download(send.seq(), np.uint64).tolist() == want_next
    assert guarded.download(recv.seq(), np.uint64).tolist() == want_next
    assert guarded.download(seq_out, np.uint64).tolist() == [r["seq"] for r in recs]
    wires, wh, _ = b.wires()
    for i, (r, w) in enumerate(zip(recs, wires)):
        assert wire_matches(r, w), (i, r["conn"], r["len"])
    opened, oh = b.opened()
    for i, (r, d) in enumerate(zip(recs, datas)):
        assert r["recv"] == "ok" and opened[i] == (0, r["ctype"], r["len"], d), (i, opened[i][:3])
    b.check_gaps("wire after seal", wh, b.wire_off, b.wlens, CANARY_W)
    b.check_gaps("data after open", oh, b.out_off, b.rooms, CANARY_O)
    b.check_inputs_unchanged()

    # the reference's TLSBadRecordMAC for another session's keys, and for the
    # right session with the neighbour's number: explicit numbers, same wire
    cross = [i for i, r in enumerate(recs) if "cross" in r]
    for how in ("other_keys", "neighbour_number"):
        b.reset_out()
        session = [r["conn"] for r in recs]
        seq = [r["seq"] for r in recs]
        for i in cross:
            assert recs[i]["cross"][how] == "TLSBadRecordMAC"
            if how == "other_keys":
                session[i] = recs[i]["cross"]["other_conn"]
            else:
                seq[i] = recs[i]["cross"]["other_seq"]
        b.inputs(session, [r["ctype"] for r in recs], [bytes.fromhex(r["iv"]) for r in recs], seq=seq)
        _open(tg, table, version, etm, b)
        torch.cuda.synchronize()
        opened, oh = b.opened()
        for i, (r, d) in enumerate(zip(recs, datas)):
            if i in cross:
                assert opened[i] == (BAD_MAC, r["ctype"], 0, b""), (how, i, opened[i][:3])
                assert _zeros_then_canary(b.room(oh, i)), (how, i)
            else:
                assert opened[i] == (0, r["ctype"], r["len"], d), (how, i, opened[i][:3])
        b.check_gaps("data after open", oh, b.out_off, b.rooms, CANARY_O)
    table.close()


# ---- keys differ inside a wave ----------------------------------------------
NMAX = 257
CONFIGS = [(keylen, mac, etm) for keylen in (16, 32) for mac in ("sha1", "sha256", "sha384") for etm in (0, 1)]
CFG_IDS = ["aes%d-%s-%s" % (c[0] * 8, c[1], "etm" if c[2] else "mte") for c in CONFIGS]
BOUNDARY = [0, 1, 11, 12, 15, 16, 42, 43, 50, 51, 98, 99, 114, 115]   # make_golden_cbc.seal_lengths, both constructions
SEQS = [2 ** 32 - 3 + 5 * i if i % 2 else (2 ** 40 + 3) * (i + 1) for i in range(NMAX)]   # low-word carries, high words
PLANT_LANES = (0, 31, 32, 63)
_wire_cache = {}


def _pool_key(keylen, mac, s):
    return bytes(detbytes("ks-ek-%d" % s, keylen)), bytes(detbytes("ks-mk-%s-%d" % (mac, s), cbc_model.DIGEST[mac]))


def _record_inputs(i):
    n = BOUNDARY[(5 * i + i // 14) % len(BOUNDARY)]
    return bytes(detbytes("ks-%d" % i, n)), bytes(detbytes("ks-iv-%d" % i, 16)), CTYPES[i % 3]


def _model_wire(cfg, i, s):
    """The model's wire record i under pool key s, computed once."""
    if (cfg, i, s) not in _wire_cache:
        keylen, mac, etm = cfg
        ek, mk = _pool_key(keylen, mac, s)
        data, iv, ct = _record_inputs(i)
        _wire_cache[(cfg, i, s)] = cbc_model.seal_record(ek, mk, mac, 0x0303, etm, SEQS[i], ct, data, iv)
    return _wire_cache[(cfg, i, s)]


def _plants(n):
    """{record: kind}: in wave w, the j-th of lanes 0, 31, 32, 63 gets kind
    (j + w) mod 3, so over three waves every kind sits at every one of them."""
    out = {}
    for w in range((n + 63) // 64):
        for j, lane in enumerate(PLANT_LANES):
            if 64 * w + lane < n:
                out[64 * w + lane] = ("tampered", "truncated", "bad_session")[(j + w) % 3]
    return out


@pytest.mark.parametrize("cfg", CONFIGS, ids=CFG_IDS)
@pytest.mark.parametrize("nsessions", [1, 3, 64, 257])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_keys_differ_inside_a_wave(torch, tg, cfg, nsessions, n):
    keylen, mac, etm = cfg
    pool = [_pool_key(keylen, mac, s) for s in range(nsessions)]
    table = tg.CbcKey.table([k[0] for k in pool], [k[1] for k in pool], mac)
    assert table.nkeys == nsessions
    ins = [_record_inputs(i) for i in range(n)]
    plants = _plants(n)
    session = [i % nsessions for i in range(n)]
    for j, i in enumerate(sorted(i for i, kind in plants.items() if kind == "bad_session")):
        session[i] = nsessions if j % 2 == 0 else 0xffffffff
    b = SBatch(torch, mac, etm, [x[0] for x in ins], aligned=(n % 2 == 0))
    b.inputs(session, [x[2] for x in ins], [x[1] for x in ins], seq=SEQS[:n])
    seq_out = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    _seal(tg, table, tg.TLS12, etm, b, seq_out=seq_out)
    torch.cuda.synchronize()
    wires, wh, wl = b.wires()
    skipped = set(i for i, kind in plants.items() if kind == "bad_session")
    so = guarded.download(seq_out, np.uint64)
    for i in range(n):
        if i in skipped:
            assert wl[i] == 0 and so[i] == 2 ** 64 - 1, i
        else:
            assert wires[i] == _model_wire(cfg, i, i % nsessions), (i, len(ins[i][0]))
            assert so[i] == SEQS[i], i
    b.check_gaps("wire after seal", wh, b.wire_off, b.wlens, CANARY_W, untouched=skipped)

    want = {}
    for i, kind in plants.items():
        if kind == "tampered":
            w = bytearray(wires[i])
            w[21 + (len(w) - 22) // 2] ^= 0x20
            wires[i] = bytes(w)
            verdict, ct, plain = cbc_model.open_record(*pool[i % nsessions], mac, tg.TLS12, etm, SEQS[i], wires[i])
            assert verdict == "TLSBadRecordMAC"
            want[i] = (BAD_MAC, ct, 0, b"")
        elif kind == "truncated":
            wires[i] = wires[i][:3]
            want[i] = (BAD_MAC, 0, 0, b"")
        else:
            wires[i] = _model_wire(cfg, i, 0)           # a good record under key 0: the session is what is wrong
            want[i] = (BAD_SESSION, 0, 0, b"")
    b.set_wires(wires)
    _open(tg, table, tg.TLS12, etm, b)
    torch.cuda.synchronize()
    opened, oh = b.opened()
    for i in range(n):
        assert opened[i] == want.get(i, (0, ins[i][2], len(ins[i][0]), ins[i][0])), (i, plants.get(i), opened[i][:3])
        if plants.get(i) == "tampered":
            assert _zeros_then_canary(b.room(oh, i)), i
    nothing = set(i for i, kind in plants.items() if kind != "tampered")
    b.check_gaps("data after open", oh, b.out_off, b.rooms, CANARY_O, untouched=nothing)
    b.check_inputs_unchanged()
    table.close()


# ---- same bytes as the single-connection path ---------------------------------
@pytest.mark.parametrize("cfg", CONFIGS, ids=CFG_IDS)
def test_one_session_equals_the_single_connection_call(torch, tg, cfg):
    keylen, mac, etm = cfg
    n, s, start = 70, 2, 2 ** 32 - 5
    pool = [_pool_key(keylen, mac, k) for k in range(3)]
    table = tg.CbcKey.table([k[0] for k in pool], [k[1] for k in pool], mac)
    ins = [_record_inputs(i) for i in range(n)]
    datas = [x[0] for x in ins]
    datas[7] = bytes(detbytes("same-big", 16384))
    out = {}
    for path in ("table", "single", "table handle in the single call"):
        b = SBatch(torch, mac, etm, datas, aligned=False)
        b.inputs([s] * n, [x[2] for x in ins], [x[1] for x in ins])
        if path == "table":
            ses = tg.CbcSessions(table, tg.TLS12, etm, seq_next=_i64(torch, [9, 9, start]))
            ses.seal(b.session, n, b.data, b.d_off, b.d_len, b.ctype, b.iv, b.wire, b.w_off, b.w_len)
        else:
            key = tg.CbcKey(*pool[s if path == "single" else 0], mac) if path == "single" else table
            tg.cbc.seal_records(key, tg.TLS12, etm, start, n, b.data, b.d_off, b.d_len, b.ctype, b.iv, b.wire,
                                b.w_off, b.w_len)
        torch.cuda.synchronize()
        wires, wh, wl = b.wires()
        w = bytearray(wires[3])                      # one refused record: its outputs must agree too
        w[30] ^= 1
        wires[3] = bytes(w)
        b.set_wires(wires)
        if path == "table":
            ses.seq_next[s] = start
            ses.open(b.session, n, b.wire, b.w_off, b.w_len, b.out, b.o_off, b.o_len, b.o_ct, b.st)
            assert guarded.download(ses.seq(), np.uint64).tolist() == [9, 9, start + n]
        else:
            tg.cbc.open_records(key, tg.TLS12, etm, start, n, b.out, b.o_off, b.o_len, b.o_ct, b.st, b.wire,
                                b.w_off, b.w_len)
            if path == "single":
                key.close()
        torch.cuda.synchronize()
        out[path] = (wh, wl.tolist(), b.out.cpu().numpy(), b.st.cpu().numpy().tolist(),
                     b.o_len.cpu().numpy().tolist(), b.o_ct.cpu().numpy().tolist())
    for k in range(6):
        assert np.array_equal(out["table"][k], out["single"][k]), k
    assert out["single"][3][3] == BAD_MAC and set(out["single"][3]) == {0, BAD_MAC}
    # entry 0 is what the single-connection call reads from a table handle
    want0 = cbc_model.seal_record(*pool[0], mac, tg.TLS12, etm, start + 1, ins[1][2], datas[1], ins[1][1])
    o = int(b.wire_off[1])
    assert out["table handle in the single call"][0][o:o + len(want0)].tobytes() == want0
    assert not np.array_equal(out["table handle in the single call"][0], out["single"][0])
    table.close()


# ---- containment ---------------------------------------------------------------
@pytest.mark.parametrize("cfg", [CONFIGS[0], CONFIGS[3], CONFIGS[8], CONFIGS[11]],
                         ids=[CFG_IDS[k] for k in (0, 3, 8, 11)])
def test_skipped_records_touch_nothing_and_may_point_anywhere(torch, tg, cfg):
    keylen, mac, etm = cfg
    n, nsessions = 130, 5
    pool = [_pool_key(keylen, mac, s) for s in range(nsessions)]
    table = tg.CbcKey.table([k[0] for k in pool], [k[1] for k in pool], mac)
    ins = [_record_inputs(i) for i in range(n)]
    datas = [x[0] for x in ins]
    datas[66] = bytes(detbytes("cont-big", 16384))
    skipped = set(range(0, n, 9)) | {63, 64, 129}
    session = [(nsessions + i) if i in skipped else i % nsessions for i in range(n)]
    b = SBatch(torch, mac, etm, datas, aligned=False)
    b.inputs(session, [x[2] for x in ins], [x[1] for x in ins], seq=SEQS[:n])
    # a skipped record's offsets are never used: point them far outside the buffers
    wild = np.array([2 ** 60 + 12345 * i for i in range(n)], np.uint64)
    keep_d, keep_w, keep_o = b.data_off.copy(), b.wire_off.copy(), b.out_off.copy()
    for i in skipped:
        b.data_off[i], b.wire_off[i], b.out_off[i] = wild[i], wild[i] + 7, wild[i] + 3
    b.d_off, b.w_off, b.o_off = b.up(b.data_off), b.up(b.wire_off), b.up(b.out_off)
    _seal(tg, table, tg.TLS12, etm, b)
    torch.cuda.synchronize()
    wires, wh, wl = b.wires()
    for i in range(n):
        if i in skipped:
            assert wl[i] == 0, i
        else:
            assert wires[i] == cbc_model.seal_record(*pool[i % nsessions], mac, tg.TLS12, etm, SEQS[i], ins[i][2],
                                                     datas[i], ins[i][1]), i
    # whole-buffer image: the model's records in canary, the skipped extents still canary
    b.check_gaps("wire after seal", wh, keep_w, b.wlens, CANARY_W, untouched=skipped)
    # give the skipped records' wire_len a value again: open must not look at it either
    wl2 = wl.copy().astype(np.uint32)
    for i in skipped:
        wl2[i] = 200
    b.w_len = b.up(wl2)
    _open(tg, table, tg.TLS12, etm, b)
    torch.cuda.synchronize()
    st, ln, ct = b.st.cpu().numpy(), b.o_len.cpu().numpy(), b.o_ct.cpu().numpy()
    oh = b.out.cpu().numpy()
    for i in range(n):
        if i in skipped:
            assert (st[i], ln[i], ct[i]) == (BAD_SESSION, 0, 0), i
        else:
            assert (st[i], ln[i], ct[i]) == (0, len(datas[i]), ins[i][2]), i
            assert oh[int(keep_o[i]):int(keep_o[i]) + len(datas[i])].tobytes() == datas[i], i
    b.check_gaps("data after open", oh, keep_o, b.rooms, CANARY_O, untouched=skipped)
    assert np.array_equal(b.wire.cpu().numpy(), wh)                      # open only reads the wire
    assert np.array_equal(b.data.cpu().numpy(), b.data_host)
    assert np.array_equal(b.iv.cpu().numpy(), b.iv_host)
    assert np.array_equal(guarded.download(b.seq, np.uint64), b.seq_host)
    assert np.array_equal(guarded.download(b.session, np.uint32), b.session_host)
    table.close()


# ---- counters --------------------------------------------------------------------
def test_counters_follow_the_stable_rank_across_two_batches(torch, tg):
    mac, etm, nsessions, n = "sha1", 0, 7, 1000
    rng = np.random.default_rng(3)
    session = np.concatenate([np.full(600, 4), rng.integers(0, nsessions, n - 600)]).astype(np.uint32)
    session = session[rng.permutation(n)]
    starts = np.array([0, 1, 2 ** 32 - 2, 2 ** 40 + 3, 2 ** 32 - 300, 255, 7], np.uint64)
    pool = [_pool_key(16, mac, s) for s in range(nsessions)]
    table = tg.CbcKey.table([k[0] for k in pool], [k[1] for k in pool], mac)
    datas = [bytes(detbytes("cnt-%d" % i, i % 23)) for i in range(n)]
    ivs = [bytes(detbytes("cnt-iv-%d" % i, 16)) for i in range(n)]
    ses = tg.CbcSessions(table, tg.TLS12, etm, seq_next=_i64(torch, starts))
    seq_out = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    s = torch.cuda.Stream()
    halves = []
    torch.cuda.synchronize()
    for a, z in ((0, n // 2), (n // 2, n)):
        b = SBatch(torch, mac, etm, datas[a:z])
        b.inputs(session[a:z], [23] * (z - a), ivs[a:z])
        halves.append(b)
    torch.cuda.synchronize()
    for b, (a, z) in zip(halves, ((0, n // 2), (n // 2, n))):
        ses.seal(b.session, b.n, b.data, b.d_off, b.d_len, b.ctype, b.iv, b.wire, b.w_off, b.w_len,
                 seq_out=seq_out[a:z], stream=s)
    s.synchronize()
    # numpy's stable rank: position among the records of the same session, in batch order
    order = np.argsort(session, kind="stable")
    rank = np.empty(n, np.uint64)
    first = {}
    for pos, i in enumerate(order):
        first.setdefault(session[i], pos)
        rank[i] = pos - first[session[i]]
    want = starts[session] + rank
    assert np.array_equal(guarded.download(seq_out, np.uint64), want)
    assert np.array_equal(guarded.download(ses.seq(), np.uint64), starts + np.bincount(session, minlength=nsessions)
                          .astype(np.uint64))
    for b, a in zip(halves, (0, n // 2)):
        wires, _, _ = b.wires()
        for i in (0, 1, b.n - 1):
            k = a + i
            assert wires[i] == cbc_model.seal_record(*pool[session[k]], mac, tg.TLS12, etm, int(want[k]), 23,
                                                     datas[k], ivs[k]), k
    table.close()


def test_argument_errors_that_need_a_live_handle(torch, tg):
    from tlsgpu import _lib
    pool = [_pool_key(16, "sha1", s) for s in range(3)]
    table = tg.CbcKey.table([k[0] for k in pool], [k[1] for k in pool], "sha1")
    b = SBatch(torch, "sha1", 0, [b"abc", b"defg"])
    b.inputs([0, 1], [23, 23], [bytes(16), bytes(16)], seq=[1, 2])
    counters = torch.zeros(3, dtype=torch.int64, device="cuda")
    for fn in (_seal, _open):
        with pytest.raises(tg.TlsGpuError) as e:            # both
            fn(tg, table, tg.TLS12, 0, b, seq_next=counters)
        assert e.value.code == _lib.TG_EINVAL and "both" in str(e.value)
    b.seq = None
    for fn in (_seal, _open):
        with pytest.raises(tg.TlsGpuError) as e:            # neither
            fn(tg, table, tg.TLS12, 0, b)
        assert e.value.code == _lib.TG_EINVAL and "neither" in str(e.value)
    lib = _lib.load()
    r = tg.cbc._session_records(table, 2, tg.TLS12, 0, b.session, None, counters, None, b.data, b.d_off, b.d_len,
                                b.ctype, b.wire, b.w_off, b.w_len, iv=b.iv, status=b.st)
    for nsessions in (2, 4):
        r.nsessions = nsessions
        for fn in (lib.tg_cbc_seal_session_records, lib.tg_cbc_open_session_records):
            assert fn(table.handle, ctypes.byref(r), None) == _lib.TG_EINVAL
            assert b"nsessions" in lib.tg_last_error()
    assert lib.tg_cbc_key_replace(table.handle, None, bytes(64), bytes(80), 20, 4, None) == _lib.TG_EINVAL
    assert b"4 rows for a table of 3 keys" in lib.tg_last_error()
    torch.cuda.synchronize()
    assert guarded.download(counters, np.uint64).tolist() == [0, 0, 0]
    assert (b.wire.cpu().numpy() == CANARY_W).all()
    # n == 0 launches nothing, in either mode
    tg.cbc.seal_session_records(table, tg.TLS12, 0, None, 0, None, None, None, None, 0x1000, None, None, None,
                                seq_next=counters)
    tg.cbc.open_session_records(table, tg.TLS12, 0, None, 0, None, None, None, None, None, None, None, None,
                                seq=0x1000)
    table.close()


# ---- replace ----------------------------------------------------------------------
def test_replace_is_ordered_on_the_stream(torch, tg):
    mac, etm, nsessions, n = "sha256", 1, 4, 66
    old = [_pool_key(32, mac, s) for s in range(nsessions)]
    new = [_pool_key(32, mac, 100 + s) for s in range(3)]
    table = tg.CbcKey.table([k[0] for k in old], [k[1] for k in old], mac)
    ses = tg.CbcSessions(table, tg.TLS12, etm, seq_next=_i64(torch, [5, 6, 7, 8]))
    ins = [_record_inputs(i) for i in range(n)]
    session = [i % nsessions for i in range(n)]
    batches = []
    for _ in range(2):
        b = SBatch(torch, mac, etm, [x[0] for x in ins])
        b.inputs(session, [x[2] for x in ins], [x[1] for x in ins], seq=SEQS[:n])
        batches.append(b)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    # one stream, no host synchronisation of the device in between
    _seal(tg, table, tg.TLS12, etm, batches[0], stream=s)
    ses.replace([1, 9, 3], [k[0] for k in new], [k[1] for k in new], stream=s)     # slot 9: out of range, skipped
    _seal(tg, table, tg.TLS12, etm, batches[1], stream=s)
    s.synchronize()
    now = [old[0], new[0], old[2], new[2]]
    for b, keys in zip(batches, (old, now)):
        wires, wh, _ = b.wires()
        for i in range(n):
            assert wires[i] == cbc_model.seal_record(*keys[i % nsessions], mac, tg.TLS12, etm, SEQS[i], ins[i][2],
                                                     ins[i][0], ins[i][1]), i
        b.check_gaps("wire after seal", wh, b.wire_off, b.wlens, CANARY_W)
    assert guarded.download(ses.seq(), np.uint64).tolist() == [5, 0, 7, 0]
    # slots=None: the first rows, in order
    table.replace(None, [old[1][0]], [old[1][1]], stream=s)
    b = batches[0]
    _seal(tg, table, tg.TLS12, etm, b, stream=s)
    s.synchronize()
    assert b.wires()[0][0] == cbc_model.seal_record(*old[1], mac, tg.TLS12, etm, SEQS[0], ins[0][2], ins[0][0],
                                                    ins[0][1])
    table.close()


# ---- housekeeping --------------------------------------------------------------------
def test_seal_then_open_on_one_stream_without_host_sync(torch, tg):
    mac, etm, nsessions, n = "sha384", 0, 3, 65
    pool = [_pool_key(16, mac, s) for s in range(nsessions)]
    table = tg.CbcKey.table([k[0] for k in pool], [k[1] for k in pool], mac)
    ins = [_record_inputs(i) for i in range(n)]
    b = SBatch(torch, mac, etm, [x[0] for x in ins])
    b.inputs([i % nsessions for i in range(n)], [x[2] for x in ins], [x[1] for x in ins])
    send = tg.CbcSessions(table, tg.TLS11, etm, seq_next=_i64(torch, [2 ** 32 - 1, 0, 77]))
    recv = tg.CbcSessions(table, tg.TLS11, etm, seq_next=_i64(torch, [2 ** 32 - 1, 0, 77]))
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    send.seal(b.session, n, b.data, b.d_off, b.d_len, b.ctype, b.iv, b.wire, b.w_off, b.w_len, stream=s)
    recv.open(b.session, n, b.wire, b.w_off, b.w_len, b.out, b.o_off, b.o_len, b.o_ct, b.st, stream=s)
    s.synchronize()
    opened, _ = b.opened()
    for i in range(n):
        assert opened[i] == (0, ins[i][2], len(ins[i][0]), ins[i][0]), (i, opened[i][:3])
    assert guarded.download(send.seq(), np.uint64).tolist() == guarded.download(recv.seq(), np.uint64).tolist() \
        == [2 ** 32 - 1 + 22, 22, 77 + 21]
    table.close()


def test_table_lifecycle_leaves_scratch_flat(torch, tg):
    mac, etm, nsessions, n = "sha1", 1, 3, 8
    pool = [_pool_key(16, mac, s) for s in range(nsessions)]
    ins = [_record_inputs(i) for i in range(n)]
    before = None
    for round_ in range(4):
        table = tg.CbcKey.table([k[0] for k in pool], [k[1] for k in pool], mac)
        ses = tg.CbcSessions(table, tg.TLS12, etm)
        b = SBatch(torch, mac, etm, [x[0] for x in ins])
        b.inputs([i % nsessions for i in range(n)], [x[2] for x in ins], [x[1] for x in ins])
        ses.seal(b.session, n, b.data, b.d_off, b.d_len, b.ctype, b.iv, b.wire, b.w_off, b.w_len)   # rank scratch
        table.replace([0], [pool[0][0]], [pool[0][1]])
        table.close()                                     # waits for the device, scrubs, frees
        assert table.handle is None
        wires, _, _ = b.wires()
        assert wires[4] == cbc_model.seal_record(*pool[1], mac, tg.TLS12, etm, 1, ins[4][2], ins[4][0], ins[4][1])
        if round_ == 0:
            before = tg.scratch_info()                    # the first counter-mode call sized the cache
    assert tg.scratch_info() == before
    with pytest.raises(TypeError):
        tg.cbc.seal_session_records(table, tg.TLS12, 1, None, 0, None, None, None, None, None, None, None, None)

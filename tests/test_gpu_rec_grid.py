"""GPU: tg_open_records / tg_open_session_records over the verdict grid of
tests/rec_grid.py -- the length and header checks, the tag, the TLS 1.3
de-padding scan and the plaintext limits, class by class and where two faults
coincide -- against the verdicts of the reference's RecordLayer
(tests/golden/rec_grid.json; test_rec_grid_oracle.py proves that the wires
built here are the bytes the reference judged).

A whole grid is opened in one call.  Buffers are canary-filled, extents lie
between 48-byte gaps behind 256-byte guards, address residues change per
record and every fourth record is on the vector path (payload and data
16-byte aligned).  ``status``, ``ctype``, ``data_len`` and the data buffer are
compared whole: an accepted record leaves its inner plaintext, a record
refused after decryption too (NO_CONTENT_TYPE, OVERFLOW by the plaintext), a
BAD_MAC record zeros, a record refused before decryption the canary.

Malformed records are malformed in content only: every offset and length
stays inside its buffer."""
import json
import os

import numpy as np
import pytest

import cbc_grid
import rec_grid as G
from conftest import ROOT
from oracle import records as R

pytestmark = pytest.mark.gpu

GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "rec_grid.json")))
CANARY_W, CANARY_O, CANARY_D = 0x5A, 0xC3, 0xA5
FILL_LEN, FILL8, SLACK = 0x6E6E6E6E, 0xEE, 16
SENTINEL = -0x0123456789abcdef

# Where the reference's answer is outside an AEAD engine's remit (include/tlsgpu.h: unprotected
# TLS 1.3 records are taken out by the caller before batching): the reference passes these through
# undecrypted and gives them no sequence number; the device refuses them by its order of checks.
OUTSIDE_REMIT = {"2-byte alert as record 0": G.TRUNCATED,
                 "ChangeCipherSpec, 1 byte": G.TRUNCATED,
                 "ChangeCipherSpec over an encrypted body": G.BAD_TYPE}
RUNTS = (0, 1, 2, 3, 4)     # wire lengths that are not even a header: no golden verdict, the ABI's own


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


def _single_key(tg, alg, key):
    if alg.startswith("chacha"):
        return tg.HipCHACHA20_POLY1305(bytearray(key))
    if "ccm" in alg:
        return tg.HipAESCCM(bytearray(key), tag_length=8 if alg.endswith("_8") else 16)
    return tg.HipAESGCM(bytearray(key))


def _table_alg(alg):
    return "chacha20-poly1305" if alg.startswith("chacha") else "aesgcm"


def _dev(torch, a):
    a = np.ascontiguousarray(a)
    signed = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(a.dtype, a.dtype)
    return torch.from_numpy(a.view(signed).copy()).cuda()


def _residues(n, seed, hdr):
    """Per-record residues of the wire and data offsets; every fourth record
    has its payload and its data extent 16-byte aligned."""
    forced = (-hdr % 16, 0)
    res = cbc_grid.residues(n, seed, forced)
    vector = (res[0] == forced[0]) & (res[1] == 0)
    assert vector[::4].all() and not vector.all()
    return res


def _first_diff(got, want, offs, sizes):
    ne = got != want
    if not ne.any():
        return None
    p = int(np.flatnonzero(ne)[0])
    offs, sizes = np.asarray(offs), np.asarray(sizes)
    dist = np.where(p < offs, offs - p, np.where(p >= offs + sizes, p - offs - sizes + 1, 0))
    i = int(np.argmin(dist))
    return i, p - int(offs[i]), "want 0x%02x" % want[p], "got 0x%02x" % got[p]


def _open_and_check(torch, cfg, built, want, seed, call):
    """Open the grid (and the runt wires behind it) with ``call(n, arrays)``
    and compare every array whole.  ``want``: rec_grid.Want per record."""
    specs = [b.spec for b in built]
    hdr, T = 5 + G.explicit(cfg), G.taglen(cfg)
    n_grid, n = len(built), len(built) + len(RUNTS)
    wires = [b.wire for b in built]
    rooms = [max(len(w) - hdr - T, 0) for w in wires] + [0] * len(RUNTS)
    wire_res, out_res = _residues(n, seed, hdr)
    wire_off, wsz = cbc_grid.place([len(w) for w in wires], wire_res[:n_grid])
    out_off, osz = cbc_grid.place(rooms, out_res)
    # a runt record ends where the allocation ends (length 0: at its last byte): whatever is
    # read of it is read from the guard, and a read past the record would leave the allocation
    wire_off += [wsz - max(k, 1) for k in RUNTS]
    wire_len = [len(w) for w in wires] + list(RUNTS)
    # bounds: every extent, with its gaps, lies inside its buffer
    assert all(256 <= o and o + k + 256 <= wsz for o, k in zip(wire_off[:n_grid], wire_len))
    assert all(wsz - 4 <= o and o + k <= wsz for o, k in zip(wire_off[n_grid:], RUNTS))
    assert all(256 <= o and o + r + 256 <= osz for o, r in zip(out_off, rooms))
    wire = np.full(wsz, CANARY_W, np.uint8)
    for o, w in zip(wire_off, wires):
        wire[o:o + len(w)] = np.frombuffer(w, np.uint8)
    inputs = dict(wire=wire, wire_off=np.array(wire_off, np.uint64), wire_len=np.array(wire_len, np.uint32),
                  data_off=np.array(out_off, np.uint64))
    d = dict((k, _dev(torch, v)) for k, v in inputs.items())
    d["data"] = torch.full((osz,), CANARY_O, dtype=torch.uint8, device="cuda")
    d["data_len"] = _dev(torch, np.full(n + SLACK, FILL_LEN, np.uint32))
    d["ctype"] = torch.full((n + SLACK,), FILL8, dtype=torch.uint8, device="cuda")
    d["status"] = torch.full((n + SLACK,), FILL8, dtype=torch.uint8, device="cuda")
    assert d["wire"].data_ptr() % 16 == 0 and d["data"].data_ptr() % 16 == 0    # residues are address residues
    call(n, d)
    torch.cuda.synchronize()
    st, ct = d["status"].cpu().numpy(), d["ctype"].cpu().numpy()
    ln = d["data_len"].cpu().numpy().view(np.uint32)
    G.check(cfg, specs, want, list(zip(st[:n_grid], ct[:n_grid], ln[:n_grid])))
    for j, k in enumerate(RUNTS):
        i = n_grid + j
        assert (st[i], ct[i], ln[i]) == (G.TRUNCATED, 0, 0), "wire length %d" % k
    assert (st[n:] == FILL8).all() and (ct[n:] == FILL8).all() and (ln[n:] == FILL_LEN).all()
    img = np.full(osz, CANARY_O, np.uint8)
    for o, b, w in zip(out_off, built, want):
        left = G.data_image(cfg, b, w)
        if left is not None:
            img[o:o + len(left)] = np.frombuffer(left, np.uint8)
    diff = _first_diff(d["data"].cpu().numpy(), img, out_off, rooms)
    assert diff is None, ("data buffer", G.describe(specs, diff[0]) if diff[0] < n_grid else "runt") + diff
    for k, v in inputs.items():
        assert np.array_equal(d[k].cpu().numpy().view(v.dtype), v), "input array %s was written" % k
    return st[:n_grid]


def _want(cfg, built):
    want = G.expected(GOLDEN, cfg, built)
    assert G.OUTSIDE_REMIT == OUTSIDE_REMIT
    return want


@pytest.mark.parametrize("cfg", G.GRIDS, ids=G.IDS)
def test_open_grid(torch, tg, oracle_mod, cfg):
    built = G.oracle_grid(cfg, oracle_mod)
    assert G.wires_digest([b.wire for b in built]) == GOLDEN[G.grid_id(cfg)]["wires_sha256"]
    want = _want(cfg, built)
    key, iv = G.keys(cfg)
    k = _single_key(tg, cfg.alg, key)
    v = tg.TLS13 if cfg.version == "tls13" else tg.TLS12

    def call(n, d):
        tg.open_records(k, v, iv, G.SEQ0, n, d["wire"], d["wire_off"], d["wire_len"], d["data"], d["data_off"],
                        d["data_len"], d["ctype"], d["status"], recv_limit=0 if cfg.limit == 2 ** 14 else cfg.limit)

    st = _open_and_check(torch, cfg, built, want, 3000 + G.GRIDS.index(cfg), call)
    if len(cfg.classes) > 1:
        assert set(st.tolist()) == (set(range(8)) if cfg.version == "tls13" else {0, 1, 2, 7})


@pytest.mark.parametrize("gid", G.SESSION_GRIDS)
@pytest.mark.parametrize("mode", ["explicit", "counter"])
def test_open_grid_many_sessions(torch, tg, oracle_mod, gid, mode):
    """The grid dealt across three sessions (keys, IVs and counters of their
    own; one record's session out of range).  Counter mode: every in-range
    record takes its session's next number whatever its status -- also the
    records the reference gives none (header overflow, unprotected)."""
    cfg = G.GRIDS[G.IDS.index(gid)]
    n_grid = len(G.plan(cfg))
    n = n_grid + len(RUNTS)
    sessions, seqs, nxt = G.deal(n)
    assert sessions[G.SKIPPED] >= G.NSESS and seqs[G.SKIPPED] is None
    built = G.build(cfg, G.oracle_seal(oracle_mod), sessions[:n_grid], seqs[:n_grid])
    want = _want(cfg, built)
    assert any(not w.advanced for w in want)        # records that cost the reference no number are in the batch
    want[G.SKIPPED] = G.Want(G.BAD_SESSION, 0, 0, False, "session out of range")
    built[G.SKIPPED] = built[G.SKIPPED]._replace(wire=built[0].wire if built[0].spec.raw is None else built[1].wire)
    table = tg.KeyTable(_table_alg(cfg.alg), [G.keys(cfg, s)[0] for s in range(G.NSESS)])
    ivs = _dev(torch, np.frombuffer(b"".join(G.keys(cfg, s)[1] for s in range(G.NSESS)), np.uint8)
               .reshape(G.NSESS, cfg.ivlen))
    d_sess = _dev(torch, np.array(sessions, np.uint32))
    seq_out = torch.full((n + SLACK,), SENTINEL, dtype=torch.int64, device="cuda")
    starts = _dev(torch, np.array(G.SESSION_STARTS, np.uint64))
    d_seq = _dev(torch, np.array([0x1111 if q is None else q for q in seqs], np.uint64))
    v = tg.TLS13 if cfg.version == "tls13" else tg.TLS12

    def call(n_, d):
        tg.open_session_records(table, v, ivs, d_sess, n_, d["wire"], d["wire_off"], d["wire_len"], d["data"],
                                d["data_off"], d["data_len"], d["ctype"], d["status"], seq_out=seq_out,
                                recv_limit=cfg.limit, **({"seq": d_seq} if mode == "explicit" else {"seq_next": starts}))

    _open_and_check(torch, cfg, built, want, 4000 + G.IDS.index(gid), call)
    got_seq = seq_out.cpu().numpy()
    want_seq = np.array([(SENTINEL if q is None else q) & (2 ** 64 - 1) for q in seqs]
                        + [SENTINEL & (2 ** 64 - 1)] * SLACK, np.uint64).view(np.int64)
    assert np.array_equal(got_seq, want_seq)
    assert starts.cpu().numpy().view(np.uint64).tolist() == (nxt if mode == "counter" else list(G.SESSION_STARTS))
    assert np.array_equal(d_sess.cpu().numpy().view(np.uint32), np.array(sessions, np.uint32))


@pytest.mark.parametrize("cfg", [c for c in G.GRIDS if len(c.classes) > 1], ids=G.IDS[:6])
def test_seal_grid(torch, tg, oracle_mod, cfg):
    """tg_seal_records over the grid's sequence numbers: the valid records'
    fragments give the grid's wires (the others seal an empty fragment)."""
    built = G.oracle_grid(cfg, oracle_mod)
    tls13, hdr, T = cfg.version == "tls13", 5 + G.explicit(cfg), G.taglen(cfg)
    key, iv = G.keys(cfg)
    n = len(built)
    frags, ctypes_, pads, valid = [], [], [], []
    for b in built:
        s = b.spec
        ok = not s.muts and s.raw is None and not s.delta and s.ctype != 0
        valid.append(ok)
        frags.append(b.plain[:s.frag] if ok else b"")
        ctypes_.append(s.ctype if ok else 23)
        pads.append(s.pad if ok and tls13 else 0)
    assert sum(valid) > n // 4
    wires = [R.seal_record(cfg.version, cfg.alg, key, iv, b.seq, c, f, p)
             for b, c, f, p in zip(built, ctypes_, frags, pads)]
    assert all(w == b.wire for w, b, ok in zip(wires, built, valid) if ok)
    inner = [len(f) + 1 + p if tls13 else len(f) for f, p in zip(frags, pads)]
    data_res, wire_res = cbc_grid.residues(n, 5000 + G.GRIDS.index(cfg), (0, -hdr % 16))
    data_off, dsz = cbc_grid.place(inner, data_res)
    wire_off, wsz = cbc_grid.place([len(w) for w in wires], wire_res)
    assert all(256 <= o and o + m + 256 <= dsz for o, m in zip(data_off, inner))
    assert all(256 <= o and o + len(w) + 256 <= wsz for o, w in zip(wire_off, wires))
    data = np.full(dsz, CANARY_D, np.uint8)
    for o, f in zip(data_off, frags):
        data[o:o + len(f)] = np.frombuffer(f, np.uint8)
    d_data = _dev(torch, data)
    d_wire = torch.full((wsz,), CANARY_W, dtype=torch.uint8, device="cuda")
    w_len = _dev(torch, np.full(n + SLACK, FILL_LEN, np.uint32))
    tg.seal_records(_single_key(tg, cfg.alg, key), tg.TLS13 if tls13 else tg.TLS12, iv, G.SEQ0, n, d_data,
                    _dev(torch, np.array(data_off, np.uint64)), _dev(torch, np.array([len(f) for f in frags], np.uint32)),
                    _dev(torch, np.array(ctypes_, np.uint8)), d_wire, _dev(torch, np.array(wire_off, np.uint64)), w_len,
                    pad_len=_dev(torch, np.array(pads, np.uint32)) if tls13 else None)
    torch.cuda.synchronize()
    got_len = w_len.cpu().numpy().view(np.uint32)
    assert got_len[:n].tolist() == [len(w) for w in wires] and (got_len[n:] == FILL_LEN).all()
    img = np.full(wsz, CANARY_W, np.uint8)
    for o, w in zip(wire_off, wires):
        img[o:o + len(w)] = np.frombuffer(w, np.uint8)
    diff = _first_diff(d_wire.cpu().numpy(), img, wire_off, [len(w) for w in wires])
    assert diff is None, ("wire buffer", G.describe([b.spec for b in built], diff[0])) + diff
    if tls13:       # the one write to the input: type and padding behind the fragment
        for o, f, c, p in zip(data_off, frags, ctypes_, pads):
            data[o + len(f)] = c
            data[o + len(f) + 1:o + len(f) + 1 + p] = 0
    diff = _first_diff(d_data.cpu().numpy(), data, data_off, inner)
    assert diff is None, ("data buffer", G.describe([b.spec for b in built], diff[0])) + diff

"""GPU: the AES-CBC + HMAC record kernels over the padding grid and with a
different alignment in every lane.

test_open_grid opens a whole grid of tests/cbc_grid.py in one call -- every
padding length at the decrypted lengths where the constant-work verdict
changes shape, each valid record next to a mutated twin -- and expects the
verdicts of the reference's RecordLayer (tests/golden/cbc_grid.json;
test_cbc_grid_oracle.py proves that the wires built here are the bytes the
reference judged).  Non-minimal padding is what a peer may send and what our
own seal kernel never produces: the digest is then taken up to four
compression calls before the last one that runs.

Every record of every test here has address residues of its own in each
buffer, and every fourth record is forced onto the vector path, so that a
wave runs the vector and the byte path side by side.  Every check compares
whole buffers with an image built on the host: extents lie between canary
gaps of at least 48 bytes, with 256 at both ends of a buffer.

Malformed records are malformed in content only: every offset and length
stays inside its buffer."""
import json
import os

import numpy as np
import pytest

import cbc_grid
import cbc_model
from conftest import ROOT
from vectors import detbytes

pytestmark = pytest.mark.gpu

GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "cbc_grid.json")))
IDS = [cbc_grid.grid_id(c, m) for c, m in cbc_grid.GRIDS]
CANARY_D, CANARY_W, CANARY_O = 0xA5, 0x5A, 0xC3
FILL_LEN, FILL_CT, FILL_ST, SLACK = -1, 0xEE, 0xEE, 64


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


def _mixed_residues(n, seed, forced):
    """Per-record residues; asserts what the layout is for: all 16 residues in
    every buffer, and the vector and the byte path both live in every wave."""
    res = cbc_grid.residues(n, seed, forced)
    vector = np.logical_and.reduce([r == f for r, f in zip(res, forced)])
    if n >= 128:
        assert all(set(r.tolist()) == set(range(16)) for r in res)
    for w in range(0, n, 64):
        assert vector[w:w + 64].any() and not vector[w:w + 64].all()
    return res


def _image(size, canary, offs, chunks):
    img = np.full(size, canary, np.uint8)
    for o, c in zip(offs, chunks):
        img[o:o + len(c)] = np.frombuffer(bytes(c), np.uint8)
    return img


def _first_diff(got, want, offs, sizes, mask=None):
    """None, or (record nearest to the first difference, offset relative to its extent, want, got)."""
    ne = got != want
    if mask is not None:
        ne &= mask
    if not ne.any():
        return None
    p = int(np.flatnonzero(ne)[0])
    offs, sizes = np.asarray(offs), np.asarray(sizes)
    dist = np.where(p < offs, offs - p, np.where(p >= offs + sizes, p - offs - sizes + 1, 0))
    i = int(np.argmin(dist))
    return i, p - int(offs[i]), "want 0x%02x" % want[p], "got 0x%02x" % got[p]


class OpenRun(object):
    """One tg_cbc_open_records call over ``wires`` laid out at ``wire_res`` /
    ``out_res`` (residues of the wire and the data offsets); ``rooms``: the
    data extent of each record (wire length - 21; 0 for a runt)."""

    def __init__(self, torch, tg, key, version, etm, seq0, wires, rooms, wire_res, out_res):
        n = self.n = len(wires)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
        self.rooms = rooms
        self.wire_off, wsz = cbc_grid.place([len(w) for w in wires], wire_res)
        self.out_off, osz = cbc_grid.place(rooms, out_res)
        # bounds: every extent, with its gaps, lies inside its buffer
        assert all(256 <= o and o + len(w) + 256 <= wsz for o, w in zip(self.wire_off, wires))
        assert all(256 <= o and o + r + 256 <= osz for o, r in zip(self.out_off, rooms))
        self.wire_host = _image(wsz, CANARY_W, self.wire_off, wires)
        self.inputs = [self.wire_host, np.array(self.wire_off, np.int64), np.array(self.out_off, np.int64),
                       np.array([len(w) for w in wires], np.int32)]
        d_wire, d_woff, d_ooff, d_wlen = self.dev_inputs = [dev(a) for a in self.inputs]
        assert d_wire.data_ptr() % 16 == 0      # the residues are address residues
        out = torch.full((osz,), CANARY_O, dtype=torch.uint8, device="cuda")
        assert out.data_ptr() % 16 == 0
        o_len = torch.full((n + SLACK,), FILL_LEN, dtype=torch.int32, device="cuda")
        o_ct = torch.full((n + SLACK,), FILL_CT, dtype=torch.uint8, device="cuda")
        st = torch.full((n + SLACK,), FILL_ST, dtype=torch.uint8, device="cuda")
        tg.cbc.open_records(key, version, etm, seq0, n, out, d_ooff, o_len, o_ct, st, d_wire, d_woff, d_wlen)
        torch.cuda.synchronize()
        self.out, self.osz = out.cpu().numpy(), osz
        self.o_len, self.o_ct, self.st = o_len.cpu().numpy(), o_ct.cpu().numpy(), st.cpu().numpy()

    def check(self, want, name):
        """``want``: (status, content type, plaintext, bytes of the extent
        that must be zero) per record; ``name(i)`` describes record i."""
        n = self.n
        wrong = []
        for i, (status, ctype, plain, _) in enumerate(want):
            got = (int(self.st[i]), int(self.o_ct[i]), int(self.o_len[i]))
            if got != (status, ctype, len(plain)):
                wrong.append("%s: (status, type, length) = %r, want %r" % (name(i), got, (status, ctype, len(plain))))
        assert not wrong, "%d of %d records, the first:\n%s" % (len(wrong), n, "\n".join(wrong[:12]))
        assert (self.st[n:] == FILL_ST).all() and (self.o_ct[n:] == FILL_CT).all() and (self.o_len[n:] == FILL_LEN).all()
        # the whole data buffer: canary, plaintext in accepted extents (the rest of such an
        # extent is unspecified), zeros where a rejected record had been decrypted
        img = np.full(self.osz, CANARY_O, np.uint8)
        mask = np.ones(self.osz, bool)
        for o, room, (status, _, plain, zeros) in zip(self.out_off, self.rooms, want):
            if status == 0:
                img[o:o + len(plain)] = np.frombuffer(plain, np.uint8)
                mask[o + len(plain):o + room] = False
            else:
                img[o:o + zeros] = 0
        d = _first_diff(self.out, img, self.out_off, self.rooms, mask)
        assert d is None, ("data buffer", name(d[0])) + d
        for dev_t, host in zip(self.dev_inputs, self.inputs):
            assert np.array_equal(dev_t.cpu().numpy(), host), "an input array was written"


@pytest.mark.parametrize("grid", cbc_grid.GRIDS, ids=IDS)
def test_open_grid(torch, tg, grid):
    cfg, mode = grid
    etm = int(mode == "etm")
    d = cbc_grid.DIGEST[cfg.mac]
    recs, wires = cbc_grid.model_grid(cfg, mode)
    assert cbc_grid.wires_digest(wires) == GOLDEN[cbc_grid.grid_id(cfg, mode)]["wires_sha256"]
    verdicts = cbc_grid.expected(GOLDEN, cfg, mode)
    n = len(recs)
    wire_res, out_res = _mixed_residues(n, 1000 + IDS.index(cbc_grid.grid_id(cfg, mode)), (11, 0))
    enc_key, mac_key = cbc_grid.keys(cfg)
    key = tg.CbcKey(enc_key, mac_key, cfg.mac)
    run = OpenRun(torch, tg, key, cfg.version, etm, cbc_grid.SEQ0, wires, [len(w) - 21 for w in wires],
                  wire_res, out_res)
    want = []
    for r, (verdict, length) in zip(recs, verdicts):
        # every grid record passes the public checks (and under EtM the MAC) and is decrypted:
        # a rejected one leaves n zero bytes, under EtM with the MAC's share of the extent untouched
        want.append((cbc_model.STATUS_CODE[verdict], r.ctype, r.body[:length] if verdict == "ok" else b"", r.case.n))
    run.check(want, lambda i: "n=%d pad=%d mutation=%s (record %d)" % (recs[i].case.n, recs[i].case.pad,
                                                                        recs[i].case.kind, i))
    assert {w[0] for w in want} == {0, 1}
    key.close()


SEAL_CONFIGS = [(c, etm) for c in cbc_grid.CONFIGS[:3] for etm in (0, 1)]
_seal_cache = {}


def _seal_model(cfg, etm):
    if (cfg.name, etm) not in _seal_cache:
        enc_key, mac_key = cbc_grid.keys(cfg)
        lens = cbc_grid.seal_lengths(cfg.mac, etm)
        datas = [bytes(detbytes("grid-seal-%d" % i, k)) for i, k in enumerate(lens)]
        ivs = [bytes(detbytes("grid-seal-iv-%d" % i, 16)) for i in range(len(lens))]
        wires = [cbc_model.seal_record(enc_key, mac_key, cfg.mac, cfg.version, etm, cbc_grid.SEQ0 + i,
                                       cbc_grid.CTYPES[i % 3], datas[i], ivs[i]) for i in range(len(lens))]
        _seal_cache[cfg.name, etm] = (datas, ivs, wires)
    return _seal_cache[cfg.name, etm]


@pytest.mark.parametrize("cfg,etm", SEAL_CONFIGS, ids=["%s/%s" % (c.name, "etm" if e else "mte") for c, e in SEAL_CONFIGS])
def test_seal_mixed_alignment(torch, tg, cfg, etm):
    datas, ivs, want = _seal_model(cfg, etm)
    n = len(datas)
    assert n == 130 and sorted(len(x) for x in datas)[-3:] == [1000, 16384, 16384]
    # a record is on the vector path when its fragment and wire + 21 are 16-byte aligned
    data_res, wire_res = _mixed_residues(n, 2000 + 2 * cbc_grid.CONFIGS.index(cfg) + etm, (0, 11))
    iv_lead = 5         # iv is n x 16 bytes at a fixed stride: one residue for all records
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    data_off, dsz = cbc_grid.place([len(x) for x in datas], data_res)
    wire_off, wsz = cbc_grid.place([len(w) for w in want], wire_res)
    assert all(256 <= o and o + len(w) + 256 <= wsz for o, w in zip(wire_off, want))
    assert all(len(w) == cbc_model.wire_len(cfg.mac, etm, len(x)) for w, x in zip(want, datas))
    inputs = [_image(dsz, CANARY_D, data_off, datas), np.array(data_off, np.int64),
              np.array([len(x) for x in datas], np.int32), np.array([cbc_grid.CTYPES[i % 3] for i in range(n)], np.uint8),
              np.concatenate([np.full(iv_lead, CANARY_D, np.uint8), np.frombuffer(b"".join(ivs), np.uint8),
                              np.full(16, CANARY_D, np.uint8)]),
              np.array(wire_off, np.int64)]
    d_data, d_doff, d_dlen, d_ct, d_iv, d_woff = dev_inputs = [dev(a) for a in inputs]
    wire = torch.full((wsz,), CANARY_W, dtype=torch.uint8, device="cuda")
    assert d_data.data_ptr() % 16 == 0 and wire.data_ptr() % 16 == 0 and d_iv.data_ptr() % 16 == 0
    w_len = torch.full((n + SLACK,), FILL_LEN, dtype=torch.int32, device="cuda")
    enc_key, mac_key = cbc_grid.keys(cfg)
    key = tg.CbcKey(enc_key, mac_key, cfg.mac)
    tg.cbc.seal_records(key, cfg.version, etm, cbc_grid.SEQ0, n, d_data, d_doff, d_dlen, d_ct, d_iv[iv_lead:], wire,
                        d_woff, w_len)
    torch.cuda.synchronize()
    got_len = w_len.cpu().numpy()
    assert got_len[:n].tolist() == [len(w) for w in want] and (got_len[n:] == FILL_LEN).all()
    diff = _first_diff(wire.cpu().numpy(), _image(wsz, CANARY_W, wire_off, want), wire_off, [len(w) for w in want])
    assert diff is None, ("wire buffer", "fragment length %d (record %d)" % (len(datas[diff[0]]), diff[0])) + diff
    for dev_t, host in zip(dev_inputs, inputs):
        assert np.array_equal(dev_t.cpu().numpy(), host), "an input array was written"
    key.close()


@pytest.mark.parametrize("cfg,etm", SEAL_CONFIGS, ids=["%s/%s" % (c.name, "etm" if e else "mte") for c, e in SEAL_CONFIGS])
def test_open_runt_wires(torch, tg, cfg, etm):
    """Wire lengths 0..4 -- not even a header -- between good records:
    TG_REC_BAD_MAC, type 0, length 0, nothing read as a record and nothing written."""
    enc_key, mac_key = cbc_grid.keys(cfg)
    seq0 = 2 ** 40
    wires, datas = [], []
    for i in range(16):
        data = bytes(detbytes("grid-runt-%d" % i, 10 * i))
        good = cbc_model.seal_record(enc_key, mac_key, cfg.mac, cfg.version, etm, seq0 + i, cbc_grid.CTYPES[i % 3],
                                     data, detbytes("grid-runt-iv-%d" % i, 16))
        runt = i % 3 == 1
        wires.append(good[:(i // 3) % 5] if runt else good)   # the start of a real record: a header cut short
        datas.append(None if runt else data)
    assert sorted(len(w) for w in wires if len(w) < 5) == [0, 1, 2, 3, 4]
    wire_res, out_res = cbc_grid.residues(len(wires), 77, (11, 0))
    key = tg.CbcKey(enc_key, mac_key, cfg.mac)
    run = OpenRun(torch, tg, key, cfg.version, etm, seq0, wires, [max(len(w) - 21, 0) for w in wires], wire_res,
                  out_res)
    want = []
    for i, (w, data) in enumerate(zip(wires, datas)):
        model = cbc_model.open_record(enc_key, mac_key, cfg.mac, cfg.version, etm, seq0 + i, w)
        assert model == (("TLSBadRecordMAC", 0, b"") if data is None else ("ok", w[0], data))
        want.append((cbc_model.STATUS_CODE[model[0]], model[1], model[2], 0))
    run.check(want, lambda i: "wire length %d (record %d)" % (len(wires[i]), i))
    key.close()

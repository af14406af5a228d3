"""GPU: batched TLS 1.1 / 1.2 AES-CBC + HMAC records (tg_cbc_seal_records /
tg_cbc_open_records) against the reference RecordLayer's wire bytes and
receive verdicts (tests/golden/cbc.json) and, for batch shapes the fixtures do
not cover, the CPU model (tests/cbc_model.py, itself held against the same
fixtures by test_cbc_oracle.py).

Malformed records are malformed in content only: every offset and length
stays inside its buffer."""
import hashlib
import json
import os

import numpy as np
import pytest

import cbc_model
from conftest import ROOT
from vectors import detbytes

pytestmark = pytest.mark.gpu

CASES = json.load(open(os.path.join(ROOT, "tests", "golden", "cbc.json")))
IDS = ["%s-%d.%d-%s" % (c["suite"], c["version"][0], c["version"][1], "etm" if c["etm"] else "mte")
       for c in CASES]
CANARY_D, CANARY_W, CANARY_O = 0xA5, 0x5A, 0xC3


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


def _offsets(sizes, lead, gap=16):
    """Offsets with off % 16 == lead and at least ``gap`` canary bytes between extents."""
    offs, at = [], gap
    for s in sizes:
        at = (at + 15) // 16 * 16 + lead
        offs.append(at)
        at += s + gap
    return np.array(offs, np.int64), at + 64


class Batch(object):
    """Device buffers of one batch: fragments in, wire, fragments out."""

    def __init__(self, torch, mac, etm, datas, aligned):
        self.torch, self.n, self.datas = torch, len(datas), datas
        lens = [len(x) for x in datas]
        self.wlens = [cbc_model.wire_len(mac, etm, n) for n in lens]
        self.data_off, dsz = _offsets(lens, 0 if aligned else 7)
        self.wire_off, wsz = _offsets(self.wlens, 11 if aligned else 4)     # wire_off + 5: 0 / 9 mod 16
        self.out_off, osz = _offsets([w - 21 for w in self.wlens], 0 if aligned else 3)
        host = np.full(dsz, CANARY_D, np.uint8)
        for o, x in zip(self.data_off, datas):
            host[o:o + len(x)] = np.frombuffer(bytes(x), np.uint8)
        self.data_host = host
        self.dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        self.data = self.dev(host)
        self.d_off, self.w_off, self.o_off = self.dev(self.data_off), self.dev(self.wire_off), self.dev(self.out_off)
        self.d_len = self.dev(np.array(lens, np.int32))
        self.wire = torch.full((wsz,), CANARY_W, dtype=torch.uint8, device="cuda")
        self.w_len = torch.zeros(self.n, dtype=torch.int32, device="cuda")
        self.out = torch.full((osz,), CANARY_O, dtype=torch.uint8, device="cuda")
        self.o_len = torch.full((self.n,), -1, dtype=torch.int32, device="cuda")
        self.o_ct = torch.full((self.n,), 255, dtype=torch.uint8, device="cuda")
        self.st = torch.full((self.n,), 255, dtype=torch.uint8, device="cuda")

    def seal(self, tg, key, version, etm, seq0, ctypes_, ivs, stream=None):
        self.ctype = self.dev(np.array(ctypes_, np.uint8))
        self.iv = self.dev(np.frombuffer(b"".join(ivs), np.uint8).copy())
        tg.cbc.seal_records(key, version, etm, seq0, self.n, self.data, self.d_off, self.d_len, self.ctype,
                            self.iv, self.wire, self.w_off, self.w_len, stream=stream)

    def open(self, tg, key, version, etm, seq0, stream=None, recv_limit=0):
        tg.cbc.open_records(key, version, etm, seq0, self.n, self.out, self.o_off, self.o_len, self.o_ct,
                            self.st, self.wire, self.w_off, self.w_len, stream=stream, recv_limit=recv_limit)

    def wires(self):
        wh, wl = self.wire.cpu().numpy(), self.w_len.cpu().numpy()
        return [wh[o:o + n].tobytes() for o, n in zip(self.wire_off, wl)], wh

    def set_wires(self, wires):
        """Replace the wire records (same extents or shorter) for an open."""
        wh = np.full(self.wire.numel(), CANARY_W, np.uint8)
        for o, w, room in zip(self.wire_off, wires, self.wlens):
            assert len(w) <= room
            wh[o:o + len(w)] = np.frombuffer(w, np.uint8)
        self.wire = self.dev(wh)
        self.w_len = self.dev(np.array([len(w) for w in wires], np.int32))

    def opened(self):
        oh = self.out.cpu().numpy()
        res = [(int(s), int(c), int(n), oh[o:o + max(n, 0)].tobytes()) for s, c, n, o in
               zip(self.st.cpu().numpy(), self.o_ct.cpu().numpy(), self.o_len.cpu().numpy(), self.out_off)]
        return res, oh

    @staticmethod
    def gaps_intact(buf, offs, sizes, canary):
        mask = np.ones(len(buf), bool)
        for o, s in zip(offs, sizes):
            mask[o:o + s] = False
        return bool((buf[mask] == canary).all())


def _zeros_then_canary(room):
    """A rejected record's extent: a zeroed prefix, then bytes nobody wrote."""
    k = int(np.count_nonzero(room == 0)) if len(room) and room[0] == 0 else 0
    return bool((room[:k] == 0).all() and (room[k:] == CANARY_O).all())


def _version(case):
    return case["version"][0] << 8 | case["version"][1]


def _key(tg, case):
    return tg.CbcKey(bytes.fromhex(case["enc_key"]), bytes.fromhex(case["mac_key"]), case["mac"])


@pytest.mark.parametrize("case", CASES, ids=IDS)
@pytest.mark.parametrize("aligned", [True, False])
def test_seal_fixtures(torch, tg, case, aligned):
    recs = case["seal"]
    datas = [bytes(detbytes("cbc-%d-%d" % (i, r["len"]), r["len"])) for i, r in enumerate(recs)]
    b = Batch(torch, case["mac"], case["etm"], datas, aligned)
    key = _key(tg, case)
    b.seal(tg, key, _version(case), case["etm"], case["seq0"], [r["ctype"] for r in recs],
           [bytes.fromhex(r["iv"]) for r in recs])
    b.open(tg, key, _version(case), case["etm"], case["seq0"])
    torch.cuda.synchronize()
    wires, wh = b.wires()
    for i, (r, w) in enumerate(zip(recs, wires)):
        assert len(w) == r["wire_len"], (i, r["len"])
        assert w[:32].hex() == r["wire_head"] and w[-16:].hex() == r["wire_tail"], (i, r["len"])
        assert hashlib.sha256(w).hexdigest() == r["wire_sha256"], (i, r["len"])
    opened, oh = b.opened()
    for i, (r, d, (st, ct, n, plain)) in enumerate(zip(recs, datas, opened)):
        assert (st, ct, n) == (0, r["ctype"], r["len"]) and plain == d, (i, r["len"], st, n)
    assert b.gaps_intact(wh, b.wire_off, b.wlens, CANARY_W)
    assert b.gaps_intact(oh, b.out_off, [w - 21 for w in b.wlens], CANARY_O)
    assert np.array_equal(b.data.cpu().numpy(), b.data_host)           # the fragments are read only
    key.close()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_open_fixtures(torch, tg, case):
    """One call per fixture: each has its own sequence number and limit."""
    opens = case["open"]
    wires = [bytes.fromhex(o["wire"]) for o in opens]
    wire_off, wsz = _offsets([len(w) for w in wires], 4)
    out_off, osz = _offsets([max(len(w) - 21, 0) for w in wires], 3)
    wh = np.full(wsz, CANARY_W, np.uint8)
    for o, w in zip(wire_off, wires):
        wh[o:o + len(w)] = np.frombuffer(w, np.uint8)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    n = len(opens)
    wire, w_off, o_off = dev(wh), dev(wire_off), dev(out_off)
    w_len = dev(np.array([len(w) for w in wires], np.int32))
    out = torch.full((osz,), CANARY_O, dtype=torch.uint8, device="cuda")
    o_len = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    o_ct = torch.full((n,), 255, dtype=torch.uint8, device="cuda")
    st = torch.full((n,), 255, dtype=torch.uint8, device="cuda")
    key = _key(tg, case)
    for i, o in enumerate(opens):
        tg.cbc.open_records(key, _version(case), case["etm"], o["seq"], 1, out, o_off[i:i + 1], o_len[i:i + 1],
                            o_ct[i:i + 1], st[i:i + 1], wire, w_off[i:i + 1], w_len[i:i + 1],
                            recv_limit=o["recv_limit"])
    torch.cuda.synchronize()
    oh, sth, lh, cth = out.cpu().numpy(), st.cpu().numpy(), o_len.cpu().numpy(), o_ct.cpu().numpy()
    for i, (o, w) in enumerate(zip(opens, wires)):
        assert int(sth[i]) == cbc_model.STATUS_CODE[o["recv"]], (o["name"], int(sth[i]))
        assert int(cth[i]) == w[0], o["name"]
        room = oh[out_off[i]:out_off[i] + max(len(w) - 21, 0)]
        if o["recv"] == "ok":
            assert int(lh[i]) == len(o["plain"]) // 2 and room[:lh[i]].tobytes().hex() == o["plain"], o["name"]
        else:
            assert int(lh[i]) == 0, o["name"]
            # nothing unauthenticated stays: what the kernel wrote is zero again, the rest
            # of the room (the MAC's share under EtM) is the untouched canary
            assert _zeros_then_canary(room), o["name"]
    assert Batch.gaps_intact(oh, out_off, [max(len(w) - 21, 0) for w in wires], CANARY_O)
    key.close()


# ---- batch shapes against the model ---------------------------------------
CONFIGS = [(16, "sha1", 0), (32, "sha256", 1), (32, "sha384", 0), (16, "sha384", 1), (32, "sha256", 0)]
SEQ0 = 2 ** 32 - 3            # the low word of the sequence number carries inside the batch
NMAX = 257
_model_cache = {}


def _shape_inputs():
    rng = np.random.default_rng(11)
    lens = [int(x) for x in rng.choice([0, 1, 43, 44, 51, 52, 1000], NMAX)]
    for i in (0, 5, 62, 64, 130, 256):
        lens[i] = 16384
    datas = [bytes(detbytes("shape-%d" % i, n)) for i, n in enumerate(lens)]
    ivs = [bytes(detbytes("shape-iv-%d" % i, 16)) for i in range(NMAX)]
    ctypes_ = [(23, 22, 21)[i % 3] for i in range(NMAX)]
    return datas, ivs, ctypes_


def _model(cfg):
    """The model's wire records of the shared inputs, computed once per key configuration."""
    if cfg not in _model_cache:
        keylen, mac, etm = cfg
        ek, mk = bytes(detbytes("shape-ek", keylen)), bytes(detbytes("shape-mk-" + mac, cbc_model.DIGEST[mac]))
        datas, ivs, ctypes_ = _shape_inputs()
        wires = [cbc_model.seal_record(ek, mk, mac, 0x0303, etm, SEQ0 + i, ctypes_[i], datas[i], ivs[i])
                 for i in range(NMAX)]
        _model_cache[cfg] = (ek, mk, datas, ivs, ctypes_, wires)
    return _model_cache[cfg]


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "aes%d-%s-%s" % (c[0] * 8, c[1], "etm" if c[2] else "mte"))
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("aligned", [True, False])
def test_batch_shapes(torch, tg, cfg, n, aligned):
    keylen, mac, etm = cfg
    ek, mk, datas, ivs, ctypes_, want = _model(cfg)
    key = tg.CbcKey(ek, mk, mac)
    b = Batch(torch, mac, etm, datas[:n], aligned)
    b.seal(tg, key, tg.TLS12, etm, SEQ0, ctypes_[:n], ivs[:n])
    b.open(tg, key, tg.TLS12, etm, SEQ0)
    torch.cuda.synchronize()
    wires, wh = b.wires()
    for i in range(n):
        assert wires[i] == want[i], (i, len(datas[i]))
    opened, oh = b.opened()
    for i in range(n):
        assert opened[i] == (0, ctypes_[i], len(datas[i]), datas[i]), (i, opened[i][:3])
    # containment: canaries between the records of all three buffers
    assert b.gaps_intact(wh, b.wire_off, b.wlens, CANARY_W)
    assert b.gaps_intact(oh, b.out_off, [w - 21 for w in b.wlens], CANARY_O)
    assert np.array_equal(b.data.cpu().numpy(), b.data_host)
    key.close()


@pytest.mark.parametrize("cfg", CONFIGS[:4], ids=lambda c: "aes%d-%s-%s" % (c[0] * 8, c[1], "etm" if c[2] else "mte"))
def test_mixed_verdicts_in_one_wave(torch, tg, cfg):
    keylen, mac, etm = cfg
    ek, mk = bytes(detbytes("mix-ek", keylen)), bytes(detbytes("mix-mk", 32))
    rng = np.random.default_rng(5)
    n = 64
    datas = [bytes(detbytes("mix-%d" % i, int(k))) for i, k in enumerate(rng.integers(0, 200, n))]
    ivs = [bytes(detbytes("mix-iv-%d" % i, 16)) for i in range(n)]
    ctypes_ = [(23, 22, 21)[i % 3] for i in range(n)]
    key = tg.CbcKey(ek, mk, mac)
    b = Batch(torch, mac, etm, datas, False)
    b.seal(tg, key, tg.TLS11, etm, 40, ctypes_, ivs)
    torch.cuda.synchronize()
    wires, _ = b.wires()
    for i in range(0, n, 3):
        w = bytearray(wires[i])
        how = (i // 3) % 3
        if how == 0:
            w[21 + (len(w) - 22) // 2] ^= 0x20                  # a ciphertext (or MAC) bit
        elif how == 1:
            w = w[:len(w) - 8]                                  # misaligned body
            w[3:5] = (len(w) - 5).to_bytes(2, "big")
        else:
            w[3:5] = (2 ** 14 + 2049).to_bytes(2, "big")        # header length over the limit
        wires[i] = bytes(w)
    b.set_wires(wires)
    b.open(tg, key, tg.TLS11, etm, 40)
    torch.cuda.synchronize()
    opened, oh = b.opened()
    seen = set()
    for i in range(n):
        verdict, ct, plain = cbc_model.open_record(ek, mk, mac, tg.TLS11, etm, 40 + i, wires[i])
        assert opened[i] == (cbc_model.STATUS_CODE[verdict], ct, len(plain), plain), (i, verdict, opened[i][:3])
        assert verdict == "ok" if i % 3 else verdict != "ok", (i, verdict)
        seen.add(verdict)
        if verdict != "ok":
            room = oh[b.out_off[i]:b.out_off[i] + b.wlens[i] - 21]
            assert _zeros_then_canary(room), i
    assert seen == {"ok", "TLSBadRecordMAC", "TLSRecordOverflow"} | (set() if etm else {"TLSDecryptionFailed"})
    assert b.gaps_intact(oh, b.out_off, [w - 21 for w in b.wlens], CANARY_O)
    key.close()


def test_seal_then_open_on_one_stream_without_host_sync(torch, tg):
    ek, mk, datas, ivs, ctypes_, want = _model(CONFIGS[0])
    n = 65
    key = tg.CbcKey(ek, mk, "sha1")
    b = Batch(torch, "sha1", 0, datas[:n], True)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    b.seal(tg, key, tg.TLS12, 0, SEQ0, ctypes_[:n], ivs[:n], stream=s)
    b.open(tg, key, tg.TLS12, 0, SEQ0, stream=s)
    s.synchronize()
    wires, _ = b.wires()
    opened, _ = b.opened()
    for i in range(n):
        assert wires[i] == want[i]
        assert opened[i] == (0, ctypes_[i], len(datas[i]), datas[i]), i
    key.close()


def test_key_lifecycle_leaves_scratch_flat(torch, tg):
    ek, mk, datas, ivs, ctypes_, want = _model(CONFIGS[1])
    n = 8
    torch.cuda.synchronize()
    before = tg.scratch_info()
    for _ in range(3):
        key = tg.CbcKey(ek, mk, "sha256")
        b = Batch(torch, "sha256", 1, datas[:n], True)
        b.seal(tg, key, tg.TLS12, 1, SEQ0, ctypes_[:n], ivs[:n])
        key.close()                                   # waits for the device, scrubs, frees
        assert key.handle is None
        wires, _ = b.wires()
        assert wires == want[:n]
    assert tg.scratch_info() == before
    with pytest.raises(TypeError):
        tg.cbc.seal_records(key, tg.TLS12, 1, 0, 0, None, None, None, None, None, None, None, None)


def test_empty_batch_launches_nothing(torch, tg):
    key = tg.CbcKey(bytes(16), bytes(20), "sha1")
    tg.cbc.seal_records(key, tg.TLS12, 0, 0, 0, None, None, None, None, 0x1000, None, None, None)
    tg.cbc.open_records(key, tg.TLS12, 0, 0, 0, None, None, None, None, None, None, None, None)
    key.close()

"""Verdicts of the padding grid (tests/cbc_grid.py), from the REFERENCE.

Builds every wire record of the grid with the reference's python_aes and the
standard hmac, hands each to a receiving RecordLayer of the reference whose
read state holds the grid's keys (recvRecord, as make_golden_cbc.py's
receive()), and writes tests/golden/cbc_grid.json.  Per grid
("<configuration>/<mte|etm>") the file holds results only:

    verdicts     one character per record: o = accepted, m = TLSBadRecordMAC,
                 d = TLSDecryptionFailed, v = TLSRecordOverflow
    lengths      the plaintext length of every accepted record, in order
    wires_sha256 SHA-256 over the concatenated wire records, so that the tests
                 can prove they rebuilt exactly the bytes judged here
    records      the number of records

Runs only in the build container through refloader:

    python tests/golden/make_golden_cbc_grid.py
"""
import hashlib
import hmac
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import refloader  # noqa: E402

refloader.load()
from tlslite.mathtls import createHMAC  # noqa: E402
from tlslite.recordlayer import ConnectionState, RecordLayer  # noqa: E402
from tlslite.utils import python_aes  # noqa: E402
from tlslite.utils.cipherfactory import createAES  # noqa: E402
from tlslite.utils.compat import compatHMAC  # noqa: E402
from mocksock import MockSocket  # noqa: E402  (reference unit_tests/mocksock.py:7)

import cbc_grid  # noqa: E402


def mac_fn(mac, mac_key, msg):
    return hmac.new(mac_key, msg, getattr(hashlib, mac)).digest()


def cbc_fn(enc_key, iv, plain):
    assert len(plain) % 16 == 0 and plain
    return bytes(python_aes.new(bytearray(enc_key), 2, bytearray(iv)).encrypt(bytearray(plain)))


def receive(cfg, mode, wire, seq):
    """What the reference's receiving RecordLayer does with one wire record."""
    enc_key, mac_key = cbc_grid.keys(cfg)
    state = ConnectionState()
    state.macContext = createHMAC(compatHMAC(bytearray(mac_key)), digestmod=getattr(hashlib, cfg.mac))
    state.encContext = createAES(bytearray(enc_key), bytearray(16), ['python'])
    state.encryptThenMAC = mode == "etm"
    state.seqnum = seq
    rl = RecordLayer(MockSocket(bytearray(wire)))
    rl.version = (cfg.version >> 8, cfg.version & 255)
    rl.client = False
    rl._readState = state
    try:
        for result in rl.recvRecord():
            assert result not in (0, 1), "blocked"
            hdr, parser = result
            return "ok", hdr.type, bytes(parser.bytes)
    except Exception as e:   # noqa: BLE001 -- the reference's own exception is the fixture
        return type(e).__name__, None, None
    raise AssertionError("nothing received")


def main():
    out = {}
    for cfg, mode in cbc_grid.GRIDS:
        recs = cbc_grid.records(cfg, mode, mac_fn)
        wires = [cbc_grid.wire(cfg, mode, r, cbc_fn, mac_fn) for r in recs]
        verdicts, lengths = [], []
        for r, w in zip(recs, wires):
            recv, ctype, plain = receive(cfg, mode, w, r.seq)
            verdicts.append(cbc_grid.VERDICT_CHAR[recv])
            if recv == "ok":
                assert ctype == r.ctype and r.body.startswith(plain), r.case
                lengths.append(len(plain))
            if r.case.kind is None:
                assert recv == "ok" and plain == r.data, (cfg.name, mode, r.case, recv)
        out[cbc_grid.grid_id(cfg, mode)] = {"verdicts": "".join(verdicts), "lengths": lengths,
                                            "wires_sha256": cbc_grid.wires_digest(wires), "records": len(recs)}
        print(cbc_grid.grid_id(cfg, mode), len(recs), "records,", len(lengths), "accepted,",
              sum(len(r.body) for r in recs) // 16, "AES blocks")
    with open(os.path.join(HERE, "cbc_grid.json"), "w") as f:
        f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(out[k], sort_keys=True,
                                                                       separators=(",", ":")))
                                   for k in sorted(out)) + "\n}\n")


if __name__ == "__main__":
    main()

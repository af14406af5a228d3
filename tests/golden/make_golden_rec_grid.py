"""Verdicts of the AEAD record grid (tests/rec_grid.py), from the REFERENCE.

Seals every record of the grid with the reference's own AEAD objects, hands
each wire record to a fresh receiving RecordLayer of the reference whose read
state holds the grid's key and fixed IV, the record's sequence number and the
grid's recv_record_limit (recvRecord through a MockSocket), and writes
tests/golden/rec_grid.json.  Per grid the file holds results only:

    verdicts     one character per record: o = accepted, m = TLSBadRecordMAC,
                 u = TLSUnexpectedMessage, i = TLSIllegalParameterException,
                 v = TLSRecordOverflow, p = passed through unprotected (the
                 payload came back as it was sent and undecrypted)
    types        content type of every accepted record, in order
    lengths      plaintext length of every accepted record, in order
    advanced     one character per record: 1 where the read state's sequence
                 number advanced, 0 where it did not
    direct       one character per record: 1 where the record cannot come
                 through a socket (header length != body, or a type byte the
                 socket reads as SSLv2) and _decryptAndUnseal was asked with a
                 crafted RecordHeader3 instead
    wires_sha256 SHA-256 over the length-prefixed wire records, so that the
                 tests can prove they rebuilt exactly the bytes judged here
    records      the number of records

Runs only in the build container through refloader:

    python tests/golden/make_golden_rec_grid.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import refloader  # noqa: E402

refloader.load()
from tlslite.messages import RecordHeader3  # noqa: E402
from tlslite.recordlayer import ConnectionState, RecordLayer  # noqa: E402
from tlslite.utils.cipherfactory import createAESCCM, createAESCCM_8, createAESGCM, createCHACHA20  # noqa: E402
from mocksock import MockSocket  # noqa: E402  (reference unit_tests/mocksock.py:7)

import rec_grid  # noqa: E402


def context(alg, key):
    make = (createCHACHA20 if alg.startswith("chacha") else createAESCCM_8 if alg.endswith("ccm_8")
            else createAESCCM if "ccm" in alg else createAESGCM)
    ctx = make(bytearray(key), ["python"])
    assert ctx.name == alg, (ctx.name, alg)
    return ctx


def seal(alg, key, nonce, plain, aad):
    return bytes(context(alg, key).seal(bytearray(nonce), bytearray(plain), bytearray(aad)))


def receive(cfg, b):
    """What the reference's receiving RecordLayer does with one wire record:
    (verdict, content type, plaintext, sequence number advanced, asked directly)."""
    key, iv = rec_grid.keys(cfg)
    state = ConnectionState()
    state.encContext = context(cfg.alg, key)
    state.fixedNonce = bytearray(iv)
    state.seqnum = before = b.seq if b.spec.ref_seq is None else b.spec.ref_seq
    rl = RecordLayer(MockSocket(bytearray(b.wire)))
    rl.version = (3, 4) if cfg.version == "tls13" else (3, 3)
    rl.tls13record = cfg.version == "tls13"
    rl.recv_record_limit = cfg.limit
    rl.client = False
    rl._readState = state
    asked_directly = rec_grid.direct(b.wire)
    try:
        if asked_directly:
            w = b.wire
            hdr = RecordHeader3().create((w[1], w[2]), w[0], w[3] << 8 | w[4])
            rl._decryptAndUnseal(hdr, bytearray(w[5:]))
            raise AssertionError("a record asked directly must be one _decryptAndUnseal refuses: %r" % (b.spec,))
        for result in rl.recvRecord():
            assert result not in (0, 1), "blocked"
            hdr, parser = result
            out = ("ok", hdr.type, bytes(parser.bytes))
            if cfg.version == "tls13" and b.wire[0] != 23:      # recvRecord :920-933: not decrypted
                assert out[1:] == (b.wire[0], b.wire[5:])
                out = ("unprotected", None, None)
            return out + (rl._readState.seqnum != before, False)
    except AssertionError:
        raise
    except Exception as e:   # noqa: BLE001 -- the reference's own exception is the fixture
        return type(e).__name__, None, None, rl._readState.seqnum != before, asked_directly
    raise AssertionError("nothing received")


def main():
    out = {}
    for cfg in rec_grid.GRIDS:
        built = rec_grid.build(cfg, seal)
        verdicts, types, lengths, advanced, asked = [], [], [], [], []
        for i, b in enumerate(built):
            verdict, ctype, plain, adv, direct = receive(cfg, b)
            verdicts.append(rec_grid.VERDICT_CHAR[verdict])
            advanced.append("1" if adv else "0")
            asked.append("1" if direct else "0")
            if verdict == "ok":
                assert b.plain.startswith(plain), rec_grid.describe([x.spec for x in built], i)
                types.append(ctype)
                lengths.append(len(plain))
        gid = rec_grid.grid_id(cfg)
        out[gid] = {"verdicts": "".join(verdicts), "types": types, "lengths": lengths,
                    "advanced": "".join(advanced), "direct": "".join(asked),
                    "wires_sha256": rec_grid.wires_digest([b.wire for b in built]), "records": len(built)}
        print(gid, len(built), "records:", " ".join("%s=%d" % (c, out[gid]["verdicts"].count(c)) for c in "omuivp"),
              "| no number:", out[gid]["advanced"].count("0"), "| direct:", out[gid]["direct"].count("1"))
    with open(os.path.join(HERE, "rec_grid.json"), "w") as f:
        f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(out[k], sort_keys=True,
                                                                       separators=(",", ":")))
                                   for k in out) + "\n}\n")


if __name__ == "__main__":
    main()

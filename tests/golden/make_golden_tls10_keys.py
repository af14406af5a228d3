"""TLS 1.0 / 1.1 key-derivation fixtures, produced by the REFERENCE.

Three groups, all from ``detbytes`` inputs the tests regenerate:

* ``prf``       -- raw tlslite.mathtls.PRF (P_MD5 xor P_SHA1) outputs where the
  device's kernel can go wrong.  With message = label + seed, both hashes
  having 64-byte blocks and an 8-byte length: the A(0) template gains a block
  at 55/56 and 119/120, the A(i) || A(0) template at 39/40 and 103/104 for MD5
  (16-byte A(i)) and at 35/36 and 99/100 for SHA-1 (20-byte A(i)); 0 and 160
  are the shortest and the longest message.  Every such message length is
  reached with every label length that can reach it.  Output lengths give a
  partial last digest for either hash and the point where both end together
  (80); secret lengths give odd ones (the halves share the middle byte) and
  128 (both halves fill a block).
* ``calc_key``  -- tlslite.mathtls.calc_key at (3, 1) and (3, 2) for a
  ``shaSuites`` AES-CBC suite with the labels "master secret", "extended master
  secret", "client finished" and "server finished" (the handshake-hash seeds,
  MD5 || SHA-1, are stored as hex), 12 and 48 bytes of output.
* ``pending``   -- both sides of RecordLayer.calcPendingStates at (3, 2) for
  TLS_RSA_WITH_AES_128_CBC_SHA and TLS_RSA_WITH_AES_256_CBC_SHA, three
  connections each: the client's and the server's MAC key and cipher key as
  createHMAC / createAES received them.

Runs only in the build container through refloader; writes
tests/golden/tls10_keys.json, which the tests replay without the reference.

    python tests/golden/make_golden_tls10_keys.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden_cbc as g  # noqa: E402  (loads the reference, wraps createAES / createHMAC)
from vectors import detbytes  # noqa: E402

from tlslite.constants import CipherSuite  # noqa: E402
from tlslite.handshakehashes import HandshakeHashes  # noqa: E402
from tlslite.mathtls import PRF, calc_key  # noqa: E402

MSG_LENGTHS = [0, 35, 36, 39, 40, 55, 56, 99, 100, 103, 104, 119, 120, 160]
LABEL_LENGTHS = [0, 13, 22, 32]
OUT_LENGTHS = [1, 12, 15, 16, 17, 19, 20, 21, 48, 72, 79, 80, 81, 104, 256]
SECRET_LENGTHS = [1, 2, 47, 48, 49, 127, 128]
BASE = {"secretlen": 48, "labellen": 13, "seedlen": 64}

CALC = [("TLS_RSA_WITH_AES_128_CBC_SHA", CipherSuite.TLS_RSA_WITH_AES_128_CBC_SHA, (3, 1)),
        ("TLS_RSA_WITH_AES_128_CBC_SHA", CipherSuite.TLS_RSA_WITH_AES_128_CBC_SHA, (3, 2))]
PENDING = [("TLS_RSA_WITH_AES_128_CBC_SHA", CipherSuite.TLS_RSA_WITH_AES_128_CBC_SHA),
           ("TLS_RSA_WITH_AES_256_CBC_SHA", CipherSuite.TLS_RSA_WITH_AES_256_CBC_SHA)]
NCONN = 3


def prf_case(secretlen, labellen, seedlen, outlen):
    tag = "%d-%d-%d" % (secretlen, labellen, seedlen)
    got = PRF(bytearray(detbytes("k10-prf-secret-" + tag, secretlen)),
              bytearray(detbytes("k10-prf-label-" + tag, labellen)),
              bytearray(detbytes("k10-prf-seed-" + tag, seedlen)), outlen)
    return {"secretlen": secretlen, "labellen": labellen, "seedlen": seedlen, "outlen": outlen,
            "out": bytes(got).hex()}


def prf_cases():
    out = []
    for outlen in OUT_LENGTHS:
        out.append(prf_case(outlen=outlen, **BASE))
    for labellen in LABEL_LENGTHS:
        for msglen in MSG_LENGTHS:
            if 0 <= msglen - labellen <= 128:
                out.append(prf_case(48, labellen, msglen - labellen, 49))
    for secretlen in SECRET_LENGTHS:
        out.append(prf_case(secretlen, 22, 48, 33))
    reached = set(c["labellen"] + c["seedlen"] for c in out)
    assert reached >= set(MSG_LENGTHS)
    return out


def calc_key_cases():
    out = []
    for name, suite, version in CALC:
        assert suite in CipherSuite.shaSuites and suite in CipherSuite.aes128Suites
        tag = "%s-%d" % (name, version[1])
        hh = HandshakeHashes()
        hh.update(bytearray(detbytes("k10-handshake-" + tag, 300)))
        secret = bytearray(detbytes("k10-secret-" + tag, 48))
        cr, sr = bytearray(detbytes("k10-cr-" + tag, 32)), bytearray(detbytes("k10-sr-" + tag, 32))
        for label in (b"master secret", b"extended master secret", b"client finished", b"server finished"):
            for outlen in (12, 48):
                got = calc_key(version, secret, suite, label, handshake_hashes=hh, client_random=cr,
                               server_random=sr, output_length=outlen)
                case = {"suite": name, "suite_id": suite, "version": list(version), "label": label.decode(),
                        "outlen": outlen, "out": bytes(got).hex()}
                if label == b"master secret":
                    case["seed"] = "client_random+server_random"
                else:   # MD5(handshake) || SHA1(handshake), mathtls.py:870-875
                    case["seed_hex"] = bytes(hh.digest("md5") + hh.digest("sha1")).hex()
                    assert len(case["seed_hex"]) == 72
                out.append(case)
    return out


def pending_cases():
    out = []
    for name, suite in PENDING:
        conns = []
        for c in range(NCONN):
            del g.captured[:]
            rl = g.RecordLayer(g.MockSocket(bytearray(0)))
            rl.version = (3, 2)
            tag = "%s-c%d" % (name, c)
            rl.calcPendingStates(suite, bytearray(detbytes("k10-ms-" + tag, 48)),
                                 bytearray(detbytes("k10-cr-" + tag, 32)),
                                 bytearray(detbytes("k10-sr-" + tag, 32)), ['python'])
            assert rl.client                      # the pending write state is the client's
            # createHMAC client, server, then createAES client, server (recordlayer.py:1223-1235)
            macs = [k for t, k in g.captured if t == "hmac"]
            keys = [k for t, k in g.captured if t == "aes"]
            assert len(macs) == 2 and len(keys) == 2
            conns.append({"client": {"mac_key": macs[0].hex(), "key": keys[0].hex()},
                          "server": {"mac_key": macs[1].hex(), "key": keys[1].hex()}})
        out.append({"suite": name, "suite_id": suite, "version": [3, 2], "conns": conns})
    return out


def main():
    doc = {"prf": prf_cases(), "calc_key": calc_key_cases(), "pending": pending_cases()}
    path = os.path.join(HERE, "tls10_keys.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(HERE, "cbc.json"))
    print("wrote", len(doc["prf"]), "prf,", len(doc["calc_key"]), "calc_key and", len(doc["pending"]),
          "pending cases,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

"""TLS 1.2 key-derivation fixtures, produced by the REFERENCE.

Three groups, all from ``detbytes`` inputs the tests regenerate:

* ``calc_key``  -- tlslite.mathtls.calc_key at (3, 3) for one SHA-256-PRF and
  one SHA-384-PRF suite with the labels "master secret", "extended master
  secret", "client finished" and "server finished" (the handshake-hash seeds
  are stored as hex), 12 and 48 bytes of output.
* ``prf``       -- raw PRF_1_2 / PRF_1_2_SHA384 outputs over the lengths where
  either hashed message moves between one and two blocks and where the
  output's last block is partial: every output length at the baseline, every
  (label length, seed length) pair, every secret length.
* ``pending``   -- both sides of RecordLayer.calcPendingStates for one suite
  per key-block shape, three connections each: the client's and the server's
  MAC key, cipher key and fixed nonce.
* ``families``  -- the reference's lists of suite ids per cipher, MAC and PRF
  family, which the tests hold tlsgpu.keysetup.TLS12_SUITES against whole.

Runs only in the build container through refloader; writes
tests/golden/tls12_keys.json, which the tests replay without the reference.

    python tests/golden/make_golden_tls12_keys.py
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
from tlslite.mathtls import PRF_1_2, PRF_1_2_SHA384, calc_key  # noqa: E402

OUT_LENGTHS = [1, 31, 32, 33, 47, 48, 49, 104, 192, 256]
SEED_LENGTHS = [0, 32, 48, 64, 128]
LABEL_LENGTHS = [0, 13, 22, 32]
SECRET_LENGTHS = {32: [1, 48, 64], 48: [1, 48, 64, 128]}
BASE = {"secretlen": 48, "labellen": 13, "seedlen": 64}

CALC_SUITES = [("TLS_RSA_WITH_AES_128_GCM_SHA256", CipherSuite.TLS_RSA_WITH_AES_128_GCM_SHA256, 32),
               ("TLS_RSA_WITH_AES_256_GCM_SHA384", CipherSuite.TLS_RSA_WITH_AES_256_GCM_SHA384, 48)]
PENDING = [("TLS_RSA_WITH_AES_128_GCM_SHA256", CipherSuite.TLS_RSA_WITH_AES_128_GCM_SHA256),
           ("TLS_RSA_WITH_AES_256_GCM_SHA384", CipherSuite.TLS_RSA_WITH_AES_256_GCM_SHA384),
           ("TLS_RSA_WITH_AES_128_CCM_8", CipherSuite.TLS_RSA_WITH_AES_128_CCM_8),
           ("TLS_ECDHE_RSA_WITH_CHACHA20_POLY1305_SHA256",
            CipherSuite.TLS_ECDHE_RSA_WITH_CHACHA20_POLY1305_SHA256),
           ("TLS_ECDHE_RSA_WITH_CHACHA20_POLY1305_draft_00",
            CipherSuite.TLS_ECDHE_RSA_WITH_CHACHA20_POLY1305_draft_00)] + [(n, s) for n, s, _ in g.SUITES]
NCONN = 3


def calc_key_cases():
    out = []
    for name, suite, hashlen in CALC_SUITES:
        hh = HandshakeHashes()
        hh.update(bytearray(detbytes("k12-handshake-" + name, 300)))
        secret = bytearray(detbytes("k12-secret-" + name, 48))
        cr, sr = bytearray(detbytes("k12-cr-" + name, 32)), bytearray(detbytes("k12-sr-" + name, 32))
        for label in (b"master secret", b"extended master secret", b"client finished", b"server finished"):
            for outlen in (12, 48):
                got = calc_key((3, 3), secret, suite, label, handshake_hashes=hh, client_random=cr,
                               server_random=sr, output_length=outlen)
                case = {"suite": name, "suite_id": suite, "hashlen": hashlen, "label": label.decode(),
                        "outlen": outlen, "out": bytes(got).hex()}
                if label == b"master secret":
                    case["seed"] = "client_random+server_random"
                else:
                    case["seed_hex"] = bytes(hh.digest("sha384" if hashlen == 48 else "sha256")).hex()
                out.append(case)
    return out


def prf_case(hashlen, secretlen, labellen, seedlen, outlen):
    tag = "%d-%d-%d-%d" % (hashlen, secretlen, labellen, seedlen)
    func = PRF_1_2_SHA384 if hashlen == 48 else PRF_1_2
    got = func(bytearray(detbytes("k12-prf-secret-" + tag, secretlen)),
               bytearray(detbytes("k12-prf-label-" + tag, labellen)),
               bytearray(detbytes("k12-prf-seed-" + tag, seedlen)), outlen)
    return {"hashlen": hashlen, "secretlen": secretlen, "labellen": labellen, "seedlen": seedlen,
            "outlen": outlen, "out": bytes(got).hex()}


def prf_cases():
    out = []
    for hashlen in (32, 48):
        for outlen in OUT_LENGTHS:
            out.append(prf_case(hashlen, outlen=outlen, **BASE))
        for labellen in LABEL_LENGTHS:
            for seedlen in SEED_LENGTHS:
                out.append(prf_case(hashlen, 48, labellen, seedlen, 49))
        for secretlen in SECRET_LENGTHS[hashlen]:
            out.append(prf_case(hashlen, secretlen, 22, 48, 33))
    return out


def pending_cases():
    out = []
    for name, suite in PENDING:
        conns = []
        for c in range(NCONN):
            del g.captured[:]
            rl = g.RecordLayer(g.MockSocket(bytearray(0)))
            rl.version = (3, 3)
            tag = "%s-c%d" % (name, c)
            rl.calcPendingStates(suite, bytearray(detbytes("k12-ms-" + tag, 48)),
                                 bytearray(detbytes("k12-cr-" + tag, 32)),
                                 bytearray(detbytes("k12-sr-" + tag, 32)), ['python'])
            assert rl.client                      # the pending write state is the client's
            cw, sw = rl._pendingWriteState, rl._pendingReadState
            if suite in CipherSuite.aeadSuites:
                conn = {"client": {"mac_key": "", "key": bytes(cw.encContext.key).hex(),
                                   "iv": bytes(cw.fixedNonce).hex()},
                        "server": {"mac_key": "", "key": bytes(sw.encContext.key).hex(),
                                   "iv": bytes(sw.fixedNonce).hex()}}
            else:
                # createHMAC client, server, then createAES client, server (recordlayer.py:1223-1235)
                macs = [k for t, k in g.captured if t == "hmac"]
                keys = [k for t, k in g.captured if t == "aes"]
                assert len(macs) == 2 and len(keys) == 2
                conn = {"client": {"mac_key": macs[0].hex(), "key": keys[0].hex(), "iv": ""},
                        "server": {"mac_key": macs[1].hex(), "key": keys[1].hex(), "iv": ""}}
            conns.append(conn)
        out.append({"suite": name, "suite_id": suite, "conns": conns})
    return out


FAMILIES = ["aes256GcmSuites", "aes128GcmSuites", "aes256Ccm_8Suites", "aes256CcmSuites", "aes128Ccm_8Suites",
            "aes128CcmSuites", "chacha20Suites", "chacha20draft00Suites", "aes128Suites", "aes256Suites",
            "aeadSuites", "shaSuites", "sha256Suites", "sha384Suites", "sha384PrfSuites", "tls13Suites"]


def families():
    """The reference's id lists that _getCipherSettings / _getMacSettings and
    calc_key decide by (tlslite/constants.py CipherSuite), as data."""
    return dict((name, sorted(set(getattr(CipherSuite, name)))) for name in FAMILIES)


def main():
    doc = {"calc_key": calc_key_cases(), "prf": prf_cases(), "pending": pending_cases(), "families": families()}
    path = os.path.join(HERE, "tls12_keys.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(HERE, "cbc.json"))
    print("wrote", len(doc["calc_key"]), "calc_key,", len(doc["prf"]), "prf and", len(doc["pending"]),
          "pending cases,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

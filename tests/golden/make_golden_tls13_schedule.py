"""TLS 1.3 key-schedule fixtures, produced by the REFERENCE.

Four groups for sha256 and sha384, all from ``detbytes`` inputs the tests
regenerate (tests/tls13_model.py holds the labels):

* ``extract``  -- tlslite.utils.cryptomath.secureHMAC(salt, ikm, alg), the
  HKDF-Extract of the schedule, at every IKM length where the padded message
  gains a block (SHA-256 holds 55 bytes in one block and 119 in two, SHA-384
  111 and 239) and at the largest the device takes, plus a zero-salt and a
  zero-IKM row.
* ``expand``   -- HKDF_expand_label over label length x context length (for
  SHA-256 the message is 11 + label + context bytes and 55 fill a block: a
  12-byte label with a 32-byte context fills it exactly, a 13-byte label
  spills), outlen = the digest plus 1 and 12 at one shape; and derive_secret
  with a real HandshakeHashes object and with None.
* ``schedule`` -- six connections per hash (three without a PSK, three with),
  shared secrets of 32, 48, 66 and 256 bytes: the chain of
  tlsconnection.py:3036-3050, :3203-3224, :3326-3360 built from the
  reference's own primitives in that order, every named secret, both Finished
  values, and "key" and "iv" of the four traffic secrets as
  RecordLayer.calcTLS1_3PendingState cuts them for every suite of the hash.
* ``binder``   -- HandshakeHelpers._calc_binder for external and resumption
  PSKs of 16, 32, 48 and 64 bytes, and calc_res_binder_psk for ticket nonces
  of 1, 8 and 32 bytes.

Runs only in the build container through refloader; writes
tests/golden/tls13_schedule.json, which the tests replay without the reference.

    python tests/golden/make_golden_tls13_schedule.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import refloader  # noqa: E402
from vectors import detbytes  # noqa: E402

refloader.load()
from tlslite.constants import CipherSuite  # noqa: E402
from tlslite.handshakehashes import HandshakeHashes  # noqa: E402
from tlslite.handshakehelpers import HandshakeHelpers  # noqa: E402
from tlslite.recordlayer import RecordLayer  # noqa: E402
from tlslite.utils.cryptomath import HKDF_expand_label, derive_secret, secureHMAC  # noqa: E402
from mocksock import MockSocket  # noqa: E402  (reference unit_tests/mocksock.py)

HASHES = [("sha256", 32), ("sha384", 48)]
IKM_LENGTHS = [1, 32, 48, 55, 56, 63, 64, 65, 66, 111, 112, 119, 120, 128, 239, 240, 256, 1024]
LABEL_LENGTHS = [0, 7, 10, 12, 13, 32]
CTX_LENGTHS = [0, 32, 48, 64]
SHORT_OUT = {"labellen": 12, "ctxlen": 32, "outlens": [1, 12]}
DERIVE_LABELS = [b"derived", b"c hs traffic", b"exp master", b"res master"]
# (PSK, shared-secret length) of the six connections: two of each kind share a length
CONNS = [(False, 32), (False, 32), (False, 66), (True, 48), (True, 48), (True, 256)]
SUITES = {"sha256": ["TLS_AES_128_GCM_SHA256", "TLS_CHACHA20_POLY1305_SHA256", "TLS_AES_128_CCM_SHA256",
                     "TLS_AES_128_CCM_8_SHA256"],
          "sha384": ["TLS_AES_256_GCM_SHA384"]}
PSK_LENGTHS = [16, 32, 48, 64]
NONCE_LENGTHS = [1, 8, 32]


def ba(label, n):
    return bytearray(detbytes(label, n))


def hh_of(label, n=300):
    """A HandshakeHashes that has seen n deterministic bytes."""
    hh = HandshakeHashes()
    hh.update(ba(label, n))
    return hh


def extract_cases(alg, hl):
    out = []
    for ikmlen in IKM_LENGTHS:
        got = secureHMAC(ba("k13-ext-salt-%s-%d" % (alg, ikmlen), hl), ba("k13-ext-ikm-%s-%d" % (alg, ikmlen), ikmlen),
                         alg)
        out.append({"hash": alg, "salt": "det", "ikm": "det", "ikmlen": ikmlen, "out": bytes(got).hex()})
    got = secureHMAC(bytearray(hl), ba("k13-ext-ikm-%s-%d" % (alg, 32), 32), alg)
    out.append({"hash": alg, "salt": "zero", "ikm": "det", "ikmlen": 32, "out": bytes(got).hex()})
    got = secureHMAC(ba("k13-ext-salt-%s-%d" % (alg, hl), hl), bytearray(hl), alg)
    out.append({"hash": alg, "salt": "det", "ikm": "zero", "ikmlen": hl, "out": bytes(got).hex()})
    return out


def expand_case(alg, hl, labellen, ctxlen, outlen):
    tag = "%s-%d-%d-%d" % (alg, labellen, ctxlen, outlen)
    got = HKDF_expand_label(ba("k13-exp-secret-" + tag, hl), ba("k13-exp-label-" + tag, labellen),
                            ba("k13-exp-ctx-" + tag, ctxlen), outlen, alg)
    return {"hash": alg, "labellen": labellen, "ctxlen": ctxlen, "outlen": outlen, "out": bytes(got).hex()}


def expand_cases(alg, hl):
    out = [expand_case(alg, hl, ll, cl, hl) for ll in LABEL_LENGTHS for cl in CTX_LENGTHS]
    out += [expand_case(alg, hl, SHORT_OUT["labellen"], SHORT_OUT["ctxlen"], ol) for ol in SHORT_OUT["outlens"]]
    return out


def derive_cases(alg, hl):
    out = []
    for label in DERIVE_LABELS:
        for transcript in (True, False):
            tag = "%s-%s-%d" % (alg, label.decode(), transcript)
            hh = hh_of("k13-der-transcript-" + tag) if transcript else None
            got = derive_secret(ba("k13-der-secret-" + tag, hl), bytearray(label), hh, alg)
            out.append({"hash": alg, "label": label.decode(), "transcript": transcript,
                        "digest": bytes(hh.digest(alg)).hex() if transcript else None, "out": bytes(got).hex()})
    return out


def cut(suite, client_secret, server_secret):
    """"key" and "iv" as calcTLS1_3PendingState installs them (recordlayer.py:1268-1323)."""
    rl = RecordLayer(MockSocket(bytearray(0)))
    rl.version = (3, 4)
    rl.client = True
    rl.calcTLS1_3PendingState(suite, client_secret, server_secret, None)
    w, r = rl._pendingWriteState, rl._pendingReadState
    return ({"key": bytes(w.encContext.key).hex(), "iv": bytes(w.fixedNonce).hex()},
            {"key": bytes(r.encContext.key).hex(), "iv": bytes(r.fixedNonce).hex()})


def schedule_case(alg, hl, c, with_psk, sharedlen):
    tag = "%s-c%d" % (alg, c)
    hexs = lambda b: bytes(b).hex()  # noqa: E731
    psk = ba("k13-sch-psk-" + tag, hl) if with_psk else bytearray(hl)
    shared = ba("k13-sch-shared-" + tag, sharedlen)
    # the transcript as the server sees it grow: ... ServerHello | ... CertificateVerify |
    # server Finished | client Finished
    hh = HandshakeHashes()
    hh.update(ba("k13-sch-hello-" + tag, 300))
    hello_hash = hh.digest(alg)
    # tlsconnection.py:3036-3050
    secret = bytearray(hl)
    secret = secureHMAC(secret, psk, alg)
    early = secret
    secret = derive_secret(secret, bytearray(b"derived"), None, alg)
    secret = secureHMAC(secret, shared, alg)
    handshake_secret = secret
    s_hs = derive_secret(secret, bytearray(b"s hs traffic"), hh, alg)
    c_hs = derive_secret(secret, bytearray(b"c hs traffic"), hh, alg)
    # :3203-3224
    hh.update(ba("k13-sch-cert-" + tag, 500))
    verify_hash = hh.digest(alg)
    finished_key = HKDF_expand_label(s_hs, b"finished", b"", hl, alg)
    server_finished = secureHMAC(finished_key, hh.digest(alg), alg)
    hh.update(bytearray([20, 0, 0, hl]) + server_finished)
    finished_hash = hh.digest(alg)
    secret = derive_secret(secret, bytearray(b"derived"), None, alg)
    secret = secureHMAC(secret, bytearray(hl), alg)
    master = secret
    c_ap = derive_secret(secret, bytearray(b"c ap traffic"), hh, alg)
    s_ap = derive_secret(secret, bytearray(b"s ap traffic"), hh, alg)
    # :3326-3360
    exp_master = derive_secret(secret, bytearray(b"exp master"), hh, alg)
    cl_finished_key = HKDF_expand_label(c_hs, b"finished", b"", hl, alg)
    client_finished = secureHMAC(cl_finished_key, hh.digest(alg), alg)
    hh.update(bytearray([20, 0, 0, hl]) + client_finished)
    resumption_hash = hh.digest(alg)
    res_master = derive_secret(secret, bytearray(b"res master"), hh, alg)
    keys = {}
    for name in SUITES[alg]:
        suite = getattr(CipherSuite, name)
        ch, sh = cut(suite, c_hs, s_hs)
        ca, sa = cut(suite, c_ap, s_ap)
        keys[name] = {"suite_id": suite, "c_hs": ch, "s_hs": sh, "c_ap": ca, "s_ap": sa}
    return {"hash": alg, "conn": c, "psk": with_psk, "sharedlen": sharedlen,
            "hello_hash": hexs(hello_hash), "verify_hash": hexs(verify_hash), "finished_hash": hexs(finished_hash),
            "resumption_hash": hexs(resumption_hash),
            "early": hexs(early), "handshake_secret": hexs(handshake_secret), "c_hs": hexs(c_hs), "s_hs": hexs(s_hs),
            "server_finished": hexs(server_finished), "master": hexs(master), "c_ap": hexs(c_ap), "s_ap": hexs(s_ap),
            "exp_master": hexs(exp_master), "client_finished": hexs(client_finished), "res_master": hexs(res_master),
            "keys": keys}


def binder_cases(alg, hl):
    out = []
    for psklen in PSK_LENGTHS:
        for external in (True, False):
            tag = "%s-%d-%d" % (alg, psklen, external)
            hh = hh_of("k13-bind-transcript-" + tag, 200)
            got = HandshakeHelpers._calc_binder(alg, ba("k13-bind-psk-" + tag, psklen), hh, external)
            out.append({"hash": alg, "psklen": psklen, "external": external, "digest": bytes(hh.digest(alg)).hex(),
                        "out": bytes(got).hex()})
    return out


class _Iden(object):
    def __init__(self, identity):
        self.identity = identity


class _Ticket(object):
    def __init__(self, ticket, nonce):
        self.ticket, self.ticket_nonce = ticket, nonce


def res_psk_cases(alg, hl):
    out = []
    for noncelen in NONCE_LENGTHS:
        tag = "%s-%d" % (alg, noncelen)
        tickets = [_Ticket(bytearray(b"other"), bytearray(b"xx")),
                   _Ticket(bytearray(b"ticket"), ba("k13-res-nonce-" + tag, noncelen))]
        got = HandshakeHelpers.calc_res_binder_psk(_Iden(bytearray(b"ticket")), ba("k13-res-master-" + tag, hl),
                                                   tickets)
        out.append({"hash": alg, "noncelen": noncelen, "out": bytes(got).hex()})
    return out


def main():
    doc = {"extract": [], "expand": [], "derive": [], "schedule": [], "binder": [], "res_psk": []}
    for alg, hl in HASHES:
        doc["extract"] += extract_cases(alg, hl)
        doc["expand"] += expand_cases(alg, hl)
        doc["derive"] += derive_cases(alg, hl)
        doc["schedule"] += [schedule_case(alg, hl, c, p, sl) for c, (p, sl) in enumerate(CONNS)]
        doc["binder"] += binder_cases(alg, hl)
        doc["res_psk"] += res_psk_cases(alg, hl)
    path = os.path.join(HERE, "tls13_schedule.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(HERE, "cbc.json"))
    print("wrote", ", ".join("%d %s" % (len(v), k) for k, v in sorted(doc.items())), "cases,",
          os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

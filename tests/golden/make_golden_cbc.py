"""AES-CBC + HMAC record fixtures, produced by the REFERENCE's RecordLayer.

TLS 1.1 / 1.2 block-cipher records, MAC-then-encrypt (recordlayer.py:476-498,
:680-719 with constanttime.py:102-204) and encrypt-then-MAC (:500-520,
:721-778).  Runs only in the build container through refloader; writes
tests/golden/cbc.json, which the tests replay without the reference.

    python tests/golden/make_golden_cbc.py

Seal cases come out of sendRecord.  The reference chains its CBC state through
the connection and sends a random block first, so bytes 5..21 of a wire record
are just a random first ciphertext block: the fixture records them as the
record's explicit IV.  The cipher and MAC keys are captured by wrapping
createAES / createHMAC in this generator's view of tlslite.recordlayer.

Open cases carry ``recv``: "ok" or the exception class the reference's
receiving RecordLayer raised for the record under its sequence number.  The
malformed ones are built here from the reference's own python_aes and hmac.
"""
import copy
import hashlib
import hmac
import json
import os
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import refloader  # noqa: E402
from vectors import detbytes  # noqa: E402

refloader.load()
import tlslite.recordlayer as reclayer  # noqa: E402
from tlslite.constants import CipherSuite  # noqa: E402
from tlslite.messages import Message  # noqa: E402
from tlslite.recordlayer import RecordLayer  # noqa: E402
from tlslite.utils import python_aes  # noqa: E402
from mocksock import MockSocket  # noqa: E402  (reference unit_tests/mocksock.py:7)

SUITES = [("TLS_RSA_WITH_AES_128_CBC_SHA", CipherSuite.TLS_RSA_WITH_AES_128_CBC_SHA, "sha1"),
          ("TLS_RSA_WITH_AES_256_CBC_SHA256", CipherSuite.TLS_RSA_WITH_AES_256_CBC_SHA256, "sha256"),
          ("TLS_ECDHE_RSA_WITH_AES_256_CBC_SHA384", CipherSuite.TLS_ECDHE_RSA_WITH_AES_256_CBC_SHA384,
           "sha384")]
DIGEST = {"sha1": 20, "sha256": 32, "sha384": 48}
CTYPES = [23, 22, 21]
LIMIT = 512            # recv_record_limit of the overflow cases (keeps them small)

captured = []
_createAES, _createHMAC = reclayer.createAES, reclayer.createHMAC


def _wrapAES(key, iv, implementations=None):
    captured.append(("aes", bytes(key)))
    return _createAES(key, iv, implementations)


def _wrapHMAC(k, digestmod=None):
    captured.append(("hmac", bytes(k)))
    return _createHMAC(k, digestmod=digestmod)


reclayer.createAES = _wrapAES
reclayer.createHMAC = _wrapHMAC


def seal_lengths(mac, etm):
    d = DIGEST[mac]
    base = 0 if etm else d
    # either side of the padding wrap: addPadding gives 0 at (base + L) % 16 == 15
    wrap = next(n for n in range(2, 40) if (base + n) % 16 == 15)
    lens = {0, 1, wrap, wrap + 1,
            42, 43, 50, 51,        # 13 + L = 55, 56, 63, 64 (SHA-1 / SHA-256 block ends)
            98, 99, 114, 115,      # 13 + L = 111, 112, 127, 128 (SHA-384)
            16383, 16384}
    # The EtM MAC input is 13 + 16 + roundup16(L + 1) = 29 mod 16 bytes long:
    # it never ends at one of those boundaries, so there is nothing to add.
    return sorted(lens)


def header(ctype, version, n):
    return bytes([ctype, version[0], version[1], n >> 8, n & 255])


def mac_of(mac, mac_key, seq, ctype, version, data):
    msg = struct.pack(">Q", seq) + bytes([ctype, version[0], version[1], len(data) >> 8, len(data) & 255])
    return hmac.new(mac_key, msg + bytes(data), getattr(hashlib, mac)).digest()


def cbc(enc_key, iv, plain):
    assert len(plain) % 16 == 0
    if not plain:
        return b""
    return bytes(python_aes.new(bytearray(enc_key), 2, bytearray(iv)).encrypt(bytearray(plain)))


def padded(data, padlen):
    return bytes(data) + bytes([padlen] * (padlen + 1))


def minpad(n):
    return 15 - n % 16


def receive(send_rl, wire, seq, limit=None):
    """What the reference's receiving RecordLayer does with one wire record."""
    sock = MockSocket(bytearray(wire))
    rl = RecordLayer(sock)
    rl.version = send_rl.version
    rl._readState = copy.copy(send_rl._writeState)
    rl._readState.seqnum = seq
    rl.client = not send_rl.client
    if limit is not None:
        rl.recv_record_limit = limit
    try:
        for result in rl.recvRecord():
            if result in (0, 1):
                return "blocked", None, None
            hdr, parser = result
            return "ok", hdr.type, bytes(parser.bytes)
    except Exception as e:   # noqa: BLE001 -- the reference's own exception is the fixture
        return type(e).__name__, None, None
    return "nothing", None, None


def open_case(send_rl, name, wire, seq, limit=None):
    recv, ctype, plain = receive(send_rl, wire, seq, limit)
    assert recv not in ("blocked", "nothing"), name
    c = {"name": name, "seq": seq, "recv_limit": limit or 0, "wire": bytes(wire).hex(), "recv": recv}
    if recv == "ok":
        c["ctype"] = ctype
        c["plain"] = plain.hex()
    return c


def flip(wire, pos, bit=1):
    b = bytearray(wire)
    b[pos] ^= bit
    return bytes(b)


def mte_open_cases(rl, mac, enc_key, mac_key, version):
    d = DIGEST[mac]
    out = []

    def build(seq, ctype, data, padlen=None, iv=None, hdr_type=None, body_plain=None):
        iv = iv or detbytes("iv-%d" % seq, 16)
        if body_plain is None:
            m = mac_of(mac, mac_key, seq, ctype, version, data)
            body_plain = padded(bytes(data) + m, minpad(len(data) + d) if padlen is None else padlen)
        body = iv + cbc(enc_key, iv, body_plain)
        return header(ctype if hdr_type is None else hdr_type, version, len(body)) + body

    data = detbytes("open-mte", 100)
    good = build(3, 23, data)
    out.append(open_case(rl, "valid", good, 3))
    out.append(open_case(rl, "valid empty", build(4, 22, b""), 4))
    out.append(open_case(rl, "flip last ciphertext block", flip(good, len(good) - 3), 3))
    out.append(open_case(rl, "flip first ciphertext block", flip(good, 21 + 2), 3))
    out.append(open_case(rl, "flip iv", flip(good, 5 + 7, 0x80), 3))
    # 64 + minimal padding bytes, one of them wrong
    longpad = minpad(len(data) + d) + 64
    m = mac_of(mac, mac_key, 3, 23, version, data)
    plain = bytearray(padded(data + m, longpad))
    out.append(open_case(rl, "valid long padding", build(3, 23, data, body_plain=bytes(plain)), 3))
    plain[len(plain) - 1 - longpad // 2] ^= 0x01
    out.append(open_case(rl, "wrong byte in the middle of the padding",
                         build(3, 23, data, body_plain=bytes(plain)), 3))
    # padding length byte larger than the record
    plain = bytearray(padded(data + m, minpad(len(data) + d)))
    plain[-1] = 200
    out.append(open_case(rl, "padding length larger than the data",
                         build(3, 23, data, body_plain=bytes(plain)), 3))
    # consistent padding that leaves fewer than a MAC's bytes in front: mac_start < 0
    n = 64
    padlen = n - 1 - 10
    plain = detbytes("short", 10) + bytes([padlen] * (padlen + 1))
    assert len(plain) == n
    out.append(open_case(rl, "padding pushes mac_start below 0",
                         build(3, 23, b"", body_plain=plain), 3))
    # every byte the same oversized padding value (pad_start clamps at 0)
    out.append(open_case(rl, "all bytes an oversized padding length",
                         build(3, 23, b"", body_plain=bytes([0x60] * 64)), 3))
    # 255 bytes of padding, valid
    d255 = detbytes("p255", next(k for k in range(40, 60) if (k + d + 256) % 16 == 0))
    out.append(open_case(rl, "valid 255 bytes of padding", build(7, 23, d255, padlen=255), 7))
    plain = bytearray(padded(d255 + mac_of(mac, mac_key, 7, 23, version, d255), 255))
    plain[len(d255) + d] ^= 0x40    # the first padding byte, 256 from the end
    out.append(open_case(rl, "255 bytes of padding, first one wrong",
                         build(7, 23, d255, body_plain=bytes(plain)), 7))
    # body lengths 0, 16, 32
    iv = detbytes("iv-b", 16)
    out.append(open_case(rl, "body 0", header(23, version, 0), 3))
    out.append(open_case(rl, "body 16", header(23, version, 16) + iv, 3))
    out.append(open_case(rl, "body 32", header(23, version, 32) + iv + detbytes("b32", 16), 3))
    out.append(open_case(rl, "body 16k + 8", header(23, version, 40) + iv + detbytes("b40", 24), 3))
    out.append(open_case(rl, "body 16k + 8, long",
                         header(23, version, len(good) - 5 + 8) + good[5:] + detbytes("x8", 8), 3))
    out.append(open_case(rl, "right MAC, wrong sequence number", good, 4))
    out.append(open_case(rl, "header type differs from the MAC'ed one", build(3, 23, data, hdr_type=22), 3))
    # limits (recv_record_limit = LIMIT)
    big = detbytes("big", LIMIT + 2048 - 16 - d - 16)
    w = build(9, 23, big)
    assert len(w) - 5 == LIMIT + 2048, len(w)
    out.append(open_case(rl, "header length at the limit", w, 9, LIMIT))
    w = build(9, 23, big + b"0123456789abcdef")
    assert len(w) - 5 == LIMIT + 2048 + 16
    out.append(open_case(rl, "header length over the limit", w, 9, LIMIT))
    out.append(open_case(rl, "plaintext at recv_limit", build(9, 23, detbytes("lim", LIMIT)), 9, LIMIT))
    out.append(open_case(rl, "plaintext of recv_limit + 1", build(9, 23, detbytes("lim1", LIMIT + 1)), 9, LIMIT))
    return out


def etm_open_cases(rl, mac, enc_key, mac_key, version):
    d = DIGEST[mac]
    out = []

    def build(seq, ctype, plain_body, iv=None, extra=b"", wrong_mac=False):
        iv = iv or detbytes("iv-%d" % seq, 16)
        buf = iv + cbc(enc_key, iv, plain_body) + extra
        m = mac_of(mac, mac_key, seq, ctype, version, buf)
        if wrong_mac:
            m = bytes([m[0] ^ 1]) + m[1:]
        body = buf + m
        return header(ctype, version, len(body)) + body

    data = detbytes("open-etm", 100)
    good = build(3, 23, padded(data, minpad(len(data))))
    out.append(open_case(rl, "valid", good, 3))
    out.append(open_case(rl, "valid empty", build(4, 21, padded(b"", 15)), 4))
    out.append(open_case(rl, "valid 255 bytes of padding", build(5, 23, padded(detbytes("e255", 16), 255)), 5))
    iv = detbytes("iv-b", 16)
    out.append(open_case(rl, "body shorter than the MAC", header(23, version, 16) + iv, 3))
    out.append(open_case(rl, "body 0", header(23, version, 0), 3))
    out.append(open_case(rl, "MAC mismatch: flipped ciphertext", flip(good, 21 + 5), 3))
    out.append(open_case(rl, "MAC mismatch: flipped MAC", flip(good, len(good) - 1), 3))
    out.append(open_case(rl, "right MAC, wrong sequence number", good, 4))
    out.append(open_case(rl, "right MAC over a misaligned body",
                         build(3, 23, padded(data, minpad(len(data))), extra=detbytes("x8", 8)), 3))
    out.append(open_case(rl, "wrong MAC over a misaligned body",
                         build(3, 23, padded(data, minpad(len(data))), extra=detbytes("x8", 8), wrong_mac=True), 3))
    out.append(open_case(rl, "right MAC, nothing after the IV", build(3, 23, b""), 3))
    plain = bytearray(padded(data, minpad(len(data)) + 32))
    plain[-10] ^= 0x04
    out.append(open_case(rl, "right MAC, bad padding bytes", build(3, 23, bytes(plain)), 3))
    plain = bytearray(padded(detbytes("e31", 31), 0))
    plain[-1] = 32
    out.append(open_case(rl, "right MAC, oversized padding length", build(3, 23, bytes(plain)), 3))
    # body = 16 + 16 k + d: the largest that is not over the limit, and the next
    big = detbytes("big", (LIMIT + 2048 - 32 - d) // 16 * 16)
    w = build(9, 23, padded(big, 15))
    assert LIMIT + 2048 - 16 < len(w) - 5 <= LIMIT + 2048, len(w)
    out.append(open_case(rl, "header length at the limit", w, 9, LIMIT))
    w = build(9, 23, padded(big + b"0123456789abcdef", 15))
    assert len(w) - 5 > LIMIT + 2048
    out.append(open_case(rl, "header length over the limit", w, 9, LIMIT))
    out.append(open_case(rl, "plaintext at recv_limit",
                         build(9, 23, padded(detbytes("lim", LIMIT), minpad(LIMIT))), 9, LIMIT))
    out.append(open_case(rl, "plaintext of recv_limit + 1",
                         build(9, 23, padded(detbytes("lim1", LIMIT + 1), minpad(LIMIT + 1))), 9, LIMIT))
    return out


def one_case(name, suite, mac, version, etm):
    del captured[:]
    sock = MockSocket(bytearray(0))
    rl = RecordLayer(sock)
    rl.version = version
    if etm:
        rl.encryptThenMAC = True
    tag = "%s-%d-%d" % (name, version[1], etm)
    rl.calcPendingStates(suite, detbytes("ms-" + tag, 48), detbytes("cr-" + tag, 32),
                         detbytes("sr-" + tag, 32), ['python'])
    rl.changeWriteState()
    rl.fixedIVBlock = bytearray(detbytes("fixed-iv-" + tag, 16))
    # the client's (= writer's) keys are created first (recordlayer.py:1223-1235)
    mac_key = next(k for t, k in captured if t == "hmac")
    enc_key = next(k for t, k in captured if t == "aes")
    assert rl._writeState.encryptThenMAC == bool(etm)
    assert rl._writeState.encContext.isBlockCipher and rl._writeState.encContext.implementation == "python"

    seal = []
    for i, n in enumerate(seal_lengths(mac, etm)):
        ctype = CTYPES[i % 3]
        data = detbytes("cbc-%d-%d" % (i, n), n)      # regenerated by the tests
        before = len(sock.sent)
        # sendRecord appends the MAC to the caller's bytearray in place: hand it a copy
        for _ in rl.sendRecord(Message(ctype, bytearray(data))):
            pass
        assert len(sock.sent) == before + 1
        wire = bytes(sock.sent[-1])
        rec = {"ctype": ctype, "len": n, "wire_len": len(wire), "iv": wire[5:21].hex(),
               "wire_sha256": hashlib.sha256(wire).hexdigest(),
               "wire_head": wire[:32].hex(), "wire_tail": wire[-16:].hex()}
        if len(wire) <= 300:
            rec["wire"] = wire.hex()
        recv, rtype, plain = receive(rl, wire, i)
        rec["recv"] = recv
        assert recv == "ok" and rtype == ctype and plain == bytes(data), (tag, n, recv)
        seal.append(rec)
    build = etm_open_cases if etm else mte_open_cases
    opens = build(rl, mac, enc_key, mac_key, version)
    return {"suite": name, "mac": mac, "version": list(version), "etm": etm, "seq0": 0,
            "enc_key": enc_key.hex(), "mac_key": mac_key.hex(), "seal": seal, "open": opens}


def main():
    out = []
    for name, suite, mac in SUITES:
        for etm in (0, 1):
            out.append(one_case(name, suite, mac, (3, 3), etm))
    name, suite, mac = SUITES[0]
    for etm in (0, 1):
        out.append(one_case(name, suite, mac, (3, 2), etm))
    for etm in (0, 1):
        seen = set(c["recv"] for case in out if case["etm"] == etm for c in case["open"])
        for want in ("ok", "TLSBadRecordMAC", "TLSDecryptionFailed", "TLSRecordOverflow"):
            assert want in seen, (etm, want, seen)
        assert seen <= {"ok", "TLSBadRecordMAC", "TLSDecryptionFailed", "TLSRecordOverflow"}, seen
    with open(os.path.join(HERE, "cbc.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote", len(out), "cases,", sum(len(c["seal"]) for c in out), "seal records,",
          sum(len(c["open"]) for c in out), "open records")


if __name__ == "__main__":
    main()

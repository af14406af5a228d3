"""Independent CPU model of the TLS 1.1 / 1.2 AES-CBC + HMAC record path.

CBC from the oracle's table AES (oracle.pyaead expand_key / aes_encrypt, and
a bytewise inverse cipher built from the same S-box), HMAC from hmac /
hashlib, and the framing rules of include/tlsgpu.h (tg_cbc_records):

    MtE   header || iv || CBC(data || MAC || padding)
    EtM   header || iv || CBC(data || padding) || MAC
    MAC input: be64(seq) || type || version(2) || be16(len) || bytes

``open_record`` follows the reference's order of checks (recordlayer.py
:219-220, :680-778, :980-981, constanttime.py:102-204) and returns the name of
the exception it raises, or "ok".  tests/test_cbc_oracle.py holds the model
against the reference's fixtures; the GPU tests then use it for shapes the
fixtures do not cover.
"""
import hashlib
import hmac
import struct

from oracle import pyaead

DIGEST = {"sha1": 20, "sha256": 32, "sha384": 48}
STATUS_CODE = {"ok": 0, "TLSBadRecordMAC": 1, "TLSRecordOverflow": 7, "TLSDecryptionFailed": 9}

_SBOX = pyaead._SBOX
_SI = [0] * 256
for _v, _s in enumerate(_SBOX):
    _SI[_s] = _v


def _mul(a, b):
    p = 0
    for _ in range(8):
        if b & 1:
            p ^= a
        a = ((a << 1) ^ (0x1b if a & 0x80 else 0)) & 0xff
        b >>= 1
    return p


_M9 = [_mul(x, 9) for x in range(256)]
_M11 = [_mul(x, 11) for x in range(256)]
_M13 = [_mul(x, 13) for x in range(256)]
_M14 = [_mul(x, 14) for x in range(256)]


def aes_decrypt(ks, block):
    """FIPS-197 5.3 InvCipher, bytewise (state[4 c + r] = row r, column c)."""
    nr, w = ks
    rk = [struct.pack(">4I", *w[4 * r:4 * r + 4]) for r in range(nr + 1)]
    s = [a ^ b for a, b in zip(bytes(block), rk[nr])]
    for r in range(nr - 1, -1, -1):
        t = [0] * 16
        for c in range(4):
            for row in range(4):
                t[4 * ((c + row) % 4) + row] = _SI[s[4 * c + row]]   # InvShiftRows + InvSubBytes
        s = [a ^ b for a, b in zip(t, rk[r])]
        if r:
            for c in range(4):
                a0, a1, a2, a3 = s[4 * c:4 * c + 4]
                s[4 * c:4 * c + 4] = [_M14[a0] ^ _M11[a1] ^ _M13[a2] ^ _M9[a3],
                                      _M9[a0] ^ _M14[a1] ^ _M11[a2] ^ _M13[a3],
                                      _M13[a0] ^ _M9[a1] ^ _M14[a2] ^ _M11[a3],
                                      _M11[a0] ^ _M13[a1] ^ _M9[a2] ^ _M14[a3]]
    return bytes(s)


def cbc_encrypt(enc_key, iv, plain):
    assert len(plain) % 16 == 0 and len(iv) == 16
    ks = pyaead.expand_key(enc_key)
    out, prev = bytearray(), bytes(iv)
    for k in range(0, len(plain), 16):
        prev = bytes(pyaead.aes_encrypt(ks, bytes(a ^ b for a, b in zip(plain[k:k + 16], prev))))
        out += prev
    return bytes(out)


def cbc_decrypt(enc_key, iv, ct):
    assert len(ct) % 16 == 0 and len(iv) == 16
    ks = pyaead.expand_key(enc_key)
    out, prev = bytearray(), bytes(iv)
    for k in range(0, len(ct), 16):
        cur = bytes(ct[k:k + 16])
        out += bytes(a ^ b for a, b in zip(aes_decrypt(ks, cur), prev))
        prev = cur
    return bytes(out)


def record_mac(mac, mac_key, seq, ctype, version, data):
    msg = struct.pack(">QBBBH", seq, ctype, version >> 8, version & 255, len(data))
    return hmac.new(bytes(mac_key), msg + bytes(data), getattr(hashlib, mac)).digest()


def _pad(n):
    padlen = 15 - n % 16                      # addPadding, recordlayer.py:453-461
    return bytes([padlen] * (padlen + 1))


def seal_record(enc_key, mac_key, mac, version, etm, seq, ctype, data, iv):
    data, iv = bytes(data), bytes(iv)
    if etm:
        buf = iv + cbc_encrypt(enc_key, iv, data + _pad(len(data)))
        body = buf + record_mac(mac, mac_key, seq, ctype, version, buf)
    else:
        plain = data + record_mac(mac, mac_key, seq, ctype, version, data)
        body = iv + cbc_encrypt(enc_key, iv, plain + _pad(len(plain)))
    return struct.pack(">BHH", ctype, version, len(body)) + body


def wire_len(mac, etm, n):
    d = DIGEST[mac]
    return 5 + 16 + ((n + 16) // 16 * 16 + d if etm else (n + d + 16) // 16 * 16)


def mte_check(mac_key, mac, version, seq, ctype, plain):
    """ct_check_cbc_mac_and_pad (constanttime.py:102-204) on the decrypted body
    behind the IV block of a MAC-then-encrypt record: the fragment, or None
    for TLSBadRecordMAC.  No cipher involved."""
    plain = bytes(plain)
    d, n = DIGEST[mac], len(plain)
    if d + 1 > n:
        return None
    padlen = plain[-1]
    pad_start = max(0, n - padlen - 1)
    mac_start = max(0, pad_start - d)
    bad = any(b != padlen for b in plain[max(pad_start, n - 256):])
    want = record_mac(mac, mac_key, seq, ctype, version, plain[:mac_start])
    bad |= not hmac.compare_digest(want, plain[mac_start:mac_start + d])
    return None if bad else plain[:mac_start]


def open_record(enc_key, mac_key, mac, version, etm, seq, wire, recv_limit=0):
    """(verdict, content type, plaintext) of one wire record."""
    wire = bytes(wire)
    if len(wire) < 5:                         # not even a header (tg_cbc_records: type 0, nothing written)
        return "TLSBadRecordMAC", 0, b""
    limit = recv_limit or 2 ** 14
    d = DIGEST[mac]
    ctype, hlen = wire[0], struct.unpack(">H", wire[3:5])[0]
    body = wire[5:]
    if hlen > limit + 2048 or len(body) > limit + 2048:
        return "TLSRecordOverflow", ctype, b""
    if etm:
        if len(body) < d:
            return "TLSBadRecordMAC", ctype, b""
        buf, check = body[:len(body) - d], body[len(body) - d:]
        if not hmac.compare_digest(record_mac(mac, mac_key, seq, ctype, version, buf), check):
            return "TLSBadRecordMAC", ctype, b""
        if len(buf) % 16:
            return "TLSDecryptionFailed", ctype, b""
        plain = cbc_decrypt(enc_key, buf[:16], buf[16:]) if len(buf) > 16 else b""
        if not plain:
            return "TLSBadRecordMAC", ctype, b""
        padlen = plain[-1]
        if padlen + 1 > len(plain) or any(b != padlen for b in plain[len(plain) - padlen - 1:]):
            return "TLSBadRecordMAC", ctype, b""
        data = plain[:len(plain) - padlen - 1]
    else:
        if len(body) % 16:
            return "TLSDecryptionFailed", ctype, b""
        plain = cbc_decrypt(enc_key, body[:16], body[16:]) if len(body) > 16 else b""
        data = mte_check(mac_key, mac, version, seq, ctype, plain)
        if data is None:
            return "TLSBadRecordMAC", ctype, b""
    if len(data) > limit:
        return "TLSRecordOverflow", ctype, b""
    return "ok", ctype, data

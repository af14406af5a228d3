"""TLS 1.1 / 1.2 AES-CBC + HMAC records on the device (tg_cbc_seal_records /
tg_cbc_open_records).

The block-cipher suites of tlslite/recordlayer.py -- AES-128 / AES-256 in CBC
mode with HMAC-SHA1 / -SHA256 / -SHA384 -- for a batch of consecutive records
of one connection direction (record i has sequence number ``seq0 + i``), as
MAC-then-encrypt (``_macThenEncrypt`` :476-498, ``_decryptThenMAC`` :680-719)
or encrypt-then-MAC (``_encryptThenMAC`` :500-520, ``_macThenDecrypt``
:721-778):

* seal: fragment + content type + a 16-byte explicit IV per record -> wire
  record ``header || iv || ciphertext``.  For TLS >= 1.1 the reference sends a
  random block first; its ciphertext is that IV, so records are independent.
* open: wire record -> plaintext, content type and a per-record status
  mirroring the reference's exceptions (``STATUS``: 0 ok, 1 bad_record_mac,
  7 record_overflow, 9 decryption_failed).  The data buffer needs room for
  ``wire_len[i] - 21`` bytes per record; a rejected record's extent is zero
  afterwards.

All buffers are device tensors (or raw device pointers).
"""
import ctypes

from . import _lib
from .batch import _ptr, _stream

MACS = {"sha1": _lib.TG_MAC_SHA1, "sha256": _lib.TG_MAC_SHA256, "sha384": _lib.TG_MAC_SHA384}
MAC_LENGTH = {"sha1": 20, "sha256": 32, "sha384": 48}
STATUS = _lib.REC_STATUS


class CbcKey(object):
    """One direction's cipher key and MAC key (tg_cbc_key_create): the AES
    schedules and the HMAC midstates live in device memory until ``close()``."""

    def __init__(self, enc_key, mac_key, mac):
        if mac not in MACS:
            raise ValueError("mac must be one of %s" % ", ".join(sorted(MACS)))
        enc_key, mac_key = bytes(enc_key), bytes(mac_key)
        self.mac = mac
        self.macLength = MAC_LENGTH[mac]
        self._lib = _lib.load()
        h = ctypes.c_void_p()
        _lib.check(self._lib.tg_cbc_key_create(enc_key, len(enc_key), mac_key, len(mac_key),
                                               MACS[mac], ctypes.byref(h)))
        self.handle = h

    def close(self):
        if self.handle is not None:
            self._lib.tg_cbc_key_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:   # noqa: BLE001 -- interpreter shutdown
            pass


def _records(n, version, etm, seq0, data, data_off, data_len, ctype, wire, wire_off, wire_len,
             iv=None, status=None, recv_limit=0):
    r = _lib.TgCbcRecords()
    r.n = int(n)
    r.version = int(version)
    r.etm = int(etm)
    r.recv_limit = int(recv_limit)
    r.seq0 = int(seq0)
    r.data = _ptr(data, "data")
    r.data_off = _ptr(data_off, "data_off")
    r.data_len = _ptr(data_len, "data_len")
    r.ctype = _ptr(ctype, "ctype")
    r.iv = _ptr(iv, "iv")
    r.wire = _ptr(wire, "wire")
    r.wire_off = _ptr(wire_off, "wire_off")
    r.wire_len = _ptr(wire_len, "wire_len")
    r.status = _ptr(status, "status")
    return r


def _key(key):
    if not isinstance(key, CbcKey) or key.handle is None:
        raise TypeError("key must be an open tlsgpu.CbcKey")
    return key


def seal_records(key, version, etm, seq0, n, data, data_off, data_len, ctype, iv, wire, wire_off,
                 wire_len, stream=None):
    """MAC, pad and encrypt ``n`` records (``etm``: encrypt-then-MAC); ``iv``
    holds 16 bytes per record and ``wire_len`` receives each record's size."""
    k = _key(key)
    r = _records(n, version, etm, seq0, data, data_off, data_len, ctype, wire, wire_off, wire_len,
                 iv=iv)
    _lib.check(k._lib.tg_cbc_seal_records(k.handle, ctypes.byref(r), _stream(stream)))


def open_records(key, version, etm, seq0, n, data, data_off, data_len, ctype, status, wire,
                 wire_off, wire_len, stream=None, recv_limit=0):
    """Decrypt and check ``n`` wire records; per-record ``status`` codes are in
    ``STATUS`` (0 = ok).  ``recv_limit``: the connection's recv_record_limit
    (0 = 2^14, recordlayer.py:56)."""
    k = _key(key)
    r = _records(n, version, etm, seq0, data, data_off, data_len, ctype, wire, wire_off, wire_len,
                 status=status, recv_limit=recv_limit)
    _lib.check(k._lib.tg_cbc_open_records(k.handle, ctypes.byref(r), _stream(stream)))

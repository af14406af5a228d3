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

The pending records of MANY connections of one suite go through one call
with a key table (``CbcKey.table``), a session index per record and explicit
numbers or per-session counters (``seal_session_records`` /
``open_session_records``, ``CbcSessions``; tg_cbc_seal_session_records /
tg_cbc_open_session_records).

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

    @classmethod
    def table(cls, enc_keys, mac_keys, mac):
        """One direction of many connections of one suite
        (tg_cbc_key_create_table): ``enc_keys`` and ``mac_keys`` are sequences
        of byte strings, one pair per session, all cipher keys of one length
        and all MAC keys of one length.  Entry ``s`` serves the records whose
        session index is ``s`` (``CbcSessions``, ``seal_session_records``)."""
        if mac not in MACS:
            raise ValueError("mac must be one of %s" % ", ".join(sorted(MACS)))
        enc, keylen, mk, mackeylen, n = _key_rows(enc_keys, mac_keys)
        if n == 0:
            raise ValueError("a key table needs at least one key")
        self = cls.__new__(cls)
        self.mac = mac
        self.macLength = MAC_LENGTH[mac]
        self._lib = _lib.load()
        self.handle = None
        h = ctypes.c_void_p()
        _lib.check(self._lib.tg_cbc_key_create_table(enc, keylen, mk, mackeylen, MACS[mac], n,
                                                     ctypes.byref(h)))
        self.handle = h
        return self

    @classmethod
    def table_from_device(cls, enc_keys, mac_keys, mac, stream=None):
        """``table`` with the keys already in device memory
        (tg_cbc_key_create_device): ``enc_keys`` (n x 16 or n x 32) and
        ``mac_keys`` (n x MAC key length) are 2-D device uint8 tensors; the
        rows are built by a kernel on ``stream``, no key visits the host."""
        if mac not in MACS:
            raise ValueError("mac must be one of %s" % ", ".join(sorted(MACS)))
        n, keylen, mackeylen = _device_rows(enc_keys, mac_keys)
        if n == 0:
            raise ValueError("a key table needs at least one key")
        self = cls.__new__(cls)
        self.mac = mac
        self.macLength = MAC_LENGTH[mac]
        self._lib = _lib.load()
        self.handle = None
        h = ctypes.c_void_p()
        _lib.check(self._lib.tg_cbc_key_create_device(_ptr(enc_keys, "enc_keys"), keylen,
                                                      _ptr(mac_keys, "mac_keys"), mackeylen, MACS[mac], n,
                                                      ctypes.byref(h), _stream(stream)))
        self.handle = h
        return self

    def replace_device(self, slots, enc_keys, mac_keys, stream=None):
        """``replace`` with everything in device memory
        (tg_cbc_key_replace_device): ``slots`` is a device int32 tensor, host
        integers (uploaded) or ``None`` (the first n entries); kernels on
        ``stream`` and nothing else -- no host synchronisation, no staging."""
        from .batch import _slot_list
        n, keylen, mackeylen = _device_rows(enc_keys, mac_keys)
        slots, ns = _slot_list(slots, n)
        if ns != n:
            raise ValueError("one slot per key pair")
        if n and keylen != self._keylen():
            raise ValueError("cipher keys must have the table's length (%d)" % self._keylen())
        self._replace_args = (slots, enc_keys, mac_keys)   # alive until the next call at least
        _lib.check(self._lib.tg_cbc_key_replace_device(_key(self).handle, _ptr(slots, "slots"),
                                                       _ptr(enc_keys, "enc_keys"), _ptr(mac_keys, "mac_keys"),
                                                       mackeylen, n, _stream(stream)))

    @property
    def nkeys(self):
        """Entries of the handle (1 for a key made by the constructor)."""
        n = ctypes.c_size_t(0)
        _lib.check(self._lib.tg_cbc_key_info(_key(self).handle, None, None, ctypes.byref(n)))
        return n.value

    def replace(self, slots, enc_keys, mac_keys, stream=None):
        """New keys for the entries ``slots`` (host integers, distinct; ``None``
        = the first ``len(enc_keys)``) of the live table (tg_cbc_key_replace):
        pair j becomes entry ``slots[j]``; a slot that is not below ``nkeys``
        is skipped.  Ordered on ``stream``: batches enqueued there before the
        call use the old keys, batches after it the new ones."""
        enc, keylen, mk, mackeylen, n = _key_rows(enc_keys, mac_keys)
        arr = None
        if slots is not None:
            slots = [int(x) for x in slots]
            if len(slots) != n:
                raise ValueError("one slot per key pair")
            arr = (ctypes.c_uint32 * n)(*slots)
        if n and keylen != self._keylen():
            raise ValueError("cipher keys must have the table's length (%d)" % self._keylen())
        _lib.check(self._lib.tg_cbc_key_replace(_key(self).handle, arr, enc, mk, mackeylen, n,
                                                _stream(stream)))

    def _keylen(self):
        n = ctypes.c_size_t(0)
        _lib.check(self._lib.tg_cbc_key_info(_key(self).handle, ctypes.byref(n), None, None))
        return n.value

    def close(self):
        if self.handle is not None:
            self._lib.tg_cbc_key_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:   # noqa: BLE001 -- interpreter shutdown
            pass


def _key_rows(enc_keys, mac_keys):
    """``(cipher keys packed, keylen, MAC keys packed, mackeylen, n)``."""
    enc = [bytes(k) for k in enc_keys]
    mk = [bytes(k) for k in mac_keys]
    if len(enc) != len(mk):
        raise ValueError("one MAC key per cipher key")
    if len(set(map(len, enc))) > 1 or len(set(map(len, mk))) > 1:
        raise ValueError("the keys of a table have one length (one suite per table)")
    return (b"".join(enc), len(enc[0]) if enc else 0, b"".join(mk), len(mk[0]) if mk else 0, len(enc))


def _device_rows(enc_keys, mac_keys):
    """``(n, keylen, mackeylen)`` of two 2-D device key tensors."""
    if enc_keys.ndim != 2 or mac_keys.ndim != 2 or enc_keys.shape[0] != mac_keys.shape[0]:
        raise ValueError("enc_keys and mac_keys must be 2-D with one row per session")
    return enc_keys.shape[0], enc_keys.shape[1], mac_keys.shape[1]


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


def _session_records(key, n, version, etm, session, seq, seq_next, seq_out, data, data_off, data_len,
                     ctype, wire, wire_off, wire_len, iv=None, status=None, recv_limit=0):
    r = _lib.TgCbcSessionRecords()
    r.n = int(n)
    r.version = int(version)
    r.etm = int(etm)
    r.recv_limit = int(recv_limit)
    r.nsessions = key.nkeys
    r.session = _ptr(session, "session")
    r.seq = _ptr(seq, "seq")
    r.seq_next = _ptr(seq_next, "seq_next")
    r.seq_out = _ptr(seq_out, "seq_out")
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


def seal_session_records(key, version, etm, session, n, data, data_off, data_len, ctype, iv, wire,
                         wire_off, wire_len, seq=None, seq_next=None, seq_out=None, stream=None):
    """``seal_records`` for the records of many sessions
    (tg_cbc_seal_session_records): record i uses entry ``session[i]`` of the
    table ``key`` and the number ``seq[i]``, or -- with ``seq_next``, one
    device int64 counter per entry -- the session's counter plus the record's
    rank among the session's records of the batch; the counters advance.  A
    record whose session is out of range is skipped (``wire_len[i] = 0``)."""
    k = _key(key)
    r = _session_records(k, n, version, etm, session, seq, seq_next, seq_out, data, data_off, data_len,
                         ctype, wire, wire_off, wire_len, iv=iv)
    _lib.check(k._lib.tg_cbc_seal_session_records(k.handle, ctypes.byref(r), _stream(stream)))


def open_session_records(key, version, etm, session, n, wire, wire_off, wire_len, data, data_off,
                         data_len, ctype, status, seq=None, seq_next=None, seq_out=None, stream=None,
                         recv_limit=0):
    """``open_records`` for the records of many sessions
    (tg_cbc_open_session_records); every in-range record consumes a number
    whatever its status, a record whose session is out of range gets status 8
    (bad_session) and consumes none."""
    k = _key(key)
    r = _session_records(k, n, version, etm, session, seq, seq_next, seq_out, data, data_off, data_len,
                         ctype, wire, wire_off, wire_len, status=status, recv_limit=recv_limit)
    _lib.check(k._lib.tg_cbc_open_session_records(k.handle, ctypes.byref(r), _stream(stream)))


class CbcSessions(object):
    """Many sessions' CBC record-layer state for one direction: the key table
    and one sequence counter per session on the device -- ``Sessions`` for the
    block-cipher suites.  ``seal`` / ``open`` take a batch that interleaves the
    pending records of any of the sessions; without ``seq`` each session's
    records are numbered in batch order from its counter, which advances
    (``getSeqNumBytes`` per record)."""

    def __init__(self, table, version, etm, seq_next=None, cipher_suite=None):
        """``cipher_suite``: the TLS 1.2 suite of the sessions -- what
        ``install`` derives new connections' keys by."""
        import torch
        self.cipher_suite = cipher_suite
        if not isinstance(table, CbcKey) or table.handle is None:
            raise TypeError("table must be an open tlsgpu.CbcKey")
        n = table.nkeys
        if seq_next is None:
            seq_next = torch.zeros(n, dtype=torch.int64, device="cuda")
        elif seq_next.numel() != n or seq_next.dtype != torch.int64:
            raise ValueError("seq_next must hold one int64 counter per key of the table")
        self.table, self.version, self.etm, self.seq_next = table, int(version), int(etm), seq_next

    @classmethod
    def from_master_secrets(cls, cipher_suite, master_secrets, client_random, server_random, side,
                            version=_lib.TG_TLS12, etm=0, stream=None):
        """One direction (``side``: "client" or "server" write keys) of many
        TLS 1.2 sessions of a CBC suite from their master secrets (n x 48
        device bytes) and randoms (n x 32 each), as calcPendingStates derives
        them (recordlayer.py:1189-1246); counters at 0.  The raw keys exist in
        registers only (tg_cbc_sessions_install_tls12).  With ``version``
        TLS 1.1 the keys come from the MD5 xor SHA-1 PRF
        (tg_cbc_sessions_install_tls11), for the HMAC-SHA1 suites with AES-128
        / AES-256; any other suite at TLS 1.1 is a ValueError."""
        import torch
        from . import keysetup
        alg, keylen, _, mac, maclen, _ = keysetup.tls12_suite(cipher_suite)
        if mac is None:
            raise ValueError("suite 0x%04x is an AEAD suite: use Sessions.from_master_secrets" % cipher_suite)
        if int(version) == _lib.TG_TLS11:
            keysetup.tls11_suite(cipher_suite)
        elif int(version) != _lib.TG_TLS12:
            raise ValueError("only TLS 1.2 keys are derived on the device")
        n = master_secrets.numel() // 48
        dev = master_secrets.device
        # the blank keys and counters are filled on ``stream``, where the table
        # build and the install that overwrite them run
        with torch.cuda.stream(keysetup.torch_stream(stream)):
            blank_enc = torch.zeros((n, keylen), dtype=torch.uint8, device=dev)
            blank_mac = torch.zeros((n, maclen), dtype=torch.uint8, device=dev)
            seq_next = torch.zeros(n, dtype=torch.int64, device=dev)
        table = CbcKey.table_from_device(blank_enc, blank_mac, mac, stream=stream)
        self = cls(table, version, etm, seq_next=seq_next, cipher_suite=cipher_suite)
        self.install(None, master_secrets, client_random, server_random, side, stream=stream)
        return self

    def install(self, slots, master_secrets, client_random, server_random, side, stream=None):
        """New connections of the sessions' version (TLS 1.2, or TLS 1.1 for
        an HMAC-SHA1 suite) take the sessions ``slots`` (distinct; a
        device int32 tensor, host integers, or ``None`` = the first n): row j
        of the three inputs belongs to ``slots[j]``; the table row is rebuilt
        from the key block's slices of ``side`` and the counter restarts at 0,
        in place and ordered on ``stream`` only."""
        from . import keysetup
        from .batch import _slot_list
        tls11 = self.version == _lib.TG_TLS11 and self.cipher_suite is not None
        if tls11:
            keysetup.tls11_suite(self.cipher_suite)
        elif self.version != _lib.TG_TLS12 or self.cipher_suite not in keysetup.TLS12_SUITES:
            raise ValueError("install needs TLS 1.2 sessions with their cipher_suite")
        slots, n = _slot_list(slots, master_secrets.numel() // 48)
        r = keysetup.tls12_install_args(n, keysetup.TLS12_SUITES[self.cipher_suite][5], side, len(self), slots,
                                        master_secrets, client_random, server_random, seq_next=self.seq_next)
        self._install_args = (slots, master_secrets, client_random, server_random)   # alive until the next call
        k = _key(self.table)
        fn = k._lib.tg_cbc_sessions_install_tls11 if tls11 else k._lib.tg_cbc_sessions_install_tls12
        _lib.check(fn(k.handle, ctypes.byref(r), _stream(stream)))

    def __len__(self):
        return self.seq_next.numel()

    def seq(self):
        """The per-session sequence counters (device int64 tensor)."""
        return self.seq_next

    def replace(self, slots, enc_keys, mac_keys, stream=None):
        """New connections take the sessions ``slots`` (``CbcKey.replace``) and
        their counters restart at 0, both ordered on ``stream``."""
        import torch
        enc_keys, mac_keys = list(enc_keys), list(mac_keys)
        slots = list(range(len(enc_keys))) if slots is None else [int(s) for s in slots]
        self.table.replace(slots, enc_keys, mac_keys, stream=stream)
        n = len(self)
        idx = [s for s in slots if 0 <= s < n]
        if not idx:
            return
        ts = stream if hasattr(stream, "cuda_stream") else (
            torch.cuda.ExternalStream(int(stream)) if stream else torch.cuda.current_stream())
        with torch.cuda.stream(ts):
            at = torch.tensor(idx, dtype=torch.int64).to(self.seq_next.device, non_blocking=False)
            self.seq_next.index_fill_(0, at, 0)

    def seal(self, session, n, data, data_off, data_len, ctype, iv, wire, wire_off, wire_len,
             seq=None, seq_out=None, stream=None):
        seal_session_records(self.table, self.version, self.etm, session, n, data, data_off, data_len,
                             ctype, iv, wire, wire_off, wire_len, seq=seq,
                             seq_next=None if seq is not None else self.seq_next, seq_out=seq_out,
                             stream=stream)

    def open(self, session, n, wire, wire_off, wire_len, data, data_off, data_len, ctype, status,
             seq=None, seq_out=None, stream=None, recv_limit=0):
        open_session_records(self.table, self.version, self.etm, session, n, wire, wire_off, wire_len,
                             data, data_off, data_len, ctype, status, seq=seq,
                             seq_next=None if seq is not None else self.seq_next, seq_out=seq_out,
                             stream=stream, recv_limit=recv_limit)

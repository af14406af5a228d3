"""Many sessions' record-layer state for one direction, all of it on the device.

What ``ConnectionState`` (tlslite/recordlayer.py:240-262) holds for one
connection -- ``encContext``, ``fixedNonce``, ``seqnum`` -- held for many:
a key table, the fixed-IV table and one sequence counter per session.
``seal`` / ``open`` frame a batch that interleaves the pending records of any
of the sessions (tg_seal_session_records / tg_open_session_records in counter
mode): each session's records are numbered in batch order and its counter
advances, as ``getSeqNumBytes`` does per record.

The state is live: ``key_update`` advances chosen sessions as a TLS 1.3
KeyUpdate does (``_calcTLS1_3KeyUpdate``, recordlayer.py:1325-1349) and
``install`` hands a slot to a new connection, both in place and ordered on
the stream only (tg_sessions_rekey).

This is the thin state holder only; gathering records from many sockets is
the caller's business.
"""
import ctypes

from . import _lib, keysetup, records
from .batch import KeyTable, _ptr, _slot_list, _stream


class Sessions(object):
    def __init__(self, table, ivs, version=records.TLS13, seq_next=None, secrets=None,
                 cipher_suite=None):
        """``table``: a KeyTable; ``ivs``: device uint8 tensor, one row (4 or
        12 bytes) per key; ``seq_next``: device int64 counters (default 0);
        ``secrets`` / ``cipher_suite``: the TLS 1.3 traffic secrets the table
        was derived from (device uint8, one row per key) and their suite --
        what ``key_update`` advances."""
        import torch
        if not isinstance(table, KeyTable):
            raise TypeError("table must be a KeyTable")
        if ivs.ndim != 2 or ivs.shape[0] != table.nkeys:
            raise ValueError("ivs must have one row per key of the table")
        if seq_next is None:
            seq_next = torch.zeros(table.nkeys, dtype=torch.int64, device=ivs.device)
        elif seq_next.numel() != table.nkeys or seq_next.dtype != torch.int64:
            raise ValueError("seq_next must hold one int64 counter per key of the table")
        self.table, self.ivs, self.version, self.seq_next = table, ivs, int(version), seq_next
        self.cipher_suite = cipher_suite
        self.hashlen = None
        if cipher_suite in keysetup.TLS13_SUITES:
            self.hashlen = keysetup.TLS13_SUITES[cipher_suite][2]
        elif cipher_suite in keysetup.TLS12_SUITES:
            self.hashlen = keysetup.TLS12_SUITES[cipher_suite][5]   # install_tls12; _rekey refuses TLS 1.2
        elif cipher_suite is not None:
            raise ValueError("cipher suite 0x%04x is in neither TLS13_SUITES nor TLS12_SUITES" % cipher_suite)
        if secrets is not None:
            if self.hashlen is None:
                raise ValueError("secrets need their cipher_suite")
            if secrets.numel() != table.nkeys * self.hashlen:
                raise ValueError("secrets must have one %d-byte row per key of the table" % self.hashlen)
        self.secrets = secrets

    @classmethod
    def from_traffic_secrets(cls, cipher_suite, secrets, stream=None):
        """One direction of many TLS 1.3 sessions from their traffic secrets
        (n x hash length device bytes), as calcTLS1_3PendingState derives key
        and IV (recordlayer.py:1291-1312); counters start at 0.  Keys, IVs and
        the key table never leave device memory.  A device copy of the secrets
        stays with the object (``secrets``) for ``key_update``."""
        table, _, ivs = keysetup.traffic_keys(cipher_suite, secrets, stream=stream)
        hashlen = keysetup.TLS13_SUITES[cipher_suite][2]
        return cls(table, ivs, records.TLS13, secrets=secrets.reshape(-1, hashlen).clone(),
                   cipher_suite=cipher_suite)

    @classmethod
    def from_master_secrets(cls, cipher_suite, master_secrets, client_random, server_random, side,
                            stream=None):
        """One direction (``side``: "client" or "server" write keys) of many
        TLS 1.2 sessions of an AEAD suite from their master secrets (n x 48
        device bytes) and randoms (n x 32 each), as calcPendingStates derives
        them (recordlayer.py:1189-1246); IV rows of 4 or 12 bytes, counters at
        0.  The raw keys exist in registers only (tg_sessions_install_tls12)."""
        import torch
        alg, keylen, ivlen, mac, _, _ = keysetup.tls12_suite(cipher_suite)
        if mac is not None:
            raise ValueError("suite 0x%04x is a CBC suite: use CbcSessions.from_master_secrets" % cipher_suite)
        n = master_secrets.numel() // 48
        dev = master_secrets.device
        # the blank key, IV and counter tensors are filled on ``stream``, where
        # the table build and the install that overwrite them run
        with torch.cuda.stream(keysetup.torch_stream(stream)):
            blank = torch.zeros((n, keylen), dtype=torch.uint8, device=dev)
            ivs = torch.zeros((n, ivlen), dtype=torch.uint8, device=dev)
            seq_next = torch.zeros(n, dtype=torch.int64, device=dev)
        table = KeyTable.from_device(alg, blank, n, keylen, stream=stream)
        self = cls(table, ivs, records.TLS12, seq_next=seq_next, cipher_suite=cipher_suite)
        self.install_tls12(None, master_secrets, client_random, server_random, side, stream=stream)
        return self

    def install_tls12(self, slots, master_secrets, client_random, server_random, side, stream=None):
        """New TLS 1.2 connections take the sessions ``slots`` (distinct; as
        ``key_update`` takes them, ``None`` = the first n): row j of the three
        inputs belongs to ``slots[j]``.  Key-table entry and fixed IV are cut
        from the key block, the counter restarts at 0, in place and ordered on
        ``stream`` only."""
        if self.version != records.TLS12 or self.cipher_suite not in keysetup.TLS12_SUITES:
            raise ValueError("install_tls12 needs TLS 1.2 Sessions with their cipher_suite")
        slots, n = _slot_list(slots, master_secrets.numel() // 48)
        r = keysetup.tls12_install_args(n, self.hashlen, side, self.table.nkeys, slots, master_secrets,
                                        client_random, server_random, fixed_iv_len=self.ivs.shape[1],
                                        iv_table=self.ivs, seq_next=self.seq_next)
        self._rekey_args = (slots, master_secrets, client_random, server_random)   # alive until the next call
        dk = self.table._dkey
        _lib.check(dk._lib.tg_sessions_install_tls12(dk.handle, ctypes.byref(r), _stream(stream)))

    def __len__(self):
        return self.table.nkeys

    def seq(self):
        """The per-session sequence counters (device int64 tensor)."""
        return self.seq_next

    def _need_tls13(self):
        """TLS 1.2 Sessions also know a PRF hash (for ``install_tls12``): they
        must never reach the TLS 1.3 HKDF with it."""
        if self.version != records.TLS13 or self.ivs.shape[1] != 12:
            raise ValueError("rekeying derives TLS 1.3 keys and 12-byte IVs")

    def _rekey(self, mode, slots, new_secrets, n, stream):
        self._need_tls13()
        r = _lib.TgRekey()
        r.n, r.mode, r.hashlen, r.nsessions = n, mode, self.hashlen, self.table.nkeys
        r.slot = _ptr(slots, "slots")
        r.new_secrets = _ptr(new_secrets, "secrets")
        r.secrets = _ptr(self.secrets, "secrets")
        r.iv_table = _ptr(self.ivs, "ivs")
        r.seq_next = _ptr(self.seq_next, "seq_next")
        self._rekey_args = (slots, new_secrets)   # alive until the next call at least
        dk = self.table._dkey
        _lib.check(dk._lib.tg_sessions_rekey(dk.handle, ctypes.byref(r), _stream(stream)))

    def key_update(self, slots, stream=None):
        """TLS 1.3 KeyUpdate of the sessions ``slots`` (distinct; a device
        int32 tensor, host integers, or ``None`` for all): the secret advances
        with "traffic upd", key-table entry and IV are re-derived from it and
        the sequence counter restarts at 0, as calcTLS1_3KeyUpdate_sender /
        _reciever install a fresh ConnectionState (recordlayer.py:1351-1375).
        In place and ordered on ``stream`` only: batches enqueued before the
        call use the old keys, batches after it the new ones."""
        self._need_tls13()
        if self.secrets is None:
            raise ValueError("these Sessions were built without traffic secrets: nothing to advance")
        slots, n = _slot_list(slots, self.table.nkeys)
        self._rekey(_lib.TG_REKEY_UPDATE, slots, None, n, stream)

    def install(self, slots, secrets, stream=None):
        """New connections take the sessions ``slots``: row j of ``secrets``
        (n x hash length device bytes) is the traffic secret of ``slots[j]``;
        key, IV and counter as ``from_traffic_secrets`` gives a new session."""
        self._need_tls13()
        if self.hashlen is None:
            raise ValueError("these Sessions have no cipher_suite: the PRF hash is unknown")
        slots, n = _slot_list(slots, secrets.numel() // self.hashlen)
        if secrets.numel() != n * self.hashlen:
            raise ValueError("secrets must hold one %d-byte row per slot" % self.hashlen)
        self._rekey(_lib.TG_REKEY_INSTALL, slots, secrets, n, stream)

    def _need_tls13_suite(self):
        self._need_tls13()
        if self.cipher_suite not in keysetup.TLS13_SUITES:
            raise ValueError("the TLS 1.3 key schedule needs Sessions with their TLS 1.3 cipher_suite")

    def install_handshake(self, slots, shared, hello_hash, side, psk=None, stream=None):
        """New TLS 1.3 connections take the sessions ``slots`` with their
        HANDSHAKE traffic keys: row j of ``shared`` ((EC)DHE shared secrets, n
        x 1..1024 device bytes), ``hello_hash`` (the transcript hash through
        ServerHello) and ``psk`` (optional), n x hash length each, belongs to
        ``slots[j]``.  The handshake stage of the schedule
        (``keysetup.tls13_handshake_secrets``, tlsconnection.py:3036-3050) and
        then ``install`` of the traffic secrets of ``side`` ("client" / "server"
        write keys, as ``keysetup.tls12_side`` takes it) on the same stream:
        table entry, IV row, secret row, counter 0.  Returns the handshake
        secrets (n x hash length), for ``install_application``."""
        self._need_tls13_suite()
        side = keysetup.tls12_side(side)
        hs, client, server = keysetup.tls13_handshake_secrets(self.cipher_suite, shared, hello_hash, psk=psk,
                                                              stream=stream)
        self.install(slots, server if side == keysetup.SERVER_WRITE else client, stream=stream)
        return hs

    def install_application(self, slots, handshake_secrets, finished_hash, side, stream=None):
        """The sessions ``slots`` move on to their APPLICATION traffic keys:
        the application stage (``keysetup.tls13_application_secrets``,
        tlsconnection.py:3218-3224) from row j of ``handshake_secrets`` and of
        ``finished_hash`` (the transcript hash through the server's Finished),
        then ``install`` of the traffic secrets of ``side`` on the same stream.
        Returns the master secrets (n x hash length): "res master" is
        ``keysetup.derive_secret`` of them once the client's Finished is in
        the transcript."""
        self._need_tls13_suite()
        side = keysetup.tls12_side(side)
        master, client, server, _ = keysetup.tls13_application_secrets(self.cipher_suite, handshake_secrets,
                                                                       finished_hash, stream=stream)
        self.install(slots, server if side == keysetup.SERVER_WRITE else client, stream=stream)
        return master

    def seal(self, session, n, data, data_off, data_len, ctype, wire, wire_off, wire_len,
             pad_len=None, seq_out=None, stream=None):
        records.seal_session_records(self.table, self.version, self.ivs, session, n, data, data_off,
                                     data_len, ctype, wire, wire_off, wire_len,
                                     seq_next=self.seq_next, seq_out=seq_out, pad_len=pad_len,
                                     stream=stream)

    def open(self, session, n, wire, wire_off, wire_len, data, data_off, data_len, ctype, status,
             seq_out=None, stream=None, recv_limit=0):
        records.open_session_records(self.table, self.version, self.ivs, session, n, wire, wire_off,
                                     wire_len, data, data_off, data_len, ctype, status,
                                     seq_next=self.seq_next, seq_out=seq_out, stream=stream,
                                     recv_limit=recv_limit)

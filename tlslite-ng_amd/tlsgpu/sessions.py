"""Many sessions' record-layer state for one direction, all of it on the device.

What ``ConnectionState`` (tlslite/recordlayer.py:240-262) holds for one
connection -- ``encContext``, ``fixedNonce``, ``seqnum`` -- held for many:
a key table, the fixed-IV table and one sequence counter per session.
``seal`` / ``open`` frame a batch that interleaves the pending records of any
of the sessions (tg_seal_session_records / tg_open_session_records in counter
mode): each session's records are numbered in batch order and its counter
advances, as ``getSeqNumBytes`` does per record.

This is the thin state holder only; gathering records from many sockets is
the caller's business.
"""
from . import keysetup, records
from .batch import KeyTable


class Sessions(object):
    def __init__(self, table, ivs, version=records.TLS13, seq_next=None):
        """``table``: a KeyTable; ``ivs``: device uint8 tensor, one row (4 or
        12 bytes) per key; ``seq_next``: device int64 counters (default 0)."""
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

    @classmethod
    def from_traffic_secrets(cls, cipher_suite, secrets, stream=None):
        """One direction of many TLS 1.3 sessions from their traffic secrets
        (n x hash length device bytes), as calcTLS1_3PendingState derives key
        and IV (recordlayer.py:1291-1312); counters start at 0.  Keys, IVs and
        the key table never leave device memory."""
        table, _, ivs = keysetup.traffic_keys(cipher_suite, secrets, stream=stream)
        return cls(table, ivs, records.TLS13)

    def __len__(self):
        return self.table.nkeys

    def seq(self):
        """The per-session sequence counters (device int64 tensor)."""
        return self.seq_next

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

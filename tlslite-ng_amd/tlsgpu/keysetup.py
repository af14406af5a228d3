"""Bulk TLS 1.3 key setup on the device.

What ``RecordLayer.calcTLS1_3PendingState`` (tlslite/recordlayer.py:1268-1323)
and ``_calcTLS1_3KeyUpdate`` (:1325-1350) do for one connection, done for many
sessions in one launch:

* ``hkdf_expand_label``  -- ``HKDF_expand_label`` (cryptomath.py:155-173) of a
  batch of secrets (``tg_hkdf_expand_label``);
* ``traffic_keys``       -- write key + fixed IV of every session from its
  traffic secret, and the key table built from those keys without leaving
  HBM (``tg_key_create_device``);
* ``key_update``         -- the "traffic upd" step of a TLS 1.3 KeyUpdate.

These build new arrays and a new table.  A live ``tlsgpu.Sessions`` is updated in
place instead (``Sessions.key_update`` / ``install``, ``tg_sessions_rekey``).

The TLS 1.3 key schedule above the traffic secrets (tlsconnection.py:3036-3050,
:3203-3224, :3326-3360; the client at :1319-1333, :1552-1568, :1659-1701), from
the (EC)DHE shared secret, an optional PSK and the transcript hashes:

* ``hkdf_extract``       -- ``secureHMAC(salt, ikm)`` (cryptomath.py:128-132),
  HKDF-Extract, of a batch (``tg_hkdf_extract``);
* ``hkdf_expand_label_rows`` / ``derive_secret`` -- ``HKDF_expand_label`` with a
  context per session, and ``derive_secret`` (:175-195), its case of one
  transcript hash per session (``tg_hkdf_expand_label_rows``);
* ``tls13_finished``     -- the Finished verify_data of every session
  (``tg_tls13_finished``);
* ``tls13_handshake_secrets`` -- early secret, "derived", handshake secret and
  both handshake traffic secrets in one launch
  (``tg_tls13_handshake_secrets``); ``Sessions.install_handshake`` installs
  one side's keys from them;
* ``tls13_application_secrets`` -- "derived", master secret, both application
  traffic secrets and the exporter master secret in one launch
  (``tg_tls13_application_secrets``); ``Sessions.install_application``;
* ``tls13_binders`` / ``tls13_resumption_psk`` -- the PSK binder of
  ``HandshakeHelpers._calc_binder`` (handshakehelpers.py:44-61) and the
  ticket PSK of ``calc_res_binder_psk`` (:64-72).

Every secret between a call's inputs and its outputs stays in registers.

TLS 1.2 (``RecordLayer.calcPendingStates``, recordlayer.py:1189-1246, and
``calc_key``, mathtls.py:827-908):

* ``tls12_prf``          -- ``PRF_1_2`` / ``PRF_1_2_SHA384`` of a batch of
  secrets (``tg_tls12_prf``): master secret, extended master secret, Finished
  values, key block;
* ``tls12_key_block``    -- the six slices of every session's key block;
* ``TLS12_SUITES``       -- what a suite id means to the two above and to
  ``Sessions.from_master_secrets`` / ``CbcSessions.from_master_secrets``, which
  install the slices into live tables without storing the raw keys
  (``tg_sessions_install_tls12`` / ``tg_cbc_sessions_install_tls12``).

TLS 1.0 / 1.1 (``PRF``, mathtls.py:701-714: P_MD5 xor P_SHA1):

* ``tls10_prf``          -- the PRF of a batch of secrets (``tg_tls10_prf``);
* ``tls11_key_block``    -- both sides' MAC key and cipher key for the
  HMAC-SHA1 AES-CBC suites; ``CbcSessions.from_master_secrets(...,
  version=TLS11)`` installs them without storing the raw keys
  (``tg_cbc_sessions_install_tls11``).

Secrets, keys and IVs are device tensors (uint8, one row per session).
"""
from . import _lib
from .batch import KeyTable, _ptr, _stream

# TLS 1.3 suites (constants.py): AEAD, key length, PRF hash length
# (recordlayer.py _getCipherSettings :1022-1079, sha384PrfSuites).
TLS13_SUITES = {
    0x1301: ("aesgcm", 16, 32),             # TLS_AES_128_GCM_SHA256
    0x1302: ("aesgcm", 32, 48),             # TLS_AES_256_GCM_SHA384
    0x1303: ("chacha20-poly1305", 32, 32),  # TLS_CHACHA20_POLY1305_SHA256
    0x1304: ("aesccm", 16, 32),             # TLS_AES_128_CCM_SHA256
    0x1305: ("aesccm_8", 16, 32),           # TLS_AES_128_CCM_8_SHA256
}


def _rows(ids, *row):
    return dict((i, row) for i in ids)


# TLS 1.2 suites (constants.py) the engine can run: algorithm, key length,
# fixed IV length, MAC (None for AEAD), MAC key length, PRF hash length
# (recordlayer.py _getCipherSettings :1022-1079, _getMacSettings :1081-1102;
# PRF hash 48 for sha384PrfSuites).  A CBC suite's "fixed IV" is the 16-byte IV
# block of the key block, unused at TLS >= 1.1.
TLS12_SUITES = {}
TLS12_SUITES.update(_rows((0x009c, 0x009e, 0x00a6, 0xc02b, 0xc02d, 0xc031, 0xc02f, 0x00a2, 0x00a4),
                          "aesgcm", 16, 4, None, 0, 32))          # *_WITH_AES_128_GCM_SHA256
TLS12_SUITES.update(_rows((0x009d, 0x009f, 0x00a7, 0xc02c, 0xc02e, 0xc032, 0xc030, 0x00a3, 0x00a5),
                          "aesgcm", 32, 4, None, 0, 48))          # *_WITH_AES_256_GCM_SHA384
TLS12_SUITES.update(_rows((0xc09c, 0xc09e, 0xc0ac), "aesccm", 16, 4, None, 0, 32))
TLS12_SUITES.update(_rows((0xc09d, 0xc09f, 0xc0ad), "aesccm", 32, 4, None, 0, 32))
TLS12_SUITES.update(_rows((0xc0a0, 0xc0a2, 0xc0ae), "aesccm_8", 16, 4, None, 0, 32))
TLS12_SUITES.update(_rows((0xc0a1, 0xc0a3, 0xc0af), "aesccm_8", 32, 4, None, 0, 32))
TLS12_SUITES.update(_rows((0xcca8, 0xcca9, 0xccaa), "chacha20-poly1305", 32, 12, None, 0, 32))
TLS12_SUITES.update(_rows((0xcca1, 0xcca2, 0xcca3), "chacha20-poly1305", 32, 4, None, 0, 32))  # draft-00
TLS12_SUITES.update(_rows((0xc01d, 0xc01e, 0xc01f, 0x002f, 0x0033, 0x0034, 0xc009, 0xc004, 0xc00e, 0xc013,
                           0xc018, 0x0030, 0x0032), "aescbc", 16, 16, "sha1", 20, 32))
TLS12_SUITES.update(_rows((0x003c, 0x0067, 0x006c, 0xc023, 0xc025, 0xc029, 0xc027),
                          "aescbc", 16, 16, "sha256", 32, 32))
TLS12_SUITES.update(_rows((0xc020, 0xc021, 0xc022, 0x0035, 0x003a, 0x0039, 0xc00a, 0xc005, 0xc00f, 0xc014,
                           0xc019, 0x0036, 0x0038), "aescbc", 32, 16, "sha1", 20, 32))
TLS12_SUITES.update(_rows((0x003d, 0x006b, 0x006d), "aescbc", 32, 16, "sha256", 32, 32))
TLS12_SUITES.update(_rows((0xc024, 0xc026, 0xc02a, 0xc028), "aescbc", 32, 16, "sha384", 48, 48))

CLIENT_WRITE = _lib.TG_TLS12_CLIENT_WRITE
SERVER_WRITE = _lib.TG_TLS12_SERVER_WRITE


def _torch():
    import torch
    return torch


def tls12_suite(cipher_suite):
    """The ``TLS12_SUITES`` row of a suite id; ValueError for an id that is not in the table."""
    try:
        return TLS12_SUITES[cipher_suite]
    except (KeyError, TypeError):
        raise ValueError("cipher suite %r is not in TLS12_SUITES" % (cipher_suite,))


def torch_stream(stream):
    """``stream`` (None = the current one, a torch stream, or a raw handle) as a torch stream."""
    torch = _torch()
    if stream is None:
        return torch.cuda.current_stream()
    if hasattr(stream, "cuda_stream"):
        return stream
    return torch.cuda.ExternalStream(int(stream))


def tls12_side(side):
    """``side`` as TG_TLS12_CLIENT_WRITE / _SERVER_WRITE: 0 / 1 or "client" / "server"."""
    if side in ("client", "server"):
        return CLIENT_WRITE if side == "client" else SERVER_WRITE
    if side in (CLIENT_WRITE, SERVER_WRITE):
        return int(side)
    raise ValueError('side must be "client" (0) or "server" (1)')


def tls12_prf(secrets, label, seeds, length, hashlen, out=None, stream=None):
    """``P_hash(secret_i, label + seed_i, length)`` (mathtls.py:679-698) for
    every row of ``secrets`` (n x secret length device bytes) with SHA-256
    (``hashlen`` 32, ``PRF_1_2``) or SHA-384 (48, ``PRF_1_2_SHA384``)
    (tg_tls12_prf).  ``seeds``: n x seed length device bytes, or ``None`` for
    an empty seed; ``label`` is host bytes shared by all rows.  Returns / fills
    ``out`` (n x length)."""
    torch = _torch()
    if secrets.ndim != 2:
        raise ValueError("secrets must be a 2-D tensor, one row per session")
    n, secretlen = secrets.shape
    seedlen = 0
    if seeds is not None:
        if seeds.ndim != 2 or seeds.shape[0] != n:
            raise ValueError("seeds must have one row per secret")
        seedlen = seeds.shape[1]
    if out is None:
        out = torch.empty((n, length), dtype=torch.uint8, device=secrets.device)
    elif out.numel() != n * length:
        raise ValueError("out must hold %d bytes per session" % length)
    label = bytes(label)
    _lib.check(_lib.load().tg_tls12_prf(hashlen, _ptr(secrets, "secrets"), secretlen, n, label or None,
                                        len(label), _ptr(seeds, "seeds") if seedlen else None, seedlen,
                                        length, _ptr(out, "out"), _stream(stream)))
    return out


def tls12_key_block(cipher_suite, master_secrets, client_random, server_random, stream=None):
    """The key block of calcPendingStates (recordlayer.py:1202-1219) for many
    sessions, cut into its six slices: ``(client MAC key, server MAC key,
    client key, server key, client IV, server IV)``, device tensors of one row
    per session (the MAC keys are n x 0 for an AEAD suite)."""
    torch = _torch()
    _, keylen, ivlen, _, maclen, hashlen = tls12_suite(cipher_suite)
    with torch.cuda.stream(torch_stream(stream)):
        # torch's own kernels (the seed rows, the output and its slices) on ``stream`` too
        seeds = torch.cat([server_random.reshape(-1, 32), client_random.reshape(-1, 32)], dim=1).contiguous()
        block = tls12_prf(master_secrets.reshape(-1, 48), b"key expansion", seeds,
                          2 * (maclen + keylen + ivlen), hashlen, stream=stream)
        out, at = [], 0
        for size in (maclen, maclen, keylen, keylen, ivlen, ivlen):
            out.append(block[:, at:at + size].contiguous())
            at += size
    return tuple(out)


def tls10_prf(secrets, label, seeds, length, out=None, stream=None):
    """``PRF(secret_i, label, seed_i, length)`` of TLS 1.0 / 1.1 (mathtls.py:701-714:
    P_MD5 over the secret's first half xor P_SHA1 over its last half) for every
    row of ``secrets`` (n x secret length device bytes, 1..128) (tg_tls10_prf).
    ``seeds``: n x seed length device bytes, or ``None`` for an empty seed;
    ``label`` is host bytes shared by all rows.  Returns / fills ``out``
    (n x length)."""
    torch = _torch()
    if secrets.ndim != 2:
        raise ValueError("secrets must be a 2-D tensor, one row per session")
    n, secretlen = secrets.shape
    seedlen = 0
    if seeds is not None:
        if seeds.ndim != 2 or seeds.shape[0] != n:
            raise ValueError("seeds must have one row per secret")
        seedlen = seeds.shape[1]
    if out is None:
        out = torch.empty((n, length), dtype=torch.uint8, device=secrets.device)
    elif out.numel() != n * length:
        raise ValueError("out must hold %d bytes per session" % length)
    label = bytes(label)
    _lib.check(_lib.load().tg_tls10_prf(_ptr(secrets, "secrets"), secretlen, n, label or None, len(label),
                                        _ptr(seeds, "seeds") if seedlen else None, seedlen, length,
                                        _ptr(out, "out"), _stream(stream)))
    return out


def tls11_suite(cipher_suite):
    """``(key length, MAC key length)`` of a suite the engine runs at TLS 1.1:
    the HMAC-SHA1 AES-CBC rows of ``TLS12_SUITES`` (the ids are the same at
    both versions; the version picks the PRF).  ValueError, naming the suite,
    for any other."""
    row = TLS12_SUITES.get(cipher_suite) if isinstance(cipher_suite, int) else None
    if row is None or row[0] != "aescbc" or row[3] != "sha1":
        raise ValueError("cipher suite %s is not an AES-CBC + HMAC-SHA1 suite: no TLS 1.1 keys for it"
                         % ("0x%04x" % cipher_suite if isinstance(cipher_suite, int) else repr(cipher_suite)))
    return row[1], row[4]


def tls11_key_block(cipher_suite, master_secrets, client_random, server_random, stream=None):
    """The key block of calcPendingStates (recordlayer.py:1202-1219) at TLS 1.1
    for many sessions of an HMAC-SHA1 AES-CBC suite, cut into ``(client MAC
    key, server MAC key, client key, server key)``, device tensors of one row
    per session.  The two IV blocks that follow are unused at TLS 1.1 and not
    derived."""
    torch = _torch()
    keylen, maclen = tls11_suite(cipher_suite)
    with torch.cuda.stream(torch_stream(stream)):
        seeds = torch.cat([server_random.reshape(-1, 32), client_random.reshape(-1, 32)], dim=1).contiguous()
        block = tls10_prf(master_secrets.reshape(-1, 48), b"key expansion", seeds, 2 * (maclen + keylen),
                          stream=stream)
        out, at = [], 0
        for size in (maclen, maclen, keylen, keylen):
            out.append(block[:, at:at + size].contiguous())
            at += size
    return tuple(out)


def tls12_install_args(n, hashlen, side, nsessions, slots, master_secrets, client_random, server_random,
                       fixed_iv_len=0, iv_table=None, seq_next=None):
    """A filled ``tg_tls12_install``; the row counts of the three inputs are checked."""
    for what, t, width in (("master_secrets", master_secrets, 48), ("client_random", client_random, 32),
                           ("server_random", server_random, 32)):
        if t.numel() != n * width:
            raise ValueError("%s must hold one %d-byte row per slot" % (what, width))
    r = _lib.TgTls12Install()
    r.n, r.hashlen, r.side, r.nsessions = n, hashlen, tls12_side(side), nsessions
    r.slot = _ptr(slots, "slots")
    r.master_secrets = _ptr(master_secrets, "master_secrets")
    r.client_random = _ptr(client_random, "client_random")
    r.server_random = _ptr(server_random, "server_random")
    r.fixed_iv_len = fixed_iv_len
    r.iv_table = _ptr(iv_table, "ivs")
    r.seq_next = _ptr(seq_next, "seq_next")
    return r


def hkdf_expand_label(secrets, label, context, length, hashlen, out=None, stream=None):
    """``HKDF_expand_label(secret_i, label, context, length)`` for every row of
    ``secrets`` (n x hashlen device bytes); returns / fills ``out`` (n x length)."""
    torch = _torch()
    n = secrets.numel() // hashlen
    if out is None:
        out = torch.empty((n, length), dtype=torch.uint8, device=secrets.device)
    label, context = bytes(label), bytes(context)
    _lib.check(_lib.load().tg_hkdf_expand_label(hashlen, _ptr(secrets, "secrets"), n, label,
                                                len(label), context or None, len(context),
                                                length, _ptr(out, "out"), _stream(stream)))
    return out


def traffic_keys(cipher_suite, secrets, stream=None):
    """Per-session write keys and fixed IVs from traffic secrets, as
    calcTLS1_3PendingState derives them (recordlayer.py:1291-1312).

    Returns ``(KeyTable, keys, ivs)``: the key table (built on the device),
    the raw keys (n x key length) and the IVs (n x 12)."""
    alg, keylen, hashlen = TLS13_SUITES[cipher_suite]
    keys = hkdf_expand_label(secrets, b"key", b"", keylen, hashlen, stream=stream)
    ivs = hkdf_expand_label(secrets, b"iv", b"", 12, hashlen, stream=stream)
    table = KeyTable.from_device(alg, keys, keys.shape[0], keylen, stream=stream)
    return table, keys, ivs


def key_update(cipher_suite, secrets, stream=None):
    """The next application traffic secrets (``_calcTLS1_3KeyUpdate``,
    recordlayer.py:1333-1336): HKDF-Expand-Label(secret, "traffic upd", "", Hash.length)."""
    hashlen = TLS13_SUITES[cipher_suite][2]
    return hkdf_expand_label(secrets, b"traffic upd", b"", hashlen, hashlen, stream=stream)


# ---- the TLS 1.3 key schedule above the traffic secrets -----------------------
def tls13_suite(cipher_suite):
    """The ``TLS13_SUITES`` row of a suite id; ValueError for an id that is not in the table."""
    try:
        return TLS13_SUITES[cipher_suite]
    except (KeyError, TypeError):
        raise ValueError("cipher suite %r is not in TLS13_SUITES" % (cipher_suite,))


def _hash_rows(t, hashlen, what, n=None):
    """The row count of ``t``, a tensor of ``hashlen``-byte rows (of ``n`` rows when given)."""
    if t.numel() % hashlen or (n is not None and t.numel() != n * hashlen):
        raise ValueError("%s must hold one %d-byte row per session" % (what, hashlen))
    return t.numel() // hashlen


def _out_rows(out, n, width, like, stream):
    """``out``, or a new n x width tensor that belongs to ``stream``'s allocations."""
    if out is None:
        torch = _torch()
        with torch.cuda.stream(torch_stream(stream)):
            return torch.empty((n, width), dtype=torch.uint8, device=like.device)
    if out.numel() != n * width:
        raise ValueError("out must hold %d bytes per session" % width)
    return out


def hkdf_extract(salts, ikm, hashlen, out=None, stream=None):
    """``secureHMAC(salt_i, ikm_i)`` (cryptomath.py:128-132), HKDF-Extract, for
    every session (tg_hkdf_extract).  ``salts``: n x hashlen device bytes, or
    ``None`` for ``hashlen`` zero bytes; ``ikm``: n x (1..1024) device bytes, or
    ``None`` for ``hashlen`` zero bytes.  One of the two, or ``out``, gives n.
    Returns / fills ``out`` (n x hashlen)."""
    if ikm is not None and ikm.ndim != 2:
        raise ValueError("ikm must be a 2-D tensor, one row per session")
    given = ikm if ikm is not None else salts if salts is not None else out
    if given is None:
        raise ValueError("salts, ikm and out are all None: the row count is unknown")
    n = ikm.shape[0] if ikm is not None else _hash_rows(given, hashlen, "salts")
    if salts is not None:
        _hash_rows(salts, hashlen, "salts", n)
    out = _out_rows(out, n, hashlen, given, stream)
    _lib.check(_lib.load().tg_hkdf_extract(hashlen, _ptr(salts, "salts"), _ptr(ikm, "ikm"),
                                           ikm.shape[1] if ikm is not None else 0, n, _ptr(out, "out"),
                                           _stream(stream)))
    return out


def hkdf_expand_label_rows(secrets, label, contexts, length, hashlen, out=None, stream=None):
    """``HKDF_expand_label(secret_i, label, context_i, length)`` (cryptomath.py:155-173)
    for every row of ``secrets`` (n x hashlen device bytes) with its own row
    of ``contexts`` (n x 0..64 device bytes; ``None`` = no context)
    (tg_hkdf_expand_label_rows).  ``label`` is host bytes shared by all rows,
    without "tls13 ".  Returns / fills ``out`` (n x length, at most a digest)."""
    n = _hash_rows(secrets, hashlen, "secrets")
    ctxlen = 0
    if contexts is not None:
        if contexts.ndim != 2 or contexts.shape[0] != n:
            raise ValueError("contexts must have one row per secret")
        ctxlen = contexts.shape[1]
    out = _out_rows(out, n, length, secrets, stream)
    label = bytes(label)
    _lib.check(_lib.load().tg_hkdf_expand_label_rows(hashlen, _ptr(secrets, "secrets"), n, label or None,
                                                     len(label), _ptr(contexts, "contexts") if ctxlen else None,
                                                     ctxlen, length, _ptr(out, "out"), _stream(stream)))
    return out


def derive_secret(secrets, label, hashes, hashlen, out=None, stream=None):
    """``derive_secret(secret_i, label, transcript_i)`` (cryptomath.py:175-195):
    ``hashes`` holds every session's transcript hash (n x hashlen device bytes);
    ``None`` is the reference's ``handshake_hashes=None``, the hash of the empty
    transcript.  Returns / fills ``out`` (n x hashlen)."""
    n = _hash_rows(secrets, hashlen, "secrets")
    out = _out_rows(out, n, hashlen, secrets, stream)
    label = bytes(label)
    if hashes is not None:
        _hash_rows(hashes, hashlen, "hashes", n)
    _lib.check(_lib.load().tg_hkdf_expand_label_rows(hashlen, _ptr(secrets, "secrets"), n, label or None,
                                                     len(label), _ptr(hashes, "hashes"), hashlen, hashlen,
                                                     _ptr(out, "out"), _stream(stream)))
    return out


def tls13_finished(secrets, hashes, hashlen, out=None, stream=None):
    """The Finished verify_data of every session (tlsconnection.py:3203-3207):
    ``secureHMAC(HKDF_expand_label(secret_i, "finished", "", hashlen), hash_i)``
    with ``secrets`` the handshake traffic secrets (or binder keys) and
    ``hashes`` the transcript hashes, n x hashlen device bytes each
    (tg_tls13_finished).  Returns / fills ``out`` (n x hashlen)."""
    n = _hash_rows(secrets, hashlen, "secrets")
    _hash_rows(hashes, hashlen, "hashes", n)
    out = _out_rows(out, n, hashlen, secrets, stream)
    _lib.check(_lib.load().tg_tls13_finished(hashlen, _ptr(secrets, "secrets"), _ptr(hashes, "hashes"), n,
                                             _ptr(out, "out"), _stream(stream)))
    return out


def tls13_handshake_secrets(cipher_suite, shared, hello_hash, psk=None, stream=None):
    """The handshake stage of the schedule (tlsconnection.py:3036-3050) for
    many sessions in one launch (tg_tls13_handshake_secrets): ``shared`` is
    every session's (EC)DHE shared secret (n x 1..1024 device bytes),
    ``hello_hash`` the transcript hash through ServerHello and ``psk`` the
    PSK (n x hashlen each; ``psk=None``: no PSK).  Returns ``(handshake_secret,
    client_hs, server_hs)``, n x hashlen each; the early secret and "derived"
    stay in registers."""
    torch = _torch()
    hashlen = tls13_suite(cipher_suite)[2]
    if shared.ndim != 2:
        raise ValueError("shared must be a 2-D tensor, one row per session")
    n = shared.shape[0]
    _hash_rows(hello_hash, hashlen, "hello_hash", n)
    if psk is not None:
        _hash_rows(psk, hashlen, "psk", n)
    with torch.cuda.stream(torch_stream(stream)):
        out = torch.empty((3, n, hashlen), dtype=torch.uint8, device=shared.device)
    _lib.check(_lib.load().tg_tls13_handshake_secrets(hashlen, _ptr(psk, "psk"), _ptr(shared, "shared"),
                                                      shared.shape[1], _ptr(hello_hash, "hello_hash"), n,
                                                      _ptr(out[0], "out"), _ptr(out[1], "out"), _ptr(out[2], "out"),
                                                      _stream(stream)))
    return out[0], out[1], out[2]


def tls13_application_secrets(cipher_suite, handshake_secrets, finished_hash, in_place=False, stream=None):
    """The application stage (tlsconnection.py:3218-3224, :3326) for many
    sessions in one launch (tg_tls13_application_secrets): from the handshake
    secrets and the transcript hash through the server's Finished (n x hashlen
    device bytes each) to ``(master, client_ap, server_ap, exporter_master)``.
    ``in_place``: the master secrets overwrite ``handshake_secrets``, which is
    returned as ``master``."""
    torch = _torch()
    hashlen = tls13_suite(cipher_suite)[2]
    n = _hash_rows(handshake_secrets, hashlen, "handshake_secrets")
    _hash_rows(finished_hash, hashlen, "finished_hash", n)
    with torch.cuda.stream(torch_stream(stream)):
        out = torch.empty((4, n, hashlen), dtype=torch.uint8, device=handshake_secrets.device)
    master = handshake_secrets if in_place else out[0]
    _lib.check(_lib.load().tg_tls13_application_secrets(hashlen, _ptr(handshake_secrets, "handshake_secrets"),
                                                        _ptr(finished_hash, "finished_hash"), n,
                                                        _ptr(master, "master"), _ptr(out[1], "out"),
                                                        _ptr(out[2], "out"), _ptr(out[3], "out"), _stream(stream)))
    return master, out[1], out[2], out[3]


def tls13_binders(psk, hashes, hashlen, external, stream=None):
    """The PSK binder of every row (``HandshakeHelpers._calc_binder``,
    handshakehelpers.py:44-61): ``psk`` n x (1..1024) device bytes, ``hashes``
    the transcript hash that includes the truncated ClientHello (n x hashlen);
    ``external`` picks "ext binder" (an out-of-band PSK) or "res binder" (a
    ticket's).  Extract, Derive-Secret over the empty transcript and Finished,
    three launches on ``stream``; returns n x hashlen device bytes."""
    early = hkdf_extract(None, psk, hashlen, stream=stream)
    key = derive_secret(early, b"ext binder" if external else b"res binder", None, hashlen, stream=stream)
    return tls13_finished(key, hashes, hashlen, stream=stream)


def tls13_resumption_psk(res_master, nonces, hashlen, stream=None):
    """The PSK of a session ticket (``calc_res_binder_psk``,
    handshakehelpers.py:64-72): ``HKDF_expand_label(res_master_i, "resumption",
    ticket_nonce_i, hashlen)`` with one nonce per row (n x 0..64 device bytes)."""
    return hkdf_expand_label_rows(res_master, b"resumption", nonces, hashlen, hashlen, stream=stream)

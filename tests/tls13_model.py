"""A hashlib / hmac model of the TLS 1.3 key schedule calls (tg_hkdf_extract,
tg_hkdf_expand_label_rows, tg_tls13_finished, tg_tls13_handshake_secrets,
tg_tls13_application_secrets, and keysetup.tls13_binders /
tls13_resumption_psk on top of them), and the inputs of
tests/golden/tls13_schedule.json, regenerated from the labels its generator
used.  test_tls13_model.py holds the model to every fixture row; the GPU tests
use it for the rows a batch has beside the fixture's own."""
import hashlib
import hmac

from vectors import detbytes

HASHLEN = {"sha256": 32, "sha384": 48}
ALG = {32: "sha256", 48: "sha384"}


def _b(label, n):
    return bytes(detbytes(label, n))


# ---- the calls -----------------------------------------------------------------
def extract(alg, salt, ikm):
    """HKDF-Extract; ``None`` for either is HASHLEN zero bytes."""
    hl = HASHLEN[alg]
    return hmac.new(bytes(hl) if salt is None else salt, bytes(hl) if ikm is None else ikm,
                    getattr(hashlib, alg)).digest()


def hkdf_label(label, context, outlen):
    full = b"tls13 " + label
    return outlen.to_bytes(2, "big") + bytes([len(full)]) + full + bytes([len(context)]) + context


def expand_label(alg, secret, label, context, outlen):
    """HKDF-Expand-Label for outlen up to one digest: T(1), cut."""
    assert 1 <= outlen <= HASHLEN[alg]
    return hmac.new(secret, hkdf_label(label, context, outlen) + b"\x01", getattr(hashlib, alg)).digest()[:outlen]


def empty_hash(alg):
    return hashlib.new(alg, b"").digest()


def derive_secret(alg, secret, label, transcript_hash):
    """``transcript_hash`` None: the empty transcript."""
    ctx = empty_hash(alg) if transcript_hash is None else transcript_hash
    return expand_label(alg, secret, label, ctx, HASHLEN[alg])


def finished(alg, secret, transcript_hash):
    key = expand_label(alg, secret, b"finished", b"", HASHLEN[alg])
    return hmac.new(key, transcript_hash, getattr(hashlib, alg)).digest()


def handshake_secrets(alg, psk, shared, hello_hash):
    """(handshake secret, client hs traffic, server hs traffic)."""
    early = extract(alg, None, psk)
    hs = extract(alg, derive_secret(alg, early, b"derived", None), shared)
    return hs, derive_secret(alg, hs, b"c hs traffic", hello_hash), derive_secret(alg, hs, b"s hs traffic", hello_hash)


def application_secrets(alg, hs, finished_hash):
    """(master, client ap traffic, server ap traffic, exporter master)."""
    master = extract(alg, derive_secret(alg, hs, b"derived", None), None)
    return (master, derive_secret(alg, master, b"c ap traffic", finished_hash),
            derive_secret(alg, master, b"s ap traffic", finished_hash),
            derive_secret(alg, master, b"exp master", finished_hash))


def binder(alg, psk, transcript_hash, external):
    early = extract(alg, None, psk)
    key = derive_secret(alg, early, b"ext binder" if external else b"res binder", None)
    return finished(alg, key, transcript_hash)


def resumption_psk(alg, res_master, nonce):
    return expand_label(alg, res_master, b"resumption", nonce, HASHLEN[alg])


def traffic_key_iv(alg, secret, keylen):
    return expand_label(alg, secret, b"key", b"", keylen), expand_label(alg, secret, b"iv", b"", 12)


# ---- the fixture's inputs ------------------------------------------------------
def extract_inputs(c):
    """(salt or None, ikm or None) of an ``extract`` row; None where the row says zero."""
    alg, hl = c["hash"], HASHLEN[c["hash"]]
    # the zero-salt row borrows the IKM of the 32-byte row, the zero-IKM row the salt of the hashlen row
    salt = None if c["salt"] == "zero" else _b("k13-ext-salt-%s-%d" % (alg, c["ikmlen"]), hl)
    ikm = None if c["ikm"] == "zero" else _b("k13-ext-ikm-%s-%d" % (alg, c["ikmlen"]), c["ikmlen"])
    return salt, ikm


def expand_inputs(c):
    """(secret, label, context) of an ``expand`` row."""
    tag = "%s-%d-%d-%d" % (c["hash"], c["labellen"], c["ctxlen"], c["outlen"])
    return (_b("k13-exp-secret-" + tag, HASHLEN[c["hash"]]), _b("k13-exp-label-" + tag, c["labellen"]),
            _b("k13-exp-ctx-" + tag, c["ctxlen"]))


def derive_inputs(c):
    """(secret, label, transcript hash or None) of a ``derive`` row."""
    tag = "%s-%s-%d" % (c["hash"], c["label"], c["transcript"])
    digest = bytes.fromhex(c["digest"]) if c["transcript"] else None
    if digest is not None:   # HandshakeHashes.digest is the plain hash of what it has seen
        assert hashlib.new(c["hash"], _b("k13-der-transcript-" + tag, 300)).digest() == digest
    return _b("k13-der-secret-" + tag, HASHLEN[c["hash"]]), c["label"].encode(), digest


def schedule_inputs(c):
    """(psk or None, shared) of a ``schedule`` row; the transcript hashes are in the row."""
    tag = "%s-c%d" % (c["hash"], c["conn"])
    psk = _b("k13-sch-psk-" + tag, HASHLEN[c["hash"]]) if c["psk"] else None
    return psk, _b("k13-sch-shared-" + tag, c["sharedlen"])


def binder_inputs(c):
    """(psk, transcript hash) of a ``binder`` row."""
    tag = "%s-%d-%d" % (c["hash"], c["psklen"], c["external"])
    return _b("k13-bind-psk-" + tag, c["psklen"]), bytes.fromhex(c["digest"])


def res_psk_inputs(c):
    """(resumption master secret, ticket nonce) of a ``res_psk`` row."""
    tag = "%s-%d" % (c["hash"], c["noncelen"])
    return _b("k13-res-master-" + tag, HASHLEN[c["hash"]]), _b("k13-res-nonce-" + tag, c["noncelen"])

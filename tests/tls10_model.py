"""Host restatement of the TLS 1.0 / 1.1 PRF and key block -- TEST INFRASTRUCTURE.

``PRF`` (tlslite/mathtls.py:701-714): the secret's first and last
``ceil(L / 2)`` bytes key ``P_hash`` (:679-698) with MD5 and with SHA-1 over
``label + seed``, and the two streams are xored; with hashlib / hmac.  The
slicing is ``RecordLayer.calcPendingStates``' (recordlayer.py:1202-1219) for the
HMAC-SHA1 AES-CBC suites.  Held against the reference's outputs in
tests/golden/tls10_keys.json and against the keys of the TLS 1.1 cases of
cbc_sessions.json by tests/test_tls10_model.py; the GPU tests compare the
device with it only where a fixture has no entry of its own.
"""
import hashlib
import hmac

from vectors import detbytes


def p_hash(digestmod, secret, seed, length):
    secret, seed = bytes(secret), bytes(seed)
    out, a = b"", seed
    while len(out) < length:
        a = hmac.new(secret, a, digestmod).digest()
        out += hmac.new(secret, a + seed, digestmod).digest()
    return out[:length]


def prf(secret, label, seed, length):
    secret, msg = bytes(secret), bytes(label) + bytes(seed)
    half = (len(secret) + 1) // 2
    md5 = p_hash(hashlib.md5, secret[:half], msg, length)
    sha = p_hash(hashlib.sha1, secret[len(secret) - half:], msg, length)
    return bytes(a ^ b for a, b in zip(md5, sha))


def key_block(keylen, master_secret, client_random, server_random):
    """``{"client": {...}, "server": {...}}`` with ``mac_key`` (20 bytes) and ``key``."""
    block = prf(master_secret, b"key expansion", bytes(server_random) + bytes(client_random), 2 * (20 + keylen))
    return {"client": {"mac_key": block[:20], "key": block[40:40 + keylen]},
            "server": {"mac_key": block[20:40], "key": block[40 + keylen:40 + 2 * keylen]}}


# ---- the fixture's detbytes inputs ----------------------------------------------
def prf_inputs(case):
    """(secret, label, seed) of a ``prf`` entry of tls10_keys.json."""
    tag = "%d-%d-%d" % (case["secretlen"], case["labellen"], case["seedlen"])
    return (bytes(detbytes("k10-prf-secret-" + tag, case["secretlen"])),
            bytes(detbytes("k10-prf-label-" + tag, case["labellen"])),
            bytes(detbytes("k10-prf-seed-" + tag, case["seedlen"])))


def calc_key_inputs(case):
    """(secret, label, seed) of a ``calc_key`` entry of tls10_keys.json."""
    name = "%s-%d" % (case["suite"], case["version"][1])
    secret = bytes(detbytes("k10-secret-" + name, 48))
    if "seed_hex" in case:
        seed = bytes.fromhex(case["seed_hex"])
    else:   # "master secret": client_random + server_random (mathtls.py:903-904)
        seed = bytes(detbytes("k10-cr-" + name, 32)) + bytes(detbytes("k10-sr-" + name, 32))
    return secret, case["label"].encode(), seed


def pending_inputs(suite_name, c):
    """(master secret, client random, server random) of connection c of a ``pending`` entry."""
    tag = "%s-c%d" % (suite_name, c)
    return (bytes(detbytes("k10-ms-" + tag, 48)), bytes(detbytes("k10-cr-" + tag, 32)),
            bytes(detbytes("k10-sr-" + tag, 32)))


# suite ids of the fixtures' TLS 1.1 cases (tlslite/constants.py)
SUITE_IDS = {"TLS_RSA_WITH_AES_128_CBC_SHA": 0x002f, "TLS_RSA_WITH_AES_256_CBC_SHA": 0x0035}

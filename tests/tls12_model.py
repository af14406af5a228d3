"""Host restatement of the TLS 1.2 PRF and key block -- TEST INFRASTRUCTURE.

``P_hash`` (tlslite/mathtls.py:679-698) as ``PRF_1_2`` / ``PRF_1_2_SHA384``
(:716-722) call it, with hashlib / hmac, and the slicing of
``RecordLayer.calcPendingStates`` (recordlayer.py:1202-1219).  Held against the
reference's outputs in tests/golden/tls12_keys.json and against the keys of
the TLS 1.2 cases of cbc_sessions.json and sessions.json by
tests/test_tls12_model.py; the GPU tests compare the device with it only where
a fixture has no entry of its own.
"""
import hashlib
import hmac

from vectors import detbytes

HASH = {32: hashlib.sha256, 48: hashlib.sha384}


def p_hash(hashlen, secret, seed, length):
    secret, seed = bytes(secret), bytes(seed)
    out, a = b"", seed
    while len(out) < length:
        a = hmac.new(secret, a, HASH[hashlen]).digest()
        out += hmac.new(secret, a + seed, HASH[hashlen]).digest()
    return out[:length]


def prf(hashlen, secret, label, seed, length):
    return p_hash(hashlen, secret, bytes(label) + bytes(seed), length)


def key_block(hashlen, maclen, keylen, ivlen, master_secret, client_random, server_random):
    """``{"client": {...}, "server": {...}}`` with ``mac_key``, ``key`` and ``iv``."""
    block = prf(hashlen, master_secret, b"key expansion", bytes(server_random) + bytes(client_random),
                2 * (maclen + keylen + ivlen))
    cut, at = [], 0
    for size in (maclen, maclen, keylen, keylen, ivlen, ivlen):
        cut.append(block[at:at + size])
        at += size
    return {"client": {"mac_key": cut[0], "key": cut[2], "iv": cut[4]},
            "server": {"mac_key": cut[1], "key": cut[3], "iv": cut[5]}}


# ---- the fixtures' detbytes inputs ---------------------------------------------
def prf_inputs(case):
    """(secret, label, seed) of a ``prf`` entry of tls12_keys.json."""
    tag = "%d-%d-%d-%d" % (case["hashlen"], case["secretlen"], case["labellen"], case["seedlen"])
    return (bytes(detbytes("k12-prf-secret-" + tag, case["secretlen"])),
            bytes(detbytes("k12-prf-label-" + tag, case["labellen"])),
            bytes(detbytes("k12-prf-seed-" + tag, case["seedlen"])))


def calc_key_inputs(case):
    """(secret, label, seed) of a ``calc_key`` entry of tls12_keys.json."""
    name = case["suite"]
    secret = bytes(detbytes("k12-secret-" + name, 48))
    if "seed_hex" in case:
        seed = bytes.fromhex(case["seed_hex"])
    else:   # "master secret": client_random + server_random (mathtls.py:903-904)
        seed = bytes(detbytes("k12-cr-" + name, 32)) + bytes(detbytes("k12-sr-" + name, 32))
    return secret, case["label"].encode(), seed


def pending_inputs(suite_name, c):
    """(master secret, client random, server random) of connection c of a ``pending`` entry."""
    tag = "%s-c%d" % (suite_name, c)
    return (bytes(detbytes("k12-ms-" + tag, 48)), bytes(detbytes("k12-cr-" + tag, 32)),
            bytes(detbytes("k12-sr-" + tag, 32)))


def cbc_sessions_inputs(case, c):
    """The same of connection c of a cbc_sessions.json case (make_golden_cbc_sessions.py)."""
    tag = "%s-%d-%d-c%d" % (case["suite"], case["version"][1], case["etm"], c)
    return (bytes(detbytes("ms-" + tag, 48)), bytes(detbytes("cr-" + tag, 32)), bytes(detbytes("sr-" + tag, 32)))


def sessions_inputs(case, c):
    """The same of connection c of a TLS 1.2 sessions.json case (make_golden_sessions.py)."""
    tag = "%s-%s-%d" % (case["version"], case["alg"], c)
    return (bytes(detbytes("s-ms-" + tag, 48)), bytes(detbytes("s-cr-" + tag, 32)),
            bytes(detbytes("s-sr-" + tag, 32)))


# suite ids of the existing fixtures' TLS 1.2 cases (tlslite/constants.py)
CBC_SUITE_IDS = {"TLS_RSA_WITH_AES_128_CBC_SHA": 0x002f, "TLS_RSA_WITH_AES_256_CBC_SHA256": 0x003d,
                 "TLS_ECDHE_RSA_WITH_AES_256_CBC_SHA384": 0xc028}
SESSIONS_SUITE_IDS = {"aes256gcm": 0x009d, "chacha20-poly1305": 0xcca8}

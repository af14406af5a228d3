"""The host restatement of the TLS 1.2 PRF (tests/tls12_model.py) against the
reference: every entry of tests/golden/tls12_keys.json, and the keys the
reference's calcPendingStates gave the TLS 1.2 connections of
cbc_sessions.json and sessions.json (client-write side).  Also holds
tlsgpu.keysetup.TLS12_SUITES to the fixtures' suites."""
import os

import pytest

import tls12_model as m
from conftest import ROOT
from vectors import load

KEYS = load("tls12_keys.json")
CBC_SESSIONS = [c for c in load("cbc_sessions.json") if c["version"] == [3, 3]]
SESSIONS = [c for c in load("sessions.json") if c["version"] == "tls12"]


def test_fixture_shape():
    golden = os.path.join(ROOT, "tests", "golden")
    assert os.path.getsize(os.path.join(golden, "tls12_keys.json")) <= os.path.getsize(os.path.join(golden, "cbc.json"))
    assert len(KEYS["calc_key"]) == 16 and len(KEYS["pending"]) == 8
    for hashlen in (32, 48):
        prf = [c for c in KEYS["prf"] if c["hashlen"] == hashlen]
        assert set(c["outlen"] for c in prf) == {1, 31, 32, 33, 47, 48, 49, 104, 192, 256}
        assert set(c["seedlen"] for c in prf) == {0, 32, 48, 64, 128}
        assert set(c["labellen"] for c in prf) == {0, 13, 22, 32}
        assert set(c["secretlen"] for c in prf) == ({1, 48, 64} if hashlen == 32 else {1, 48, 64, 128})
    assert len(CBC_SESSIONS) == 6 and len(SESSIONS) == 2


@pytest.mark.parametrize("i", range(len(KEYS["prf"])))
def test_prf_entries(i):
    c = KEYS["prf"][i]
    secret, label, seed = m.prf_inputs(c)
    assert m.prf(c["hashlen"], secret, label, seed, c["outlen"]).hex() == c["out"]


@pytest.mark.parametrize("i", range(len(KEYS["calc_key"])))
def test_calc_key_entries(i):
    c = KEYS["calc_key"][i]
    secret, label, seed = m.calc_key_inputs(c)
    assert m.prf(c["hashlen"], secret, label, seed, c["outlen"]).hex() == c["out"]


@pytest.mark.parametrize("case", KEYS["pending"], ids=[c["suite"] for c in KEYS["pending"]])
def test_pending_states_both_sides(case):
    from tlsgpu import keysetup
    _, keylen, ivlen, mac, maclen, hashlen = keysetup.TLS12_SUITES[case["suite_id"]]
    for c, conn in enumerate(case["conns"]):
        got = m.key_block(hashlen, maclen, keylen, ivlen, *m.pending_inputs(case["suite"], c))
        for side in ("client", "server"):
            assert got[side]["key"].hex() == conn[side]["key"], (c, side)
            assert got[side]["mac_key"].hex() == conn[side]["mac_key"], (c, side)
            if mac is None:
                assert got[side]["iv"].hex() == conn[side]["iv"], (c, side)


@pytest.mark.parametrize("case", CBC_SESSIONS, ids=["%s-%d" % (c["suite"], c["etm"]) for c in CBC_SESSIONS])
def test_cbc_sessions_keys_are_the_key_block(case):
    from tlsgpu import keysetup
    _, keylen, ivlen, mac, maclen, hashlen = keysetup.TLS12_SUITES[m.CBC_SUITE_IDS[case["suite"]]]
    assert mac == case["mac"]
    for c in range(5):
        got = m.key_block(hashlen, maclen, keylen, ivlen, *m.cbc_sessions_inputs(case, c))["client"]
        assert got["key"].hex() == case["enc_keys"][c] and got["mac_key"].hex() == case["mac_keys"][c], c


@pytest.mark.parametrize("case", SESSIONS, ids=[c["alg"] for c in SESSIONS])
def test_sessions_keys_are_the_key_block(case):
    from tlsgpu import keysetup
    _, keylen, ivlen, mac, maclen, hashlen = keysetup.TLS12_SUITES[m.SESSIONS_SUITE_IDS[case["alg"]]]
    assert mac is None
    for c in range(5):
        got = m.key_block(hashlen, maclen, keylen, ivlen, *m.sessions_inputs(case, c))["client"]
        assert got["key"].hex() == case["keys"][c] and got["iv"].hex() == case["ivs"][c], c


def _reference_table():
    """TLS12_SUITES as the reference's id lists imply it: _getCipherSettings'
    order of tests (recordlayer.py:1022-1079), _getMacSettings' (:1081-1102;
    an id in none of its lists makes calcPendingStates raise and is left out),
    PRF hash 48 for sha384PrfSuites, TLS 1.3 ids aside."""
    f = dict((k, set(v)) for k, v in KEYS["families"].items())
    cipher = [("aes256GcmSuites", "aesgcm", 32, 4), ("aes128GcmSuites", "aesgcm", 16, 4),
              ("aes256Ccm_8Suites", "aesccm_8", 32, 4), ("aes256CcmSuites", "aesccm", 32, 4),
              ("aes128Ccm_8Suites", "aesccm_8", 16, 4), ("aes128CcmSuites", "aesccm", 16, 4),
              ("chacha20Suites", "chacha20-poly1305", 32, 12), ("chacha20draft00Suites", "chacha20-poly1305", 32, 4),
              ("aes128Suites", "aescbc", 16, 16), ("aes256Suites", "aescbc", 32, 16)]
    macs = [("aeadSuites", None, 0), ("shaSuites", "sha1", 20), ("sha256Suites", "sha256", 32),
            ("sha384Suites", "sha384", 48)]
    table = {}
    for family, alg, keylen, ivlen in cipher:
        for sid in f[family] - f["tls13Suites"]:
            if sid in table:
                continue
            mac = next(((name, size) for fam, name, size in macs if sid in f[fam]), None)
            if mac is None or (mac[0] is None) != (alg != "aescbc"):
                continue
            table[sid] = (alg, keylen, ivlen, mac[0], mac[1], 48 if sid in f["sha384PrfSuites"] else 32)
    return table


def test_suite_table_is_the_references_whole():
    from tlsgpu import keysetup
    want = _reference_table()
    assert len(want) > 60 and 0x00a3 in want and 0x00a5 in want
    assert keysetup.TLS12_SUITES == want, (sorted(set(want) ^ set(keysetup.TLS12_SUITES)),
                                            [hex(k) for k in want if keysetup.TLS12_SUITES.get(k) != want[k]])
    with pytest.raises(ValueError, match="not in TLS12_SUITES"):
        keysetup.tls12_suite(0x1301)


def test_suite_table_rows():
    from tlsgpu import keysetup
    t = keysetup.TLS12_SUITES
    assert t[0x009c] == ("aesgcm", 16, 4, None, 0, 32) and t[0x009d] == ("aesgcm", 32, 4, None, 0, 48)
    assert t[0xc0a0] == ("aesccm_8", 16, 4, None, 0, 32) and t[0xc09d] == ("aesccm", 32, 4, None, 0, 32)
    assert t[0xcca8] == ("chacha20-poly1305", 32, 12, None, 0, 32)
    assert t[0xcca1] == ("chacha20-poly1305", 32, 4, None, 0, 32)
    assert t[0x002f] == ("aescbc", 16, 16, "sha1", 20, 32) and t[0x003d] == ("aescbc", 32, 16, "sha256", 32, 32)
    assert t[0xc028] == ("aescbc", 32, 16, "sha384", 48, 48)
    assert not set(t) & set(keysetup.TLS13_SUITES)
    for case in KEYS["pending"] + KEYS["calc_key"]:
        assert case["suite_id"] in t

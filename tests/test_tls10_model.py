"""CPU: the host model of the TLS 1.0 / 1.1 PRF and key block
(tests/tls10_model.py) reproduces every output the reference gave
(tests/golden/tls10_keys.json) and the keys of the TLS 1.1 connections of
cbc_sessions.json -- which the reference derived through calcPendingStates
from master secrets the tests regenerate.  The GPU tests lean on the model for
the rows that sit beside the fixture's own, so it is pinned here first."""
import tls10_model as m
import tls12_model
from vectors import load

KEYS = load("tls10_keys.json")
TLS11_CASES = [c for c in load("cbc_sessions.json") if c["version"] == [3, 2]]


def test_fixture_covers_the_lengths_the_kernel_branches_on():
    prf = KEYS["prf"]
    msg = set(c["labellen"] + c["seedlen"] for c in prf)
    # A(0): 55/56, 119/120; A(i) || A(0): MD5 39/40, 103/104, SHA-1 35/36, 99/100; the ends
    assert msg >= {0, 35, 36, 39, 40, 55, 56, 99, 100, 103, 104, 119, 120, 160}
    assert set(c["labellen"] for c in prf) == {0, 13, 22, 32}
    assert set(c["outlen"] for c in prf) >= {1, 12, 15, 16, 17, 19, 20, 21, 48, 72, 79, 80, 81, 104, 256}
    assert set(c["secretlen"] for c in prf) == {1, 2, 47, 48, 49, 127, 128}
    assert all(len(c["out"]) == 2 * c["outlen"] for c in prf)
    assert sorted(set(tuple(c["version"]) for c in KEYS["calc_key"])) == [(3, 1), (3, 2)]
    assert len(KEYS["calc_key"]) == 2 * 4 * 2
    assert [c["suite"] for c in KEYS["pending"]] == ["TLS_RSA_WITH_AES_128_CBC_SHA", "TLS_RSA_WITH_AES_256_CBC_SHA"]


def test_model_reproduces_every_prf_entry():
    for c in KEYS["prf"]:
        secret, label, seed = m.prf_inputs(c)
        assert m.prf(secret, label, seed, c["outlen"]).hex() == c["out"], c


def test_model_reproduces_every_calc_key_entry():
    for c in KEYS["calc_key"]:
        secret, label, seed = m.calc_key_inputs(c)
        assert len(seed) == (64 if c["label"] == "master secret" else 36)
        assert m.prf(secret, label, seed, c["outlen"]).hex() == c["out"], c


def test_model_reproduces_both_sides_of_every_pending_connection():
    for case in KEYS["pending"]:
        assert m.SUITE_IDS[case["suite"]] == case["suite_id"]
        for c, conn in enumerate(case["conns"]):
            keylen = len(conn["client"]["key"]) // 2
            got = m.key_block(keylen, *m.pending_inputs(case["suite"], c))
            for side in ("client", "server"):
                assert got[side]["key"].hex() == conn[side]["key"], (case["suite"], c, side)
                assert got[side]["mac_key"].hex() == conn[side]["mac_key"], (case["suite"], c, side)


def test_model_reproduces_the_tls11_keys_of_cbc_sessions():
    assert len(TLS11_CASES) == 2 and sorted(c["etm"] for c in TLS11_CASES) == [0, 1]
    pairs = 0
    for case in TLS11_CASES:
        assert case["suite"] == "TLS_RSA_WITH_AES_128_CBC_SHA" and case["mac"] == "sha1"
        for c in range(5):
            got = m.key_block(16, *tls12_model.cbc_sessions_inputs(case, c))["client"]
            assert got["key"].hex() == case["enc_keys"][c] and got["mac_key"].hex() == case["mac_keys"][c], c
            pairs += 1
    assert pairs == 10

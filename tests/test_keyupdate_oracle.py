"""Pin the KeyUpdate fixture (tests/golden/keyupdate.json, the reference
RecordLayer's own output for four connections per suite across two rounds of
calcTLS1_3KeyUpdate_reciever, from make_golden_keyupdate.py) and the oracles
against each other: oracle.keysetup's key_update / traffic_keys, chained,
give every secret, key and IV the reference held after each phase, and
oracle.records seals every record to the reference's wire bytes."""
import hashlib

import pytest

from vectors import detbytes, load
from oracle import keysetup as K
from oracle import records as R

CASES = load("keyupdate.json")


def test_fixture_shape():
    assert [(c["alg"], c["suite"], c["hashlen"]) for c in CASES] == [
        ("aes128gcm", 0x1301, 32), ("aes256gcm", 0x1302, 48), ("chacha20-poly1305", 0x1303, 32),
        ("aes128ccm_8", 0x1305, 32)]
    for c in CASES:
        assert c["starts"] == [2 ** 32 - 2, 0, 0, 0] and c["updates"] == [[1, 3], [1, 0]]
        assert len(c["phases"]) == 3 and len(set(c["initial_secrets"])) == 4
        lens = {r["len"] for p in c["phases"] for r in p["records"]}
        assert lens == {0, 1, 15, 16, 17, 100, 1000, 16384}
        for p in c["phases"]:
            assert {r["conn"] for r in p["records"]} == {0, 1, 2, 3}
        # connection 0 is past 2^32 before its update and restarts at 0
        assert c["phases"][1]["after"][0]["seqnum"] > 2 ** 32
        assert c["phases"][2]["after"][0]["seqnum"] == sum(r["conn"] == 0 for r in c["phases"][2]["records"])
        # connection 2 never updates: one secret throughout
        assert {p["after"][2]["secret"] for p in c["phases"]} == {c["initial_secrets"][2]}
        # connection 1 reaches a second generation: three distinct secrets
        assert len({p["after"][1]["secret"] for p in c["phases"]}) == 3


@pytest.mark.parametrize("ci", range(len(CASES)))
def test_chained_oracle_reproduces_reference_states_and_records(ci):
    c = CASES[ci]
    suite = c["suite"]
    secrets = [bytes.fromhex(s) for s in c["initial_secrets"]]
    seq = list(c["starts"])
    for p, phase in enumerate(c["phases"]):
        keys = [K.traffic_keys(suite, s) for s in secrets]
        for r in phase["records"]:
            s = r["conn"]
            data = detbytes("kurec-%d-%d" % (r["index"], r["len"]), r["len"])
            wire = R.seal_record("tls13", c["alg"], keys[s][0], keys[s][1], seq[s], r["ctype"], data, r["pad"])
            assert len(wire) == r["wire_len"], r["index"]
            assert hashlib.sha256(wire).hexdigest() == r["wire_sha256"], r["index"]
            if "wire" in r:
                assert wire.hex() == r["wire"], r["index"]
            seq[s] += 1
        for s, st in enumerate(phase["after"]):
            assert secrets[s].hex() == st["secret"], (p, s)
            assert (keys[s][0].hex(), keys[s][1].hex()) == (st["key"], st["iv"]), (p, s)
            assert seq[s] == st["seqnum"], (p, s)
        if p < len(c["updates"]):
            for s in c["updates"][p]:
                secrets[s] = K.key_update(suite, secrets[s])
                seq[s] = 0

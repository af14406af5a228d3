"""Pin the many-session fixture (tests/golden/sessions.json, the reference
RecordLayer's own output for five interleaved connections per suite, from
make_golden_sessions.py) and the framing oracle (oracle/records.py) against
each other: each record sealed under its connection's key and IV with the
connection's running sequence number gives the reference's wire bytes."""
import hashlib

import pytest

from vectors import detbytes, load
from oracle import records as R

CASES = load("sessions.json")


def test_fixture_shape():
    assert [(c["version"], c["alg"]) for c in CASES] == [
        ("tls13", "aes128gcm"), ("tls13", "chacha20-poly1305"), ("tls13", "aes128ccm_8"),
        ("tls12", "aes256gcm"), ("tls12", "chacha20-poly1305")]
    for c in CASES:
        assert c["starts"] == [0, 1, 2 ** 32 - 2, 2 ** 40 + 3, 255]
        assert len(set(c["keys"])) == 5 and len(set(c["ivs"])) == 5
        counts = [sum(1 for r in c["records"] if r["conn"] == k) for k in range(5)]
        assert counts == [10, 9, 20, 1, 0]
        assert {r["len"] for r in c["records"]} == {0, 1, 15, 16, 17, 100, 1000, 16384}
        if c["version"] == "tls13":
            assert len({r["pad"] for r in c["records"]}) > 4


@pytest.mark.parametrize("ci", range(len(CASES)))
def test_interleaved_seal_matches_reference(ci):
    c = CASES[ci]
    keys = [bytes.fromhex(k) for k in c["keys"]]
    ivs = [bytes.fromhex(v) for v in c["ivs"]]
    seq = list(c["starts"])
    for i, r in enumerate(c["records"]):
        s = r["conn"]
        data = detbytes("srec-%d-%d" % (i, r["len"]), r["len"])
        wire = R.seal_record(c["version"], c["alg"], keys[s], ivs[s], seq[s], r["ctype"], data, r["pad"])
        assert len(wire) == r["wire_len"], i
        assert hashlib.sha256(wire).hexdigest() == r["wire_sha256"], i
        if "wire" in r:
            assert wire.hex() == r["wire"], i
        assert R.open_record(c["version"], c["alg"], keys[s], ivs[s], seq[s], wire) \
            == (R.OK, r["ctype"], bytes(data)), i
        seq[s] += 1

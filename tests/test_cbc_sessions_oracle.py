"""The CPU model (tests/cbc_model.py) against the reference's many-session
AES-CBC + HMAC fixtures (tests/golden/cbc_sessions.json): every record of
every connection from (the session's keys, its number, the record's IV), every
receive verdict, and the two wrong-context verdicts -- another session's keys,
the neighbour's number -- that the reference calls TLSBadRecordMAC."""
import hashlib
import json
import os

import pytest

import cbc_model
from conftest import ROOT
from vectors import detbytes

CASES = json.load(open(os.path.join(ROOT, "tests", "golden", "cbc_sessions.json")))
IDS = ["%s-%d.%d-%s" % (c["suite"], c["version"][0], c["version"][1], "etm" if c["etm"] else "mte")
       for c in CASES]


def record_data(i, rec):
    return bytes(detbytes("cbcs-%d-%d" % (i, rec["len"]), rec["len"]))


def wire_matches(rec, wire):
    """The fixture stores short records whole, long ones as hash, head and tail."""
    if len(wire) != rec["wire_len"]:
        return False
    if "wire" in rec:
        return wire.hex() == rec["wire"]
    return (hashlib.sha256(wire).hexdigest() == rec["wire_sha256"] and wire[:32].hex() == rec["wire_head"]
            and wire[-16:].hex() == rec["wire_tail"])


def test_fixture_shape():
    assert len(CASES) == 8 and os.path.getsize(os.path.join(ROOT, "tests", "golden", "cbc_sessions.json")) <= \
        os.path.getsize(os.path.join(ROOT, "tests", "golden", "cbc.json"))
    for case in CASES:
        assert case["starts"] == [0, 1, 2 ** 32 - 2, 2 ** 40 + 3, 255]
        assert len(set(zip(case["enc_keys"], case["mac_keys"]))) == 5
        per = [sum(1 for r in case["records"] if r["conn"] == c) for c in range(5)]
        assert sorted(per) == [0, 1, 9, 10, 20]
        assert sum(1 for r in case["records"] if r["len"] == 16384) == 1
        assert sum(1 for r in case["records"] if "cross" in r) >= 3
        # each connection's numbers run from its start in batch order
        for c in range(5):
            seqs = [r["seq"] for r in case["records"] if r["conn"] == c]
            assert seqs == list(range(case["starts"][c], case["starts"][c] + len(seqs)))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_model_reproduces_every_record_and_verdict(case):
    version = case["version"][0] << 8 | case["version"][1]
    keys = [(bytes.fromhex(e), bytes.fromhex(m)) for e, m in zip(case["enc_keys"], case["mac_keys"])]
    mac, etm = case["mac"], case["etm"]
    for i, rec in enumerate(case["records"]):
        ek, mk = keys[rec["conn"]]
        data = record_data(i, rec)
        wire = cbc_model.seal_record(ek, mk, mac, version, etm, rec["seq"], rec["ctype"], data,
                                     bytes.fromhex(rec["iv"]))
        assert wire_matches(rec, wire), (i, rec["conn"], rec["len"])
        assert cbc_model.open_record(ek, mk, mac, version, etm, rec["seq"], wire) == (rec["recv"], rec["ctype"], data)
        if "cross" in rec:
            x = rec["cross"]
            ok, omk = keys[x["other_conn"]]
            assert cbc_model.open_record(ok, omk, mac, version, etm, rec["seq"], wire)[0] == x["other_keys"]
            assert cbc_model.open_record(ek, mk, mac, version, etm, x["other_seq"], wire)[0] == x["neighbour_number"]
            assert x["other_keys"] == x["neighbour_number"] == "TLSBadRecordMAC"

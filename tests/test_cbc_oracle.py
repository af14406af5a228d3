"""The CPU model of the AES-CBC + HMAC record path (tests/cbc_model.py)
against the reference's fixtures (tests/golden/cbc.json, written by
make_golden_cbc.py from the reference's RecordLayer): every sealed record is
reproduced bit for bit from its key, IV and sequence number alone -- no CBC
state is carried from record to record -- and every receive-side verdict, for
valid and malformed records, is the reference's."""
import hashlib
import json
import os

import pytest

import cbc_model
from conftest import ROOT
from vectors import detbytes

CASES = json.load(open(os.path.join(ROOT, "tests", "golden", "cbc.json")))
IDS = ["%s-%d.%d-%s" % (c["suite"], c["version"][0], c["version"][1], "etm" if c["etm"] else "mte")
       for c in CASES]


def test_fixture_coverage():
    assert len(CASES) == 8
    assert {(c["mac"], c["etm"]) for c in CASES} == {(m, e) for m in ("sha1", "sha256", "sha384") for e in (0, 1)}
    assert {tuple(c["version"]) for c in CASES} == {(3, 2), (3, 3)}
    assert {len(bytes.fromhex(c["enc_key"])) for c in CASES} == {16, 32}
    for etm in (0, 1):
        seen = {o["recv"] for c in CASES if c["etm"] == etm for o in c["open"]}
        assert seen == {"ok", "TLSBadRecordMAC", "TLSDecryptionFailed", "TLSRecordOverflow"}
    lens = {r["len"] for c in CASES for r in c["seal"]}
    assert {0, 1, 16383, 16384} <= lens
    assert {r["ctype"] for c in CASES for r in c["seal"]} == {21, 22, 23}


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_model_reproduces_sealed_records(case):
    ek, mk = bytes.fromhex(case["enc_key"]), bytes.fromhex(case["mac_key"])
    version = case["version"][0] << 8 | case["version"][1]
    for i, rec in enumerate(case["seal"]):
        data = detbytes("cbc-%d-%d" % (i, rec["len"]), rec["len"])
        wire = cbc_model.seal_record(ek, mk, case["mac"], version, case["etm"], case["seq0"] + i,
                                     rec["ctype"], data, bytes.fromhex(rec["iv"]))
        assert len(wire) == rec["wire_len"] == cbc_model.wire_len(case["mac"], case["etm"], rec["len"])
        assert hashlib.sha256(wire).hexdigest() == rec["wire_sha256"], (i, rec["len"])
        if "wire" in rec:
            assert wire.hex() == rec["wire"]
        if rec["len"] <= 300:   # the 16 KiB ones cost the bytewise inverse cipher a second each
            assert cbc_model.open_record(ek, mk, case["mac"], version, case["etm"], case["seq0"] + i,
                                         wire) == ("ok", rec["ctype"], data)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_model_agrees_with_every_receive_verdict(case):
    ek, mk = bytes.fromhex(case["enc_key"]), bytes.fromhex(case["mac_key"])
    version = case["version"][0] << 8 | case["version"][1]
    for o in case["open"]:
        verdict, ctype, plain = cbc_model.open_record(ek, mk, case["mac"], version, case["etm"], o["seq"],
                                                      bytes.fromhex(o["wire"]), o["recv_limit"])
        assert verdict == o["recv"], o["name"]
        if verdict == "ok":
            assert ctype == o["ctype"] and plain.hex() == o["plain"], o["name"]

"""CPU: the hashlib / hmac model of the TLS 1.3 key schedule (tests/tls13_model.py)
reproduces every row the reference wrote into tests/golden/tls13_schedule.json,
and RFC 5869's first test case.  The GPU tests lean on the model for the rows
of a batch beside the fixture's own, so this is what holds it."""
import os

import tls13_model as m
from vectors import GOLDEN_DIR, load

F = load("tls13_schedule.json")
H = bytes.fromhex


def test_fixture_has_every_group_and_stays_small():
    assert sorted(F) == ["binder", "derive", "expand", "extract", "res_psk", "schedule"]
    assert len(F["extract"]) == 2 * (18 + 2)
    assert len(F["expand"]) == 2 * (6 * 4 + 2)
    assert len(F["derive"]) == 2 * 4 * 2
    assert len(F["schedule"]) == 2 * 6
    assert len(F["binder"]) == 2 * 4 * 2 and len(F["res_psk"]) == 2 * 3
    size = os.path.getsize(os.path.join(GOLDEN_DIR, "tls13_schedule.json"))
    assert size <= os.path.getsize(os.path.join(GOLDEN_DIR, "cbc.json"))


def test_rfc5869_case_1():
    """RFC 5869 A.1 (SHA-256).  Its salt has 13 bytes, so it exercises the
    model only: the device's Extract takes salts of the hash length (the only
    kind the TLS 1.3 schedule has)."""
    prk = m.extract("sha256", H("000102030405060708090a0b0c"), H("0b" * 22))
    assert prk.hex() == "077709362c2e32df0ddc3f0dc47bba6390b6c73bb50f9c3122ec844ad7c2b3e5"


def test_extract_rows():
    lengths = set()
    for c in F["extract"]:
        salt, ikm = m.extract_inputs(c)
        assert m.extract(c["hash"], salt, ikm).hex() == c["out"], c
        lengths.add((c["hash"], c["ikmlen"], c["salt"], c["ikm"]))
    for alg in ("sha256", "sha384"):   # the block boundaries of both hashes, for both
        for n in (1, 55, 56, 63, 64, 65, 111, 112, 119, 120, 239, 240, 1024):
            assert (alg, n, "det", "det") in lengths
        assert (alg, 32, "zero", "det") in lengths and (alg, m.HASHLEN[alg], "det", "zero") in lengths


def test_expand_rows():
    for c in F["expand"]:
        secret, label, ctx = m.expand_inputs(c)
        assert m.expand_label(c["hash"], secret, label, ctx, c["outlen"]).hex() == c["out"], c
    # the SHA-256 message is 11 + label + context bytes; 55 fill one block
    shapes = set((c["hash"], c["labellen"], c["ctxlen"]) for c in F["expand"])
    assert ("sha256", 12, 32) in shapes and ("sha256", 13, 32) in shapes and ("sha384", 32, 64) in shapes
    assert len(m.hkdf_label(bytes(12), bytes(32), 32)) + 1 == 55


def test_derive_rows():
    for c in F["derive"]:
        secret, label, digest = m.derive_inputs(c)
        assert m.derive_secret(c["hash"], secret, label, digest).hex() == c["out"], c
    assert set(c["transcript"] for c in F["derive"]) == {True, False}


def test_schedule_rows():
    for c in F["schedule"]:
        alg = c["hash"]
        psk, shared = m.schedule_inputs(c)
        assert m.extract(alg, None, psk).hex() == c["early"]
        hs, c_hs, s_hs = m.handshake_secrets(alg, psk, shared, H(c["hello_hash"]))
        assert (hs.hex(), c_hs.hex(), s_hs.hex()) == (c["handshake_secret"], c["c_hs"], c["s_hs"]), c["conn"]
        assert m.finished(alg, s_hs, H(c["verify_hash"])).hex() == c["server_finished"]
        master, c_ap, s_ap, exp = m.application_secrets(alg, hs, H(c["finished_hash"]))
        assert (master.hex(), c_ap.hex(), s_ap.hex(), exp.hex()) == (c["master"], c["c_ap"], c["s_ap"],
                                                                     c["exp_master"]), c["conn"]
        assert m.finished(alg, c_hs, H(c["finished_hash"])).hex() == c["client_finished"]
        assert m.derive_secret(alg, master, b"res master", H(c["resumption_hash"])).hex() == c["res_master"]
        for name, k in c["keys"].items():
            for which in ("c_hs", "s_hs", "c_ap", "s_ap"):
                key, iv = m.traffic_key_iv(alg, H(c[which]), len(k[which]["key"]) // 2)
                assert (key.hex(), iv.hex()) == (k[which]["key"], k[which]["iv"]), (name, which)
    kinds = set((c["hash"], c["psk"], c["sharedlen"]) for c in F["schedule"])
    assert set(k[2] for k in kinds) == {32, 48, 66, 256} and set(k[1] for k in kinds) == {True, False}


def test_binder_rows():
    for c in F["binder"]:
        psk, digest = m.binder_inputs(c)
        assert m.binder(c["hash"], psk, digest, c["external"]).hex() == c["out"], c
    for c in F["res_psk"]:
        res_master, nonce = m.res_psk_inputs(c)
        assert m.resumption_psk(c["hash"], res_master, nonce).hex() == c["out"], c

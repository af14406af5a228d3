"""The padding grid (tests/cbc_grid.py) on the CPU: the wires rebuilt here
from the CPU model's AES are the bytes the reference judged (their SHA-256 is
in tests/golden/cbc_grid.json, written by make_golden_cbc_grid.py from the
reference's RecordLayer), the model gives the reference's verdict and length
for every one of them, and the grid covers what it claims to cover."""
import json
import os

import pytest

import cbc_grid
import cbc_model
from conftest import ROOT

GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "cbc_grid.json")))
IDS = [cbc_grid.grid_id(c, m) for c, m in cbc_grid.GRIDS]


def test_golden_names_every_grid():
    assert sorted(GOLDEN) == sorted(IDS)
    for cfg, mode in cbc_grid.GRIDS:
        g = GOLDEN[cbc_grid.grid_id(cfg, mode)]
        assert g["records"] == len(g["verdicts"]) == len(cbc_grid.plan(cfg, mode))
        assert set(g["verdicts"]) <= {"o", "m"}
        assert len(g["lengths"]) == g["verdicts"].count("o")
    # the case counts: valid records per MtE grid, and as many mutated twins
    valid = {i: sum(c.kind is None for c in cbc_grid.plan(cfg, m)) for (cfg, m), i in zip(cbc_grid.GRIDS, IDS)}
    assert (valid["aes128-sha1/mte"], valid["aes256-sha256/mte"], valid["aes256-sha384/mte"]) == (1772, 1744, 1680)
    assert valid["aes128-sha1/etm"] == valid["aes256-sha384/etm"] == 16 + 32 + 240 + 3 * 256
    assert all(GOLDEN[i]["records"] == 2 * v for i, v in valid.items())


@pytest.mark.parametrize("grid", cbc_grid.GRIDS, ids=IDS)
def test_wires_are_the_generators(grid):
    cfg, mode = grid
    recs, wires = cbc_grid.model_grid(cfg, mode)
    assert cbc_grid.wires_digest(wires) == GOLDEN[cbc_grid.grid_id(cfg, mode)]["wires_sha256"]
    assert max(len(w) for w in wires) <= 5 + 16 + 528 + (cbc_grid.DIGEST[cfg.mac] if mode == "etm" else 0)


@pytest.mark.parametrize("grid", cbc_grid.GRIDS, ids=IDS)
def test_model_gives_the_reference_verdicts(grid):
    cfg, mode = grid
    recs, wires = cbc_grid.model_grid(cfg, mode)
    want = cbc_grid.expected(GOLDEN, cfg, mode)
    enc_key, mac_key = cbc_grid.keys(cfg)
    for r, w, (verdict, length) in zip(recs, wires, want):
        got = cbc_model.open_record(enc_key, mac_key, cfg.mac, cfg.version, mode == "etm", r.seq, w)
        assert got[0] == verdict and len(got[2]) == length, (r.case, got[0], len(got[2]), verdict, length)
        assert got[1] == r.ctype, r.case
        if verdict == "ok":
            assert got[2] == r.body[:length], r.case
        if mode == "mte":   # the cipher-free half of the model, as the host check of the device code uses it
            data = cbc_model.mte_check(mac_key, cfg.mac, cfg.version, r.seq, r.ctype, r.body)
            assert (data is None, len(data or b"")) == (verdict != "ok", length), r.case


@pytest.mark.parametrize("grid", cbc_grid.GRIDS, ids=IDS)
def test_grid_covers_what_it_claims(grid):
    cfg, mode = grid
    cases = cbc_grid.plan(cfg, mode)
    want = cbc_grid.expected(GOLDEN, cfg, mode)
    d = cbc_grid.DIGEST[cfg.mac]
    assert [c.kind is None for c in cases] == [i % 2 == 0 for i in range(len(cases))]
    for c, (verdict, length) in zip(cases, want):
        if c.kind is None:      # every unmutated record is accepted, with its whole fragment
            assert (verdict, length) == ("ok", c.n - 1 - c.pad - (d if mode == "mte" else 0)), c
        elif c.kind != "len":   # a lying length byte may by chance say the truth; nothing else may pass
            assert verdict == "TLSBadRecordMAC", c
    lying = [(c, v) for c, (v, _) in zip(cases, want) if c.kind == "len"]
    assert sum(v != "ok" for _, v in lying) > 0.9 * len(lying) > 100
    for c, v in lying:          # accepted only where the clamp to 255 gives back the record's own padding
        assert (v == "ok") == (c.val == c.pad), c
    kinds = {c.kind for c in cases}
    assert kinds == ({None, "pad", "mac", "frag", "len"} if mode == "mte" else {None, "pad", "len"})
    # sequence numbers: the low word carries inside the grid
    assert cbc_grid.SEQ0 < 2 ** 32 < cbc_grid.SEQ0 + len(cases)
    pads = [c for c in cases if c.kind == "pad"]
    assert all(c.n - 1 - c.pad <= c.pos < c.n - 1 for c in pads)
    assert sum(c.pos == c.n - 1 - c.pad for c in pads) >= len(pads) // 4     # the first padding byte
    assert any(c.n - 256 <= c.pos < c.n - 240 for c in pads)                  # in the first block of the 256-byte window
    if mode == "etm":
        assert {c.val for c in cases if c.kind == "len"} >= {16, 17, 32, 33, 240, 241, 255}
        return
    valid = [c for c in cases if c.kind is None]
    block = cbc_grid.HASH_BLOCK[cfg.mac]
    if cfg.max_n is None:
        # where the message ends inside a hash block: every residue
        assert {cbc_grid.mte_message_end(cfg, c) % block for c in valid} == set(range(block))
        # how many compression calls before the last one the digest is taken
        assert {cbc_grid.mte_block_gap(cfg, c) for c in valid} == set(range(3 if block == 128 else 5))
    else:
        assert cfg.version == cbc_grid.TLS11 and max(c.n for c in cases) == cfg.max_n
    assert min(cbc_grid.mte_block_gap(cfg, c) for c in valid) == 0
    # every MAC byte is flipped somewhere, first and last included
    macs = {c.pos - (c.n - d - 1 - c.pad) for c in cases if c.kind == "mac"}
    assert macs == set(range(d))
    # lying length bytes make pad_start clamp (value >= n) and mac_start clamp (pad_start < D)
    assert any(c.val >= c.n for c in cases if c.kind == "len")
    assert any(c.n - d <= c.val < c.n for c in cases if c.kind == "len")
    assert any(c.val == 255 and c.n > 256 + d for c in cases if c.kind == "len")

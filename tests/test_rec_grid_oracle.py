"""The AEAD record grid (tests/rec_grid.py) on the CPU: the wires rebuilt here
with the C oracle's AEAD are the bytes the reference judged (their SHA-256 is
in tests/golden/rec_grid.json, written by make_golden_rec_grid.py from the
reference's RecordLayer), the framing oracle (oracle/records.py) gives the
status, content type and length that the reference's verdict maps to for
every one of them, the grid covers what it claims to cover, and the grid
check fails at a named class and record for each planted fault."""
import itertools
import json
import os

import pytest

import rec_grid as G
from conftest import ROOT
from oracle import records as R

GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "rec_grid.json")))


def test_status_codes_are_the_oracles():
    assert (G.OK, G.BAD_MAC, G.TRUNCATED, G.LENGTH, G.BAD_TYPE, G.BAD_VERSION, G.NO_CONTENT_TYPE, G.OVERFLOW) == (
        R.OK, R.BAD_MAC, R.TRUNCATED, R.LENGTH, R.BAD_TYPE, R.BAD_VERSION, R.NO_CONTENT_TYPE, R.OVERFLOW)
    assert [G.taglen(c) for c in G.GRIDS] == [R.taglen(c.alg) for c in G.GRIDS]


def test_golden_names_every_grid():
    assert sorted(GOLDEN) == sorted(G.IDS) and len(set(G.IDS)) == len(G.GRIDS) == 8
    for cfg in G.GRIDS:
        g = GOLDEN[G.grid_id(cfg)]
        n = len(G.plan(cfg))
        # no record of the plan is left unjudged
        assert g["records"] == len(g["verdicts"]) == len(g["advanced"]) == len(g["direct"]) == n
        assert set(g["verdicts"]) <= set(G.CHAR_VERDICT)
        assert len(g["lengths"]) == len(g["types"]) == g["verdicts"].count("o")
    assert [GOLDEN[i]["records"] for i in G.IDS] == [339, 339, 315, 90, 90, 78, 10, 8]


def _open(cfg, b, limit=None):
    key, iv = G.keys(cfg)
    st, ct, pt = R.open_record(cfg.version, cfg.alg, key, iv, b.seq, b.wire, cfg.limit if limit is None else limit)
    return st, ct, pt


@pytest.mark.parametrize("cfg", G.GRIDS, ids=G.IDS)
def test_wires_are_the_generators(oracle_mod, cfg):
    built = G.oracle_grid(cfg, oracle_mod)
    assert G.wires_digest([b.wire for b in built]) == GOLDEN[G.grid_id(cfg)]["wires_sha256"]
    assert "".join("1" if G.direct(b.wire) else "0" for b in built) == GOLDEN[G.grid_id(cfg)]["direct"]
    assert sum(len(b.wire) >= 2 ** 14 for b in built) <= 11


@pytest.mark.parametrize("cfg", G.GRIDS, ids=G.IDS)
def test_oracle_gives_the_reference_verdicts(oracle_mod, cfg):
    built = G.oracle_grid(cfg, oracle_mod)
    want = G.expected(GOLDEN, cfg, built)
    got = [_open(cfg, b) for b in built]
    G.check(cfg, [b.spec for b in built], want, [(st, ct, len(pt)) for st, ct, pt in got])
    for b, w, (st, ct, pt) in zip(built, want, got):
        if st == R.OK:
            assert b.plain.startswith(pt), b.spec
        # what the record leaves in the data buffer is decided by its status and its length alone
        img = G.data_image(cfg, b, w)
        assert (img is None) == (st in (R.TRUNCATED, R.LENGTH, R.BAD_TYPE, R.BAD_VERSION)
                                 or (st == R.OVERFLOW and G.header_overflow(cfg, b.wire))), b.spec


@pytest.mark.parametrize("cfg", G.GRIDS[:6], ids=G.IDS[:6])
def test_runt_wires_are_the_projects_own_statement(oracle_mod, cfg):
    """Wire lengths 0..4 cannot reach the reference's RecordLayer (its socket
    waits for a header): include/tlsgpu.h says TRUNCATED, type 0, length 0."""
    key, iv = G.keys(cfg)
    wire = G.oracle_grid(cfg, oracle_mod)[1].wire
    for k in range(5):
        assert R.open_record(cfg.version, cfg.alg, key, iv, G.SEQ0, wire[:k], cfg.limit) == (R.TRUNCATED, 0, b"")


@pytest.mark.parametrize("cfg", G.GRIDS, ids=G.IDS)
def test_sequence_numbers_the_reference_does_not_consume(oracle_mod, cfg):
    """include/tlsgpu.h: the device gives every record of a session a number;
    the reference gives none to a record refused by the header's length and
    none to an unprotected record -- and to every other record one."""
    built = G.oracle_grid(cfg, oracle_mod)
    for b, w in zip(built, G.expected(GOLDEN, cfg, built)):
        none = w.verdict == "unprotected" or (w.verdict == "TLSRecordOverflow" and G.header_overflow(cfg, b.wire))
        assert w.advanced == (not none), b.spec
    assert any(G.header_overflow(cfg, b.wire) for b in built)
    assert G.SEQ0 < 2 ** 32 <= G.SEQ0 + len(built) - 1      # the low word carries inside the grid


@pytest.mark.parametrize("gid", G.SESSION_GRIDS)
def test_verdicts_do_not_depend_on_the_session(oracle_mod, gid):
    """The many-session GPU test seals the grid again under three sessions'
    keys and counters: the oracle's statuses are those of the fixture."""
    cfg = G.GRIDS[G.IDS.index(gid)]
    n = len(G.plan(cfg))
    sessions, seqs, nxt = G.deal(n)
    assert [a - b for a, b in zip(nxt, G.SESSION_STARTS)] == [len(range(s, n, 3)) - (s == G.SKIPPED % 3) for s in range(3)]
    assert all(a < 2 ** 32 <= b for a, b in list(zip(G.SESSION_STARTS, nxt))[:2])   # both carry
    built = G.build(cfg, G.oracle_seal(oracle_mod), sessions, seqs)
    want = G.expected(GOLDEN, cfg, built)
    got = []
    for i, b in enumerate(built):
        if seqs[i] is None:
            got.append(tuple(want[i][:3]))
            continue
        key, iv = G.keys(cfg, sessions[i])
        st, ct, pt = R.open_record(cfg.version, cfg.alg, key, iv, seqs[i], b.wire, cfg.limit)
        got.append((st, ct, len(pt)))
    G.check(cfg, [b.spec for b in built], want, got)


@pytest.mark.parametrize("cfg", G.GRIDS, ids=G.IDS)
def test_grid_covers_what_it_claims(oracle_mod, cfg):
    built = G.oracle_grid(cfg, oracle_mod)
    specs = [b.spec for b in built]
    want = G.expected(GOLDEN, cfg, built)
    tls13, T, E = cfg.version == "tls13", G.taglen(cfg), G.explicit(cfg)
    assert {s.cls for s in specs} == set(cfg.classes)
    # an unmutated record is accepted, unless the plan built it to break a limit or to hold no type
    for s, w in zip(specs, want):
        if not s.muts and s.raw is None and not s.delta and s.cls in "acdf":
            assert w.verdict == "ok", s
        if s.cls == "f" and (s.muts or s.delta):
            assert w.status == G.BAD_MAC, s
    # class e: the bad tag wins over a refusal after decryption, the header's overflow over the bad tag
    lim = [(b, w) for b, w in zip(built, want) if b.spec.cls == "e"]
    assert len(lim) == (10 if tls13 else 8)
    for (b, w), (b2, w2) in zip(lim[0::2], lim[1::2]):
        assert b2.spec.muts == (G.BAD_TAG,) and b2.spec.name == b.spec.name + ", bad tag"
        assert w2.status == (G.OVERFLOW if G.header_overflow(cfg, b.wire) else G.BAD_MAC), b.spec
    assert [w.status for _, w in lim[0::2]] == ([G.OK, G.OK, G.OVERFLOW, G.OVERFLOW, G.OVERFLOW] if tls13 else
                                               [G.OK, G.OVERFLOW, G.OVERFLOW, G.OVERFLOW])
    assert [len(b.wire) - 5 - cfg.limit for b, _ in lim[0::2]] == (
        [1 + T, 1 + T, 2 + T, 256, 257] if tls13 else [E + T, 1 + E + T, 2048, 2049])
    if cfg.classes == "e":
        return
    # every status code occurs where the version can produce it
    assert {w.status for w in want} == (set(range(8)) if tls13 else {G.OK, G.BAD_MAC, G.TRUNCATED, G.OVERFLOW})
    # class a: every wire length from 5 to one byte of ciphertext, truncated below nonce + tag
    cuts = [(b, w) for b, w in zip(built, want) if b.spec.cls == "a" and G.has(b.spec, "cut")]
    assert [len(b.wire) for b, _ in cuts] == list(range(5, 5 + E + T + 2))
    assert [w.status for _, w in cuts] == [G.TRUNCATED] * (E + T) + [G.BAD_MAC] * 2
    assert [(w.status, w.length) for b, w in zip(built, want) if b.spec.name == "shortest"] == [(G.OK, 0)]
    # class f: every tag byte, both bits
    flips = [m for s in specs if s.cls == "f" for m in s.muts if m[1] < 0]
    assert {m[1] for m in flips} == set(range(-T, 0)) and {m[2] for m in flips} == {0x01, 0x80}
    if not tls13:
        d = [(s, w) for s, w in zip(specs, want) if s.cls == "d" and s.muts]
        assert [w.status for s, w in d if G.has(s, "ver")] == [G.OK, G.OK]      # the reference ignores the version
        assert all(w.status == G.BAD_MAC for s, w in d if not G.has(s, "ver")) and len(d) == (6 if E else 4)
        return
    # class b: every (inner length <= 33, last non-zero position) pair, and the all-zero inner plaintext
    inner = {}
    for b, w in zip(built, want):
        if b.spec.cls == "b" and b.spec.name.startswith("inner "):
            n = len(b.plain)
            last = max([k for k in range(n) if b.plain[k]], default=None)
            inner.setdefault(n, set()).add(last)
            assert (w.status, w.ctype, w.length) == ((G.NO_CONTENT_TYPE, 0, 0) if last is None else
                                                     (G.OK, b.plain[last], last)), b.spec
    for n in G.SMALL_INNER:
        assert inner[n] == set(range(n)) | {None}
    for n in G.LARGE_INNER:
        edge = (n - 1) // 16 * 16
        assert inner[n] >= {None, 0, 1, n - 1, edge - 1, edge, edge - 16, edge - 17}
    assert {w.ctype for s, w in zip(specs, want) if s.cls == "b" and w.status == G.OK} == set(G.INNER_TYPES)
    pad_to_limit = [(b, w) for b, w in zip(built, want) if b.spec.name == "empty fragment, limit zeros"]
    assert [(len(b.plain), w.status, w.length) for b, w in pad_to_limit] == [(cfg.limit + 1, G.OK, 0)]
    # class c: every single fault, every pair and the triple of {type, version, length};
    # type before version before length, the cut before all of them
    combos = {tuple(k for k in ("type", "ver", "len") if G.has(s, k)) for s in specs if s.cls == "c" and s.muts}
    fields = ("type", "ver", "len")
    assert combos == {c for r in (1, 2, 3) for c in itertools.combinations(fields, r)}
    for b, w in zip(built, want):
        s = b.spec
        if s.cls == "c" and s.muts:
            first = (G.TRUNCATED if G.has(s, "cut") else G.BAD_TYPE if G.has(s, "type") else
                     G.BAD_VERSION if G.has(s, "ver") else G.LENGTH)
            assert w.status == first, s
    assert sum(G.has(s, "cut") for s in specs if s.cls == "c") == sum(
        G.BAD_TAG in s.muts for s in specs if s.cls == "c") == len(G.HEADER_FAULTS)
    # class g: what the reference passes through, and the same alert once numbers have been used
    g = dict((s.name, w.verdict) for s, w in zip(specs, want) if s.cls == "g")
    assert specs[0].name == "2-byte alert as record 0" and set(g) == set(G.OUTSIDE_REMIT) | {
        "2-byte alert later in the batch"}
    assert all(g[name] == "unprotected" for name in G.OUTSIDE_REMIT)
    assert g["2-byte alert later in the batch"] == "TLSBadRecordMAC"


# ---- planted faults: the oracle standing in for the device ----------------------------------

def _last_nonzero(b):
    return max([k for k in range(len(b.plain)) if b.plain[k]], default=None)


def depad_stops_at_one(cfg, b, st, ct, n):
    """while (pos > 1 && ...): an all-zero inner plaintext is "type 0, empty"."""
    return (R.OK, 0, 0) if st == R.NO_CONTENT_TYPE else (st, ct, n)


def limit_plus_one_read_as_limit(cfg, b, st, ct, n):
    inner = len(b.wire) - 5 - G.taglen(cfg)
    return (R.OVERFLOW, 0, 0) if cfg.version == "tls13" and st == R.OK and inner > cfg.limit else (st, ct, n)


def type_and_version_swapped(cfg, b, st, ct, n):
    return (R.BAD_VERSION, 0, 0) if st == R.BAD_TYPE and b.wire[1:3] != b"\x03\x03" else (st, ct, n)


def tls12_check_after_decryption_dropped(cfg, b, st, ct, n):
    if cfg.version == "tls12" and st == R.OVERFLOW and not G.header_overflow(cfg, b.wire):
        return R.OK, b.wire[0], len(b.plain)
    return st, ct, n


def data_len_left_on_a_refused_record(cfg, b, st, ct, n):
    if cfg.version == "tls12" and st == R.OVERFLOW and not G.header_overflow(cfg, b.wire):
        return st, b.wire[0], len(b.plain)
    return st, ct, n


PLANTED = [(depad_stops_at_one, "tls13/aes128gcm", "b", "inner 1 all zero"),
           (depad_stops_at_one, "tls13/aes128ccm_8", "b", "inner 4097 all zero"),
           (limit_plus_one_read_as_limit, "tls13/chacha20-poly1305", "e", "inner limit+1"),
           (limit_plus_one_read_as_limit, "tls13/aes128gcm@512", "e", "inner limit+1, padded"),
           (limit_plus_one_read_as_limit, "tls13/aes128gcm", "b", "empty fragment, limit zeros"),
           (type_and_version_swapped, "tls13/aes128gcm", "c", "type+version"),
           (type_and_version_swapped, "tls13/chacha20-poly1305", "c", "type+version+length, bad tag"),
           (tls12_check_after_decryption_dropped, "tls12/aes256gcm", "e", "plaintext limit+1"),
           (tls12_check_after_decryption_dropped, "tls12/aes256gcm@512", "e", "body limit+2048"),
           (data_len_left_on_a_refused_record, "tls12/chacha20-poly1305", "e", "plaintext limit+1"),
           (data_len_left_on_a_refused_record, "tls12/aes128ccm", "e", "body limit+2048")]


@pytest.mark.parametrize("fault,gid,cls,name", PLANTED, ids=["%s-%s-%s" % (f.__name__, g, n) for f, g, _, n in PLANTED])
def test_planted_fault_fails_at_a_named_record(oracle_mod, fault, gid, cls, name):
    cfg = G.GRIDS[G.IDS.index(gid)]
    built = G.oracle_grid(cfg, oracle_mod)
    specs = [b.spec for b in built]
    want = G.expected(GOLDEN, cfg, built)
    got = []
    for b in built:
        st, ct, pt = _open(cfg, b)
        got.append(fault(cfg, b, st, ct, len(pt)))
    with pytest.raises(AssertionError) as e:
        G.check(cfg, specs, want, got)
    text = str(e.value)
    hit = [i for i, s in enumerate(specs) if s.name == name]
    assert any("class %s record %d (%s):" % (cls, i, name) in text for i in hit), text
    # and nothing but the records the fault touches
    touched = [i for i, (b, g) in enumerate(zip(built, got)) if g != tuple(want[i][:3])]
    assert touched and "%d of %d records differ" % (len(touched), len(specs)) in text
    assert all(specs[i].cls == cls or {cls, specs[i].cls} == {"e", "b"} for i in touched), [specs[i] for i in touched]

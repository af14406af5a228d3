"""The verdict grid of the AEAD receive path (csrc/records.hip: open_one and
finish_one): the length and header checks before the AEAD, the tag, the TLS
1.3 de-padding scan and the two plaintext limits after it, class by class,
and which check wins where two faults coincide.

Pure Python, shared by the fixture generator (tests/golden/
make_golden_rec_grid.py, which seals with the reference's AEAD objects and
asks the reference's RecordLayer for the verdicts), the CPU tests
(test_rec_grid_oracle.py) and the GPU tests (test_gpu_rec_grid.py).  The AEAD
comes in as a function ``seal(alg, key, nonce, plaintext, aad) -> ct || tag``,
so the generator and the tests build the same bytes from different
implementations; the SHA-256 over the wires in tests/golden/rec_grid.json ties
the two together.  Record i of a grid has sequence number SEQ0 + i: the low
word carries inside every grid.

Classes (T = tag length, E = 8 for the TLS 1.2 AES suites' explicit nonce):
  a  wire-length ladder: a short record cut to every wire length 5 .. 5+E+T+1
     (header length rewritten), and the genuine shortest records
  b  TLS 1.3 inner plaintext: every position of the last non-zero byte at the
     small lengths, the edges and 16-byte boundaries at the large ones,
     all-zero, fragments ending in zeros, every content-type byte
  c  TLS 1.3 header: type, version, length wrong alone, in pairs and all three,
     each also with a bad tag and with the body cut below T
  d  TLS 1.2 header: type / version changed after sealing, explicit nonce,
     a byte appended
  e  the limits at the grid's recv_limit, each with a bad-tag twin
  f  every tag byte, first / last ciphertext byte, a record of seq + 1
  g  unprotected TLS 1.3 records (ChangeCipherSpec, an early short alert),
     which the reference passes through without a sequence number
A valid record is followed by its mutated twin where there is one.

A record whose header length differs from its body, or whose type byte the
reference's socket would read as an SSLv2 header, cannot come through a
socket: the generator hands those to _decryptAndUnseal with a crafted header
(``direct``).  The early alert "as record 0" is judged by the reference at
sequence number 0 (its rule is ``seqnum == 0``); the device's answer for that
record does not depend on the number.
"""
import collections
import hashlib

from vectors import detbytes

OK, BAD_MAC, TRUNCATED, LENGTH, BAD_TYPE, BAD_VERSION, NO_CONTENT_TYPE, OVERFLOW, BAD_SESSION = range(9)
STATUS_NAME = ("OK", "BAD_MAC", "TRUNCATED", "LENGTH", "BAD_TYPE", "BAD_VERSION", "NO_CONTENT_TYPE", "OVERFLOW",
               "BAD_SESSION")
SEQ0 = 2 ** 32 - 7
APP = 23

VERDICT_CHAR = {"ok": "o", "TLSBadRecordMAC": "m", "TLSUnexpectedMessage": "u",
                "TLSIllegalParameterException": "i", "TLSRecordOverflow": "v", "unprotected": "p"}
CHAR_VERDICT = dict((v, k) for k, v in VERDICT_CHAR.items())

Config = collections.namedtuple("Config", "version alg keylen ivlen limit classes")
FULL13, FULL12 = "abcefg", "adef"
GRIDS = [Config("tls13", "aes128gcm", 16, 12, 2 ** 14, FULL13),
         Config("tls13", "chacha20-poly1305", 32, 12, 2 ** 14, FULL13),
         Config("tls13", "aes128ccm_8", 16, 12, 2 ** 14, FULL13),
         Config("tls12", "aes256gcm", 32, 4, 2 ** 14, FULL12),
         Config("tls12", "aes128ccm", 16, 4, 2 ** 14, FULL12),
         Config("tls12", "chacha20-poly1305", 32, 12, 2 ** 14, FULL12),
         Config("tls13", "aes128gcm", 16, 12, 512, "e"),
         Config("tls12", "aes256gcm", 32, 4, 512, "e")]

# One record of the plan.
#   frag, zeros  the fragment: ``frag`` deterministic bytes, the last ``zeros`` of them zero
#   ctype, pad   TLS 1.3: the inner plaintext is fragment || ctype || pad zeros (ctype 0: no type byte
#                but a zero); TLS 1.2: ctype is the header's type
#   delta        sealed under sequence number seq + delta
#   muts         applied in order to the sealed wire:
#                ("type", t) ("ver", v) header bytes; ("len", d) header length += d;
#                ("cut", n) wire cut to n bytes, header length rewritten to n - 5;
#                ("xor", pos, bits) wire[pos] ^= bits (pos < 0: from the end);
#                ("append", b) one byte appended, header length += 1
#   raw          an unprotected record: header(ctype, 0x0303) || raw, nothing sealed
#   ref_seq      the read state's sequence number the reference judges it at (None: its own)
Spec = collections.namedtuple("Spec", "cls name frag zeros ctype pad delta muts raw ref_seq")


def _spec(cls, name, frag, ctype=APP, pad=0, zeros=0, delta=0, muts=(), raw=None, ref_seq=None):
    return Spec(cls, name, frag, zeros, ctype, pad, delta, tuple(muts), raw, ref_seq)


def grid_id(cfg):
    return "%s/%s%s" % (cfg.version, cfg.alg, "" if cfg.limit == 2 ** 14 else "@%d" % cfg.limit)


IDS = [grid_id(c) for c in GRIDS]


def taglen(cfg):
    return 8 if cfg.alg.endswith("ccm_8") else 16


def explicit(cfg):
    return 8 if cfg.version == "tls12" and not cfg.alg.startswith("chacha") else 0


def keys(cfg, session=None):
    tag = grid_id(cfg) + ("" if session is None else "/s%d" % session)
    return bytes(detbytes("recgrid-key-" + tag, cfg.keylen)), bytes(detbytes("recgrid-iv-" + tag, cfg.ivlen))


# ---- the plan ---------------------------------------------------------------------

SMALL_INNER = (1, 2, 15, 16, 17, 31, 32, 33)
LARGE_INNER = (255, 256, 257, 4096, 4097)
INNER_TYPES = (20, 21, 22, 23, 24, 0x01, 0xff)
BAD_TAG = ("xor", -1, 0x80)


def large_positions(n):
    """Last non-zero byte at 0, 1, n - 1 and either side of each 16-byte
    boundary next to the end."""
    edge = (n - 1) // 16 * 16
    return sorted({0, 1, n - 1, edge - 17, edge - 16, edge - 1, edge} & set(range(n)))


def _ladder(cfg):
    tls13, E, T = cfg.version == "tls13", explicit(cfg), taglen(cfg)
    out = [_spec("a", "short", 3)]
    for wl in range(5, 5 + E + T + 2):
        out.append(_spec("a", "short cut to %d" % wl, 3, muts=[("cut", wl)]))
    out.append(_spec("a", "shortest", 0))   # TLS 1.3: the type byte alone; TLS 1.2: an empty fragment
    if tls13:
        out.append(_spec("a", "shortest, bad tag", 0, muts=[BAD_TAG]))
    return out


def _inner(cfg):
    out, k = [], 0
    for n in SMALL_INNER + LARGE_INNER:
        for p in (range(n) if n in SMALL_INNER else large_positions(n)):
            out.append(_spec("b", "inner %d last %d" % (n, p), p, INNER_TYPES[k % 7], n - 1 - p))
            k += 1
        out.append(_spec("b", "inner %d all zero" % n, n - 1, 0, 0, zeros=n - 1))
    for L, z in ((40, 1), (40, 17), (33, 32)):
        out.append(_spec("b", "fragment %d ends in %d zeros" % (L, z), L, 22, 5, zeros=z))
    out.append(_spec("b", "all-zero fragment, type 22", 48, 22, 0, zeros=48))
    out.append(_spec("b", "all-zero fragment, type 23, padded", 17, 23, 31, zeros=17))
    for t in INNER_TYPES:
        out.append(_spec("b", "content type 0x%02x" % t, 21, t, 2))
    out.append(_spec("b", "empty fragment, limit zeros", 0, 23, cfg.limit))
    return out


HEADER_FAULTS = [("type 0", [("type", 0)]), ("type 21", [("type", 21)]), ("type 22", [("type", 22)]),
                 ("type 24", [("type", 24)]),
                 ("version 0300", [("ver", 0x0300)]), ("version 0301", [("ver", 0x0301)]),
                 ("version 0304", [("ver", 0x0304)]), ("version 0203", [("ver", 0x0203)]),
                 ("length +1", [("len", 1)]), ("length -1", [("len", -1)]),
                 ("type+version", [("type", 22), ("ver", 0x0304)]), ("type+length", [("type", 22), ("len", 1)]),
                 ("version+length", [("ver", 0x0304), ("len", -1)]),
                 ("type+version+length", [("type", 21), ("ver", 0x0301), ("len", 1)])]


def _header13(cfg):
    T = taglen(cfg)
    out = []
    for name, muts in HEADER_FAULTS:
        out.append(_spec("c", "full record", 40, 23, 3))
        out.append(_spec("c", name, 40, 23, 3, muts=muts))
        out.append(_spec("c", name + ", bad tag", 40, 23, 3, muts=[BAD_TAG] + muts))
        out.append(_spec("c", name + ", body cut below T", 40, 23, 3, muts=[("cut", 5 + T - 1)] + muts))
    return out


def _header12(cfg):
    E = explicit(cfg)
    out = []
    for name, muts in (("type 22 after sealing", [("type", 22)]), ("version 0301", [("ver", 0x0301)]),
                       ("version 0304", [("ver", 0x0304)]), ("byte appended", [("append", 0x5c)])):
        out += [_spec("d", "full record", 40), _spec("d", name, 40, muts=muts)]
    if E:
        out += [_spec("d", "full record", 40), _spec("d", "explicit nonce byte 0", 40, muts=[("xor", 5, 1)]),
                _spec("d", "full record", 40), _spec("d", "explicit nonce byte 7", 40, muts=[("xor", 12, 0x80)])]
    return out


def _limits(cfg):
    lim, T, E = cfg.limit, taglen(cfg), explicit(cfg)
    if cfg.version == "tls13":
        cases = [("inner limit+1", lim, 0), ("inner limit+1, padded", lim - 10, 10), ("inner limit+2", lim, 1),
                 ("body limit+256", 100, lim + 256 - T - 101), ("body limit+257", 100, lim + 257 - T - 101)]
    else:
        cases = [("plaintext limit", lim, 0), ("plaintext limit+1", lim + 1, 0),
                 ("body limit+2048", lim + 2048 - E - T, 0), ("body limit+2049", lim + 2049 - E - T, 0)]
    out = []
    for name, frag, pad in cases:
        out += [_spec("e", name, frag, 23, pad), _spec("e", name + ", bad tag", frag, 23, pad, muts=[BAD_TAG])]
    return out


def _tags(cfg):
    T = taglen(cfg)
    tls13 = cfg.version == "tls13"
    part, full = (36, 47) if tls13 else (37, 48)      # plaintext of 37 and of 48 bytes
    out = []
    for k in range(T):
        out += [_spec("f", "partial block", part),
                _spec("f", "tag byte %d bit %s" % (k, "01" if k % 2 == 0 else "80"), part,
                      muts=[("xor", -T + k, 0x01 if k % 2 == 0 else 0x80)])]
    hdr = 5 + explicit(cfg)
    for name, frag in (("partial", part), ("full", full)):
        n = frag + (1 if tls13 else 0)
        out += [_spec("f", name + " block", frag), _spec("f", name + ": first ciphertext byte", frag,
                                                         muts=[("xor", hdr, 0x04)]),
                _spec("f", name + " block", frag), _spec("f", name + ": last ciphertext byte", frag,
                                                         muts=[("xor", hdr + n - 1, 0x20)])]
    out += [_spec("f", "partial block", part), _spec("f", "sealed under seq + 1", part, delta=1)]
    return out


def _unprotected(cfg):
    return [_spec("g", "ChangeCipherSpec, 1 byte", 0, 20, raw=b"\x01"),
            _spec("g", "ChangeCipherSpec over an encrypted body", 40, 23, 3, muts=[("type", 20)]),
            _spec("g", "2-byte alert later in the batch", 0, 21, raw=b"\x02\x28")]


def plan(cfg):
    out = []
    if "g" in cfg.classes:      # record 0: the alert before the first protected record
        out.append(_spec("g", "2-byte alert as record 0", 0, 21, raw=b"\x02\x28", ref_seq=0))
    for cls, fn in (("a", _ladder), ("b", _inner), ("c", _header13), ("d", _header12), ("e", _limits),
                    ("f", _tags), ("g", _unprotected)):
        if cls in cfg.classes:
            out += fn(cfg)
    return out


def describe(specs, i):
    return "class %s record %d (%s)" % (specs[i].cls, i, specs[i].name)


# ---- building the bytes -------------------------------------------------------------

def plaintext(cfg, spec, label):
    """What is sealed: the TLS 1.3 inner plaintext, or the TLS 1.2 fragment."""
    frag = bytearray(detbytes("recgrid-%s-%d" % (label, spec.frag), spec.frag))
    if spec.zeros:
        frag[spec.frag - spec.zeros:] = bytes(spec.zeros)
    if cfg.version == "tls13":
        frag += bytes([spec.ctype]) + bytes(spec.pad)
    return bytes(frag)


def nonce(cfg, iv, seq):
    s = int(seq).to_bytes(8, "big")
    if cfg.version == "tls13" or len(iv) == 12:
        return bytes(a ^ b for a, b in zip(iv, bytes(4) + s))
    return iv[:4] + s


def sealed(cfg, spec, key, iv, seq, plain, seal):
    """The unmutated wire record."""
    T, E = taglen(cfg), explicit(cfg)
    if spec.raw is not None:
        return bytes([spec.ctype, 3, 3, 0, len(spec.raw)]) + spec.raw
    q = (seq + spec.delta) & (2 ** 64 - 1)
    if cfg.version == "tls13":
        n = len(plain) + T
        hdr = bytes([APP, 3, 3, n >> 8, n & 255])
        return hdr + bytes(seal(cfg.alg, key, nonce(cfg, iv, q), plain, hdr))
    aad = q.to_bytes(8, "big") + bytes([spec.ctype, 3, 3, len(plain) >> 8, len(plain) & 255])
    body = (q.to_bytes(8, "big") if E else b"") + bytes(seal(cfg.alg, key, nonce(cfg, iv, q), plain, aad))
    return bytes([spec.ctype, 3, 3, len(body) >> 8, len(body) & 255]) + body


def mutate(wire, muts):
    w = bytearray(wire)

    def set_len(n):
        w[3], w[4] = (n >> 8) & 255, n & 255
    for m in muts:
        if m[0] == "type":
            w[0] = m[1]
        elif m[0] == "ver":
            w[1], w[2] = m[1] >> 8, m[1] & 255
        elif m[0] == "len":
            set_len((w[3] << 8 | w[4]) + m[1])
        elif m[0] == "cut":
            del w[m[1]:]
            set_len(len(w) - 5)
        elif m[0] == "xor":
            w[m[1]] ^= m[2]
        elif m[0] == "append":
            w.append(m[1])
            set_len(len(w) - 5)
        else:
            raise ValueError(m)
    return bytes(w)


Built = collections.namedtuple("Built", "spec seq plain wire")


def build(cfg, seal, sessions=None, seqs=None):
    """Every record of the grid.  ``sessions`` / ``seqs``: per record the
    session whose key and IV seal it and its sequence number (default: the
    grid's one key and SEQ0 + i)."""
    out = []
    for i, spec in enumerate(plan(cfg)):
        key, iv = keys(cfg, None if sessions is None else sessions[i])
        seq = SEQ0 + i if seqs is None else (seqs[i] or 0)     # None: a skipped record, any number
        plain = plaintext(cfg, spec, "%s-%d" % (grid_id(cfg), i))
        out.append(Built(spec, seq, plain, mutate(sealed(cfg, spec, key, iv, seq, plain, seal), spec.muts)))
    return out


def wires_digest(wires):
    h = hashlib.sha256()
    for w in wires:
        h.update(len(w).to_bytes(4, "big"))
        h.update(w)
    return h.hexdigest()


def direct(wire):
    """True where the reference's socket cannot deliver the record as it is."""
    return (wire[3] << 8 | wire[4]) != len(wire) - 5 or wire[0] not in (20, 21, 22, 23, 24)


def oracle_seal(oracle_mod):
    """``seal`` from the C oracle (oracle/oracle.py)."""
    def seal(alg, key, n, plain, aad):
        if alg.startswith("chacha"):
            return oracle_mod.chacha_seal(key, n, plain, aad)
        if "ccm" in alg:
            return oracle_mod.ccm_seal(key, n, plain, aad, 8 if alg.endswith("_8") else 16)
        return oracle_mod.gcm_seal(key, n, plain, aad)
    return seal


_cache = {}


def oracle_grid(cfg, oracle_mod):
    """build() with the C oracle's AEAD, once per process."""
    if grid_id(cfg) not in _cache:
        _cache[grid_id(cfg)] = build(cfg, oracle_seal(oracle_mod))
    return _cache[grid_id(cfg)]


# ---- the fixture and what it maps to --------------------------------------------------

# The reference's verdict for a record the reference does not decrypt at all (class g): an AEAD engine
# has no "pass through" answer, so the device refuses these by its usual order of checks (include/
# tlsgpu.h: the caller takes them out of the batch).  name -> device status.
OUTSIDE_REMIT = {"2-byte alert as record 0": TRUNCATED,
                 "ChangeCipherSpec, 1 byte": TRUNCATED,
                 "ChangeCipherSpec over an encrypted body": BAD_TYPE}

Want = collections.namedtuple("Want", "status ctype length advanced verdict")


def has(spec, kind):
    return any(m[0] == kind for m in spec.muts)


def status_of(cfg, spec, verdict, wire):
    """The TG_REC_* code of the reference's verdict.  TLSBadRecordMAC splits
    into TRUNCATED / LENGTH / BAD_MAC, TLSUnexpectedMessage into BAD_TYPE /
    NO_CONTENT_TYPE, by the class of fault the plan put into the record."""
    if verdict == "ok":
        return OK
    if verdict == "unprotected":
        return OUTSIDE_REMIT[spec.name]
    if verdict == "TLSRecordOverflow":
        return OVERFLOW
    if verdict == "TLSIllegalParameterException":
        return BAD_VERSION
    if verdict == "TLSUnexpectedMessage":
        return BAD_TYPE if has(spec, "type") or spec.raw is not None else NO_CONTENT_TYPE
    assert verdict == "TLSBadRecordMAC", verdict
    if len(wire) - 5 < explicit(cfg) + taglen(cfg):     # the body holds no nonce and tag (:787-799)
        return TRUNCATED
    if cfg.version == "tls13" and has(spec, "len"):
        return LENGTH
    return BAD_MAC


def expected(golden, cfg, built):
    """[Want] of a grid from tests/golden/rec_grid.json."""
    g = golden[grid_id(cfg)]
    assert len(g["verdicts"]) == len(g["advanced"]) == len(built) == g["records"]
    oks = iter(zip(g["types"], g["lengths"]))
    out = []
    for b, ch, adv in zip(built, g["verdicts"], g["advanced"]):
        verdict = CHAR_VERDICT[ch]
        ctype, length = next(oks) if verdict == "ok" else (0, 0)
        out.append(Want(status_of(cfg, b.spec, verdict, b.wire), ctype, length, adv == "1", verdict))
    assert next(oks, None) is None
    return out


def header_overflow(cfg, wire):
    """The body is longer than RecordSocket.recv reads (recordlayer.py:219-222)."""
    return len(wire) - 5 > cfg.limit + (256 if cfg.version == "tls13" else 2048)


def data_image(cfg, b, want):
    """What an open leaves in the record's data extent: the bytes, or None for
    an extent that stays as it was.  The extent is wire - header - tag bytes."""
    room = max(len(b.wire) - 5 - explicit(cfg) - taglen(cfg), 0)
    if want.status == BAD_MAC:                               # decrypted, refused: zeroed
        return bytes(room)
    if want.status in (OK, NO_CONTENT_TYPE) or (want.status == OVERFLOW and not header_overflow(cfg, b.wire)):
        assert room == len(b.plain)                          # authentic: the plaintext stays
        return b.plain
    return None                                              # refused before decryption


def check(cfg, specs, want, got):
    """``got``: (status, content type, length) per record.  Raises an
    AssertionError that names the class and the record of every difference."""
    wrong = []
    for i, (w, g) in enumerate(zip(want, got)):
        g = tuple(int(x) for x in g)
        if g != (w.status, w.ctype, w.length):
            wrong.append("%s: (status, type, length) = (%s, %d, %d), the reference's %s wants (%s, %d, %d)"
                         % (describe(specs, i), STATUS_NAME[g[0]] if g[0] < 9 else g[0], g[1], g[2], w.verdict,
                            STATUS_NAME[w.status], w.ctype, w.length))
    assert len(want) == len(got) == len(specs)
    assert not wrong, "%s: %d of %d records differ:\n%s" % (grid_id(cfg), len(wrong), len(specs), "\n".join(wrong[:16]))


# ---- sessions (GPU tests) --------------------------------------------------------------

SESSION_GRIDS = ("tls13/chacha20-poly1305", "tls12/aes256gcm")    # also run through tg_open_session_records
NSESS = 3
SESSION_STARTS = (2 ** 32 - 5, SEQ0, 2 ** 40 + 1)
SKIPPED = 5                     # this record's session is out of range


def deal(n):
    """(session per record, sequence number per record or None, counters
    after the batch): records dealt 0, 1, 2, 0, ... with record SKIPPED in no
    session; every in-range record takes its session's next number."""
    sessions = [i % NSESS for i in range(n)]
    sessions[SKIPPED] = NSESS + 4
    nxt, seqs = list(SESSION_STARTS), []
    for s in sessions:
        if s < NSESS:
            seqs.append(nxt[s])
            nxt[s] += 1
        else:
            seqs.append(None)
    return sessions, seqs, nxt

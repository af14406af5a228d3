"""The padding grid of the AES-CBC + HMAC receive path: every padding length
at the decrypted lengths where the constant-work verdict (csrc/cbc_record.h:
hmac_record, msg_word, pad_differs, mte_verdict, etm_padding) changes shape,
each valid record with one mutated twin.

Pure Python, shared by the fixture generator (tests/golden/
make_golden_cbc_grid.py, which builds the wires with the reference's AES and
asks the reference's RecordLayer for the verdicts), the CPU tests
(test_cbc_grid_oracle.py, test_cbc_host.py) and the GPU tests
(test_gpu_cbc_grid.py).  The crypto comes in as functions, so the generator
and the tests build the same bytes from different implementations; the
SHA-256 over the wires in tests/golden/cbc_grid.json ties the two together.

MAC-then-encrypt, per key configuration (D = digest size):
  n     the two smallest multiples of 16 >= D + 1 (padding window = whole
        record, pad_start / mac_start clamp at 0 for a lying length byte),
        240, 256, 272 (either side of the 256-byte window), 288, 384, 400, 528
  pad   every value with pad + 1 + D <= n, up to 255
  body  data[L] || HMAC || (pad + 1) x pad,   L = n - D - 1 - pad
Encrypt-then-MAC (the MAC is always right: these reach etm_padding):
  n     16, 32, 240, 256, 272, 528;  pad: every value with pad + 1 <= n

Records alternate valid, mutated, valid, ...; record i of a grid has sequence
number SEQ0 + i and content type CTYPES[i % 3], and a mutated record's MAC is
right for its own sequence number before the mutation is applied.
"""
import collections
import hashlib
import struct

from vectors import detbytes

DIGEST = {"sha1": 20, "sha256": 32, "sha384": 48}
HASH_BLOCK = {"sha1": 64, "sha256": 64, "sha384": 128}
HASH_LENBYTES = {"sha1": 8, "sha256": 8, "sha384": 16}
SEQ0 = 2 ** 32 - 7            # the low word of the sequence number carries inside every grid
CTYPES = (23, 22, 21)
TLS11, TLS12 = 0x0302, 0x0303

Config = collections.namedtuple("Config", "name keylen mac version modes max_n")
CONFIGS = [Config("aes128-sha1", 16, "sha1", TLS12, ("mte", "etm"), None),
           Config("aes256-sha256", 32, "sha256", TLS12, ("mte", "etm"), None),
           Config("aes256-sha384", 32, "sha384", TLS12, ("mte", "etm"), None),
           Config("aes128-sha1-tls11", 16, "sha1", TLS11, ("mte",), 288)]
GRIDS = [(c, m) for c in CONFIGS for m in c.modes]

MTE_N = (240, 256, 272, 288, 384, 400, 528)
ETM_N = (16, 32, 240, 256, 272, 528)

# kind: None (valid) / "pad" / "mac" / "frag" (body[pos] ^= val) / "len" (body[-1] = val)
Case = collections.namedtuple("Case", "n pad kind pos val")
Record = collections.namedtuple("Record", "case seq ctype iv data body")

VERDICT_CHAR = {"ok": "o", "TLSBadRecordMAC": "m", "TLSDecryptionFailed": "d", "TLSRecordOverflow": "v"}
CHAR_VERDICT = dict((v, k) for k, v in VERDICT_CHAR.items())


def grid_id(cfg, mode):
    return "%s/%s" % (cfg.name, mode)


def keys(cfg):
    return bytes(detbytes("grid-ek-" + cfg.name, cfg.keylen)), bytes(detbytes("grid-mk-" + cfg.name, DIGEST[cfg.mac]))


def mte_lengths(cfg):
    first = (DIGEST[cfg.mac] + 1 + 15) // 16 * 16
    return [n for n in (first, first + 16) + MTE_N if cfg.max_n is None or n <= cfg.max_n]


def _flip_bit(count, span):
    return 1 << ((count // span) % 8)


def mte_plan(cfg):
    """The MtE cases: each valid one followed by its mutated twin."""
    d = DIGEST[cfg.mac]
    kinds = ("pad", "mac", "frag", "len")
    count = dict.fromkeys(kinds, 0)
    out, k = [], 0
    for n in mte_lengths(cfg):
        for pad in range(min(255, n - d - 1) + 1):
            L = n - d - 1 - pad
            out.append(Case(n, pad, None, 0, 0))
            kind = kinds[k % 4]
            if kind == "pad" and pad == 0:
                kind = "mac"                        # no padding byte but the length byte
            if kind == "frag" and L == 0:
                kind = "mac"                        # no fragment byte
            j = count[kind]
            count[kind] += 1
            if kind == "pad":                       # a padding byte, never the length byte
                off = 0 if j % 4 == 0 else j % pad  # every fourth: the first one
                out.append(Case(n, pad, kind, n - 1 - pad + off, _flip_bit(j, 7)))
            elif kind == "mac":                     # every MAC byte in turn
                out.append(Case(n, pad, kind, L + j % d, _flip_bit(j, d)))
            elif kind == "frag":
                out.append(Case(n, pad, kind, (7 * j) % L, _flip_bit(j, 5)))
            else:                                   # a length that points outside the record
                out.append(Case(n, pad, kind, n - 1, min(255, (n - d, n - 1, n, 255)[j % 4])))
            k += 1
    return out


def etm_plan(cfg):
    out, k = [], 0
    count = {"pad": 0, "len": 0}
    for n in ETM_N:
        for pad in range(min(255, n - 1) + 1):
            out.append(Case(n, pad, None, 0, 0))
            kind = "pad" if k % 2 == 0 and pad else "len"
            j = count[kind]
            count[kind] += 1
            if kind == "pad":
                off = 0 if j % 4 == 0 else j % pad
                out.append(Case(n, pad, kind, n - 1 - pad + off, _flip_bit(j, 7)))
            else:
                out.append(Case(n, pad, kind, n - 1, min(255, (n, n + 1, 255)[j % 3])))
            k += 1
    return out


def plan(cfg, mode):
    return mte_plan(cfg) if mode == "mte" else etm_plan(cfg)


def mac_input_header(seq, ctype, version, length):
    return struct.pack(">QBBBH", seq, ctype, version >> 8, version & 255, length)


def records(cfg, mode, mac_fn):
    """The decrypted bodies of a grid.  ``mac_fn(mac, mac_key, message)`` is
    HMAC; no cipher is needed (the host check of the verdict code stops here)."""
    d = DIGEST[cfg.mac]
    _, mac_key = keys(cfg)
    out = []
    for i, c in enumerate(plan(cfg, mode)):
        seq, ctype = SEQ0 + i, CTYPES[i % 3]
        tag = "%s-%d" % (grid_id(cfg, mode), i)
        L = c.n - 1 - c.pad - (d if mode == "mte" else 0)
        data = bytes(detbytes("grid-data-" + tag, L))
        body = bytearray(data)
        if mode == "mte":
            body += mac_fn(cfg.mac, mac_key, mac_input_header(seq, ctype, cfg.version, L) + data)
        body += bytes([c.pad]) * (c.pad + 1)
        assert len(body) == c.n
        if c.kind == "len":
            body[-1] = c.val
        elif c.kind:
            assert 0 <= c.pos < c.n - 1
            body[c.pos] ^= c.val
        out.append(Record(c, seq, ctype, bytes(detbytes("grid-iv-" + tag, 16)), data, bytes(body)))
    return out


def wire(cfg, mode, rec, cbc_fn, mac_fn):
    """The wire record of ``rec``.  ``cbc_fn(enc_key, iv, plain)`` is AES-CBC."""
    enc_key, mac_key = keys(cfg)
    buf = rec.iv + cbc_fn(enc_key, rec.iv, rec.body)
    if mode == "etm":   # over the bytes actually sent
        buf += mac_fn(cfg.mac, mac_key, mac_input_header(rec.seq, rec.ctype, cfg.version, len(buf)) + buf)
    return struct.pack(">BHH", rec.ctype, cfg.version, len(buf)) + buf


def wires_digest(wires):
    h = hashlib.sha256()
    for w in wires:
        h.update(w)
    return h.hexdigest()


def mte_message_end(cfg, case):
    """13 + L of a valid case: where the MAC'ed message really ends."""
    return 13 + case.n - DIGEST[cfg.mac] - 1 - case.pad


def mte_compressions(mac, n):
    """Inner compression calls the verdict runs for a decrypted length n
    (the longest message the record could hold), plus the outer one."""
    return (13 + n - DIGEST[mac] - 1 + HASH_LENBYTES[mac]) // HASH_BLOCK[mac] + 2


def mte_block_gap(cfg, case):
    """Compression calls between the block that holds the real end's length
    field and the last block that is run."""
    b, lb = HASH_BLOCK[cfg.mac], HASH_LENBYTES[cfg.mac]
    return (mte_compressions(cfg.mac, case.n) - 2) - (mte_message_end(cfg, case) + lb) // b


def expected(golden, cfg, mode):
    """[(verdict, plaintext length)] of a grid from tests/golden/cbc_grid.json."""
    g = golden[grid_id(cfg, mode)]
    lens = iter(g["lengths"])
    out = [(CHAR_VERDICT[ch], next(lens) if ch == "o" else 0) for ch in g["verdicts"]]
    assert next(lens, None) is None
    return out


def hmac_fn(mac, mac_key, msg):
    import hmac
    return hmac.new(mac_key, msg, getattr(hashlib, mac)).digest()


_model_cache = {}


def model_grid(cfg, mode):
    """(records, wire records) of a grid from the CPU model's AES (tests/
    cbc_model.py), built once per process."""
    key = grid_id(cfg, mode)
    if key not in _model_cache:
        import cbc_model
        recs = records(cfg, mode, hmac_fn)
        _model_cache[key] = (recs, [wire(cfg, mode, r, cbc_model.cbc_encrypt, hmac_fn) for r in recs])
    return _model_cache[key]


# ---- seal lengths and buffer placement (GPU tests) --------------------------

def seal_lengths(mac, etm, count=130):
    """``count`` fragment lengths: those of make_golden_cbc.py's seal_lengths
    below 16 KiB (0, 1, either side of the padding wrap and of the hash block
    ends) and 1000 in turn, with two full 16384-byte records among them."""
    base = 0 if etm else DIGEST[mac]
    wrap = next(n for n in range(2, 40) if (base + n) % 16 == 15)
    small = [0, 1, wrap, wrap + 1, 42, 43, 50, 51, 98, 99, 114, 115, 1000]
    lens = [small[i % len(small)] for i in range(count)]
    lens[5] = lens[count - 60] = 16384
    return lens


def residues(n, seed, forced):
    """Per-record address residues mod 16 from a seeded generator, for as
    many buffers as ``forced`` has entries: independent shuffles of 0..15,
    one after the other (so 16 records or more see every residue), except
    that every fourth record takes the residues ``forced`` (the kernels'
    vector path)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    res = []
    for f in forced:
        free = iter(np.concatenate([rng.permutation(16) for _ in range(n // 16 + 1)]))
        res.append(np.array([f if i % 4 == 0 else next(free) for i in range(n)], np.int64))
    return res


def place(sizes, leads, gap=48, guard=256):
    """Offsets with ``off % 16 == lead``, at least ``gap`` bytes between
    extents and ``guard`` bytes at both ends; (offsets, buffer size)."""
    offs, pos = [], guard
    for size, lead in zip(sizes, leads):
        pos += (int(lead) - pos) % 16
        offs.append(pos)
        pos += int(size) + gap
    return offs, pos - gap + guard if offs else 2 * guard

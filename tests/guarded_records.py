"""Guarded record framing: the discipline of tests/guarded.py for
tg_seal_records / tg_open_records and their many-session forms.

``data``, ``wire`` and the open side's output are canary-filled, the extents
lie between 48-byte canary gaps behind 256-byte guards, and a data extent is
exactly what the ABI promises: ``L + 1 + pad`` bytes for TLS 1.3, ``L`` for
TLS 1.2 -- no room for the tag.  Every array of a call is compared whole with
an expected image from the framing oracle (oracle/records.py); the per-record
result arrays are 16 entries longer than the batch and prefilled.

A record is ``(key, iv, seq)`` or ``None`` (a many-session record whose
session is out of range: skipped).  The thing that runs a call is a function
``call(op, arrays) -> arrays``, so the checks also run on the CPU against the
oracle (tests/test_guarded_host.py).
"""
import numpy as np

from guarded import CANARY_BACK, CANARY_IN, CANARY_SEALED, ContainmentError, _first_diff, _place
from oracle import records as R

GAP, GUARD, SLACK = 48, 256, 16
FILL8, FILL32 = 0xEE, 0x6E6E6E6E
BAD_SESSION = 8

LENS = [0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 16384 - 300]
PADS = [0, 1, 15, 16, 255]
N = 48


def case_records(version, seed, n=N):
    """(lens, pads, content types, fragments) of a batch of ``n`` records."""
    rng = np.random.default_rng(seed)
    lens = LENS + [int(x) for x in rng.integers(0, 3000, n - len(LENS))]
    lens = [lens[j] for j in rng.permutation(n)]
    pads = [PADS[(3 * i + 1) % 5] if version == "tls13" else 0 for i in range(n)]
    ctypes_ = [int(x) for x in rng.choice([21, 22, 23], n)]
    return lens, pads, ctypes_, [rng.bytes(L) for L in lens]


def header_len(version, alg):
    return 5 + (8 if version == "tls12" and not alg.startswith("chacha") else 0)


def _extents(sizes, leads):
    off, total = _place(sizes, leads, GAP, GUARD)
    off, sizes = off.astype(np.int64), np.asarray(sizes, np.int64)
    assert (off % 16 == np.asarray(leads) % 16).all()
    assert (off - GAP >= 0).all() and (off + sizes + GAP <= total).all()     # nothing leaves the buffer
    assert (off[1:] - (off + sizes)[:-1] >= GAP).all()
    return off, sizes, total


def _wire_extents(sizes, hdr, aligned):
    """aligned: the payload after the header (and explicit nonce) on a
    16-byte boundary; else packed at a lead that changes per record."""
    n = len(sizes)
    return _extents(sizes, np.full(n, -hdr % 16) if aligned else (5 * np.arange(n) + 9) % 16)


def _locate(off, size, pos):
    end = off + size
    dist = np.where(pos < off, off - pos, np.where(pos >= end, pos - end + 1, 0))
    i = int(np.argmin(dist))
    return i, int(pos - off[i]), int(size[i])


def _compare(step, got, want, where):
    """Every array of the call against its expected image; ``where`` maps the
    byte buffers to their (offsets, sizes) for the report."""
    for name, w in want.items():
        if w is None:
            continue
        g = got[name]
        if g.shape == w.shape and np.array_equal(g, w):
            continue
        p = _first_diff(g.reshape(-1), w.reshape(-1))
        if name in where:
            i, rel, size = _locate(where[name][0], where[name][1], p)
            raise ContainmentError("%s: %s buffer" % (step, name), i, rel, size, w[p], g[p], p)
        raise ContainmentError("%s: array %s[%d] (n = %d): expected %r, got %r"
                               % (step, name, p, where["n"], w.reshape(-1)[p], g.reshape(-1)[p]),
                               p if p < where["n"] else None, None, None, None, None, p)


def _padded(values, dtype, fill, n):
    a = np.full(n + SLACK, fill, dtype)
    a[:n] = values
    return a


# ---- tampering -------------------------------------------------------------------

def tamper_classes(version, alg):
    """name -> function of a wire record: one bad record of each class."""
    hdr, tag = header_len(version, alg), R.taglen(alg)
    limit = R.RECV_LIMIT + (256 if version == "tls13" else 2048)
    c = {
        "bad_tag": lambda w: w[:-1] + bytes([w[-1] ^ 0x80]),
        "flipped_ct": lambda w: w[:hdr + 7] + bytes([w[hdr + 7] ^ 1]) + w[hdr + 8:],
        "truncated": lambda w: w[:hdr + tag - 1],
        "over_limit": lambda w: w[:3] + bytes([(limit + 1) >> 8, (limit + 1) & 0xff]) + bytes(limit + 1),
    }
    if version == "tls13":
        c["bad_type"] = lambda w: b"\x16" + w[1:]
        c["bad_version"] = lambda w: w[:1] + b"\x03\x04" + w[3:]
        c["length_mismatch"] = lambda w: w[:3] + bytes([w[3], w[4] ^ 1]) + w[5:]
    return c


def pick_tampered(version, alg, lens, recs):
    """record index -> tamper function: one record of each class, all of them
    long enough for every class and none of them skipped."""
    fit = [i for i, L in enumerate(lens) if recs[i] is not None and 100 <= L < 3000]
    return dict((i, f) for i, f in zip(fit[1::2], tamper_classes(version, alg).values()))


# ---- the checks --------------------------------------------------------------------

def run_guarded_records(call, version, alg, recs, lens, pads, ctypes_, datas, aligned,
                        extras=None, want_extras=None):
    """Seal, open what was sealed, open a copy with one bad record of each
    class; every array of every call compared whole.  ``extras(op)`` /
    ``want_extras(op)``: further arrays of the call (the many-session forms'
    session, IV and sequence-number arrays) and their expected images (an
    array not named there must come back as it was sent)."""
    n, tls13 = len(recs), version == "tls13"
    hdr, tag = header_len(version, alg), R.taglen(alg)
    extras = extras or (lambda op: {})
    want_extras = want_extras or (lambda op: {})
    inner = [L + 1 + p if tls13 else L for L, p in zip(lens, pads)]
    d_off, d_size, d_total = _extents(inner, np.zeros(n) if aligned else (7 * np.arange(n) + 3) % 16)
    w_off, w_size, w_total = _wire_extents([hdr + m + tag for m in inner], hdr, aligned)

    # 1. seal
    data = np.full(d_total, CANARY_IN, np.uint8)
    for o, x in zip(d_off, datas):
        data[o:o + len(x)] = np.frombuffer(x, np.uint8)
    sent = dict(data=data, data_off=d_off.astype(np.uint64), data_len=_padded(lens, np.uint32, FILL32, n),
                ctype=_padded(ctypes_, np.uint8, FILL8, n), pad_len=np.array(pads, np.uint32) if tls13 else None,
                wire=np.full(w_total, CANARY_SEALED, np.uint8), wire_off=w_off.astype(np.uint64),
                wire_len=np.full(n + SLACK, FILL32, np.uint32), status=None, **extras("seal"))
    want = dict(sent, data=data.copy(), wire=sent["wire"].copy(), wire_len=sent["wire_len"].copy())
    wires = []
    for i, rec in enumerate(recs):
        if rec is None:     # skipped: nothing in data or wire, length 0
            wires.append(None)
            want["wire_len"][i] = 0
            continue
        if tls13:           # the one write to an input: type and padding appended in place
            o = d_off[i] + lens[i]
            want["data"][o] = ctypes_[i]
            want["data"][o + 1:o + 1 + pads[i]] = 0
        w = R.seal_record(version, alg, rec[0], rec[1], rec[2], ctypes_[i], datas[i], pads[i])
        assert len(w) == w_size[i]
        want["wire"][w_off[i]:w_off[i] + len(w)] = np.frombuffer(w, np.uint8)
        want["wire_len"][i] = len(w)
        wires.append(w)
    want.update(want_extras("seal"))
    _compare("seal", call("seal", sent), want, {"data": (d_off, d_size), "wire": (w_off, w_size), "n": n})

    # 2. open what was sealed, 3. open with one bad record of each class
    some = next(w for w in wires if w is not None)
    good = [some if w is None else w for w in wires]   # a skipped record carries a well-formed record
    bad = pick_tampered(version, alg, lens, recs)
    assert len(bad) == (7 if tls13 else 4)
    for step, sent_wires in (("open", good), ("open tampered", [bad[i](w) if i in bad else w
                                                                for i, w in enumerate(good)])):
        o_off, o_size, o_total = _wire_extents([len(w) for w in sent_wires], hdr, aligned)
        wire = np.full(o_total, CANARY_SEALED, np.uint8)
        for o, w in zip(o_off, sent_wires):
            wire[o:o + len(w)] = np.frombuffer(w, np.uint8)
        sent = dict(data=np.full(d_total, CANARY_BACK, np.uint8), data_off=d_off.astype(np.uint64),
                    data_len=np.full(n + SLACK, FILL32, np.uint32), ctype=np.full(n + SLACK, FILL8, np.uint8),
                    pad_len=None, wire=wire, wire_off=o_off.astype(np.uint64),
                    wire_len=_padded([len(w) for w in sent_wires], np.uint32, FILL32, n),
                    status=np.full(n + SLACK, FILL8, np.uint8), **extras("open"))
        want = dict(sent, data=sent["data"].copy(), data_len=sent["data_len"].copy(),
                    ctype=sent["ctype"].copy(), status=sent["status"].copy())
        statuses = set()
        for i, rec in enumerate(recs):
            if rec is None:
                st, ct, pt = BAD_SESSION, 0, b""
            else:
                st, ct, pt = R.open_record(version, alg, rec[0], rec[1], rec[2], sent_wires[i])
            statuses.add(st)
            want["status"][i], want["ctype"][i], want["data_len"][i] = st, ct, len(pt)
            o, m = d_off[i], len(sent_wires[i]) - hdr - tag
            if st == R.OK:            # the inner plaintext: content, then type, then zeros (TLS 1.3)
                assert (step == "open" or i not in bad) and m == inner[i] and (ct, pt) == (ctypes_[i], datas[i])
                want["data"][o:o + m] = 0
                want["data"][o:o + len(pt)] = np.frombuffer(pt, np.uint8)
                if tls13:
                    want["data"][o + len(pt)] = ct
            elif st == R.BAD_MAC:     # decrypted and rejected: its inner_len bytes zeroed, no more
                assert m == inner[i]
                want["data"][o:o + m] = 0
            else:                     # decided before decryption (or skipped): not a byte written
                assert st in (R.TRUNCATED, R.LENGTH, R.BAD_TYPE, R.BAD_VERSION, R.OVERFLOW, BAD_SESSION)
        if step == "open tampered":
            assert {R.BAD_MAC, R.TRUNCATED, R.OVERFLOW} <= statuses
            assert not tls13 or {R.BAD_TYPE, R.BAD_VERSION, R.LENGTH} <= statuses
        want.update(want_extras("open"))
        _compare(step, call("open", sent), want, {"data": (d_off, d_size), "wire": (o_off, np.array(
            [len(w) for w in sent_wires], np.int64)), "n": n})


# ---- the oracle as the device ---------------------------------------------------------

def oracle_records_device(version, alg, recs, after=None):
    """``call`` for run_guarded_records that computes every result with the
    framing oracle; ``after(op, sent, result)`` fills in the extras."""
    hdr, tag, tls13 = header_len(version, alg), R.taglen(alg), version == "tls13"

    def call(op, a):
        r = dict((k, None if v is None else v.copy()) for k, v in a.items())
        for i, rec in enumerate(recs):
            o, wo = int(a["data_off"][i]), int(a["wire_off"][i])
            if op == "seal":
                if rec is None:
                    r["wire_len"][i] = 0
                    continue
                L, ct = int(a["data_len"][i]), int(a["ctype"][i])
                pad = int(a["pad_len"][i]) if tls13 else 0
                frag = a["data"][o:o + L].tobytes()
                if tls13:
                    r["data"][o + L] = ct
                    r["data"][o + L + 1:o + L + 1 + pad] = 0
                w = R.seal_record(version, alg, rec[0], rec[1], rec[2], ct, frag, pad)
                r["wire"][wo:wo + len(w)] = np.frombuffer(w, np.uint8)
                r["wire_len"][i] = len(w)
            else:
                if rec is None:
                    r["status"][i], r["ctype"][i], r["data_len"][i] = BAD_SESSION, 0, 0
                    continue
                wl = int(a["wire_len"][i])
                st, ct, pt = R.open_record(version, alg, rec[0], rec[1], rec[2], a["wire"][wo:wo + wl].tobytes())
                m = wl - hdr - tag
                if st in (R.OK, R.BAD_MAC):
                    r["data"][o:o + m] = 0
                if st == R.OK:
                    r["data"][o:o + len(pt)] = np.frombuffer(pt, np.uint8)
                    if tls13:
                        r["data"][o + len(pt)] = ct
                r["status"][i], r["ctype"][i], r["data_len"][i] = st, ct, len(pt)
        if after:
            after(op, a, r)
        return r
    return call

"""The first-round rule of a record's ChaCha20 blocks and the wave-span
predicate of the ChaCha20-Poly1305 tile loop (tlslite-ng_amd/csrc/
chacha_poly.hip, keymath.h wave_span_fits), restated on the oracle's block.

Within a record only state word 12, the block counter, changes.  Of the first
double round the column quarter rounds on words (1, 5, 9, 13), (2, 6, 10, 14)
and (3, 7, 11, 15) and the first adds x0 + x4, x1 + x6 and x2 + x7 read key,
nonce and constants only: twelve words per record -- the three finished
columns, x1 and x2 already as the sums x1 + x6 and x2 + x7 -- and x0 + x4 per
key let every block start 39 of its 960 + 32 operations later, for any key,
nonce and counter.

The kernel source does not spell this out: the compiler already moves that
work out of the block loops of chacha_block's inlined copies (the tile loop's
ISA holds 967 add / xor / rotate instructions, not 992; written out by hand it
compiled to the same instructions, profiles/r11/chacha_insts/).  This test
keeps the rule and its count on record.
"""
import os
import random
import shutil
import struct
import subprocess

import pytest

from conftest import ROOT
from oracle import pyaead

M = 0xffffffff
SIGMA = (0x61707865, 0x3320646e, 0x79622d32, 0x6b206574)


class Ops(object):
    """32-bit add / xor / rotate, counted."""

    def __init__(self):
        self.n = 0

    def add(self, a, b):
        self.n += 1
        return (a + b) & M

    def xor(self, a, b):
        self.n += 1
        return a ^ b

    def rotl(self, v, c):
        self.n += 1
        return ((v << c) & M) | (v >> (32 - c))


def qr_tail(o, a, b, c, d):
    """A quarter round after its first add (``a`` already holds a + b)."""
    d = o.rotl(o.xor(d, a), 16)
    c = o.add(c, d); b = o.rotl(o.xor(b, c), 12)
    a = o.add(a, b); d = o.rotl(o.xor(d, a), 8)
    c = o.add(c, d); b = o.rotl(o.xor(b, c), 7)
    return a, b, c, d


def qr(o, a, b, c, d):
    return qr_tail(o, o.add(a, b), b, c, d)


ROUND = ((0, 4, 8, 12), (1, 5, 9, 13), (2, 6, 10, 14), (3, 7, 11, 15),
         (0, 5, 10, 15), (1, 6, 11, 12), (2, 7, 8, 13), (3, 4, 9, 14))


def full_block(o, kw, ctr, nw):
    st = list(SIGMA) + kw + [ctr] + nw
    x = st[:]
    for _ in range(10):
        for a, b, c, d in ROUND:
            x[a], x[b], x[c], x[d] = qr(o, x[a], x[b], x[c], x[d])
    return [o.add(p, q) for p, q in zip(x, st)]


def round1(o, kw, nw):
    """(the twelve words of a record, the key's x0 + x4)."""
    x = list(SIGMA) + kw + [0] + nw
    for a, b, c, d in ROUND[1:4]:
        x[a], x[b], x[c], x[d] = qr(o, x[a], x[b], x[c], x[d])
    rc = {"s16": o.add(x[1], x[6]), "s27": o.add(x[2], x[7])}
    for w in (5, 9, 13, 6, 10, 14, 3, 7, 11, 15):
        rc[w] = x[w]
    return rc, o.add(SIGMA[0], kw[0])


def block_from_round1(o, kw, rc, s04, ctr, nw):
    """The rest of the first double round, nine more, the unchanged
    feed-forward."""
    st = list(SIGMA) + kw + [ctr] + nw
    x = [None] * 16
    for w in (5, 9, 13, 6, 10, 14, 3, 7, 11, 15):
        x[w] = rc[w]
    x[4], x[8], x[12] = kw[0], kw[4], ctr
    x[0], x[4], x[8], x[12] = qr_tail(o, s04, x[4], x[8], x[12])
    x[0], x[5], x[10], x[15] = qr(o, x[0], x[5], x[10], x[15])
    x[1], x[6], x[11], x[12] = qr_tail(o, rc["s16"], x[6], x[11], x[12])
    x[2], x[7], x[8], x[13] = qr_tail(o, rc["s27"], x[7], x[8], x[13])
    x[3], x[4], x[9], x[14] = qr(o, x[3], x[4], x[9], x[14])
    for _ in range(9):
        for a, b, c, d in ROUND:
            x[a], x[b], x[c], x[d] = qr(o, x[a], x[b], x[c], x[d])
    return [o.add(p, q) for p, q in zip(x, st)]


COUNTERS = (0, 1, 2, 257, 2 ** 31, 2 ** 32 - 1)


def test_block_from_round1_equals_the_chacha_block():
    rng = random.Random(12)
    for _ in range(200):
        kw = [rng.getrandbits(32) for _ in range(8)]
        nw = [rng.getrandbits(32) for _ in range(3)]
        rc, s04 = round1(Ops(), kw, nw)
        assert len(rc) == 12
        for ctr in COUNTERS:
            got = struct.pack("<16I", *block_from_round1(Ops(), kw, rc, s04, ctr, nw))
            assert got == pyaead._chacha_block(kw, ctr, nw), (kw, nw, ctr)


def test_operation_count():
    """992 operations for a full block of a record -- 960 in the quarter
    rounds, 16 feed-forward adds, 16 payload XORs -- and 39 fewer from the
    record's constants; the constants themselves cost 3 quarter rounds and
    3 adds, once."""
    kw, nw = list(range(1, 9)), [9, 10, 11]
    payload = list(range(100, 116))
    full, once, rest = Ops(), Ops(), Ops()
    want = [full.xor(a, b) for a, b in zip(full_block(full, kw, 7, nw), payload)]
    rc, s04 = round1(once, kw, nw)
    assert [rest.xor(a, b) for a, b in zip(block_from_round1(rest, kw, rc, s04, 7, nw), payload)] == want
    assert full.n == 960 + 32 == 992
    assert rest.n == full.n - 39
    assert once.n == 3 * 12 + 3


# ---- the wave-span predicate --------------------------------------------------------

def wave_span(stride, extent):
    """keymath.h wave_span: the 64 slots of ``stride`` bytes, or up to the end
    of the last record's ``extent`` bytes if that is further."""
    return 63 * stride + max(stride, extent)


def wave_span_fits(stride, extent):
    return stride < 2 ** 31 and extent < 2 ** 31 and wave_span(stride, extent) < 2 ** 31


# (stride, extent): spans of 2^31 - 1, 2^31 and 2^31 + 1 bytes through the
# extent (stride 1 008) and through the stride (2^25 with a zero extent is
# exactly 2^31; 2^25 - 16 is the largest 16-byte multiple below it), and
# values whose product would wrap 64 bits
EDGES = [(1008, 2 ** 31 - 1 - 63 * 1008), (1008, 2 ** 31 - 63 * 1008), (1008, 2 ** 31 + 1 - 63 * 1008),
         (2 ** 25, 0), (2 ** 25, 192), (2 ** 25 - 16, 16384), (2 ** 25 - 16, 2 ** 25 - 16 + 1024), (2 ** 25 - 16, 2 ** 25 + 1008),
         (2 ** 25 - 16, 2 ** 25 + 1009), (0, 0), (0, 2 ** 31 - 1), (0, 2 ** 31), (16400, 16384), (2 ** 31, 0),
         (2 ** 58, 0), (2 ** 63, 64), (64, 2 ** 63), (2 ** 64 - 1, 2 ** 64 - 1)]


def test_wave_span_edges():
    assert [wave_span(s, e) for s, e in EDGES[:3]] == [2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1]
    assert [wave_span_fits(s, e) for s, e in EDGES[:3]] == [True, False, False]
    # strides of 2^25 (a 64-record span of 2^31 bytes) are too large, whatever the length
    assert wave_span(2 ** 25, 0) == 2 ** 31 and not wave_span_fits(2 ** 25, 0) and not wave_span_fits(2 ** 25, 192)
    assert wave_span(2 ** 25 - 16, 2 ** 25 + 1008) == 2 ** 31
    assert wave_span_fits(2 ** 25 - 16, 2 ** 25 + 1007) and not wave_span_fits(2 ** 25 - 16, 2 ** 25 + 1008)
    assert wave_span_fits(16400, 16384)       # the headline's records


def test_wave_span_header_agrees(tmp_path):
    """The header's function, compiled for the host, on the same edges."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src = tmp_path / "span.cpp"
    src.write_text('#include <cstdio>\n#include "keymath.h"\nint main() {\n'
                   + "".join('  std::printf("%%d\\n", (int)tg::wave_span_fits(%dull, %dull));\n' % e for e in EDGES)
                   + "  return 0;\n}\n")
    exe = str(tmp_path / "span")
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "tlslite-ng_amd", "csrc"), "-o", exe, str(src)],
                   check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    assert [int(v) for v in out] == [int(wave_span_fits(s, e)) for s, e in EDGES]

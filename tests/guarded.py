"""Guarded record batches: does a batch kernel write a record's own bytes and
nothing else?

Every buffer of a guarded batch is filled with a canary, the record extents
lie between canary gaps at chosen address residues (input and output chosen
independently), and every check compares the WHOLE buffer with an expected
image built on the host from the C oracle: a store past a partial last block,
a tag written one block late, a zeroing loop that runs a block long or a
stray store of zeros all land on canary and fail the comparison.  The status
array is longer than the batch and prefilled, and every input the call must
only read is compared with its host copy afterwards.

Plain numpy on the host; ``torch`` only uploads and downloads (it is passed
in, as in ``batchpack``).  ``run_guarded`` takes the thing that runs a batch
as a function, so tests/test_guarded_host.py can drive the same checks with
the oracle standing in for the GPU and with faults planted in its results.
"""
import numpy as np

CANARY_IN, CANARY_SEALED, CANARY_BACK = 0xA5, 0x5A, 0xC3
STATUS_FILL = 0xEE
STATUS_SLACK = 64
MODES = ("aligned", "skewed", "in0_out5")

# Record lengths: every one is the smallest at which a store path changes.
LENS = ([0, 1, 15, 16, 17, 31, 32, 33, 47, 63, 64, 65]            # tails and block edges
        + [1023, 1024, 1025] + [1024 + r for r in range(2, 16)]   # one octet row (8 lanes x 8 blocks) + every tail
        + [4063, 4064, 4065, 4080, 4081]                          # first 256-counter window edge (block 254)
        + [999, 1000, 1001, 1535, 1536, 1537, 2047, 2048, 2049]   # key-table splits
        + [4095, 4096, 4097]                                      # the 32-lane row (32 x 8 blocks)
        + [16383, 16384, 16385, 16400, 16640])                    # full TLS records; 16385: lone last block
PLANNED_N = 2100    # above the planner's threshold (kPlanMinRecords = 2049)


def case_lens(seed, n=None):
    """``LENS`` shuffled by ``seed``; with ``n``, first padded with short
    records (0..199 bytes) to ``n`` records for the planned-order paths."""
    rng = np.random.default_rng(seed)
    lens = list(LENS)
    if n is not None:
        lens += [int(x) for x in rng.integers(0, 200, n - len(lens))]
    return [lens[j] for j in rng.permutation(len(lens))]


def mode_leads(mode, n):
    """(in leads, out leads) of a mode: the residue mod 16 of each extent's
    address in the plaintext buffers and in the sealed buffer."""
    i = np.arange(n)
    if mode == "aligned":
        return np.zeros(n, np.int64), np.zeros(n, np.int64)
    if mode == "skewed":
        # both run through all 16 residues; the in lead is 0 at i = 11 (mod 16)
        # where the out lead is 15, the out lead 0 at i = 8 where the in lead
        # is 11.  (With 5 i + 9 both would be 0 at i = 11, and no record would
        # have one side aligned and the other not.)
        return (7 * i + 3) % 16, (5 * i + 8) % 16
    if mode == "in0_out5":
        return np.zeros(n, np.int64), np.full(n, 5, np.int64)
    raise ValueError("unknown mode %r" % (mode,))


class ContainmentError(AssertionError):
    """A guarded check failed.  ``what`` names the check and the buffer;
    for a byte difference ``record`` / ``rel`` / ``extent`` locate it: the
    record whose extent is nearest, the offset relative to that extent's
    start (negative in the gap before it, >= ``extent`` in the gap after)."""

    def __init__(self, what, record=None, rel=None, extent=None, expected=None, got=None, offset=None):
        self.what, self.record, self.rel, self.extent = what, record, rel, extent
        self.expected, self.got, self.offset = expected, got, offset
        AssertionError.__init__(
            self, "%s: first difference at (record %r, offset %r relative to its extent, extent length %r, "
            "expected %s, got %s) [buffer offset %r]" % (what, record, rel, extent, _hex(expected), _hex(got), offset))


def _hex(v):
    return "None" if v is None else "0x%02x" % int(v)


def _place(sizes, leads, gap, guard):
    """Offsets with ``off % 16 == lead``, at least ``gap`` bytes after the
    previous extent, ``guard`` bytes before the first and after the last."""
    offs, pos = [], guard
    for size, lead in zip(sizes, leads):
        pos += (int(lead) - pos) % 16
        offs.append(pos)
        pos += int(size) + gap
    total = pos - gap + guard if offs else 2 * guard
    return np.array(offs, dtype=np.uint64), int(total)


class GuardedLayout(object):
    """Three canary-guarded buffers for one batch: plaintext in (extents of
    ``lens[i]`` bytes at residue ``in_lead[i]``), sealed (``lens[i] + tag``
    bytes at residue ``out_lead[i]``) and plaintext back (as plaintext in).
    ``in_lead`` / ``out_lead`` default to the leads of ``mode``."""

    def __init__(self, lens, tag, mode, in_lead=None, out_lead=None, gap=48, guard=256, seed=0, key_count=1):
        rng = np.random.default_rng(seed)
        self.n = n = len(lens)
        self.tag, self.mode, self.gap, self.guard = int(tag), mode, int(gap), int(guard)
        self.lens = np.asarray(lens, dtype=np.uint32)
        mi, mo = mode_leads(mode, n) if (in_lead is None or out_lead is None) else (None, None)
        self.in_lead = np.asarray(mi if in_lead is None else in_lead, dtype=np.int64)
        self.out_lead = np.asarray(mo if out_lead is None else out_lead, dtype=np.int64)
        L = self.lens.astype(np.int64)
        self.in_off, self.in_bytes = _place(L, self.in_lead, gap, guard)
        self.sealed_off, self.sealed_bytes = _place(L + self.tag, self.out_lead, gap, guard)
        self.back_off, self.back_bytes = self.in_off.copy(), self.in_bytes
        self.inp = np.full(self.in_bytes, CANARY_IN, np.uint8)
        for o, l in zip(self.in_off, L):
            self.inp[int(o):int(o) + int(l)] = rng.integers(0, 256, int(l), dtype=np.uint8)
        self.nonces = rng.integers(0, 256, 12 * n, dtype=np.uint8)
        self.aad_len = rng.integers(0, 41, n).astype(np.uint32)       # random lengths 0..40, packed
        self.aad_off = np.concatenate([[0], np.cumsum(self.aad_len)[:-1]]).astype(np.uint64)
        self.aad = rng.integers(0, 256, int(self.aad_len.sum()) + 16, dtype=np.uint8)
        self.key_idx = rng.integers(0, key_count, n).astype(np.uint32) if key_count > 1 else None
        self.check_bounds()

    def extents(self, buf):
        """(offsets, sizes, buffer bytes) of ``buf``: "in", "sealed" or "back"."""
        L = self.lens.astype(np.int64)
        if buf == "sealed":
            return self.sealed_off.astype(np.int64), L + self.tag, self.sealed_bytes
        off = self.in_off if buf == "in" else self.back_off
        return off.astype(np.int64), L, self.in_bytes if buf == "in" else self.back_bytes

    def check_bounds(self):
        """Every extent, with a full gap either side of it, lies inside its
        buffer (a block plus a tag past an extent is still canary of this
        allocation), extents keep their residues and never share a gap."""
        assert self.gap >= 48 and self.guard >= self.gap
        for buf, lead in (("in", self.in_lead), ("sealed", self.out_lead), ("back", self.in_lead)):
            off, size, total = self.extents(buf)
            assert np.array_equal(off % 16, lead), buf
            if self.n:
                assert int(off.min()) - self.guard >= 0 and int((off + size).max()) + self.guard <= total, buf
                assert (off - self.gap >= 0).all() and (off + size + self.gap <= total).all(), buf
                assert (off[1:] - (off + size)[:-1] >= self.gap).all(), buf

    def locate(self, buf, pos):
        """(record, relative offset, extent length) of buffer offset ``pos``:
        the record whose extent holds it or lies nearest (a tie goes to the
        extent before)."""
        off, size, _ = self.extents(buf)
        end = off + size
        dist = np.where(pos < off, off - pos, np.where(pos >= end, pos - end + 1, 0))
        i = int(np.argmin(dist))
        return i, int(pos - off[i]), int(size[i])

    def canary_image(self, buf):
        _, _, total = self.extents(buf)
        return np.full(total, {"in": CANARY_IN, "sealed": CANARY_SEALED, "back": CANARY_BACK}[buf], np.uint8)

    def expected_sealed(self, oracle_mod, alg, keys, nthreads=8):
        """The whole sealed buffer: canary, with the oracle's ct || tag in every extent."""
        img = self.canary_image("sealed")
        oracle_mod.batch(alg, "seal", keys, self.nonces, self.aad, self.aad_off, self.aad_len, self.inp,
                         self.in_off, self.lens, img.size, self.sealed_off, key_idx=self.key_idx,
                         nthreads=nthreads, out=img)
        return img

    def expected_back(self, rejected=()):
        """The whole plaintext-back buffer: canary, the plaintext in every
        accepted record's ``L`` bytes, ``L`` zero bytes in every rejected one's."""
        img = self.canary_image("back")
        for i in range(self.n):
            o, s, L = int(self.back_off[i]), int(self.in_off[i]), int(self.lens[i])
            img[o:o + L] = 0 if i in rejected else self.inp[s:s + L]
        return img


# ---- tampering -------------------------------------------------------------------

def make_reject(layout, seed=0):
    """record index -> tamper class for the third call of ``run_guarded``:
    ("tag", j, bit) for every tag byte j < T with bits 0x01 and 0x80,
    ("ct_first",), ("ct_last",) on a record with L % 16 != 0 and on one with
    L % 16 == 0, ("aad",) and ("nonce",).  Records of length 0 take tag
    tampering only (and one of them always does)."""
    rng = np.random.default_rng(seed)
    T, lens, alen = layout.tag, layout.lens, layout.aad_len
    # candidates in random order, a long record and a short one in turn, so
    # that a batch padded with short records still rejects the long ones
    perm = [int(i) for i in rng.permutation(layout.n)]
    long_, short = [i for i in perm if lens[i] >= 200], [i for i in perm if lens[i] < 200]
    free = [i for pair in zip(long_, short) for i in pair] + long_[len(short):] + short[len(long_):]
    reject = {}

    def take(pred, prefer=lambda i: True):
        for want in (lambda i: pred(i) and prefer(i), pred):
            for i in free:
                if want(i):
                    free.remove(i)
                    return i
        raise ValueError("no record left for a tamper class")

    many_rows = lambda i: lens[i] >= 1000   # noqa: E731  (zeroed by several lanes, over several rows)
    reject[take(lambda i: lens[i] > 0 and lens[i] % 16 != 0, many_rows)] = ("ct_last",)
    reject[take(lambda i: lens[i] > 0 and lens[i] % 16 == 0, many_rows)] = ("ct_last",)
    reject[take(lambda i: lens[i] > 0)] = ("ct_first",)
    reject[take(lambda i: lens[i] > 16 and lens[i] % 16 != 0)] = ("ct_first",)
    reject[take(lambda i: alen[i] > 0 and lens[i] > 0)] = ("aad",)
    reject[take(lambda i: lens[i] > 0)] = ("nonce",)
    classes = [("tag", j, bit) for j in range(T) for bit in (0x01, 0x80)]
    if (lens == 0).any():
        reject[take(lambda i: lens[i] == 0)] = classes.pop(0)
    for c in classes:
        reject[take(lambda i: True)] = c
    return reject


def tamper(layout, sealed, reject):
    """(sealed, aad, nonces) copies with the records of ``reject`` tampered."""
    sealed, aad, nonces = sealed.copy(), layout.aad.copy(), layout.nonces.copy()
    for i, c in reject.items():
        o, L = int(layout.sealed_off[i]), int(layout.lens[i])
        if c[0] == "tag":
            assert 0 <= c[1] < layout.tag and c[2] in (0x01, 0x80)
            sealed[o + L + c[1]] ^= c[2]
        elif c[0] in ("ct_first", "ct_last"):
            assert L > 0, "a record of length 0 takes tag tampering only"
            sealed[o + (0 if c[0] == "ct_first" else L - 1)] ^= 0x10
        elif c[0] == "aad":
            assert layout.aad_len[i] > 0
            aad[int(layout.aad_off[i]) + int(layout.aad_len[i]) // 2] ^= 0x04
        elif c[0] == "nonce":
            nonces[12 * i + (i % 12)] ^= 0x40
        else:
            raise ValueError("unknown tamper class %r" % (c,))
    return sealed, aad, nonces


def check_reject_coverage(layout, reject):
    """The set of tamper classes section by section: every tag byte with both
    bits, first / last ciphertext byte (last on a partial and on a full last
    block), AAD and nonce."""
    cls = list(reject.values())
    for j in range(layout.tag):
        for bit in (0x01, 0x80):
            assert ("tag", j, bit) in cls, (j, bit)
    last = [int(layout.lens[i]) % 16 for i, c in reject.items() if c == ("ct_last",)]
    assert any(r != 0 for r in last) and any(r == 0 for r in last)
    for c in (("ct_first",), ("aad",), ("nonce",)):
        assert c in cls, c
    assert all(c[0] == "tag" for i, c in reject.items() if layout.lens[i] == 0)
    if (layout.lens >= 1000).any():    # the zeroing of a record of many rows, with and without a tail
        assert any(layout.lens[i] >= 1000 and layout.lens[i] % 16 for i in reject)
        assert any(layout.lens[i] >= 1000 and layout.lens[i] % 16 == 0 for i in reject)


# ---- the device ---------------------------------------------------------------------

_SIGNED = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}


def upload(torch, a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(_SIGNED.get(a.dtype, a.dtype)).copy()).to("cuda")


def download(t, dtype):
    return t.cpu().numpy().view(dtype)


def gpu_device(torch, tg, key_obj):
    """The function ``run_guarded`` drives: ``call(op, arrays)`` uploads the
    host arrays of one batch, runs tg_seal_batch / tg_open_batch on them and
    returns every array as the device left it."""
    def call(op, a):
        d = dict((k, upload(torch, v)) for k, v in a.items() if v is not None)
        # torch's allocations are 256-byte aligned: the layout's leads are address residues
        assert d["inp"].data_ptr() % 16 == 0 and d["out"].data_ptr() % 16 == 0
        b = tg.make_batch(len(a["lens"]), d["inp"], d["out"], d["nonces"], aad=d["aad"], lens=d["lens"],
                          in_off=d["in_off"], out_off=d["out_off"], aad_off=d["aad_off"],
                          aad_len=d["aad_len"], key_idx=d.get("key_idx"), status=d.get("status"))
        (tg.seal_batch if op == "seal" else tg.open_batch)(key_obj, b)
        torch.cuda.synchronize()
        return dict((k, download(t, a[k].dtype)) for k, t in d.items())
    return call


READ_ONLY = ("inp", "aad", "nonces", "lens", "in_off", "out_off", "aad_off", "aad_len", "key_idx")


def _first_diff(a, b):
    return int(np.flatnonzero(a != b)[0])


def _check_call(layout, step, got, sent, out_buf, in_buf, want_out, want_status):
    """One call's results: the whole output image, the status array, and every
    read-only input against what was sent."""
    if got["out"].shape != want_out.shape or not np.array_equal(got["out"], want_out):
        p = _first_diff(got["out"], want_out)
        i, rel, size = layout.locate(out_buf, p)
        raise ContainmentError("%s: %s buffer" % (step, out_buf), i, rel, size, want_out[p], got["out"][p], p)
    if want_status is not None:
        st = got["status"]
        if not np.array_equal(st, want_status):
            p = _first_diff(st, want_status)
            raise ContainmentError("%s: status[%d] (n = %d)" % (step, p, layout.n), p if p < layout.n else None,
                                   None, None, want_status[p], st[p], p)
    for name in READ_ONLY:
        if sent[name] is None:
            continue
        if not np.array_equal(got[name], sent[name]):
            p = _first_diff(got[name], sent[name])
            if name == "inp":
                i, rel, size = layout.locate(in_buf, p)
                raise ContainmentError("%s: input %s buffer was written" % (step, in_buf), i, rel, size,
                                       sent[name][p], got[name][p], p)
            raise ContainmentError("%s: read-only array %s was written at entry %d" % (step, name, p),
                                   None, None, None, None, None, p)


def _status(layout, rejected=()):
    st = np.full(layout.n + STATUS_SLACK, STATUS_FILL, np.uint8)
    st[:layout.n] = 1
    st[list(rejected)] = 0
    return st


def run_guarded(torch, tg, oracle_mod, layout, alg, keys, key_obj, reject, device=None):
    """One seal and two opens of ``layout``, each checked over whole buffers:
    1. seal: the sealed image equals canary + the oracle's ct || tag;
    2. open of the untampered sealed buffer: every status 1, the plaintext
       image equals canary + plaintext (the gap after each ``L`` bytes
       still canary: neither the tag nor the rest of a tail block lands there);
    3. open of a copy tampered as ``reject`` says: those records status 0 with
       exactly ``L`` zero bytes, the others status 1 with their plaintext.
    After every call the status entries past ``n`` still hold their fill and
    the inputs equal their host copies.  ``device``: see ``gpu_device``."""
    call = device if device is not None else gpu_device(torch, tg, key_obj)
    lay = layout
    common = {"lens": lay.lens, "aad_off": lay.aad_off, "aad_len": lay.aad_len, "key_idx": lay.key_idx}
    # 1. seal
    sent = dict(common, inp=lay.inp, out=lay.canary_image("sealed"), nonces=lay.nonces, aad=lay.aad,
                in_off=lay.in_off, out_off=lay.sealed_off, status=None)
    sealed = lay.expected_sealed(oracle_mod, alg, keys)
    _check_call(lay, "seal", call("seal", sent), sent, "sealed", "in", sealed, None)
    # 2. open what was sealed
    sent = dict(common, inp=sealed, out=lay.canary_image("back"), nonces=lay.nonces, aad=lay.aad,
                in_off=lay.sealed_off, out_off=lay.back_off,
                status=np.full(lay.n + STATUS_SLACK, STATUS_FILL, np.uint8))
    _check_call(lay, "open", call("open", sent), sent, "back", "sealed", lay.expected_back(), _status(lay))
    # 3. open a tampered copy
    bad, aad, nonces = tamper(lay, sealed, reject)
    sent = dict(sent, inp=bad, aad=aad, nonces=nonces, out=lay.canary_image("back"),
                status=np.full(lay.n + STATUS_SLACK, STATUS_FILL, np.uint8))
    _check_call(lay, "open tampered", call("open", sent), sent, "back", "sealed",
                lay.expected_back(set(reject)), _status(lay, reject))

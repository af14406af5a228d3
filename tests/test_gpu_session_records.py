"""GPU: record framing for many sessions in one batch
(tg_seal_session_records / tg_open_session_records, tlsgpu.Sessions) against
the reference RecordLayer's wire bytes for interleaved connections
(tests/golden/sessions.json), the framing oracle (oracle/records.py), the
single-connection path and numpy's stable rank."""
import functools
import hashlib

import numpy as np
import pytest

from vectors import detbytes, load

pytestmark = pytest.mark.gpu

CASES = load("sessions.json")
COMBOS = [("tls13", "aes128gcm", 16, 12), ("tls13", "chacha20-poly1305", 32, 12),
          ("tls12", "aes256gcm", 32, 4), ("tls12", "chacha20-poly1305", 32, 12),
          ("tls13", "aes128ccm_8", 16, 12), ("tls12", "aes256ccm", 32, 4)]
SENTINEL = -0x0123456789abcdef   # seq_out of a skipped record stays as it was


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    return t


@pytest.fixture(scope="module")
def tg(torch):
    import tlsgpu
    return tlsgpu


def _table_alg(alg):
    if alg.startswith("chacha"):
        return "chacha20-poly1305"
    if "ccm" in alg:
        return "aesccm_8" if alg.endswith("_8") else "aesccm"
    return "aesgcm"


def _tag(alg):
    return 8 if alg.endswith("ccm_8") else 16


def _hdr(version, alg):
    return 5 + (8 if version == "tls12" and not alg.startswith("chacha") else 0)


def _i64(values):
    """64-bit sequence numbers / 32-bit sessions as the signed arrays torch takes."""
    return np.array([int(v) & (2 ** 64 - 1) for v in values], np.uint64).view(np.int64)


def _i32(values):
    return np.array([int(v) & (2 ** 32 - 1) for v in values], np.uint32).view(np.int32)


def _host_rank(sessions, starts):
    """The contract in plain Python: in batch order, every in-range record
    takes its session's counter and advances it."""
    nxt = [int(s) for s in starts]
    seq = []
    for s in sessions:
        if s < len(nxt):
            seq.append(nxt[s])
            nxt[s] += 1
        else:
            seq.append(None)
    return seq, nxt


class Batch(object):
    """Host layout and device tensors of one many-session batch: data offsets
    16-aligned with slack for ctype + padding + tag, wire payloads 16-aligned
    if ``aligned`` else records packed back to back."""

    def __init__(self, torch, version, alg, sessions, ctypes_, datas, pads, aligned=True):
        self.torch, self.version, self.alg = torch, version, alg
        self.n = len(datas)
        self.sessions, self.ctypes, self.datas, self.pads = list(sessions), list(ctypes_), datas, list(pads)
        self.hdr, self.tag = _hdr(version, alg), _tag(alg)
        data_off, wire_off, d, w = [], [], 0, 0
        for x, p in zip(datas, pads):
            data_off.append(d)
            d += (len(x) + 1 + p + self.tag + 15) // 16 * 16
            if aligned:
                w = (w + self.hdr + 15) // 16 * 16 - self.hdr
            wire_off.append(w)
            w += self.hdr + len(x) + 1 + p + self.tag
        self.data_off, self.wire_off = np.array(data_off, np.int64), np.array(wire_off, np.int64)
        self.dsz, self.wsz = d + 16, w + 64
        host = np.zeros(self.dsz, np.uint8)
        for o, x in zip(data_off, datas):
            host[o:o + len(x)] = np.frombuffer(bytes(x), np.uint8)
        self.host = host
        self.d_off, self.w_off = self.dev(self.data_off), self.dev(self.wire_off)
        self.d_sess = self.dev(_i32(sessions))

    def dev(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def room(self, i, wire):
        """Bytes record i owns in the wire buffer (the most its record can
        take) or in the data buffer."""
        return (self.hdr if wire else 0) + len(self.datas[i]) + 1 + self.pads[i] + self.tag

    def seal(self, tg, table, ivs, seq=None, seq_next=None):
        """-> (wire bytes per record, seq_out, whole wire buffer)"""
        torch = self.torch
        v = tg.TLS13 if self.version == "tls13" else tg.TLS12
        data = self.dev(self.host)
        d_len = self.dev(np.array([len(x) for x in self.datas], np.int32))
        ctype = self.dev(np.array(self.ctypes, np.uint8))
        pad = self.dev(np.array(self.pads, np.int32)) if self.version == "tls13" else None
        wire = torch.zeros(self.wsz, dtype=torch.uint8, device="cuda")
        w_len = torch.full((self.n,), 77, dtype=torch.int32, device="cuda")
        seq_out = torch.full((self.n,), SENTINEL, dtype=torch.int64, device="cuda")
        tg.seal_session_records(table, v, ivs, self.d_sess, self.n, data, self.d_off, d_len, ctype, wire,
                                self.w_off, w_len, seq=seq, seq_next=seq_next, seq_out=seq_out, pad_len=pad)
        torch.cuda.synchronize()
        wh, wl = wire.cpu().numpy(), w_len.cpu().numpy()
        wires = [wh[o:o + l].tobytes() for o, l in zip(self.wire_off, wl)]
        return wires, seq_out.cpu().numpy(), wh

    def open(self, tg, table, ivs, wires, seq=None, seq_next=None):
        """-> ((status, ctype, data) per record, seq_out, whole output buffer)"""
        torch = self.torch
        v = tg.TLS13 if self.version == "tls13" else tg.TLS12
        wh = np.zeros(self.wsz, np.uint8)
        for o, w in zip(self.wire_off, wires):
            wh[o:o + len(w)] = np.frombuffer(w, np.uint8)
        wire = self.dev(wh)
        w_len = self.dev(np.array([len(w) for w in wires], np.int32))
        out = torch.full((self.dsz,), 0xA5, dtype=torch.uint8, device="cuda")
        o_len = torch.full((self.n,), 77, dtype=torch.int32, device="cuda")
        o_ct = torch.full((self.n,), 77, dtype=torch.uint8, device="cuda")
        st = torch.full((self.n,), 255, dtype=torch.uint8, device="cuda")
        seq_out = torch.full((self.n,), SENTINEL, dtype=torch.int64, device="cuda")
        tg.open_session_records(table, v, ivs, self.d_sess, self.n, wire, self.w_off, w_len, out, self.d_off,
                                o_len, o_ct, st, seq=seq, seq_next=seq_next, seq_out=seq_out)
        torch.cuda.synchronize()
        oh = out.cpu().numpy()
        opened = [(int(s), int(c), oh[o:o + l].tobytes()) for s, c, o, l in
                  zip(st.cpu().numpy(), o_ct.cpu().numpy(), self.data_off, o_len.cpu().numpy())]
        return opened, seq_out.cpu().numpy(), oh


def _ivs(torch, ivs):
    return torch.from_numpy(np.frombuffer(b"".join(ivs), np.uint8).reshape(len(ivs), len(ivs[0])).copy()).cuda()


# ---- 1. the reference's wire bytes, counter mode ------------------------------

@pytest.mark.parametrize("ci", range(len(CASES)))
@pytest.mark.parametrize("aligned", [True, False])
def test_reference_wire_bytes_counter_mode(torch, tg, ci, aligned):
    c = CASES[ci]
    recs = c["records"]
    keys = [bytes.fromhex(k) for k in c["keys"]]
    ivs = _ivs(torch, [bytes.fromhex(v) for v in c["ivs"]])
    sessions = [r["conn"] for r in recs]
    datas = [bytes(detbytes("srec-%d-%d" % (i, r["len"]), r["len"])) for i, r in enumerate(recs)]
    b = Batch(torch, c["version"], c["alg"], sessions, [r["ctype"] for r in recs], datas,
              [r["pad"] for r in recs], aligned)
    table = tg.KeyTable(_table_alg(c["alg"]), keys)
    want_seq, want_next = _host_rank(sessions, c["starts"])
    assert want_next[4] == c["starts"][4]                       # the session without records
    assert any(q == 2 ** 32 for q in want_seq)                  # the carry is inside the batch
    nxt = torch.from_numpy(_i64(c["starts"])).cuda()
    wires, seq_out, _ = b.seal(tg, table, ivs, seq_next=nxt)
    for r, w in zip(recs, wires):
        assert len(w) == r["wire_len"]
        assert hashlib.sha256(w).hexdigest() == r["wire_sha256"], (c["version"], c["alg"])
    assert np.array_equal(seq_out, _i64(want_seq))
    assert np.array_equal(nxt.cpu().numpy(), _i64(want_next))
    nxt2 = torch.from_numpy(_i64(c["starts"])).cuda()
    opened, seq_out2, _ = b.open(tg, table, ivs, wires, seq_next=nxt2)
    for r, d, o in zip(recs, datas, opened):
        assert o == (0, r["ctype"], d)
    assert np.array_equal(seq_out2, _i64(want_seq))
    assert np.array_equal(nxt2.cpu().numpy(), _i64(want_next))


# ---- 2. a random batch against the oracle, explicit mode -----------------------

NSESS = 7
BOUNDARY = [0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 1535, 1536, 1537, 2047, 2048, 2049,
            4095, 4096, 4097, 16384]
BAD = {30: NSESS, 77: 2 ** 32 - 1}      # record -> out-of-range session


@functools.lru_cache(maxsize=None)
def _random_case(version, alg, klen, ivlen):
    """Host side of the 120-record batch of tests 2 and 3 (built once)."""
    rng = np.random.default_rng(1000 + klen + ivlen + len(alg))
    n = 120
    keys = [rng.bytes(klen) for _ in range(NSESS)]
    ivs = [rng.bytes(ivlen) for _ in range(NSESS)]
    lens = [int(x) for x in rng.integers(0, 3000, n - len(BOUNDARY))] + BOUNDARY
    lens = [lens[j] for j in rng.permutation(n)]
    # padding as far as the receiver's inner-plaintext limit allows
    pads = [min(int(rng.integers(0, 256)), 16384 - L) if version == "tls13" else 0 for L in lens]
    ctypes_ = [int(x) for x in rng.choice([21, 22, 23], n)]
    datas = [rng.bytes(L) for L in lens]
    sessions = [int(x) for x in rng.integers(0, NSESS, n)]
    for i, s in BAD.items():
        sessions[i] = s
    seq = [int(x) for x in rng.integers(0, 2 ** 64, n, dtype=np.uint64)]
    return keys, ivs, lens, pads, ctypes_, datas, sessions, seq


def _tamper_at(lens):
    """Three in-range records long enough for every tampering below."""
    return [i for i, L in enumerate(lens) if i not in BAD and 100 <= L < 3000][:3]


def _untouched(b, i, buf, wire, value):
    lo = int((b.wire_off if wire else b.data_off)[i])
    return bool((buf[lo:lo + b.room(i, wire)] == value).all())


@pytest.mark.parametrize("version,alg,klen,ivlen", COMBOS)
def test_random_batch_vs_oracle_explicit_mode(torch, tg, version, alg, klen, ivlen):
    from oracle import records as R
    keys, ivs, lens, pads, ctypes_, datas, sessions, seq = _random_case(version, alg, klen, ivlen)
    n = len(datas)
    assert set(BOUNDARY) <= set(lens) and set(range(NSESS)) <= set(sessions)
    b = Batch(torch, version, alg, sessions, ctypes_, datas, pads)
    table = tg.KeyTable(_table_alg(alg), keys)
    d_ivs = _ivs(torch, ivs)
    d_seq = torch.from_numpy(_i64(seq)).cuda()
    wires, seq_out, wh = b.seal(tg, table, d_ivs, seq=d_seq)
    want = {}
    for i in range(n):
        if i in BAD:   # skipped: length 0, not a byte of its wire room written, no number
            assert wires[i] == b"" and _untouched(b, i, wh, True, 0), i
            assert seq_out[i] == SENTINEL
            continue
        s = sessions[i]
        want[i] = R.seal_record(version, alg, keys[s], ivs[s], seq[i], ctypes_[i], datas[i], pads[i])
        assert wires[i] == want[i], (i, lens[i])
    assert np.array_equal(np.delete(seq_out, list(BAD)), np.delete(_i64(seq), list(BAD)))
    t0, t1, t2 = _tamper_at(lens)
    tamper = {t0: lambda w: w[:-1] + bytes([w[-1] ^ 1]),               # bad tag
              t1: lambda w: w[:21] if version == "tls13" else w[:12]}  # truncated
    if version == "tls13":
        tamper[t2] = lambda w: b"\x16" + w[1:]                         # wrong outer type
    sent = [tamper[i](w) if i in tamper else w for i, w in enumerate(wires)]
    # the skipped records carry a well-formed record of session 0: status 8 all the same
    for i in BAD:
        sent[i] = R.seal_record(version, alg, keys[0], ivs[0], seq[i], 23, datas[i][:64], 0)
    opened, _, oh = b.open(tg, table, d_ivs, sent, seq=d_seq)
    for i in range(n):
        if i in BAD:
            assert opened[i] == (8, 0, b"") and _untouched(b, i, oh, False, 0xA5), i
        elif i in tamper:
            s = sessions[i]
            exp = R.open_record(version, alg, keys[s], ivs[s], seq[i], tamper[i](want[i]))
            assert opened[i][0] == exp[0] != 0, (i, opened[i][0], exp[0])
        else:
            assert opened[i] == (0, ctypes_[i], datas[i]), (i, lens[i])


# ---- 3. the same bytes as the single-connection path ---------------------------

def _single_key(tg, alg, key):
    if alg.startswith("chacha"):
        return tg.HipCHACHA20_POLY1305(bytearray(key))
    if "ccm" in alg:
        return tg.HipAESCCM(bytearray(key), tag_length=8 if alg.endswith("_8") else 16)
    return tg.HipAESGCM(bytearray(key))


@pytest.mark.parametrize("version,alg,klen,ivlen", COMBOS)
def test_counter_mode_equals_single_connection_path(torch, tg, version, alg, klen, ivlen):
    keys, ivs, lens, pads, ctypes_, datas, sessions, _ = _random_case(version, alg, klen, ivlen)
    starts = [3, 2 ** 32 - 5, 2 ** 40 + 3, 0, 2 ** 63 + 11, 255, 2 ** 16]
    b = Batch(torch, version, alg, sessions, ctypes_, datas, pads)
    nxt = torch.from_numpy(_i64(starts)).cuda()
    wires, seq_out, _ = b.seal(tg, tg.KeyTable(_table_alg(alg), keys), _ivs(torch, ivs), seq_next=nxt)
    want_seq, want_next = _host_rank(sessions, starts)
    assert np.array_equal(seq_out, _i64([SENTINEL if q is None else q for q in want_seq]))
    assert np.array_equal(nxt.cpu().numpy(), _i64(want_next))
    s0 = 1   # its counter crosses 2^32 when it owns more than five records
    mine = [i for i in range(len(datas)) if sessions[i] == s0]
    assert len(mine) > 5
    sub = Batch(torch, version, alg, [0] * len(mine), [ctypes_[i] for i in mine], [datas[i] for i in mine],
                [pads[i] for i in mine])
    v = tg.TLS13 if version == "tls13" else tg.TLS12
    # tg_seal_records, single-key handle, seq0 = the session's counter
    wire = torch.zeros(sub.wsz, dtype=torch.uint8, device="cuda")
    w_len = torch.zeros(sub.n, dtype=torch.int32, device="cuda")
    tg.seal_records(_single_key(tg, alg, keys[s0]), v, ivs[s0], starts[s0], sub.n, sub.dev(sub.host), sub.d_off,
                    sub.dev(np.array([len(x) for x in sub.datas], np.int32)),
                    sub.dev(np.array(sub.ctypes, np.uint8)), wire, sub.w_off, w_len,
                    pad_len=sub.dev(np.array(sub.pads, np.int32)) if version == "tls13" else None)
    torch.cuda.synchronize()
    wh, wl = wire.cpu().numpy(), w_len.cpu().numpy()
    single = [wh[o:o + l].tobytes() for o, l in zip(sub.wire_off, wl)]
    assert single == [wires[i] for i in mine]
    # a table of one key, nsessions == 1 (KeyTable and the AEAD object alike),
    # with two out-of-range records in the middle: they take no number
    k = len(mine) // 2
    sess1 = [0] * k + [1, 2 ** 32 - 1] + [0] * (len(mine) - k)
    pick = mine[:k] + [mine[0], mine[1]] + mine[k:]
    one = Batch(torch, version, alg, sess1, [ctypes_[i] for i in pick], [datas[i] for i in pick],
                [pads[i] for i in pick])
    for table in (tg.KeyTable(_table_alg(alg), [keys[s0]]), _single_key(tg, alg, keys[s0])):
        nxt1 = torch.from_numpy(_i64([starts[s0]])).cuda()
        w1, q1, wh1 = one.seal(tg, table, _ivs(torch, [ivs[s0]]), seq_next=nxt1)
        assert w1[:k] + w1[k + 2:] == single
        assert w1[k] == b"" and w1[k + 1] == b""
        assert _untouched(one, k, wh1, True, 0) and _untouched(one, k + 1, wh1, True, 0)
        assert q1[k] == SENTINEL and q1[k + 1] == SENTINEL
        assert int(nxt1[0]) == int(_i64([starts[s0] + len(mine)])[0])
        nxt2 = torch.from_numpy(_i64([starts[s0]])).cuda()
        sent = list(w1)
        sent[k] = sent[k + 1] = single[0]
        opened, _, oh = one.open(tg, table, _ivs(torch, [ivs[s0]]), sent, seq_next=nxt2)
        for j, i in enumerate(pick):
            if j in (k, k + 1):
                assert opened[j] == (8, 0, b"") and _untouched(one, j, oh, False, 0xA5)
            else:
                assert opened[j] == (0, ctypes_[i], datas[i]), j
        assert int(nxt2[0]) == int(nxt1[0])


# ---- 4. the rank pass at size ----------------------------------------------------

def test_rank_pass_at_size(torch, tg):
    from oracle import records as R
    n, nsess, L, stride = 70000, 300, 8, 32
    big = 7
    rng = np.random.default_rng(70000)
    active = np.setdiff1d(np.arange(nsess), rng.choice(np.setdiff1d(np.arange(nsess), [big]), 50, replace=False))
    sess = np.where(rng.random(n) < 0.6, big, rng.choice(active, n)).astype(np.int64)
    bad_pos = np.unique(np.concatenate([[0, n - 1], np.linspace(1000, n - 1000, 48).astype(np.int64)]))
    assert len(bad_pos) == 50
    bad_val = np.array([nsess, 2 ** 32 - 1, nsess + 1, 65536, 2 ** 31], np.int64)[np.arange(50) % 5]
    sess[bad_pos] = bad_val
    ok = sess < nsess
    counts = np.bincount(sess[ok], minlength=nsess)
    assert counts[big] > 40000 and int((counts == 0).sum()) >= 50
    starts = rng.integers(0, 2 ** 62, nsess, dtype=np.uint64)
    starts[big] = 2 ** 32 - 2
    # numpy's stable rank: position inside the session's run of a stable sort
    idx = np.flatnonzero(ok)
    order = idx[np.argsort(sess[idx], kind="stable")]
    _, first, cnt = np.unique(sess[order], return_index=True, return_counts=True)
    rank = np.arange(len(order)) - np.repeat(first, cnt)
    want_seq = np.zeros(n, np.uint64)
    want_seq[order] = starts[sess[order]] + rank.astype(np.uint64)
    want_seq = want_seq.view(np.int64).copy()
    want_seq[~ok] = SENTINEL
    want_next = (starts + counts.astype(np.uint64)).view(np.int64)

    keys = [bytes(detbytes("rank-key-%d" % s, 32)) for s in range(nsess)]
    ivs = [bytes(detbytes("rank-iv-%d" % s, 12)) for s in range(nsess)]
    table = tg.KeyTable("chacha20-poly1305", keys)
    d_ivs = _ivs(torch, ivs)
    g = torch.Generator(device="cuda").manual_seed(7)
    data = torch.randint(0, 256, (n * stride,), dtype=torch.uint8, device="cuda", generator=g)
    payload = data.view(n, stride)[:, :L].cpu().numpy()
    off = torch.arange(n, dtype=torch.int64, device="cuda") * stride
    d_len = torch.full((n,), L, dtype=torch.int32, device="cuda")
    ctype = torch.full((n,), 23, dtype=torch.uint8, device="cuda")
    d_sess = torch.from_numpy(_i32(sess)).cuda()

    def seal(lo, hi, nxt, wire, w_len, seq_out):
        tg.seal_session_records(table, tg.TLS13, d_ivs, d_sess[lo:hi], hi - lo, data, off[lo:hi],
                                d_len[lo:hi], ctype[lo:hi], wire, off[lo:hi], w_len[lo:hi], seq_next=nxt,
                                seq_out=seq_out[lo:hi])

    def fresh():
        return (torch.from_numpy(starts.view(np.int64).copy()).cuda(),
                torch.zeros(n * stride, dtype=torch.uint8, device="cuda"),
                torch.full((n,), 77, dtype=torch.int32, device="cuda"),
                torch.full((n,), SENTINEL, dtype=torch.int64, device="cuda"))

    nxt, wire, w_len, seq_out = fresh()
    seal(0, n, nxt, wire, w_len, seq_out)
    torch.cuda.synchronize()
    assert np.array_equal(seq_out.cpu().numpy(), want_seq)
    assert np.array_equal(nxt.cpu().numpy(), want_next)
    wl = w_len.cpu().numpy()
    assert np.array_equal(wl, np.where(ok, 5 + L + 1 + 16, 0))
    wh = wire.cpu().numpy().reshape(n, stride)
    assert not wh[~ok].any()
    # 512 records against the oracle: the large session's first and last, every
    # neighbour of a skipped record, the rest drawn at random
    of_big = np.flatnonzero(sess == big)
    sample = {int(of_big[0]), int(of_big[-1])}
    for p in bad_pos:
        sample.update(int(q) for q in (p - 1, p + 1) if 0 <= q < n and ok[q])
    sample.update([int(q) for q in rng.permutation(idx) if int(q) not in sample][:512 - len(sample)])
    assert len(sample) == 512
    for i in sorted(sample):
        s = int(sess[i])
        w = R.seal_record("tls13", "chacha20-poly1305", keys[s], ivs[s], int(want_seq[i]) & (2 ** 64 - 1), 23,
                          payload[i].tobytes())
        assert wh[i, :wl[i]].tobytes() == w, i
    # two consecutive half batches: the second's numbers continue the first's
    nxt2, wire2, w_len2, seq_out2 = fresh()
    seal(0, n // 2, nxt2, wire2, w_len2, seq_out2)
    mid = nxt2.cpu().numpy()
    assert np.array_equal(mid, (starts + np.bincount(sess[:n // 2][ok[:n // 2]], minlength=nsess)
                                .astype(np.uint64)).view(np.int64))
    seal(n // 2, n, nxt2, wire2, w_len2, seq_out2)
    torch.cuda.synchronize()
    assert torch.equal(seq_out2, seq_out) and torch.equal(nxt2, nxt)
    assert torch.equal(wire2, wire) and torch.equal(w_len2, w_len)


# ---- 5. the key-setup chain on the device ----------------------------------------

@pytest.mark.parametrize("suite,alg,hashlen", [(0x1301, "aes128gcm", 32), (0x1302, "aes256gcm", 48)])
def test_sessions_from_traffic_secrets(torch, tg, suite, alg, hashlen):
    from oracle import keysetup as K
    from oracle import records as R
    nsess, per = 33, 3
    secrets = [bytes(detbytes("sess-secret-%x-%d" % (suite, s), hashlen)) for s in range(nsess)]
    d_sec = torch.from_numpy(np.frombuffer(b"".join(secrets), np.uint8).reshape(nsess, hashlen).copy()).cuda()
    tx = tg.Sessions.from_traffic_secrets(suite, d_sec)
    assert len(tx) == nsess and int(tx.seq().abs().sum()) == 0
    host = [K.traffic_keys(suite, s) for s in secrets]
    rng = np.random.default_rng(suite)
    sessions = [int(x) for x in rng.permutation(np.repeat(np.arange(nsess), per))]
    lens = [int(x) for x in rng.choice([0, 1, 16, 17, 100, 1000, 5000], len(sessions))]
    datas = [rng.bytes(L) for L in lens]
    pads = [int(x) for x in rng.integers(0, 40, len(sessions))]
    b = Batch(torch, "tls13", alg, sessions, [23] * len(sessions), datas, pads)
    wires, seq_out, _ = b.seal(tg, tx.table, tx.ivs, seq_next=tx.seq())
    want_seq, _ = _host_rank(sessions, [0] * nsess)
    assert seq_out.tolist() == want_seq
    for i, s in enumerate(sessions):
        key, iv = host[s]
        assert wires[i] == R.seal_record("tls13", alg, key, iv, want_seq[i], 23, datas[i], pads[i]), i
    assert bool((tx.seq() == per).all())
    # the receiving side: same keys and IVs, counters of its own, through Sessions.open
    rx = tg.Sessions(tx.table, tx.ivs)
    wh = np.zeros(b.wsz, np.uint8)
    for o, w in zip(b.wire_off, wires):
        wh[o:o + len(w)] = np.frombuffer(w, np.uint8)
    out = torch.zeros(b.dsz, dtype=torch.uint8, device="cuda")
    o_len = torch.zeros(b.n, dtype=torch.int32, device="cuda")
    o_ct = torch.zeros(b.n, dtype=torch.uint8, device="cuda")
    st = torch.full((b.n,), 255, dtype=torch.uint8, device="cuda")
    rx.open(b.d_sess, b.n, b.dev(wh), b.w_off, b.dev(np.array([len(w) for w in wires], np.int32)), out,
            b.d_off, o_len, o_ct, st)
    torch.cuda.synchronize()
    oh, ol = out.cpu().numpy(), o_len.cpu().numpy()
    assert not st.any() and bool((o_ct == 23).all())
    for i, d in enumerate(datas):
        assert oh[b.data_off[i]:b.data_off[i] + ol[i]].tobytes() == d, i
    assert bool((rx.seq() == per).all())
    # Sessions.seal is the same call
    tx2 = tg.Sessions(tx.table, tx.ivs)
    wire = torch.zeros(b.wsz, dtype=torch.uint8, device="cuda")
    w_len = torch.zeros(b.n, dtype=torch.int32, device="cuda")
    tx2.seal(b.d_sess, b.n, b.dev(b.host), b.d_off, b.dev(np.array(lens, np.int32)),
             b.dev(np.full(b.n, 23, np.uint8)), wire, b.w_off, w_len, pad_len=b.dev(np.array(pads, np.int32)))
    torch.cuda.synchronize()
    assert np.array_equal(wire.cpu().numpy(), wh) and bool((tx2.seq() == per).all())


# ---- 6. refusals -------------------------------------------------------------------

def test_refusals_launch_nothing(torch, tg):
    z = lambda n, dt=torch.uint8: torch.zeros(n, dtype=dt, device="cuda")  # noqa: E731
    keys = [bytes([k]) * 16 for k in range(4)]
    table = tg.KeyTable("aesgcm", keys)
    nxt = torch.full((4,), 5, dtype=torch.int64, device="cuda")
    wire, w_len = z(256), torch.full((2,), 77, dtype=torch.int32, device="cuda")
    args = lambda: (z(2, torch.int32), 2, z(128), z(2, torch.int64), z(2, torch.int32), z(2),  # noqa: E731
                    wire, z(2, torch.int64), w_len)
    with pytest.raises(tg.TlsGpuError, match="nsessions"):       # three IV rows, four keys
        tg.seal_session_records(table, tg.TLS13, z(36).view(3, 12), *args(), seq_next=nxt)
    with pytest.raises(tg.TlsGpuError, match="fixed IV"):        # TLS 1.2 AES-GCM takes a 4-byte IV
        tg.seal_session_records(table, tg.TLS12, z(48).view(4, 12), *args(), seq_next=nxt)
    with pytest.raises(tg.TlsGpuError, match="both"):
        tg.seal_session_records(table, tg.TLS13, z(48).view(4, 12), *args(), seq_next=nxt,
                                seq=z(2, torch.int64))
    with pytest.raises(tg.TlsGpuError, match="neither"):
        tg.seal_session_records(table, tg.TLS13, z(48).view(4, 12), *args())
    with pytest.raises(tg.TlsGpuError, match="both"):
        tg.open_session_records(table, tg.TLS13, z(48).view(4, 12), z(2, torch.int32), 2, wire,
                                z(2, torch.int64), w_len, z(128), z(2, torch.int64), z(2, torch.int32), z(2),
                                z(2), seq_next=nxt, seq=z(2, torch.int64))
    torch.cuda.synchronize()
    assert not wire.any() and bool((w_len == 77).all()) and bool((nxt == 5).all())
    # the single-connection entry point still refuses a key table
    with pytest.raises(tg.TlsGpuError, match="single-key"):
        tg.seal_records(table, tg.TLS13, bytes(12), 0, 2, z(128), z(2, torch.int64), z(2, torch.int32),
                        z(2), wire, z(2, torch.int64), w_len)
    torch.cuda.synchronize()
    assert not wire.any() and bool((w_len == 77).all())


# ---- 7. the rank pass above 2^20 records ---------------------------------------------

def test_rank_pass_above_two_to_the_twenty(torch, tg):
    """2^20 + 4 099 records: past the size up to which rocPRIM's own radix sort
    would have merge-sorted, so the sort under the rank pass is shown to be the
    same one on both sides of it.  Numbers and counters in full against numpy,
    64 wire records against the oracle."""
    from oracle import records as R
    n, nsess, L, stride = (1 << 20) + 4099, 1000, 8, 32
    big = 3
    rng = np.random.default_rng(1 << 20)
    sess = np.where(rng.random(n) < 0.25, big, rng.integers(0, nsess, n)).astype(np.int64)
    bad_pos = np.array([0, 1 << 19, 1 << 20, n - 1])
    sess[bad_pos] = [nsess, 2 ** 32 - 1, nsess + 7, 2 ** 31]
    ok = sess < nsess
    counts = np.bincount(sess[ok], minlength=nsess)
    assert counts[big] > 1 << 18
    starts = rng.integers(0, 2 ** 62, nsess, dtype=np.uint64)
    starts[big] = 2 ** 32 - 2
    idx = np.flatnonzero(ok)
    order = idx[np.argsort(sess[idx], kind="stable")]
    _, first, cnt = np.unique(sess[order], return_index=True, return_counts=True)
    want_seq = np.zeros(n, np.uint64)
    want_seq[order] = starts[sess[order]] + (np.arange(len(order)) - np.repeat(first, cnt)).astype(np.uint64)
    want_seq = want_seq.view(np.int64).copy()
    want_seq[~ok] = SENTINEL
    keys = [bytes(detbytes("rank2-key-%d" % s, 32)) for s in range(nsess)]
    ivs = [bytes(detbytes("rank2-iv-%d" % s, 12)) for s in range(nsess)]
    g = torch.Generator(device="cuda").manual_seed(11)
    data = torch.randint(0, 256, (n * stride,), dtype=torch.uint8, device="cuda", generator=g)
    payload = data.view(n, stride)[:, :L].cpu().numpy()
    off = torch.arange(n, dtype=torch.int64, device="cuda") * stride
    wire = torch.zeros(n * stride, dtype=torch.uint8, device="cuda")
    w_len = torch.full((n,), 77, dtype=torch.int32, device="cuda")
    seq_out = torch.full((n,), SENTINEL, dtype=torch.int64, device="cuda")
    nxt = torch.from_numpy(starts.view(np.int64).copy()).cuda()
    tg.seal_session_records(tg.KeyTable("chacha20-poly1305", keys), tg.TLS13, _ivs(torch, ivs),
                            torch.from_numpy(_i32(sess)).cuda(), n, data, off,
                            torch.full((n,), L, dtype=torch.int32, device="cuda"),
                            torch.full((n,), 23, dtype=torch.uint8, device="cuda"), wire, off, w_len,
                            seq_next=nxt, seq_out=seq_out)
    torch.cuda.synchronize()
    assert np.array_equal(seq_out.cpu().numpy(), want_seq)
    assert np.array_equal(nxt.cpu().numpy(), (starts + counts.astype(np.uint64)).view(np.int64))
    wl = w_len.cpu().numpy()
    assert np.array_equal(wl, np.where(ok, 5 + L + 1 + 16, 0))
    wh = wire.cpu().numpy().reshape(n, stride)
    assert not wh[~ok].any()
    of_big = np.flatnonzero(sess == big)
    sample = {int(of_big[0]), int(of_big[-1]), 1, n - 2, (1 << 20) - 1, (1 << 20) + 1}
    sample.update(int(q) for q in rng.choice(idx, 64 - len(sample), replace=False))
    for i in sorted(sample):
        s = int(sess[i])
        w = R.seal_record("tls13", "chacha20-poly1305", keys[s], ivs[s], int(want_seq[i]) & (2 ** 64 - 1), 23,
                          payload[i].tobytes())
        assert wh[i, :wl[i]].tobytes() == w, i

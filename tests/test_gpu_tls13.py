"""GPU: the TLS 1.3 key schedule on the device -- tg_hkdf_extract,
tg_hkdf_expand_label_rows, tg_tls13_finished, the fused handshake and
application stages, and Sessions.install_handshake / install_application on
top of them -- against the reference's outputs (tests/golden/tls13_schedule.json).
A batch carries the fixture's row at r % 7 == 0 and variants of it elsewhere,
whose expected outputs come from the host model (tests/tls13_model.py, held to
every fixture row by test_tls13_model.py).  Outputs lie between canaries, and
every comparison is bit-exact.

No test provokes a fault: the one out-of-range slot is a documented skip."""
import functools

import numpy as np
import pytest

import guarded
import tls13_model as m
from vectors import detbytes, load

pytestmark = pytest.mark.gpu

F = load("tls13_schedule.json")
H = bytes.fromhex
CANARY = guarded.CANARY_SEALED
GUARD = 64
VARIANTS = 7   # row r carries the fixture's inputs when r % 7 == 0, else a variant of them
# n: a lone lane, a partial wave, a whole wave, a wave and a lane, a second block of lanes;
# odd: every input and output base pointer one byte past a 256-byte boundary
RUNS = [(1, False), (63, False), (64, False), (65, False), (257, False), (65, True)]
RUN_IDS = ["n%d%s" % (n, "-odd" if odd else "") for n, odd in RUNS]
SUITE_OF = {"sha256": 0x1301, "sha384": 0x1302}
SUITE_NAMES = {0x1301: ("TLS_AES_128_GCM_SHA256", "aes128gcm"), 0x1302: ("TLS_AES_256_GCM_SHA384", "aes256gcm"),
               0x1303: ("TLS_CHACHA20_POLY1305_SHA256", "chacha20-poly1305")}


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


def _rows(torch, rows, odd=False):
    """Byte strings of one length as an n x len device tensor (None if rows is
    None); ``odd``: at an address 1 past a 256-byte boundary."""
    if rows is None:
        return None
    n, w = len(rows), len(rows[0])
    host = torch.from_numpy(np.frombuffer(b"".join(rows), np.uint8).copy().reshape(n, w))
    if not odd:
        return host.cuda()
    flat = torch.zeros(n * w + 1, dtype=torch.uint8, device="cuda")
    assert flat.data_ptr() % 4 == 0
    view = flat[1:].view(n, w)
    view.copy_(host)
    return view


class Out(object):
    """An n x width output between two canary guards."""

    def __init__(self, torch, n, width, odd=False):
        self.n, self.width, self.lead = n, width, GUARD + (1 if odd else 0)
        self.flat = torch.full((self.lead + n * width + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
        self.view = self.flat[self.lead:self.lead + n * width].view(n, width)
        assert self.view.data_ptr() % 4 == (1 if odd else 0)

    def check(self, want, what):
        """The rows equal ``want`` (None: nothing was written) and both guards are whole."""
        host = self.flat.cpu().numpy()
        body = host[self.lead:self.lead + self.n * self.width]
        if want is None:
            assert (body == CANARY).all(), what
        else:
            assert body.tobytes() == b"".join(want), what
        assert (host[:self.lead] == CANARY).all() and (host[self.lead + self.n * self.width:] == CANARY).all(), what


def _var(tag, v, n):
    return bytes(detbytes("k13-var-%s-%d" % (tag, v), n))


# ---- 1. Extract -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _extract_row(ei, v):
    c = F["extract"][ei]
    salt, ikm = m.extract_inputs(c)
    if v == 0:
        return salt, ikm, H(c["out"])
    salt = None if salt is None else _var("ext-salt-%d" % ei, v, len(salt))
    ikm = None if ikm is None else _var("ext-ikm-%d" % ei, v, len(ikm))
    return salt, ikm, m.extract(c["hash"], salt, ikm)


@pytest.mark.parametrize("n,odd", RUNS, ids=RUN_IDS)
def test_extract_matches_every_fixture_row(torch, tg, n, odd):
    for ei, c in enumerate(F["extract"]):
        hl = m.HASHLEN[c["hash"]]
        rows = [_extract_row(ei, r % VARIANTS) for r in range(n)]
        salts = _rows(torch, None if rows[0][0] is None else [r[0] for r in rows], odd)
        ikm = _rows(torch, None if rows[0][1] is None else [r[1] for r in rows], odd)
        out = Out(torch, n, hl, odd)
        assert tg.keysetup.hkdf_extract(salts, ikm, hl, out=out.view) is out.view
        torch.cuda.synchronize()
        out.check([r[2] for r in rows], (ei, c["hash"], c["ikmlen"], c["salt"], c["ikm"]))


def test_extract_null_ikm_takes_either_length(torch, tg):
    """ikm NULL is hashlen zero bytes whether ikmlen says 0 or hashlen."""
    from tlsgpu import _lib
    for alg, hl in m.HASHLEN.items():
        salts = [_var("ext-null-%s" % alg, r, hl) for r in range(5)]
        d = _rows(torch, salts)
        for ikmlen in (0, hl):
            out = Out(torch, 5, hl)
            assert _lib.load().tg_hkdf_extract(hl, d.data_ptr(), None, ikmlen, 5, out.view.data_ptr(), None) == 0
            torch.cuda.synchronize()
            out.check([m.extract(alg, s, None) for s in salts], (alg, ikmlen))


# ---- 2. Expand-Label with a context per row, Derive-Secret ---------------------------
@functools.lru_cache(maxsize=None)
def _expand_row(ei, v):
    c = F["expand"][ei]
    secret, label, ctx = m.expand_inputs(c)
    if v == 0:
        return secret, ctx, H(c["out"])
    secret, ctx = _var("exp-secret-%d" % ei, v, len(secret)), _var("exp-ctx-%d" % ei, v, len(ctx))
    return secret, ctx, m.expand_label(c["hash"], secret, label, ctx, c["outlen"])


@pytest.mark.parametrize("n,odd", RUNS, ids=RUN_IDS)
def test_expand_label_rows_matches_every_fixture_row(torch, tg, n, odd):
    for ei, c in enumerate(F["expand"]):
        hl = m.HASHLEN[c["hash"]]
        label = m.expand_inputs(c)[1]
        rows = [_expand_row(ei, r % VARIANTS) for r in range(n)]
        secrets = _rows(torch, [r[0] for r in rows], odd)
        ctx = _rows(torch, [r[1] for r in rows], odd) if c["ctxlen"] else None
        out = Out(torch, n, c["outlen"], odd)
        tg.keysetup.hkdf_expand_label_rows(secrets, label, ctx, c["outlen"], hl, out=out.view)
        torch.cuda.synchronize()
        out.check([r[2] for r in rows], (ei, c["hash"], c["labellen"], c["ctxlen"], c["outlen"]))


@functools.lru_cache(maxsize=None)
def _derive_row(ei, v):
    c = F["derive"][ei]
    secret, label, digest = m.derive_inputs(c)
    if v == 0:
        return secret, digest, H(c["out"])
    secret = _var("der-secret-%d" % ei, v, len(secret))
    digest = None if digest is None else _var("der-hash-%d" % ei, v, len(digest))
    return secret, digest, m.derive_secret(c["hash"], secret, label, digest)


@pytest.mark.parametrize("n,odd", RUNS, ids=RUN_IDS)
def test_derive_secret_matches_every_fixture_row(torch, tg, n, odd):
    for ei, c in enumerate(F["derive"]):
        hl = m.HASHLEN[c["hash"]]
        rows = [_derive_row(ei, r % VARIANTS) for r in range(n)]
        secrets = _rows(torch, [r[0] for r in rows], odd)
        hashes = _rows(torch, [r[1] for r in rows], odd) if c["transcript"] else None   # None: the empty transcript
        out = Out(torch, n, hl, odd)
        tg.keysetup.derive_secret(secrets, c["label"].encode(), hashes, hl, out=out.view)
        torch.cuda.synchronize()
        out.check([r[2] for r in rows], (ei, c["hash"], c["label"], c["transcript"]))


def test_resumption_master_of_every_connection(torch, tg):
    """ "res master": Derive-Secret of the master secret over the transcript through the client's Finished."""
    for alg, hl in m.HASHLEN.items():
        conns = [c for c in F["schedule"] if c["hash"] == alg]
        got = tg.keysetup.derive_secret(_rows(torch, [H(c["master"]) for c in conns]), b"res master",
                                        _rows(torch, [H(c["resumption_hash"]) for c in conns]), hl)
        torch.cuda.synchronize()
        assert [bytes(r).hex() for r in got.cpu().numpy()] == [c["res_master"] for c in conns], alg


def test_key_and_iv_of_every_traffic_secret(torch, tg):
    """The fixture's "key" and "iv" rows (calcTLS1_3PendingState's cut) from its traffic secrets."""
    for alg, hl in m.HASHLEN.items():
        conns = [c for c in F["schedule"] if c["hash"] == alg]
        rows = [(c, which) for c in conns for which in ("c_hs", "s_hs", "c_ap", "s_ap")]
        secrets = _rows(torch, [H(c[which]) for c, which in rows])
        for name in conns[0]["keys"]:
            keylen = len(conns[0]["keys"][name]["c_hs"]["key"]) // 2
            keys = tg.keysetup.hkdf_expand_label(secrets, b"key", b"", keylen, hl)
            ivs = tg.keysetup.hkdf_expand_label(secrets, b"iv", b"", 12, hl)
            torch.cuda.synchronize()
            assert [bytes(r).hex() for r in keys.cpu().numpy()] == [c["keys"][name][w]["key"] for c, w in rows], name
            assert [bytes(r).hex() for r in ivs.cpu().numpy()] == [c["keys"][name][w]["iv"] for c, w in rows], name


# ---- 3. Finished ---------------------------------------------------------------------
FINISHED = [(c, who) for c in F["schedule"] for who in ("server", "client")]


@functools.lru_cache(maxsize=None)
def _finished_row(ei, v):
    c, who = FINISHED[ei]
    secret = H(c["s_hs"] if who == "server" else c["c_hs"])
    digest = H(c["verify_hash"] if who == "server" else c["finished_hash"])
    if v == 0:
        return secret, digest, H(c[who + "_finished"])
    secret, digest = _var("fin-secret-%d" % ei, v, len(secret)), _var("fin-hash-%d" % ei, v, len(digest))
    return secret, digest, m.finished(c["hash"], secret, digest)


@pytest.mark.parametrize("n,odd", RUNS, ids=RUN_IDS)
def test_finished_matches_every_fixture_row(torch, tg, n, odd):
    for ei, (c, who) in enumerate(FINISHED):
        hl = m.HASHLEN[c["hash"]]
        rows = [_finished_row(ei, r % VARIANTS) for r in range(n)]
        out = Out(torch, n, hl, odd)
        tg.keysetup.tls13_finished(_rows(torch, [r[0] for r in rows], odd), _rows(torch, [r[1] for r in rows], odd),
                                   hl, out=out.view)
        torch.cuda.synchronize()
        out.check([r[2] for r in rows], (c["hash"], c["conn"], who))


# ---- 4. the handshake stage ------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _hs_row(ci, v):
    """(psk or None, shared, hello hash, (hs, client, server)) of variant v of connection ci."""
    c = F["schedule"][ci]
    psk, shared = m.schedule_inputs(c)
    hello = H(c["hello_hash"])
    if v == 0:
        return psk, shared, hello, (H(c["handshake_secret"]), H(c["c_hs"]), H(c["s_hs"]))
    psk = None if psk is None else _var("hs-psk-%d" % ci, v, len(psk))
    shared, hello = _var("hs-shared-%d" % ci, v, len(shared)), _var("hs-hello-%d" % ci, v, len(hello))
    return psk, shared, hello, m.handshake_secrets(c["hash"], psk, shared, hello)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _handshake_call(torch, ci, n, odd, which):
    """tg_tls13_handshake_secrets on n rows with the outputs ``which`` (three
    flags) given and the others NULL; every output buffer checked."""
    from tlsgpu import _lib
    c = F["schedule"][ci]
    hl = m.HASHLEN[c["hash"]]
    rows = [_hs_row(ci, r % VARIANTS) for r in range(n)]
    psk = _rows(torch, [r[0] for r in rows], odd) if c["psk"] else None
    shared, hello = _rows(torch, [r[1] for r in rows], odd), _rows(torch, [r[2] for r in rows], odd)
    before = [t.cpu().numpy().copy() for t in (shared, hello)]
    outs = [Out(torch, n, hl, odd) for _ in range(3)]
    rc = _lib.load().tg_tls13_handshake_secrets(hl, _ptr(psk), shared.data_ptr(), c["sharedlen"], hello.data_ptr(), n,
                                                *([o.view.data_ptr() if w else None for o, w in zip(outs, which)]
                                                  + [None]))
    assert rc == 0, _lib.load().tg_last_error()
    torch.cuda.synchronize()
    for k, (o, w) in enumerate(zip(outs, which)):
        o.check([r[3][k] for r in rows] if w else None, (c["hash"], c["conn"], n, odd, which, k))
    for t, was in zip((shared, hello), before):   # the inputs are only read
        assert np.array_equal(t.cpu().numpy(), was)


@pytest.mark.parametrize("n,odd", RUNS, ids=RUN_IDS)
def test_handshake_stage_matches_every_connection(torch, tg, n, odd):
    for ci in range(len(F["schedule"])):
        _handshake_call(torch, ci, n, odd, (True, True, True))


def test_handshake_stage_null_outputs_are_not_written(torch, tg):
    for ci in (0, 5, 6, 11):   # both hashes, without and with a PSK
        for which in ((True, False, False), (False, True, False), (False, False, True), (True, False, True)):
            _handshake_call(torch, ci, 65, False, which)


def test_handshake_stage_python_call(torch, tg):
    for ci, c in enumerate(F["schedule"]):
        rows = [_hs_row(ci, r % VARIANTS) for r in range(9)]
        got = tg.keysetup.tls13_handshake_secrets(SUITE_OF[c["hash"]], _rows(torch, [r[1] for r in rows]),
                                                  _rows(torch, [r[2] for r in rows]),
                                                  psk=_rows(torch, [r[0] for r in rows]) if c["psk"] else None)
        torch.cuda.synchronize()
        for k in range(3):
            assert got[k].cpu().numpy().tobytes() == b"".join(r[3][k] for r in rows), (ci, k)


# ---- 5. the application stage ------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ap_row(ci, v):
    """(handshake secret, finished hash, (master, client, server, exporter)) of variant v."""
    c = F["schedule"][ci]
    hs, fh = H(c["handshake_secret"]), H(c["finished_hash"])
    if v == 0:
        return hs, fh, (H(c["master"]), H(c["c_ap"]), H(c["s_ap"]), H(c["exp_master"]))
    hs, fh = _var("ap-hs-%d" % ci, v, len(hs)), _var("ap-fh-%d" % ci, v, len(fh))
    return hs, fh, m.application_secrets(c["hash"], hs, fh)


def _application_call(torch, ci, n, odd, which, in_place=False):
    from tlsgpu import _lib
    c = F["schedule"][ci]
    hl = m.HASHLEN[c["hash"]]
    rows = [_ap_row(ci, r % VARIANTS) for r in range(n)]
    fh = _rows(torch, [r[1] for r in rows], odd)
    outs = [Out(torch, n, hl, odd) for _ in range(4)]
    if in_place:   # the handshake secrets live in the master secrets' guarded buffer
        assert which[0]
        outs[0].view.copy_(_rows(torch, [r[0] for r in rows]))
        hs = outs[0].view
    else:
        hs = _rows(torch, [r[0] for r in rows], odd)
    before = [t.cpu().numpy().copy() for t in ((fh,) if in_place else (hs, fh))]
    rc = _lib.load().tg_tls13_application_secrets(hl, hs.data_ptr(), fh.data_ptr(), n,
                                                  *([o.view.data_ptr() if w else None for o, w in zip(outs, which)]
                                                    + [None]))
    assert rc == 0, _lib.load().tg_last_error()
    torch.cuda.synchronize()
    for k, (o, w) in enumerate(zip(outs, which)):
        o.check([r[2][k] for r in rows] if w else None, (c["hash"], c["conn"], n, odd, which, in_place, k))
    for t, was in zip((fh,) if in_place else (hs, fh), before):
        assert np.array_equal(t.cpu().numpy(), was)


@pytest.mark.parametrize("n,odd", RUNS, ids=RUN_IDS)
def test_application_stage_matches_every_connection(torch, tg, n, odd):
    for ci in range(len(F["schedule"])):
        _application_call(torch, ci, n, odd, (True, True, True, True))


def test_application_stage_null_outputs_are_not_written(torch, tg):
    for ci in (0, 6):
        for k in range(4):
            _application_call(torch, ci, 65, False, tuple(j == k for j in range(4)))
        _application_call(torch, ci, 65, False, (False, True, True, False))


@pytest.mark.parametrize("n,odd", [(65, False), (257, True)], ids=["n65", "n257-odd"])
def test_application_stage_in_place(torch, tg, n, odd):
    """master_secret == handshake_secret: the same four outputs as out of place
    (which test_application_stage_matches_every_connection holds to the same rows)."""
    for ci in range(len(F["schedule"])):
        _application_call(torch, ci, n, odd, (True, True, True, True), in_place=True)
    c = F["schedule"][0]
    rows = [_ap_row(0, r % VARIANTS) for r in range(9)]
    hs = _rows(torch, [r[0] for r in rows])
    got = tg.keysetup.tls13_application_secrets(SUITE_OF[c["hash"]], hs, _rows(torch, [r[1] for r in rows]),
                                                in_place=True)
    torch.cuda.synchronize()
    assert got[0] is hs
    for k in range(4):
        assert got[k].cpu().numpy().tobytes() == b"".join(r[2][k] for r in rows), k


# ---- 6. Sessions, end to end ---------------------------------------------------------------
NS = 8
SLOTS = [5, 2]
OUT_OF_RANGE = NS          # a documented skip (tg_sessions_rekey): nothing of it is read or written
START = 100                # the counters before the first install


class Probe(object):
    """One 64-byte record per session of an 8-slot table through Sessions.seal."""

    def __init__(self, torch):
        self.torch = torch
        self.datas = [bytes(detbytes("k13-probe-%d" % i, 64)) for i in range(NS)]
        host = np.zeros(128 * NS, np.uint8)    # room for the inner plaintext's type byte and the tag
        for i, d in enumerate(self.datas):
            host[128 * i:128 * i + 64] = np.frombuffer(d, np.uint8)
        self.host = host
        self.off = guarded.upload(torch, np.arange(NS, dtype=np.uint64) * 128)
        self.session = guarded.upload(torch, np.arange(NS, dtype=np.uint32))
        self.ctype = guarded.upload(torch, np.full(NS, 23, np.uint8))

    def seal(self, s, stream=None):
        """-> (wire, w_len) device tensors; nothing is synchronised."""
        t = self.torch
        data = guarded.upload(t, self.host)
        d_len = guarded.upload(t, np.full(NS, 64, np.uint32))
        wire = t.zeros(128 * NS, dtype=t.uint8, device="cuda")
        w_len = t.full((NS,), -1, dtype=t.int32, device="cuda")
        s.seal(self.session, NS, data, self.off, d_len, self.ctype, wire, self.off, w_len, stream=stream)
        return wire, w_len, data

    def host_wires(self, sealed):
        wire, w_len = sealed[0].cpu().numpy(), sealed[1].cpu().numpy()
        return [wire[128 * i:128 * i + max(int(w_len[i]), 0)].tobytes() for i in range(NS)]


def _old_sessions(torch, tg, suite):
    hl = tg.keysetup.TLS13_SUITES[suite][2]
    old = [bytes(detbytes("k13-old-%x-%d" % (suite, j), hl)) for j in range(NS)]
    s = tg.Sessions.from_traffic_secrets(suite, _rows(torch, old))
    s.seq().copy_(torch.arange(START, START + NS, dtype=torch.int64, device="cuda"))
    return s, old


def _pair(suite, psk):
    """The two fixture connections of the suite's hash that share (psk, sharedlen)."""
    alg = "sha384" if suite == 0x1302 else "sha256"
    conns = [c for c in F["schedule"] if c["hash"] == alg and c["psk"] == psk]
    pair = [c for c in conns if c["sharedlen"] == conns[0]["sharedlen"]][:2]
    assert len(pair) == 2
    return alg, pair


def _stage_inputs(torch, pair, alg):
    """Rows for SLOTS + [OUT_OF_RANGE]: the two connections and a row that no slot takes."""
    hl = m.HASHLEN[alg]
    ins = [m.schedule_inputs(c) for c in pair]
    skip = (_var("skip-psk", 0, hl) if pair[0]["psk"] else None, _var("skip-shared", 0, pair[0]["sharedlen"]))
    psk = _rows(torch, [i[0] for i in ins] + [skip[0]]) if pair[0]["psk"] else None
    shared = _rows(torch, [i[1] for i in ins] + [skip[1]])
    hello = _rows(torch, [H(c["hello_hash"]) for c in pair] + [_var("skip-hello", 0, hl)])
    fh = _rows(torch, [H(c["finished_hash"]) for c in pair] + [_var("skip-fh", 0, hl)])
    return psk, shared, hello, fh


def _expect(old_keys, alg_name, probe, installed, seqs):
    """The oracle's record of every slot: ``installed`` maps a slot to its (key, iv)."""
    from oracle import records as R
    out = []
    for slot in range(NS):
        key, iv = installed.get(slot, old_keys[slot])
        out.append(R.seal_record("tls13", alg_name, key, iv, seqs[slot], 23, probe.datas[slot], 0))
    return out


@pytest.mark.parametrize("psk", [False, True], ids=["nopsk", "psk"])
@pytest.mark.parametrize("side", ["client", "server"])
@pytest.mark.parametrize("suite", [0x1301, 0x1302, 0x1303], ids=["0x1301", "0x1302", "0x1303"])
def test_sessions_install_handshake_then_application(torch, tg, suite, side, psk):
    from oracle import keysetup as K
    name, alg_name = SUITE_NAMES[suite]
    alg, pair = _pair(suite, psk)
    hl = m.HASHLEN[alg]
    s, old = _old_sessions(torch, tg, suite)
    old_keys = [K.traffic_keys(suite, x) for x in old]
    probe = Probe(torch)
    d_psk, shared, hello, fh = _stage_inputs(torch, pair, alg)
    slots = SLOTS + [OUT_OF_RANGE]
    seqs = list(range(START, START + NS))
    tag = "c" if side == "client" else "s"

    def keys_of(stage):
        return dict((slot, (H(c["keys"][name][stage]["key"]), H(c["keys"][name][stage]["iv"])))
                    for slot, c in zip(SLOTS, pair))

    def state_is(stage):
        sec, ivs, ctr = s.secrets.cpu().numpy(), s.ivs.cpu().numpy(), guarded.download(s.seq(), np.uint64).tolist()
        for slot in range(NS):
            if slot in SLOTS:
                c = pair[SLOTS.index(slot)]
                assert sec[slot].tobytes().hex() == c[stage] and ivs[slot].tobytes().hex() == c["keys"][name][stage]["iv"]
            else:
                assert sec[slot].tobytes() == old[slot] and ivs[slot].tobytes() == bytes(old_keys[slot][1])
        assert ctr == seqs, (stage, ctr)

    hs = s.install_handshake(slots, shared, hello, side, psk=d_psk)
    for slot in SLOTS:
        seqs[slot] = 0
    torch.cuda.synchronize()
    assert [bytes(r).hex() for r in hs.cpu().numpy()[:2]] == [c["handshake_secret"] for c in pair]
    state_is(tag + "_hs")
    wires = probe.host_wires(probe.seal(s))
    assert wires == _expect(old_keys, alg_name, probe, keys_of(tag + "_hs"), seqs)
    seqs = [q + 1 for q in seqs]

    master = s.install_application(slots, hs, fh, side)
    for slot in SLOTS:
        seqs[slot] = 0
    torch.cuda.synchronize()
    assert [bytes(r).hex() for r in master.cpu().numpy()[:2]] == [c["master"] for c in pair]
    assert [bytes(r).hex() for r in hs.cpu().numpy()[:2]] == [c["handshake_secret"] for c in pair]   # not in place
    state_is(tag + "_ap")
    wires = probe.host_wires(probe.seal(s))
    assert wires == _expect(old_keys, alg_name, probe, keys_of(tag + "_ap"), seqs)
    assert all(len(w) == 5 + 64 + 1 + 16 for w in wires)
    # what the caller derives later from the returned master secrets
    res = tg.keysetup.derive_secret(master[:2].contiguous(), b"res master",
                                    _rows(torch, [H(c["resumption_hash"]) for c in pair]), hl)
    assert [bytes(r).hex() for r in res.cpu().numpy()] == [c["res_master"] for c in pair]


def test_sessions_stage_calls_need_a_tls13_suite(torch, tg):
    table = tg.KeyTable("aesgcm", [bytes(16)] * 2)
    s = tg.Sessions(table, torch.zeros((2, 12), dtype=torch.uint8, device="cuda"))
    x = torch.zeros((2, 32), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="cipher_suite"):
        s.install_handshake(None, x, x, "client")
    with pytest.raises(ValueError, match="cipher_suite"):
        s.install_application(None, x, x, "server")


# ---- 7. two streams: batch | install | batch, ordered by events ------------------------------
def test_install_is_ordered_against_batches_by_events(torch, tg):
    from oracle import keysetup as K
    suite, side = 0x1302, "server"
    name, alg_name = SUITE_NAMES[suite]
    alg, pair = _pair(suite, False)
    s, old = _old_sessions(torch, tg, suite)
    old_keys = [K.traffic_keys(suite, x) for x in old]
    probe = Probe(torch)
    _, shared, hello, _ = _stage_inputs(torch, pair, alg)
    slots = guarded.upload(torch, np.array(SLOTS + [OUT_OF_RANGE], np.uint32))
    torch.cuda.synchronize()
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    sealed_first, installed = torch.cuda.Event(), torch.cuda.Event()
    with torch.cuda.stream(a):
        first = probe.seal(s, stream=a)
        sealed_first.record(a)
    with torch.cuda.stream(b):
        b.wait_event(sealed_first)
        s.install_handshake(slots, shared, hello, side, stream=b)
        installed.record(b)
    with torch.cuda.stream(a):
        a.wait_event(installed)
        second = probe.seal(s, stream=a)
    a.synchronize()
    b.synchronize()
    seqs = list(range(START, START + NS))
    assert probe.host_wires(first) == _expect(old_keys, alg_name, probe, {}, seqs)
    new = dict((slot, (H(c["keys"][name]["s_hs"]["key"]), H(c["keys"][name]["s_hs"]["iv"])))
               for slot, c in zip(SLOTS, pair))
    seqs = [0 if slot in SLOTS else q + 1 for slot, q in enumerate(seqs)]
    assert probe.host_wires(second) == _expect(old_keys, alg_name, probe, new, seqs)


# ---- 8. binders and ticket PSKs -----------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 65])
def test_binders_match_the_reference(torch, tg, n):
    for ei, c in enumerate(F["binder"]):
        hl = m.HASHLEN[c["hash"]]
        psk, digest = m.binder_inputs(c)
        rows = [(psk, digest, H(c["out"]))]
        for r in range(1, n):
            p, d = _var("bind-psk-%d" % ei, r, len(psk)), _var("bind-hash-%d" % ei, r, hl)
            rows.append((p, d, m.binder(c["hash"], p, d, c["external"])))
        got = tg.keysetup.tls13_binders(_rows(torch, [r[0] for r in rows]), _rows(torch, [r[1] for r in rows]), hl,
                                        c["external"])
        torch.cuda.synchronize()
        assert got.cpu().numpy().tobytes() == b"".join(r[2] for r in rows), (c["hash"], c["psklen"], c["external"])


@pytest.mark.parametrize("n", [1, 65])
def test_resumption_psk_matches_the_reference(torch, tg, n):
    for ei, c in enumerate(F["res_psk"]):
        hl = m.HASHLEN[c["hash"]]
        res_master, nonce = m.res_psk_inputs(c)
        rows = [(res_master, nonce, H(c["out"]))]
        for r in range(1, n):
            rm, nc = _var("res-master-%d" % ei, r, hl), _var("res-nonce-%d" % ei, r, len(nonce))
            rows.append((rm, nc, m.resumption_psk(c["hash"], rm, nc)))
        got = tg.keysetup.tls13_resumption_psk(_rows(torch, [r[0] for r in rows]), _rows(torch, [r[1] for r in rows]),
                                               hl)
        torch.cuda.synchronize()
        assert got.cpu().numpy().tobytes() == b"".join(r[2] for r in rows), (c["hash"], c["noncelen"])

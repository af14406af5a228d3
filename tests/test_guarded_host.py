"""The guarded-batch harness (tests/guarded.py) on the CPU: with the C oracle
standing in for the device its three checks pass, and every planted fault --
a store before or after an extent, a tag left behind the plaintext, a
rejected record zeroed a block long, not fully or not at all, a status entry
past ``n``, a status never written, a changed input, a zero in a gap -- fails
the right check and is attributed to the right record and offset."""
import numpy as np
import pytest

import guarded as G

ALGS = [("aesgcm", 16, 16), ("aesgcm", 32, 16), ("chacha", 32, 16), ("aesccm", 16, 16), ("aesccm8", 32, 8)]


def oracle_device(oracle_mod, alg, keys, tag):
    """A "device" that fills the buffers with the C oracle's results at the
    layout's offsets, rejected records zeroed."""
    def call(op, a):
        r = dict((k, None if v is None else v.copy()) for k, v in a.items())
        inlen = a["lens"] + (tag if op == "open" else 0)
        _, st = oracle_mod.batch(alg, op, keys, a["nonces"], a["aad"], a["aad_off"], a["aad_len"], a["inp"],
                                 a["in_off"], inlen, r["out"].size, a["out_off"], key_idx=a["key_idx"],
                                 out=r["out"])
        if op == "open":
            for i in np.flatnonzero(st == 0):
                o = int(a["out_off"][i])
                r["out"][o:o + int(a["lens"][i])] = 0
            r["status"][:len(st)] = st
        return r
    return call


def _setup(oracle_mod, alg, klen, tag, mode, lens, seed=7, nkeys=1):
    lay = G.GuardedLayout(lens, tag, mode, seed=seed, key_count=nkeys)
    rng = np.random.default_rng(seed + 1)
    keys = np.frombuffer(rng.bytes(klen * nkeys), np.uint8)
    if nkeys > 1:
        keys = keys.reshape(nkeys, klen)
    reject = G.make_reject(lay, seed + 2)
    G.check_reject_coverage(lay, reject)
    return lay, keys, reject, oracle_device(oracle_mod, alg, keys, tag)


@pytest.mark.parametrize("alg,klen,tag", ALGS)
@pytest.mark.parametrize("mode", G.MODES)
def test_oracle_device_passes(oracle_mod, alg, klen, tag, mode):
    lay, keys, reject, dev = _setup(oracle_mod, alg, klen, tag, mode, G.case_lens(3))
    G.run_guarded(None, None, oracle_mod, lay, alg, keys, None, reject, device=dev)


def test_oracle_device_passes_key_table_planned_size(oracle_mod):
    lay, keys, reject, dev = _setup(oracle_mod, "aesgcm", 16, 16, "skewed", G.case_lens(5, G.PLANNED_N), nkeys=7)
    assert lay.n == G.PLANNED_N and set(G.LENS) <= set(int(x) for x in lay.lens)
    G.run_guarded(None, None, oracle_mod, lay, "aesgcm", keys, None, reject, device=dev)


# ---- planted faults --------------------------------------------------------------

SMALL = [0, 1, 15, 16, 17, 31, 32, 33, 47, 63, 64, 65] * 4
SEAL, OPEN, OPEN_BAD = 0, 1, 2


def _planted(oracle_mod, alg, klen, tag, when, plant):
    """Run the three checks with ``plant(result arrays, layout, reject)``
    applied to the results of call number ``when``; -> the error raised."""
    lay, keys, reject, dev = _setup(oracle_mod, alg, klen, tag, "skewed", SMALL)
    calls = []

    def faulty(op, a):
        r = dev(op, a)
        if len(calls) == when:
            plant(r, lay, reject)
        calls.append(op)
        return r

    with pytest.raises(G.ContainmentError) as e:
        G.run_guarded(None, None, oracle_mod, lay, alg, keys, None, reject, device=faulty)
    assert len(calls) == when + 1, "the fault must fail the call it was planted in"
    return e.value, lay, reject


def _pick(lay, pred):
    return next(i for i in range(lay.n) if pred(i))


@pytest.mark.parametrize("alg,klen,tag", ALGS)
def test_byte_before_an_extent(oracle_mod, alg, klen, tag):
    k = 5

    def seal(r, lay, rej):
        r["out"][int(lay.sealed_off[k]) - 1] ^= 0xff

    def open_(r, lay, rej):
        r["out"][int(lay.back_off[k]) - 1] ^= 0xff
    e, lay, _ = _planted(oracle_mod, alg, klen, tag, SEAL, seal)
    assert (e.record, e.rel, e.extent) == (k, -1, int(lay.lens[k]) + tag) and "seal: sealed" in e.what
    assert (e.expected, e.got) == (G.CANARY_SEALED, G.CANARY_SEALED ^ 0xff)
    e, lay, _ = _planted(oracle_mod, alg, klen, tag, OPEN, open_)
    assert (e.record, e.rel, e.extent) == (k, -1, int(lay.lens[k])) and "open: back" in e.what


@pytest.mark.parametrize("alg,klen,tag", ALGS)
def test_byte_after_an_extent(oracle_mod, alg, klen, tag):
    k = 9

    def seal(r, lay, rej):
        r["out"][int(lay.sealed_off[k]) + int(lay.lens[k]) + tag] = 0x11

    def open_(r, lay, rej):
        r["out"][int(lay.back_off[k]) + int(lay.lens[k])] = 0x11
    e, lay, _ = _planted(oracle_mod, alg, klen, tag, SEAL, seal)
    assert (e.record, e.rel, e.extent) == (k, int(lay.lens[k]) + tag, int(lay.lens[k]) + tag)
    e, lay, _ = _planted(oracle_mod, alg, klen, tag, OPEN, open_)
    assert (e.record, e.rel, e.extent) == (k, int(lay.lens[k]), int(lay.lens[k]))
    assert (e.expected, e.got) == (G.CANARY_BACK, 0x11)


@pytest.mark.parametrize("alg,klen,tag", ALGS)
def test_tag_copied_after_the_plaintext_on_open(oracle_mod, alg, klen, tag):
    k = 14

    def plant(r, lay, rej):
        s, o, L = int(lay.sealed_off[k]), int(lay.back_off[k]), int(lay.lens[k])
        assert r["inp"][s + L] != G.CANARY_BACK
        r["out"][o + L:o + L + tag] = r["inp"][s + L:s + L + tag]
    e, lay, _ = _planted(oracle_mod, alg, klen, tag, OPEN, plant)
    assert (e.record, e.rel, e.extent) == (k, int(lay.lens[k]), int(lay.lens[k]))
    assert e.expected == G.CANARY_BACK


def test_rejected_record_zeroed_a_block_long(oracle_mod):
    def plant(r, lay, rej):
        k = _pick(lay, lambda i: i in rej and lay.lens[i] % 16 not in (0, 15))
        o, L = int(lay.back_off[k]), int(lay.lens[k])
        r["out"][o:o + (L + 15) // 16 * 16] = 0
    e, lay, rej = _planted(oracle_mod, "aesgcm", 16, 16, OPEN_BAD, plant)
    k = _pick(lay, lambda i: i in rej and lay.lens[i] % 16 not in (0, 15))
    assert (e.record, e.rel, e.extent) == (k, int(lay.lens[k]), int(lay.lens[k]))
    assert (e.expected, e.got) == (G.CANARY_BACK, 0) and "open tampered" in e.what


def test_rejected_record_left_with_one_plaintext_byte(oracle_mod):
    def plant(r, lay, rej):
        k = _pick(lay, lambda i: i in rej and lay.lens[i] > 20)
        r["out"][int(lay.back_off[k]) + 20] = 0x77
    e, lay, rej = _planted(oracle_mod, "chacha", 32, 16, OPEN_BAD, plant)
    k = _pick(lay, lambda i: i in rej and lay.lens[i] > 20)
    assert (e.record, e.rel, e.expected, e.got) == (k, 20, 0, 0x77)


def test_rejected_record_not_written_at_all(oracle_mod):
    def plant(r, lay, rej):
        k = _pick(lay, lambda i: i in rej and lay.lens[i] > 0)
        o, L = int(lay.back_off[k]), int(lay.lens[k])
        r["out"][o:o + L] = G.CANARY_BACK
    e, lay, rej = _planted(oracle_mod, "aesccm8", 16, 8, OPEN_BAD, plant)
    k = _pick(lay, lambda i: i in rej and lay.lens[i] > 0)
    assert (e.record, e.rel, e.expected, e.got) == (k, 0, 0, G.CANARY_BACK)


@pytest.mark.parametrize("when", [OPEN, OPEN_BAD])
def test_status_past_n_written(oracle_mod, when):
    def plant(r, lay, rej):
        r["status"][lay.n] = 1
    e, lay, _ = _planted(oracle_mod, "aesgcm", 32, 16, when, plant)
    assert "status[%d]" % lay.n in e.what and e.offset == lay.n and e.record is None
    assert (e.expected, e.got) == (G.STATUS_FILL, 1)


@pytest.mark.parametrize("when", [OPEN, OPEN_BAD])
def test_status_never_written(oracle_mod, when):
    k = 11

    def plant(r, lay, rej):
        r["status"][k] = G.STATUS_FILL
    e, lay, rej = _planted(oracle_mod, "aesccm", 32, 16, when, plant)
    assert e.record == k and "status[%d]" % k in e.what
    assert (e.expected, e.got) == (0 if (when == OPEN_BAD and k in rej) else 1, G.STATUS_FILL)


@pytest.mark.parametrize("when,buf", [(SEAL, "in"), (OPEN, "sealed"), (OPEN_BAD, "sealed")])
def test_input_byte_changed(oracle_mod, when, buf):
    k = 7

    def plant(r, lay, rej):
        off = lay.in_off if buf == "in" else lay.sealed_off
        r["inp"][int(off[k]) + 3] ^= 1
    e, lay, _ = _planted(oracle_mod, "aesgcm", 16, 16, when, plant)
    assert (e.record, e.rel) == (k, 3) and "input %s buffer" % buf in e.what


@pytest.mark.parametrize("name", ["aad", "nonces", "lens", "in_off", "out_off", "aad_off", "aad_len"])
def test_read_only_array_changed(oracle_mod, name):
    def plant(r, lay, rej):
        r[name][4] ^= 1
    e, _, _ = _planted(oracle_mod, "chacha", 32, 16, OPEN, plant)
    assert name in e.what and e.offset == 4


@pytest.mark.parametrize("when", [SEAL, OPEN, OPEN_BAD])
def test_zero_byte_in_a_gap(oracle_mod, when):
    k = 21

    def plant(r, lay, rej):
        off, size, _ = lay.extents("sealed" if when == SEAL else "back")
        r["out"][int(off[k] + size[k]) + 20] = 0
    e, lay, _ = _planted(oracle_mod, "aesgcm", 16, 16, when, plant)
    size = int(lay.lens[k]) + (16 if when == SEAL else 0)
    assert (e.record, e.rel, e.extent, e.got) == (k, size + 20, size, 0)


# ---- the layouts ---------------------------------------------------------------------

def test_skewed_leads_cover_the_unequal_cases():
    """In mode ``skewed`` some record has its input aligned and its output
    not, some the reverse, some both misaligned and unequal -- the cases the
    packed batches of the other tests never reach."""
    i_lead, o_lead = G.mode_leads("skewed", len(G.LENS))
    pairs = set(zip(i_lead.tolist(), o_lead.tolist()))
    assert any(a == 0 and b != 0 for a, b in pairs)
    assert any(a != 0 and b == 0 for a, b in pairs)
    assert any(a != 0 and b != 0 and a != b for a, b in pairs)
    lay = G.GuardedLayout(G.LENS, 16, "skewed")
    assert np.array_equal(lay.in_off % 16, i_lead) and np.array_equal(lay.sealed_off % 16, o_lead)
    assert np.array_equal(lay.back_off % 16, i_lead)
    lay = G.GuardedLayout(G.LENS, 16, "in0_out5")
    assert not (lay.in_off % 16).any() and (lay.sealed_off % 16 == 5).all()
    lay = G.GuardedLayout(G.LENS, 8, "aligned")
    assert not (lay.in_off % 16).any() and not (lay.sealed_off % 16).any()


def test_gpu_layouts_stay_inside_their_buffers():
    """No extent of any layout the GPU matrix uses, with a full gap (a block
    and a tag) either side of it, reaches outside its buffer; the canaries
    are in place; every case's tamper set covers every class."""
    import test_gpu_containment as T
    assert len(T.CASES) > 90
    for case in T.CASES:
        for mode in case.modes:
            lay = case.layout(mode)
            lay.check_bounds()
            assert lay.gap == 48 and lay.guard == 256
            assert lay.n == (case.n or len(G.LENS)) and set(G.LENS) <= set(int(x) for x in lay.lens)
            for buf in ("in", "sealed", "back"):
                off, size, total = lay.extents(buf)
                assert off[0] == lay.guard + (lay.in_lead if buf != "sealed" else lay.out_lead)[0]
                assert total - int(off[-1] + size[-1]) == lay.guard
            assert (lay.inp[:lay.guard] == G.CANARY_IN).all() and (lay.inp[-lay.guard:] == G.CANARY_IN).all()
            G.check_reject_coverage(lay, G.make_reject(lay, case.seed(mode) + 3))


# ---- record framing (tests/guarded_records.py) -------------------------------------------

def _records_setup(version, alg, klen, ivlen, seed=11):
    import guarded_records as GR
    rng = np.random.default_rng(seed)
    key, iv = rng.bytes(klen), rng.bytes(ivlen)
    lens, pads, ctypes_, datas = GR.case_records(version, seed + 1)
    recs = [(key, iv, 2 ** 40 + 3 + i) for i in range(len(lens))]
    return GR, recs, lens, pads, ctypes_, datas


@pytest.mark.parametrize("aligned", [True, False])
def test_records_harness_passes_with_the_oracle(oracle_mod, aligned):
    import test_gpu_containment_records as T
    for version, alg, klen, ivlen in T.SUITES:
        GR, recs, lens, pads, ctypes_, datas = _records_setup(version, alg, klen, ivlen)
        assert set(GR.LENS) <= set(lens) and len(lens) == 48
        assert version != "tls13" or set(GR.PADS) <= set(pads)
        GR.run_guarded_records(GR.oracle_records_device(version, alg, recs), version, alg, recs, lens, pads,
                               ctypes_, datas, aligned)


def test_session_records_harness_passes_with_the_oracle(oracle_mod):
    import guarded_records as GR
    import test_gpu_containment_records as T
    for alg, klen in (("aes128gcm", 16), ("chacha20-poly1305", 32)):
        keys, ivs, sessions, recs, extras, want_extras = T.session_case(alg, klen, 5)
        assert sum(r is None for r in recs) == 1 and len(set(sessions)) == 6
        lens, pads, ctypes_, datas = GR.case_records("tls13", 6)

        def after(op, a, r):
            r.update((k, v.copy()) for k, v in want_extras(op).items())
        GR.run_guarded_records(GR.oracle_records_device("tls13", alg, recs, after), "tls13", alg, recs, lens,
                               pads, ctypes_, datas, False, extras=extras, want_extras=want_extras)


def _records_planted(version, alg, klen, ivlen, step, plant):
    GR, recs, lens, pads, ctypes_, datas = _records_setup(version, alg, klen, ivlen)
    dev, calls = GR.oracle_records_device(version, alg, recs), []

    def faulty(op, a):
        r = dev(op, a)
        if len(calls) == step:
            plant(a, r)
        calls.append(op)
        return r

    with pytest.raises(G.ContainmentError) as e:
        GR.run_guarded_records(faulty, version, alg, recs, lens, pads, ctypes_, datas, False)
    assert len(calls) == step + 1
    return e.value, lens, pads


def test_records_planted_faults(oracle_mod):
    k = 9
    # the tag written behind the inner plaintext on open (no room for it in the data extent)
    e, lens, pads = _records_planted("tls13", "aes128gcm", 16, 12, OPEN, lambda a, r: r["data"].__setitem__(
        slice(int(a["data_off"][k]) + lens_of(a, r, k), int(a["data_off"][k]) + lens_of(a, r, k) + 16), 0x33))
    assert (e.record, e.rel, e.extent) == (k, lens[k] + 1 + pads[k], lens[k] + 1 + pads[k])
    assert (e.expected, e.got) == (G.CANARY_BACK, 0x33) and "open: data" in e.what
    # a TLS 1.2 seal that appends a content type to its input
    e, lens, _ = _records_planted("tls12", "aes256gcm", 32, 4, SEAL, lambda a, r: r["data"].__setitem__(
        int(a["data_off"][k]) + int(a["data_len"][k]), 23))
    assert (e.record, e.rel, e.extent) == (k, lens[k], lens[k]) and "seal: data" in e.what
    # a record refused before decryption whose extent is zeroed all the same
    def zero_refused(a, r):
        i = int(np.flatnonzero(r["status"][:48] > 1)[0])
        r["data"][int(a["data_off"][i])] = 0
    e, _, _ = _records_planted("tls13", "chacha20-poly1305", 32, 12, OPEN_BAD, zero_refused)
    assert e.rel == 0 and (e.expected, e.got) == (G.CANARY_BACK, 0) and "open tampered: data" in e.what
    # entries past n of the result arrays
    for name in ("wire_len", "status", "data_len", "ctype"):
        e, _, _ = _records_planted("tls12", "chacha20-poly1305", 32, 12, SEAL if name == "wire_len" else OPEN,
                                   lambda a, r: r[name].__setitem__(48, 0))
        assert name + "[48]" in e.what and e.record is None


def lens_of(a, r, k):
    """Inner plaintext length of record k of an open call (TLS 1.3 AES-GCM)."""
    return int(a["wire_len"][k]) - 5 - 16

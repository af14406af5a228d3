"""GPU: record framing writes nothing outside a record's extents
(tg_seal_records / tg_open_records, tg_seal_session_records /
tg_open_session_records), held the way tests/test_gpu_containment.py holds the
AEAD batch: canary-filled ``data``, ``wire`` and output buffers with data
extents of exactly ``L + 1 + pad`` (TLS 1.3) or ``L`` (TLS 1.2) bytes, whole
buffers and whole result arrays compared with the framing oracle's image
(tests/guarded_records.py)."""
import zlib

import numpy as np
import pytest

import guarded as G
import guarded_records as GR
from test_gpu_session_records import _host_rank, _table_alg

pytestmark = pytest.mark.gpu

SUITES = [("tls13", "aes128gcm", 16, 12), ("tls13", "chacha20-poly1305", 32, 12),
          ("tls13", "aes128ccm_8", 16, 12), ("tls12", "aes256gcm", 32, 4),
          ("tls12", "chacha20-poly1305", 32, 12)]
SEQ_FILL = 0x0123456789abcdef


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


def _single_key(tg, alg, key):
    if alg.startswith("chacha"):
        return tg.HipCHACHA20_POLY1305(bytearray(key))
    if "ccm" in alg:
        return tg.HipAESCCM(bytearray(key), tag_length=8 if alg.endswith("_8") else 16)
    return tg.HipAESGCM(bytearray(key))


def _device(torch, tg, version, run):
    """call(op, arrays): upload, ``run(op, version code, n, device arrays)``, download."""
    def call(op, a):
        d = dict((k, G.upload(torch, v)) for k, v in a.items() if v is not None)
        assert d["data"].data_ptr() % 16 == 0 and d["wire"].data_ptr() % 16 == 0
        run(op, tg.TLS13 if version == "tls13" else tg.TLS12, len(a["data_off"]), d)
        torch.cuda.synchronize()
        return dict((k, G.download(t, a[k].dtype).reshape(a[k].shape)) for k, t in d.items())
    return call


@pytest.mark.parametrize("version,alg,klen,ivlen", SUITES)
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "packed"])
def test_records_write_only_their_extents(torch, tg, version, alg, klen, ivlen, aligned):
    seed = zlib.crc32(("%s/%s/%d" % (version, alg, aligned)).encode())
    rng = np.random.default_rng(seed)
    key, iv, seq0 = rng.bytes(klen), rng.bytes(ivlen), 2 ** 40 + 3
    lens, pads, ctypes_, datas = GR.case_records(version, seed + 1)
    recs = [(key, iv, seq0 + i) for i in range(len(lens))]
    k = _single_key(tg, alg, key)

    def run(op, v, n, d):
        if op == "seal":
            tg.seal_records(k, v, iv, seq0, n, d["data"], d["data_off"], d["data_len"], d["ctype"], d["wire"],
                            d["wire_off"], d["wire_len"], pad_len=d.get("pad_len"))
        else:
            tg.open_records(k, v, iv, seq0, n, d["wire"], d["wire_off"], d["wire_len"], d["data"],
                            d["data_off"], d["data_len"], d["ctype"], d["status"])

    GR.run_guarded_records(_device(torch, tg, version, run), version, alg, recs, lens, pads, ctypes_, datas,
                           aligned)


def session_case(alg, klen, seed, nsess=5):
    """A counter-mode batch of ``nsess`` sessions with one record whose
    session is out of range: (keys, ivs, sessions, starts, per-record
    (key, iv, seq) or None, extras, want_extras) for run_guarded_records."""
    rng = np.random.default_rng(seed)
    keys = [rng.bytes(klen) for _ in range(nsess)]
    ivs = [rng.bytes(12) for _ in range(nsess)]
    sessions = [int(x) for x in rng.integers(0, nsess, GR.N)]
    sessions[17] = nsess + 2
    starts = [3, 2 ** 32 - 5, 2 ** 40 + 3, 0, 2 ** 63 + 11][:nsess]
    seq, nxt = _host_rank(sessions, starts)
    recs = [None if q is None else (keys[s], ivs[s], q) for s, q in zip(sessions, seq)]
    seq_out = np.full(GR.N + GR.SLACK, SEQ_FILL, np.uint64)
    for i, q in enumerate(seq):
        if q is not None:
            seq_out[i] = q

    def extras(op):
        return {"iv_table": np.frombuffer(b"".join(ivs), np.uint8).reshape(nsess, 12).copy(),
                "session": np.array(sessions, np.uint32), "seq_next": np.array(starts, np.uint64),
                "seq_out": np.full(GR.N + GR.SLACK, SEQ_FILL, np.uint64)}

    def want_extras(op):
        return {"seq_next": np.array(nxt, np.uint64), "seq_out": seq_out}

    return keys, ivs, sessions, recs, extras, want_extras


@pytest.mark.parametrize("alg,klen", [("aes128gcm", 16), ("chacha20-poly1305", 32)])
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "packed"])
def test_session_records_write_only_their_extents(torch, tg, alg, klen, aligned):
    seed = zlib.crc32(("sessions/%s/%d" % (alg, aligned)).encode())
    keys, ivs, sessions, recs, extras, want_extras = session_case(alg, klen, seed)
    lens, pads, ctypes_, datas = GR.case_records("tls13", seed + 1)
    table = tg.KeyTable(_table_alg(alg), keys)

    def run(op, v, n, d):
        if op == "seal":
            tg.seal_session_records(table, v, d["iv_table"], d["session"], n, d["data"], d["data_off"],
                                    d["data_len"], d["ctype"], d["wire"], d["wire_off"], d["wire_len"],
                                    seq_next=d["seq_next"], seq_out=d["seq_out"], pad_len=d["pad_len"])
        else:
            tg.open_session_records(table, v, d["iv_table"], d["session"], n, d["wire"], d["wire_off"],
                                    d["wire_len"], d["data"], d["data_off"], d["data_len"], d["ctype"],
                                    d["status"], seq_next=d["seq_next"], seq_out=d["seq_out"])

    GR.run_guarded_records(_device(torch, tg, "tls13", run), "tls13", alg, recs, lens, pads, ctypes_, datas,
                           aligned, extras=extras, want_extras=want_extras)

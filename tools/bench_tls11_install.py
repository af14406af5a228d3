#!/usr/bin/env python3
"""Cost of giving many TLS 1.1 CBC sessions their keys: on the device against
the host route, and against the TLS 1.2 install of the same table shape.

65 536 AES-256-CBC-SHA sessions (TLS_RSA_WITH_AES_256_CBC_SHA), all slots of a
live table:

  (a) device  CbcSessions.install at TLS 1.1 -- tg_cbc_sessions_install_tls11:
              template pack kernel + fused MD5 xor SHA-1 PRF / key schedules /
              midstates kernel.  Timed with device events on one stream after a
              warm-up; the host time the call takes to return is recorded
              beside it.
  (b) host    the only way before: the key block by hashlib / hmac on the host
              (P_MD5 xor P_SHA1, what calcPendingStates does per connection),
              then tg_cbc_key_replace (rows built on the host, copied through
              pinned staging, the call blocks).  Wall-clock time, the two parts
              apart.
  (c) tls12   the same suite id installed at TLS 1.2 -- the SHA-256 PRF of
              tg_cbc_sessions_install_tls12, the closest existing kernel: one
              SHA-256 chain where (a) runs an MD5 and a SHA-1 chain in a lane.
              Timed like (a), alternating with it step by step.

Verified afterwards: the tables filled by (a) and (b) seal a sample batch to
the same bytes.  Prints one JSON line; --out writes it.

    python tools/bench_tls11_install.py --out profiles/r14/tls11_install/bench.json
"""
import argparse
import hashlib
import hmac
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tlslite-ng_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

SUITE = 0x0035


def p_hash(digestmod, secret, seed, length):
    out, a = b"", seed
    while len(out) < length:
        a = hmac.new(secret, a, digestmod).digest()
        out += hmac.new(secret, a + seed, digestmod).digest()
    return out[:length]


def prf(secret, seed, length):
    a = p_hash(hashlib.md5, secret[:24], seed, length)
    b = p_hash(hashlib.sha1, secret[24:], seed, length)
    return bytes(x ^ y for x, y in zip(a, b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-steps", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import tlsgpu
    if not torch.cuda.is_available():
        sys.exit("bench_tls11_install.py needs a GPU")
    torch.cuda.set_device(0)
    n = args.sessions
    stream = torch.cuda.current_stream()
    g = torch.Generator(device="cuda").manual_seed(0x1102)
    ms = torch.randint(0, 256, (n, 48), dtype=torch.uint8, device="cuda", generator=g)
    cr = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device="cuda", generator=g)
    sr = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device="cuda", generator=g)
    dev = tlsgpu.CbcSessions.from_master_secrets(SUITE, ms, cr, sr, "client", version=tlsgpu.TLS11)
    dev12 = tlsgpu.CbcSessions.from_master_secrets(SUITE, ms, cr, sr, "client", version=tlsgpu.TLS12)
    for _ in range(args.warmup):
        dev.install(None, ms, cr, sr, "client", stream=stream)
        dev12.install(None, ms, cr, sr, "client", stream=stream)
    torch.cuda.synchronize()
    events = {"tls11": [], "tls12": []}
    host_call = {"tls11": [], "tls12": []}
    for _ in range(args.steps):   # (a) and (c) alternate
        for name, obj in (("tls11", dev), ("tls12", dev12)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            t0 = time.perf_counter()
            obj.install(None, ms, cr, sr, "client", stream=stream)
            host_call[name].append((time.perf_counter() - t0) * 1e3)
            e1.record(stream)
            events[name].append((e0, e1))
    torch.cuda.synchronize()

    def stats(t):
        t = sorted(t)
        return {"ms": round(sum(t) / len(t), 4), "ms_median": round(t[len(t) // 2], 4),
                "ms_min": round(t[0], 4), "ms_max": round(t[-1], 4)}

    # the host route: secrets as a server holds them (host bytes), keys by hashlib, rows by tg_cbc_key_replace
    h_ms, h_cr, h_sr = (t.cpu().numpy() for t in (ms, cr, sr))
    host = tlsgpu.CbcKey.table([bytes(32)] * n, [bytes(20)] * n, "sha1")
    prf_ms, replace_ms = [], []
    for _ in range(args.host_steps):
        t0 = time.perf_counter()
        enc, mk = [], []
        for j in range(n):
            block = prf(h_ms[j].tobytes(), b"key expansion" + h_sr[j].tobytes() + h_cr[j].tobytes(), 104)
            mk.append(block[0:20])
            enc.append(block[40:72])
        t1 = time.perf_counter()
        host.replace(None, enc, mk, stream=stream)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        prf_ms.append((t1 - t0) * 1e3)
        replace_ms.append((t2 - t1) * 1e3)

    # both tables seal a sample batch to the same bytes
    m, L = 4096, 100
    rng = np.random.default_rng(0x1103)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    sess = d(rng.integers(0, n, m).astype(np.int32))
    seq = d(rng.integers(0, 2 ** 40, m).astype(np.int64))
    data = torch.randint(0, 256, (m * 128,), dtype=torch.uint8, device="cuda", generator=g)
    iv = torch.randint(0, 256, (m * 16,), dtype=torch.uint8, device="cuda", generator=g)
    d_off, w_off = d(np.arange(m, dtype=np.int64) * 128), d(np.arange(m, dtype=np.int64) * 256 + 11)
    d_len = torch.full((m,), L, dtype=torch.int32, device="cuda")
    ctype = torch.full((m,), 23, dtype=torch.uint8, device="cuda")
    outs = []
    for table in (dev.table, host):
        wire = torch.zeros(m * 256 + 16, dtype=torch.uint8, device="cuda")
        w_len = torch.zeros(m, dtype=torch.int32, device="cuda")
        tlsgpu.cbc.seal_session_records(table, tlsgpu.TLS11, 0, sess, m, data, d_off, d_len, ctype, iv, wire, w_off,
                                        w_len, seq=seq)
        outs.append(wire)
    torch.cuda.synchronize()
    ok = bool(torch.equal(outs[0], outs[1])) and bool(outs[0].any())
    t11 = [a.elapsed_time(b) for a, b in events["tls11"]]
    t12 = [a.elapsed_time(b) for a, b in events["tls12"]]
    device_ms, tls12_ms = stats(t11), stats(t12)
    host_total = [a + b for a, b in zip(prf_ms, replace_ms)]
    line = {"metric": "ms to install %d AES-256-CBC-SHA TLS 1.1 sessions: tg_cbc_sessions_install_tls11 vs "
                      "hashlib PRF + tg_cbc_key_replace, and vs the TLS 1.2 install of the same table" % n,
            "unit": "ms", "sessions": n, "steps": args.steps, "warmup": args.warmup, "host_steps": args.host_steps,
            "device": torch.cuda.get_device_name(0),
            "device_install": {"device": device_ms, "host_call": stats(host_call["tls11"])},
            "tls12_install": {"device": tls12_ms, "host_call": stats(host_call["tls12"])},
            "tls11_over_tls12": round(device_ms["ms_median"] / tls12_ms["ms_median"], 3),
            "host_route": {"total": stats(host_total), "hashlib_prf": stats(prf_ms),
                           "tg_cbc_key_replace": stats(replace_ms)},
            "host_over_device": round(stats(host_total)["ms"] / device_ms["ms"], 1), "verified": ok}
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    dev.table.close()
    dev12.table.close()
    host.close()
    if not ok:
        sys.exit(3)


if __name__ == "__main__":
    main()

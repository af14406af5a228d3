#!/usr/bin/env python3
"""Cost of running the TLS 1.3 key schedule for many sessions: on the device
against the host route.

65 536 sessions of TLS_AES_256_GCM_SHA384 (0x1302, SHA-384), 48-byte (EC)DHE
shared secrets, no PSK, the server's write keys, all slots of a live table:

  (a) device  timed with device events on one stream after a warm-up:
              handshake    keysetup.tls13_handshake_secrets (one fused kernel)
              application  keysetup.tls13_application_secrets (one fused kernel)
              installs     Sessions.install_handshake followed by
                           Sessions.install_application (each: the stage kernel,
                           then tg_sessions_rekey)
              The host time the calls take to return is recorded beside them.
  (b) host    the only way before: the same chain per session by hashlib / hmac
              (what tlsconnection.py does per connection), the traffic secrets
              uploaded and installed with Sessions.install, after each stage.
              Wall-clock time, the two parts apart.

Verified afterwards: Sessions filled by (a) and by (b) seal a 4 096-record
sample to the same bytes.  Prints one JSON line; --out writes it.

    python tools/bench_tls13_schedule.py --out profiles/r15/tls13_schedule/bench.json
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

SUITE, HL = 0x1302, 48
EMPTY = hashlib.sha384(b"").digest()


def hm(key, msg):
    return hmac.new(key, msg, hashlib.sha384).digest()


def derive(secret, label, transcript_hash):
    full = b"tls13 " + label
    return hm(secret, HL.to_bytes(2, "big") + bytes([len(full)]) + full + bytes([HL]) + transcript_hash + b"\x01")


def host_chain(shared, hello, fhash):
    """(server hs traffic, server ap traffic) of one session, tlsconnection.py:3036-3050, :3218-3224."""
    early = hm(bytes(HL), bytes(HL))
    hs = hm(derive(early, b"derived", EMPTY), shared)
    s_hs = derive(hs, b"s hs traffic", hello)
    derive(hs, b"c hs traffic", hello)
    master = hm(derive(hs, b"derived", EMPTY), bytes(HL))
    s_ap = derive(master, b"s ap traffic", fhash)
    derive(master, b"c ap traffic", fhash)
    derive(master, b"exp master", fhash)
    return s_hs, s_ap


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-steps", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import tlsgpu
    from tlsgpu import keysetup
    if not torch.cuda.is_available():
        sys.exit("bench_tls13_schedule.py needs a GPU")
    torch.cuda.set_device(0)
    n = args.sessions
    stream = torch.cuda.current_stream()
    g = torch.Generator(device="cuda").manual_seed(0x1302)
    rnd = lambda w: torch.randint(0, 256, (n, w), dtype=torch.uint8, device="cuda", generator=g)  # noqa: E731
    shared, hello, fhash, blank = rnd(48), rnd(HL), rnd(HL), rnd(HL)
    dev = tlsgpu.Sessions.from_traffic_secrets(SUITE, blank)
    host = tlsgpu.Sessions.from_traffic_secrets(SUITE, blank)

    def handshake():
        return keysetup.tls13_handshake_secrets(SUITE, shared, hello, stream=stream)

    hs0 = handshake()[0]

    def application():
        return keysetup.tls13_application_secrets(SUITE, hs0, fhash, stream=stream)

    def installs():
        hs = dev.install_handshake(None, shared, hello, "server", stream=stream)
        return dev.install_application(None, hs, fhash, "server", stream=stream)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        events, calls = [], []
        for _ in range(args.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            t0 = time.perf_counter()
            fn()
            calls.append((time.perf_counter() - t0) * 1e3)
            e1.record(stream)
            events.append((e0, e1))
        torch.cuda.synchronize()
        return {"device": stats([a.elapsed_time(b) for a, b in events]), "host_call": stats(calls)}

    def stats(t):
        t = sorted(t)
        return {"ms": round(sum(t) / len(t), 4), "ms_median": round(t[len(t) // 2], 4),
                "ms_min": round(t[0], 4), "ms_max": round(t[-1], 4)}

    device = {"handshake_stage": timed(handshake), "application_stage": timed(application),
              "install_handshake_then_application": timed(installs)}

    # the host route: inputs as a server holds them (host bytes), the chain by hashlib, Sessions.install twice
    h_shared, h_hello, h_fhash = (t.cpu().numpy() for t in (shared, hello, fhash))
    chain_ms, install_ms = [], []
    for _ in range(args.host_steps):
        t0 = time.perf_counter()
        s_hs, s_ap = [], []
        for j in range(n):
            a, b = host_chain(h_shared[j].tobytes(), h_hello[j].tobytes(), h_fhash[j].tobytes())
            s_hs.append(a)
            s_ap.append(b)
        t1 = time.perf_counter()
        for rows in (s_hs, s_ap):
            up = torch.from_numpy(np.frombuffer(b"".join(rows), np.uint8).reshape(n, HL).copy()).cuda()
            host.install(None, up, stream=stream)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        chain_ms.append((t1 - t0) * 1e3)
        install_ms.append((t2 - t1) * 1e3)

    # both seal a sample of records to the same bytes
    m, L = 4096, 100
    rng = np.random.default_rng(0x1303)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    sess = d(rng.permutation(n)[:m].astype(np.int32))
    data = torch.randint(0, 256, (m * 128,), dtype=torch.uint8, device="cuda", generator=g)
    off = d(np.arange(m, dtype=np.int64) * 128)
    ctype = torch.full((m,), 23, dtype=torch.uint8, device="cuda")
    outs = []
    for s in (dev, host):
        wire = torch.zeros(m * 128, dtype=torch.uint8, device="cuda")
        w_len = torch.zeros(m, dtype=torch.int32, device="cuda")
        d_len = torch.full((m,), L, dtype=torch.int32, device="cuda")
        s.seal(sess, m, data.clone(), off, d_len, ctype, wire, off, w_len)
        outs.append((wire, w_len))
    torch.cuda.synchronize()
    ok = (bool(torch.equal(outs[0][0], outs[1][0])) and bool(torch.equal(outs[0][1], outs[1][1]))
          and bool((outs[0][1] == 5 + L + 1 + 16).all()) and bool(torch.equal(dev.secrets, host.secrets)))
    host_total = [a + b for a, b in zip(chain_ms, install_ms)]
    line = {"metric": "ms for the TLS 1.3 key schedule of %d TLS_AES_256_GCM_SHA384 sessions: device stages and "
                      "installs vs hashlib chain + Sessions.install" % n,
            "unit": "ms", "sessions": n, "steps": args.steps, "warmup": args.warmup, "host_steps": args.host_steps,
            "device": torch.cuda.get_device_name(0), "device_route": device,
            "host_route": {"total": stats(host_total), "hashlib_chain": stats(chain_ms),
                           "upload_and_install_x2": stats(install_ms)},
            "verified": ok}
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    if not ok:
        sys.exit(3)


if __name__ == "__main__":
    main()

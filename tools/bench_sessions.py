#!/usr/bin/env python3
"""Cost of framing many sessions' records in one call, on config 4's workload.

BASELINE configs[3] as bench.py --config c4 generates it: AES-256-GCM, 65 536
session keys (PCG64 0x7716), --records records (default 2^20) with Zipf(1.2)
lengths 64 B-16 KiB (PCG64 0x7717), TLS 1.2 framing.  Three ways to seal and
open the same payloads, timed with device events around each call, warm-up
first, the variants alternating inside every step:

  (a) raw      tg_seal_batch / tg_open_batch on the key table, nonces and AAD
               prebuilt by the host -- what a caller had before the
               many-session framing, and the yardstick;
  (b) explicit tg_seal_session_records / tg_open_session_records with a
               per-record sequence number array;
  (c) counter  the same calls with per-session counters (the rank pass).

(b) and (c) also write the 5-byte header and the 8-byte explicit nonce of
every record and parse them back, which (a) leaves to the caller.  Every
variant is verified (all records open back to their payload; sampled wire
records against the C oracle; counter mode's numbers against a stable rank
computed with numpy).  Prints one JSON line; --out writes it to a file.

    python tools/bench_sessions.py --steps 10 --warmup 3 --out profiles/r07/sessions/bench_sessions.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tlslite-ng_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

# The single-connection framing beside its raw AEAD, from committed numbers of
# one run directory: config 5 (tg_seal_records, TLS 1.3 AES-128-GCM, 2^20 x
# 16 KiB) against the headline's AES-128-GCM seal.
CONTEXT = {"config5_seal_GiBps": 1299.17, "headline_aes128gcm_seal_GiBps": 1349.9,
           "ratio": round(1299.17 / 1349.9, 4),
           "source": "profiles/r06/fin/bench_c5.json, profiles/r06/fin/bench.json"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--variants", default="raw,explicit,counter",
                    help="comma-separated subset to run (a profiler run of one variant attributes "
                         "every kernel to it); ratios need raw")
    args = ap.parse_args()
    import numpy as np
    import torch
    import tlsgpu
    from oracle import oracle as O
    if not torch.cuda.is_available():
        sys.exit("bench_sessions.py needs a GPU")
    torch.cuda.set_device(0)
    n, nkeys = args.records, 65536
    variants = [v for v in ("raw", "explicit", "counter") if v in args.variants.split(",")]
    rk = np.random.default_rng(0x7716)
    keys = rk.integers(0, 256, (nkeys, 32), dtype=np.uint8)
    key_idx = rk.integers(0, nkeys, n).astype(np.uint32)
    rl = np.random.default_rng(0x7717)
    lens = np.clip(64 * rl.zipf(1.2, n), 64, 16384).astype(np.int64)
    ivs = np.random.default_rng(0x7718).integers(0, 256, (nkeys, 4), dtype=np.uint8)
    seq = np.arange(n, dtype=np.uint64)          # explicit mode and (a): record i has number i
    in_sz = (lens + 15) // 16 * 16
    in_off = np.concatenate([[0], np.cumsum(in_sz)[:-1]]).astype(np.int64)
    # wire record = 5-byte header || 8-byte explicit nonce || ct || tag, placed
    # so that the ciphertext starts 16-byte aligned; (a) writes ct || tag to
    # the same place and leaves the 13 bytes in front alone
    w_sz = 16 + (lens + 16 + 15) // 16 * 16
    ct_off = np.concatenate([[0], np.cumsum(w_sz)[:-1]]).astype(np.int64) + 16
    wire_off = ct_off - 13
    aad = np.zeros((n, 13), dtype=np.uint8)
    aad[:, :8] = seq[:, None].view(np.uint8).reshape(n, 8)[:, ::-1]
    aad[:, 8], aad[:, 9], aad[:, 10] = 0x17, 3, 3
    aad[:, 11], aad[:, 12] = lens >> 8, lens & 0xff
    nonce = np.zeros((n, 12), dtype=np.uint8)
    nonce[:, :4] = ivs[key_idx]
    nonce[:, 4:] = aad[:, :8]
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    g = torch.Generator(device="cuda").manual_seed(0x7717)
    inp = torch.randint(0, 256, (int(in_sz.sum()),), dtype=torch.uint8, device="cuda", generator=g)
    wire = torch.zeros(int(w_sz.sum()), dtype=torch.uint8, device="cuda")
    back = torch.empty_like(inp)
    status = torch.zeros(n, dtype=torch.uint8, device="cuda")
    d_lens, d_in_off = d(lens.astype(np.int32)), d(in_off)
    d_ct_off, d_wire_off = d(ct_off), d(wire_off)
    d_aad, d_nonce, d_kidx = d(aad.reshape(-1)), d(nonce.reshape(-1)), d(key_idx.view(np.int32))
    d_ivs, d_seq = d(ivs), d(seq.view(np.int64))
    ctype = torch.full((n,), 0x17, dtype=torch.uint8, device="cuda")
    w_len = torch.zeros(n, dtype=torch.int32, device="cuda")
    o_len = torch.zeros(n, dtype=torch.int32, device="cuda")
    o_ct = torch.zeros(n, dtype=torch.uint8, device="cuda")
    seq_out = torch.zeros(n, dtype=torch.int64, device="cuda")
    tx_next = torch.zeros(nkeys, dtype=torch.int64, device="cuda")
    rx_next = torch.zeros(nkeys, dtype=torch.int64, device="cuda")
    table = tlsgpu.KeyTable("aesgcm", [bytes(k) for k in keys])
    sb = tlsgpu.make_batch(n, inp, wire, d_nonce, aad=d_aad, lens=d_lens, in_off=d_in_off,
                           out_off=d_ct_off, aad_stride=13, fixed_aad_len=13, key_idx=d_kidx)
    ob = tlsgpu.make_batch(n, wire, back, d_nonce, aad=d_aad, lens=d_lens, in_off=d_ct_off,
                           out_off=d_in_off, aad_stride=13, fixed_aad_len=13, key_idx=d_kidx,
                           status=status)
    stream = torch.cuda.current_stream()

    def seal_s(**kw):
        tlsgpu.seal_session_records(table, tlsgpu.TLS12, d_ivs, d_kidx, n, inp, d_in_off, d_lens, ctype,
                                    wire, d_wire_off, w_len, stream=stream, **kw)

    def open_s(**kw):
        tlsgpu.open_session_records(table, tlsgpu.TLS12, d_ivs, d_kidx, n, wire, d_wire_off, w_len, back,
                                    d_in_off, o_len, o_ct, status, stream=stream, **kw)

    ops = [("raw_seal", lambda: tlsgpu.seal_batch(table, sb, stream)),
           ("raw_open", lambda: tlsgpu.open_batch(table, ob, stream)),
           ("explicit_seal", lambda: seal_s(seq=d_seq)),
           ("explicit_open", lambda: open_s(seq=d_seq)),
           ("counter_seal", lambda: seal_s(seq_next=tx_next)),
           ("counter_open", lambda: open_s(seq_next=rx_next))]
    run = [(name, fn) for name, fn in ops if name.split("_")[0] in variants]

    # ---- verification (untimed; also the first warm-up of every path) ----
    pick = sorted(set(list(range(0, n, max(1, n // 62)))[:62] + [n - 1]))
    h_lens32 = d_lens

    def sample_mismatches(seq_of, framed):
        wh = wire
        bad = 0
        for i in pick:
            L = int(lens[i])
            pt = inp[int(in_off[i]):int(in_off[i]) + L].cpu().numpy().tobytes()
            q = int(seq_of[i])
            a = q.to_bytes(8, "big") + bytes([0x17, 3, 3, L >> 8, L & 0xff])
            body = bytes(O.gcm_seal(bytes(keys[key_idx[i]]), bytes(ivs[key_idx[i]]) + q.to_bytes(8, "big"), pt, a))
            lo = int(wire_off[i]) if framed else int(ct_off[i])
            want = (bytes([0x17, 3, 3, (L + 24) >> 8, (L + 24) & 0xff]) + q.to_bytes(8, "big") + body) \
                if framed else body
            bad += int(wh[lo:lo + len(want)].cpu().numpy().tobytes() != want)
        return bad

    def opened_ok(framed):
        ok = torch.equal(back, inp)
        if framed:
            return ok and not bool(status.any()) and torch.equal(o_len, h_lens32) and bool((o_ct == 0x17).all())
        return ok and int(status.sum().item()) == n

    verified = {}
    for name, framed, seal, open_, seq_of in (
            ("raw", False, ops[0][1], ops[1][1], lambda: seq),
            ("explicit", True, ops[2][1], ops[3][1], lambda: seq),
            ("counter", True, lambda: seal_s(seq_next=tx_next, seq_out=seq_out), ops[5][1],
             lambda: seq_out.cpu().numpy().view(np.uint64))):
        if name not in variants:
            continue
        wire.zero_()
        back.zero_()
        status.fill_(255 if framed else 0)
        seal()
        torch.cuda.synchronize()
        mism = sample_mismatches(seq_of(), framed)
        open_()
        torch.cuda.synchronize()
        verified[name] = {"oracle_checked_records": len(pick), "oracle_mismatches": mism,
                          "all_records_open": bool(opened_ok(framed))}
    # counter mode from zeroed counters: numpy's stable per-session rank
    order = np.argsort(key_idx, kind="stable")
    _, first, cnt = np.unique(key_idx[order], return_index=True, return_counts=True)
    rank = np.empty(n, np.int64)
    rank[order] = np.arange(n) - np.repeat(first, cnt)
    counts = np.bincount(key_idx, minlength=nkeys)
    if "counter" in variants:
        verified["counter"]["seq_equals_stable_rank"] = bool(
            np.array_equal(seq_out.cpu().numpy(), rank) and np.array_equal(tx_next.cpu().numpy(), counts)
            and np.array_equal(rx_next.cpu().numpy(), counts))

    for _ in range(args.warmup):
        for _, fn in run:
            fn()
    ms = {name: [] for name, _ in run}
    for _ in range(args.steps):
        for name, fn in run:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            ms[name].append((e0, e1))
    torch.cuda.synchronize()
    if "counter" in variants:   # the last timed pair was counter mode: its round trip still holds
        verified["counter"]["all_records_open_after_timing"] = bool(opened_ok(True))
        verified["counter"]["counters_after_timing"] = bool(
            torch.equal(tx_next, rx_next) and
            np.array_equal(tx_next.cpu().numpy(), counts * (1 + args.warmup + args.steps)))
    payload = float(lens.sum())
    res = {}
    for name, lst in ms.items():
        t = [a.elapsed_time(b) for a, b in lst]
        mean = sum(t) / len(t)
        res[name] = {"ms": round(mean, 3), "ms_min": round(min(t), 3), "ms_max": round(max(t), 3),
                     "payload_GiBps": round(payload / (mean / 1e3) / 2 ** 30, 1)}

    def both(v):
        return round(2 * payload / ((res[v + "_seal"]["ms"] + res[v + "_open"]["ms"]) / 1e3) / 2 ** 30, 1)

    rates = {v: both(v) for v in variants}
    ratios = {}
    for v in [v for v in variants if v != "raw" and "raw" in variants]:
        ratios[v + "_over_raw"] = {
            "seal": round(res["raw_seal"]["ms"] / res[v + "_seal"]["ms"], 4),
            "open": round(res["raw_open"]["ms"] / res[v + "_open"]["ms"], 4),
            "seal+open": round(rates[v] / rates["raw"], 4)}
    ok = all(v["oracle_mismatches"] == 0 and v["all_records_open"] for v in verified.values()) and \
        all(verified["counter"][k] for k in ("seq_equals_stable_rank", "all_records_open_after_timing",
                                             "counters_after_timing") if "counter" in variants)
    line = {"metric": "GiB/s payload, seal+open, AES-256-GCM, 65536 sessions, Zipf 64B-16KiB, TLS 1.2 "
                      "(BASELINE configs[3] workload): raw key-table batch vs many-session framing",
            "unit": "GiB/s", "records": n, "sessions": nkeys, "steps": args.steps, "warmup": args.warmup,
            "mean_len": round(float(lens.mean()), 1), "payload_bytes": int(payload),
            "seal+open_GiBps": rates, "per_op": res, "ratios": ratios,
            "single_connection_context": CONTEXT, "verified_detail": verified, "verified": bool(ok)}
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

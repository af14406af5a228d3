#!/usr/bin/env python3
"""What a key per lane costs the AES-CBC + HMAC record kernels, on config 4's
record lengths.

BASELINE configs[3]'s shape carried to the block-cipher suites: 65 536
sessions (PCG64 0x7716), --records records with Zipf(1.2) lengths 64 B-16 KiB
(PCG64 0x7717), AES-256 with each HMAC, MAC-then-encrypt and encrypt-then-MAC,
TLS 1.2.  Three ways to seal and open the same records, timed with device
events around each call, warm-up first, the variants alternating inside every
step:

  (a) single    tg_cbc_seal_records / tg_cbc_open_records: one key for every
                record, numbers seq0 + i -- the kernels as they were before key
                tables, and the yardstick;
  (b) explicit  tg_cbc_seal_session_records / _open_ with a session index and
                a sequence number per record;
  (c) counter   the same calls with per-session counters (the rank pass).

Every variant is verified: all records open back to their payload with status
0, sampled wire records against the CPU model (tests/cbc_model.py), counter
mode's numbers against numpy's stable rank.  Prints one JSON line per (record
count, MAC, construction); --out appends them to a file.

    python tools/bench_cbc_sessions.py --records 262144,1048576 --steps 5 --warmup 2 \\
        --out profiles/r12/cbc_sessions/bench_cbc_sessions.jsonl
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tlslite-ng_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

DIGEST = {"sha1": 20, "sha256": 32, "sha384": 48}


def run(n, mac, etm, args, np, torch, tlsgpu, cbc_model):
    nkeys, keylen, D = 65536, 32, DIGEST[mac]
    rk = np.random.default_rng(0x7716)
    enc_keys = rk.integers(0, 256, (nkeys, keylen), dtype=np.uint8)
    mac_keys = rk.integers(0, 256, (nkeys, D), dtype=np.uint8)
    session = rk.integers(0, nkeys, n).astype(np.uint32)
    lens = np.clip(64 * np.random.default_rng(0x7717).zipf(1.2, n), 64, 16384).astype(np.int64)
    seq = np.arange(n, dtype=np.uint64)                  # (a) and (b): record i has number i
    in_sz = (lens + 15) // 16 * 16
    in_off = np.concatenate([[0], np.cumsum(in_sz)[:-1]]).astype(np.int64)
    # wire record = header || iv || ciphertext [|| MAC], placed so that the IV starts 16-byte aligned
    w_sz = 16 + 16 + (lens + 48 + 16) // 16 * 16 + 48
    wire_off = np.concatenate([[0], np.cumsum(w_sz)[:-1]]).astype(np.int64) + 11
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    g = torch.Generator(device="cuda").manual_seed(0x7717)
    inp = torch.randint(0, 256, (int(in_sz.sum()),), dtype=torch.uint8, device="cuda", generator=g)
    iv = torch.randint(0, 256, (16 * n,), dtype=torch.uint8, device="cuda", generator=g)
    wire = torch.zeros(int(w_sz.sum()) + 16, dtype=torch.uint8, device="cuda")
    back = torch.zeros(int(w_sz.sum()) + 16, dtype=torch.uint8, device="cuda")
    d_lens, d_in_off, d_wire_off = d(lens.astype(np.int32)), d(in_off), d(wire_off)
    d_back_off = d(wire_off + 5)
    d_session, d_seq = d(session.view(np.int32)), d(seq.view(np.int64))
    ctype = torch.full((n,), 0x17, dtype=torch.uint8, device="cuda")
    w_len = torch.zeros(n, dtype=torch.int32, device="cuda")
    o_len = torch.zeros(n, dtype=torch.int32, device="cuda")
    o_ct = torch.zeros(n, dtype=torch.uint8, device="cuda")
    status = torch.zeros(n, dtype=torch.uint8, device="cuda")
    seq_out = torch.zeros(n, dtype=torch.int64, device="cuda")
    tx_next = torch.zeros(nkeys, dtype=torch.int64, device="cuda")
    rx_next = torch.zeros(nkeys, dtype=torch.int64, device="cuda")
    single = tlsgpu.CbcKey(bytes(enc_keys[0]), bytes(mac_keys[0]), mac)
    table = tlsgpu.CbcKey.table([bytes(k) for k in enc_keys], [bytes(k) for k in mac_keys], mac)
    stream = torch.cuda.current_stream()
    V = tlsgpu.TLS12

    def seal_s(**kw):
        tlsgpu.cbc.seal_session_records(table, V, etm, d_session, n, inp, d_in_off, d_lens, ctype, iv, wire,
                                        d_wire_off, w_len, stream=stream, **kw)

    def open_s(**kw):
        tlsgpu.cbc.open_session_records(table, V, etm, d_session, n, wire, d_wire_off, w_len, back, d_back_off,
                                        o_len, o_ct, status, stream=stream, **kw)

    ops = [("single_seal", lambda: tlsgpu.cbc.seal_records(single, V, etm, 0, n, inp, d_in_off, d_lens, ctype, iv,
                                                           wire, d_wire_off, w_len, stream=stream)),
           ("single_open", lambda: tlsgpu.cbc.open_records(single, V, etm, 0, n, back, d_back_off, o_len, o_ct,
                                                           status, wire, d_wire_off, w_len, stream=stream)),
           ("explicit_seal", lambda: seal_s(seq=d_seq)),
           ("explicit_open", lambda: open_s(seq=d_seq)),
           ("counter_seal", lambda: seal_s(seq_next=tx_next)),
           ("counter_open", lambda: open_s(seq_next=rx_next))]

    # ---- verification (untimed; also the first warm-up of every path) ----
    pick = [i for i in sorted(set(list(range(0, n, max(1, n // 40)))[:40] + [n - 1])) if lens[i] <= 2048][:24]
    gather_idx = (d_back_off[:, None] + torch.arange(64, device="cuda")[None, :]).reshape(-1)
    in_idx = (d_in_off[:, None] + torch.arange(64, device="cuda")[None, :]).reshape(-1)

    def sample_mismatches(seq_of, key_of):
        bad = 0
        for i in pick:
            L = int(lens[i])
            pt = inp[int(in_off[i]):int(in_off[i]) + L].cpu().numpy().tobytes()
            ek, mk = key_of(i)
            want = cbc_model.seal_record(ek, mk, mac, V, etm, int(seq_of[i]), 0x17, pt,
                                         iv[16 * i:16 * i + 16].cpu().numpy().tobytes())
            lo = int(wire_off[i])
            bad += int(wire[lo:lo + len(want)].cpu().numpy().tobytes() != want)
        return bad

    def opened_ok():
        # status, type and length of every record; the first 64 payload bytes of every record (all are >= 64)
        return (not bool(status.any()) and torch.equal(o_len, d_lens) and bool((o_ct == 0x17).all())
                and torch.equal(back[gather_idx], inp[in_idx]))

    verified = {}
    for name, seal, open_, seq_of, key_of in (
            ("single", ops[0][1], ops[1][1], lambda: seq, lambda i: (bytes(enc_keys[0]), bytes(mac_keys[0]))),
            ("explicit", ops[2][1], ops[3][1], lambda: seq,
             lambda i: (bytes(enc_keys[session[i]]), bytes(mac_keys[session[i]]))),
            ("counter", lambda: seal_s(seq_next=tx_next, seq_out=seq_out), ops[5][1],
             lambda: seq_out.cpu().numpy().view(np.uint64),
             lambda i: (bytes(enc_keys[session[i]]), bytes(mac_keys[session[i]])))):
        wire.zero_()
        back.zero_()
        status.fill_(255)
        seal()
        torch.cuda.synchronize()
        mism = sample_mismatches(seq_of(), key_of)
        open_()
        torch.cuda.synchronize()
        verified[name] = {"model_checked_records": len(pick), "model_mismatches": mism,
                          "all_records_open": bool(opened_ok())}
    order = np.argsort(session, kind="stable")
    _, first, cnt = np.unique(session[order], return_index=True, return_counts=True)
    rank = np.empty(n, np.int64)
    rank[order] = np.arange(n) - np.repeat(first, cnt)
    counts = np.bincount(session, minlength=nkeys)
    verified["counter"]["seq_equals_stable_rank"] = bool(
        np.array_equal(seq_out.cpu().numpy(), rank) and np.array_equal(tx_next.cpu().numpy(), counts)
        and np.array_equal(rx_next.cpu().numpy(), counts))

    for _ in range(args.warmup):
        for _, fn in ops:
            fn()
    ms = {name: [] for name, _ in ops}
    for _ in range(args.steps):
        for name, fn in ops:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            ms[name].append((e0, e1))
    torch.cuda.synchronize()
    verified["counter"]["all_records_open_after_timing"] = bool(opened_ok())
    payload = float(lens.sum())
    res, t = {}, {}
    for name, lst in ms.items():
        t[name] = [a.elapsed_time(b) for a, b in lst]
        mean = sum(t[name]) / len(t[name])
        res[name] = {"ms": round(mean, 3), "ms_min": round(min(t[name]), 3), "ms_max": round(max(t[name]), 3),
                     "payload_GiBps": round(payload / (mean / 1e3) / 2 ** 30, 1)}
    ratios = {}
    for v in ("explicit", "counter"):
        for op in ("seal", "open"):
            # rate of the variant over the yardstick's, step by step (the variants alternate inside a step)
            per_step = [a / b for a, b in zip(t["single_" + op], t[v + "_" + op])]
            ratios["%s_over_single_%s" % (v, op)] = {
                "mean": round(res["single_" + op]["ms"] / res[v + "_" + op]["ms"], 4),
                "min": round(min(per_step), 4), "max": round(max(per_step), 4)}
    ok = all(v["model_mismatches"] == 0 and v["all_records_open"] for v in verified.values()) and \
        verified["counter"]["seq_equals_stable_rank"] and verified["counter"]["all_records_open_after_timing"]
    single.close()
    table.close()
    return {"metric": "payload GiB/s, AES-256-CBC + HMAC, 65536 sessions, Zipf 64B-16KiB, TLS 1.2: single-key "
                      "call vs key-table call (explicit numbers, counters)",
            "unit": "GiB/s", "mac": mac, "construction": "etm" if etm else "mte", "records": n, "sessions": nkeys,
            "steps": args.steps, "warmup": args.warmup, "mean_len": round(float(lens.mean()), 1),
            "payload_bytes": int(payload), "per_op": res, "ratios": ratios, "verified_detail": verified,
            "verified": bool(ok)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", default="262144,1048576", help="comma-separated record counts")
    ap.add_argument("--macs", default="sha1,sha256,sha384")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import tlsgpu
    import cbc_model
    if not torch.cuda.is_available():
        sys.exit("bench_cbc_sessions.py needs a GPU")
    torch.cuda.set_device(0)
    ok = True
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for n in [int(x) for x in args.records.split(",")]:
        for mac in args.macs.split(","):
            for etm in (0, 1):
                line = run(n, mac, etm, args, np, torch, tlsgpu, cbc_model)
                torch.cuda.empty_cache()
                text = json.dumps(line)
                print(text, flush=True)
                if args.out:
                    with open(args.out, "a") as f:
                        f.write(text + "\n")
                ok = ok and line["verified"]
    if not ok:
        sys.exit(3)


if __name__ == "__main__":
    main()

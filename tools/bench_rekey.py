#!/usr/bin/env python3
"""Cost of a TLS 1.3 KeyUpdate on a live many-session state.

65 536 AES-256-GCM / SHA-384 sessions (TLS_AES_256_GCM_SHA384).  Timed with
device events around each variant, a stream sync at the end, warm-up first,
the variants alternating inside every repetition; the host time each call
takes to return is recorded beside the device time.

  (a) rebuild   the only way before tg_sessions_rekey: keysetup.key_update on
                all secrets, then keysetup.traffic_keys (every key re-derived,
                a second table allocated and built, a stream sync inside
                tg_key_create_device, the previous repetition's table
                destroyed behind a device sync);
  (b) in place  Sessions.key_update for n = 1, 64, 4 096 and 65 536 slots;
  (c) batch     a config-4-shaped seal batch (--records records, default 2^20,
                Zipf(1.2) lengths 64 B-16 KiB, TLS 1.3 counter mode) alone,
                against the same batch with a KeyUpdate of 1 % of the sessions
                enqueued in front of it on the same stream.

Verified afterwards: the live state is consistent (IVs and key table equal
what tg_hkdf_expand_label / tg_key_create_device derive from the live
secrets, on a sealed sample batch).  Prints one JSON line; --out writes it.

    python tools/bench_rekey.py --out profiles/r09/rekey/bench_rekey.json
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tlslite-ng_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

SUITE = 0x1302
NS = (1, 64, 4096, 65536)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", type=int, default=65536)
    ap.add_argument("--records", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--variants", default="rebuild,inplace,batch",
                    help="comma-separated subset (a profiler run of one variant attributes every kernel to it)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import tlsgpu
    from tlsgpu import keysetup
    if not torch.cuda.is_available():
        sys.exit("bench_rekey.py needs a GPU")
    torch.cuda.set_device(0)
    nsess, n = args.sessions, args.records
    variants = args.variants.split(",")
    stream = torch.cuda.current_stream()
    g = torch.Generator(device="cuda").manual_seed(0x9e11)
    secrets = torch.randint(0, 256, (nsess, 48), dtype=torch.uint8, device="cuda", generator=g)
    tx = tlsgpu.Sessions.from_traffic_secrets(SUITE, secrets)
    rng = np.random.default_rng(0x9e12)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    slots = {k: d(rng.permutation(nsess)[:k].astype(np.int32)) for k in NS if k <= nsess}
    one_pct = d(rng.permutation(nsess)[:max(1, nsess // 100)].astype(np.int32))

    ops = []
    state = {"secrets": secrets.clone(), "table": None}

    def rebuild():
        state["secrets"] = keysetup.key_update(SUITE, state["secrets"], stream=stream)
        state["table"] = keysetup.traffic_keys(SUITE, state["secrets"], stream=stream)

    if "rebuild" in variants:
        ops.append(("rebuild_all", rebuild))
    if "inplace" in variants:
        for k, s in slots.items():
            ops.append(("inplace_n%d" % k, lambda s=s: tx.key_update(s, stream=stream)))
    if "batch" in variants:
        rl = np.random.default_rng(0x7717)
        lens = np.clip(64 * rl.zipf(1.2, n), 64, 16384).astype(np.int64)
        sess = np.random.default_rng(0x7716).integers(0, nsess, n).astype(np.int32)
        d_sz = (lens + 1 + 16 + 15) // 16 * 16
        d_off = np.concatenate([[0], np.cumsum(d_sz)[:-1]]).astype(np.int64)
        w_sz = 16 + d_sz
        w_off = np.concatenate([[0], np.cumsum(w_sz)[:-1]]).astype(np.int64) + 11   # payload 16-aligned
        data = torch.randint(0, 256, (int(d_sz.sum()),), dtype=torch.uint8, device="cuda", generator=g)
        wire = torch.zeros(int(w_sz.sum()), dtype=torch.uint8, device="cuda")
        a = (d(sess), n, data, d(d_off), d(lens.astype(np.int32)),
             torch.full((n,), 23, dtype=torch.uint8, device="cuda"), wire, d(w_off),
             torch.zeros(n, dtype=torch.int32, device="cuda"))

        def batch(update):
            if update:
                tx.key_update(one_pct, stream=stream)
            tx.seal(*a, stream=stream)

        ops.append(("batch_alone", lambda: batch(False)))
        ops.append(("batch_after_1pct_update", lambda: batch(True)))

    for _ in range(args.warmup):
        for _, fn in ops:
            fn()
        torch.cuda.synchronize()
    dev = {name: [] for name, _ in ops}
    host = {name: [] for name, _ in ops}
    for _ in range(args.steps):
        for name, fn in ops:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            t0 = time.perf_counter()
            fn()
            host[name].append((time.perf_counter() - t0) * 1e3)
            e1.record(stream)
            dev[name].append((e0, e1))
    torch.cuda.synchronize()

    def stats(t):
        t = sorted(t)
        return {"ms": round(sum(t) / len(t), 4), "ms_median": round(t[len(t) // 2], 4),
                "ms_min": round(t[0], 4), "ms_max": round(t[-1], 4)}

    res = {name: {"device": stats([x.elapsed_time(y) for x, y in dev[name]]), "host_call": stats(host[name])}
           for name, _ in ops}
    ratios = {}
    if "rebuild_all" in res:
        for name in res:
            if name.startswith("inplace_"):
                ratios[name + "_over_rebuild_all"] = round(res[name]["device"]["ms"] /
                                                           res["rebuild_all"]["device"]["ms"], 4)
    if "batch_alone" in res:
        ratios["batch_after_1pct_update_over_batch_alone"] = round(
            res["batch_after_1pct_update"]["device"]["ms"] / res["batch_alone"]["device"]["ms"], 4)

    # the live state is still what the creation-time path derives from its secrets
    ivs = keysetup.hkdf_expand_label(tx.secrets, b"iv", b"", 12, 48)
    fresh, _, _ = keysetup.traffic_keys(SUITE, tx.secrets)
    m = 4096
    sample = d(rng.integers(0, nsess, m).astype(np.int32))
    pt = torch.randint(0, 256, (m * 256,), dtype=torch.uint8, device="cuda", generator=g)
    nonce = torch.randint(0, 256, (m * 12,), dtype=torch.uint8, device="cuda", generator=g)
    outs = []
    for table in (tx.table, fresh):
        out = torch.zeros(m * 272, dtype=torch.uint8, device="cuda")
        tlsgpu.seal_batch(table, tlsgpu.make_batch(m, pt, out, nonce, fixed_len=256, in_stride=256, out_stride=272,
                                                   key_idx=sample))
        outs.append(out)
    torch.cuda.synchronize()
    ok = bool(torch.equal(ivs, tx.ivs)) and bool(torch.equal(outs[0], outs[1])) and bool(outs[0].any())
    line = {"metric": "ms per TLS 1.3 KeyUpdate, AES-256-GCM / SHA-384, %d sessions: rebuilding the whole state "
                      "vs tg_sessions_rekey in place" % nsess,
            "unit": "ms", "sessions": nsess, "records": n if "batch" in variants else 0, "steps": args.steps,
            "warmup": args.warmup, "per_op": res, "ratios": ratios, "verified": ok}
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

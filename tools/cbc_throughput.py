"""Throughput of the AES-CBC + HMAC record kernels (csrc/aes_cbc.hip), per MAC,
construction and direction: device-resident batches, device events around
``--iters`` back-to-back calls after a warm-up call, payload bytes (the
fragments, not the wire) over the mean call time.  DESIGN.md quotes one run of

    python tools/cbc_throughput.py --records 65536 --length 16384

Prints one JSON line per configuration.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tlslite-ng_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=65536)
    ap.add_argument("--length", type=int, default=16384)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--keylen", type=int, default=16)
    args = ap.parse_args()
    import torch
    import tlsgpu
    assert torch.cuda.is_available(), "needs a GPU"
    n, L = args.records, args.length
    stride = (L + 48 + 16 + 21 + 15) // 16 * 16 + 16          # room for any MAC, 16-byte aligned payloads
    data = torch.randint(0, 256, (n * L,), dtype=torch.uint8, device="cuda")
    d_off = torch.arange(n, dtype=torch.int64, device="cuda") * L
    w_off = torch.arange(n, dtype=torch.int64, device="cuda") * stride + 11
    d_len = torch.full((n,), L, dtype=torch.int32, device="cuda")
    ctype = torch.full((n,), 23, dtype=torch.uint8, device="cuda")
    iv = torch.randint(0, 256, (16 * n,), dtype=torch.uint8, device="cuda")
    wire = torch.zeros(n * stride + 16, dtype=torch.uint8, device="cuda")
    w_len = torch.zeros(n, dtype=torch.int32, device="cuda")
    out = torch.zeros(n * stride, dtype=torch.uint8, device="cuda")
    o_off = torch.arange(n, dtype=torch.int64, device="cuda") * stride
    o_len = torch.zeros(n, dtype=torch.int32, device="cuda")
    o_ct = torch.zeros(n, dtype=torch.uint8, device="cuda")
    st = torch.zeros(n, dtype=torch.uint8, device="cuda")

    def timed(fn):
        fn()                                                  # warm-up: code object load, LDS attribute
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / args.iters

    for mac in ("sha1", "sha256", "sha384"):
        for etm in (0, 1):
            key = tlsgpu.CbcKey(bytes(range(args.keylen)), bytes(range(tlsgpu.cbc.MAC_LENGTH[mac])), mac)
            ms_seal = timed(lambda: tlsgpu.cbc.seal_records(key, tlsgpu.TLS12, etm, 0, n, data, d_off, d_len, ctype,
                                                            iv, wire, w_off, w_len))
            ms_open = timed(lambda: tlsgpu.cbc.open_records(key, tlsgpu.TLS12, etm, 0, n, out, o_off, o_len, o_ct,
                                                            st, wire, w_off, w_len))
            torch.cuda.synchronize()
            ok = bool((st == 0).all()) and bool((o_len == L).all())
            sample = [0, n // 2, n - 1]
            ok = ok and all(torch.equal(out[i * stride:i * stride + L], data[i * L:(i + 1) * L]) for i in sample)
            gib = n * L / 2.0 ** 30
            print(json.dumps({"aes": args.keylen * 8, "mac": mac, "construction": "etm" if etm else "mte",
                              "records": n, "length": L, "iters": args.iters,
                              "seal_ms": round(ms_seal, 3), "open_ms": round(ms_open, 3),
                              "seal_GiBps": round(gib / (ms_seal / 1e3), 2),
                              "open_GiBps": round(gib / (ms_open / 1e3), 2), "round_trip_ok": ok}), flush=True)
            key.close()


if __name__ == "__main__":
    main()

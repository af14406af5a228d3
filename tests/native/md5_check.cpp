// md5_check.cpp -- the device's MD5 (csrc/md5.h) on the CPU.
//
// Reads lines "md5 <message hex|-> <digest hex>" and
// "hmac <key hex> <message hex|-> <digest hex>" (keys of at most one block),
// hashes each with Md5::init / Md5::compress -- padding, little-endian words and
// the little-endian bit length done here as the device helpers do them -- and
// compares.  Prints "CASES n=<lines> bad=<mismatches>" and "OK".
// tests/test_md5_host.py writes the file and builds this with g++.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "md5.h"

using tg::Md5;
typedef std::vector<uint8_t> Bytes;

static Bytes unhex(const std::string& s) {
    Bytes out;
    if (s == "-") return out;
    for (size_t k = 0; k + 1 < s.size(); k += 2) out.push_back((uint8_t)strtoul(s.substr(k, 2).c_str(), nullptr, 16));
    return out;
}

// st: a state (fresh, or a midstate that has taken `before` bytes); the digest of before + msg.
static Bytes finish(uint32_t st[8], const Bytes& msg, uint64_t before) {
    Bytes m(msg);
    const uint64_t bits = (before + msg.size()) * 8;
    m.push_back(0x80);
    while (m.size() % Md5::kBlock != (size_t)(Md5::kBlock - Md5::kLenBytes)) m.push_back(0);
    for (int k = 0; k < 8; ++k) m.push_back((uint8_t)(bits >> (8 * k)));
    for (size_t at = 0; at < m.size(); at += Md5::kBlock) {
        uint32_t w[16];
        for (int k = 0; k < 16; ++k)
            w[k] = (uint32_t)m[at + 4 * k] | ((uint32_t)m[at + 4 * k + 1] << 8) | ((uint32_t)m[at + 4 * k + 2] << 16) |
                   ((uint32_t)m[at + 4 * k + 3] << 24);
        Md5::compress(st, w);
    }
    Bytes d;
    for (int k = 0; k < Md5::kHash; ++k) d.push_back((uint8_t)(st[k / 4] >> (8 * (k % 4))));
    return d;
}

static Bytes md5(const Bytes& msg) {
    uint32_t st[8];
    Md5::init(st);
    return finish(st, msg, 0);
}

static Bytes hmac_md5(const Bytes& key, const Bytes& msg) {
    uint32_t in[8], out[8], w[16];
    uint8_t blk[64] = {0};
    memcpy(blk, key.data(), key.size());
    for (int pass = 0; pass < 2; ++pass) {
        for (int k = 0; k < 16; ++k) {
            w[k] = (uint32_t)blk[4 * k] | ((uint32_t)blk[4 * k + 1] << 8) | ((uint32_t)blk[4 * k + 2] << 16) |
                   ((uint32_t)blk[4 * k + 3] << 24);
            w[k] ^= pass ? 0x5c5c5c5cu : 0x36363636u;
        }
        Md5::init(pass ? out : in);
        Md5::compress(pass ? out : in, w);
    }
    const Bytes inner = finish(in, msg, 64);
    return finish(out, inner, 64);
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::ifstream f(argv[1]);
    std::string line;
    unsigned n = 0, bad = 0;
    while (std::getline(f, line)) {
        std::istringstream ss(line);
        std::string kind, a, b, c;
        ss >> kind >> a >> b;
        Bytes got, want;
        if (kind == "md5") {
            got = md5(unhex(a));
            want = unhex(b);
        } else if (kind == "hmac") {
            ss >> c;
            const Bytes key = unhex(a);
            if (key.size() > 64) return 2;
            got = hmac_md5(key, unhex(b));
            want = unhex(c);
        } else {
            return 2;
        }
        ++n;
        if (got != want || want.size() != 16) {
            ++bad;
            printf("MISMATCH line %u\n", n);
        }
    }
    printf("CASES n=%u bad=%u\n", n, bad);
    if (bad || !n) return 1;
    printf("OK\n");
    return 0;
}

// cbc_verdict_check -- the host build of the device's record verdict code
// (csrc/cbc_record.h, csrc/sha.h), run by tests/test_cbc_host.py.
//
//   cbc_verdict_check FILE
//
// (a) FILE holds one line per MAC-then-encrypt receive fixture:
//       mac version seq type limit hlen body mac_key_hex plain_hex|- status len
//     (mac 1 / 2 / 3 = SHA-1 / -256 / -384; plain: the decrypted body behind
//     its IV block, "-" when the record is not decrypted; status / len: what
//     the reference's receiving RecordLayer gave).  The public checks, the
//     verdict and the limit check must give exactly that.  Every line is
//     answered with "LINE k mac n compressions" (n: the decrypted length;
//     the compression calls of its verdict, 0 when it was never decrypted),
//     so that the caller can hold the count constant per (mac, n).
// (b) For each MAC, valid records of one wire length with every padding
//     length 0..255, and the same with a wrong padding byte and with a wrong
//     MAC byte: the verdicts are right and the number of compression calls
//     is the same for all of them.
#define TG_SHA_COUNT 1
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

unsigned long tg_sha_count = 0;

#include "cbc_record.h"

using namespace tg;

struct HostMem {
    static cbc::W4 ld16(const uint8_t* p) {
        cbc::W4 v;
        memcpy(&v, p, 16);
        return v;
    }
    static cbc::W4 ldn(const uint8_t* p, uint32_t n) {
        cbc::W4 v = {0, 0, 0, 0};
        memcpy(&v, p, n);
        return v;
    }
    static uint32_t ld4(const uint8_t* p) {
        uint32_t v;
        memcpy(&v, p, 4);
        return v;
    }
    static uint32_t ld1(const uint8_t* p) { return *p; }
};

static std::vector<uint8_t> unhex(const std::string& s) {
    std::vector<uint8_t> out;
    if (s == "-") return out;
    for (size_t k = 0; k + 1 < s.size(); k += 2) out.push_back((uint8_t)strtoul(s.substr(k, 2).c_str(), nullptr, 16));
    return out;
}

template <class H>
static uint32_t run_fixture(const std::vector<uint8_t>& key, uint32_t version, uint64_t seq, uint32_t type,
                            uint32_t limit, uint32_t hlen, uint32_t body, const std::vector<uint8_t>& plain,
                            uint32_t* len, unsigned long* cost) {
    *len = 0;
    *cost = 0;
    uint32_t st = cbc::mte_public_status(H::kHash, hlen, body, limit);
    if (st != cbc::kRecOk) return st;
    if (plain.size() != body - 16) return 0xffffffffu;   // the test fed the wrong bytes
    cbc::Mid mid;
    cbc::hmac_midstates<H>(key.data(), (uint32_t)key.size(), &mid);
    // an exact-size copy, so that a read past the record shows under the sanitizer
    std::vector<uint8_t> p(plain);
    const unsigned long before = tg_sha_count;
    const uint32_t bad = cbc::mte_verdict<H, HostMem>(mid, seq, type, version, p.data(), (uint32_t)p.size(), len);
    *cost = tg_sha_count - before;
    st = cbc::final_status(bad, *len, limit);
    if (st != cbc::kRecOk) *len = 0;
    return st;
}

template <class H>
static int constant_work(const char* name) {
    const uint32_t D = H::kHash, n = 384;                  // >= D + 256: every padding length fits
    uint8_t key[20];
    for (int k = 0; k < 20; ++k) key[k] = (uint8_t)(0xa0 + k);
    cbc::Mid mid;
    cbc::hmac_midstates<H>(key, 20, &mid);
    int bad = 0;
    unsigned long want = 0;
    for (uint32_t pad = 0; pad < 256; ++pad) {
        const uint32_t L = n - D - 1 - pad;
        std::vector<uint8_t> p(n);
        for (uint32_t k = 0; k < L; ++k) p[k] = (uint8_t)(k * 7 + pad);
        uint32_t dig[12];
        cbc::hmac_record<H, HostMem>(mid, 0x1ffffffffull, 23, 0x0303, p.data(), L, L, cbc::hmac_blocks<H>(L), dig);
        for (uint32_t k = 0; k < D; ++k) p[L + k] = (uint8_t)(dig[k / 4] >> (24 - 8 * (k % 4)));
        for (uint32_t k = L + D; k < n; ++k) p[k] = (uint8_t)pad;
        for (int variant = 0; variant < 3; ++variant) {
            std::vector<uint8_t> q(p);
            if (variant == 1 && pad) q[n - 1 - (pad + 1) / 2] ^= 0x10;   // a padding byte (not the length)
            if (variant == 2) q[L + D / 2] ^= 0x01;                        // a MAC byte
            const bool expect_bad = (variant == 1 && pad) || variant == 2;
            uint32_t len = 0;
            const unsigned long before = tg_sha_count;
            const uint32_t v = cbc::mte_verdict<H, HostMem>(mid, 0x1ffffffffull, 23, 0x0303, q.data(), n, &len);
            const unsigned long cost = tg_sha_count - before;
            if (!want) want = cost;
            if (cost != want || (v != 0) != expect_bad || (!expect_bad && len != L)) {
                printf("%s pad=%u variant=%d: verdict %u len %u (want %u) compressions %lu (want %lu)\n", name, pad,
                       variant, v, len, L, cost, want);
                ++bad;
            }
        }
    }
    printf("WORK %s n=%u compressions=%lu bad=%d\n", name, n, want, bad);
    return bad;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    static char key_hex[1024], plain_hex[1 << 16];
    unsigned mac, version, type, limit, hlen, body, status, len;
    unsigned long long seq;
    int bad = 0, n = 0;
    while (fscanf(f, "%u %u %llu %u %u %u %u %1023s %65535s %u %u", &mac, &version, &seq, &type, &limit, &hlen, &body,
                  key_hex, plain_hex, &status, &len) == 11) {
        const std::vector<uint8_t> key = unhex(key_hex), plain = unhex(plain_hex);
        uint32_t got_len = 0, got;
        unsigned long cost = 0;
        if (mac == 1) got = run_fixture<Sha1>(key, version, seq, type, limit, hlen, body, plain, &got_len, &cost);
        else if (mac == 2) got = run_fixture<Sha256>(key, version, seq, type, limit, hlen, body, plain, &got_len, &cost);
        else got = run_fixture<Sha384>(key, version, seq, type, limit, hlen, body, plain, &got_len, &cost);
        ++n;
        printf("LINE %d %u %zu %lu\n", n, mac, plain.size(), cost);
        if (got != status || got_len != len) {
            printf("fixture %d (mac %u body %u): status %u len %u, want %u %u\n", n, mac, body, got, got_len, status,
                   len);
            ++bad;
        }
    }
    fclose(f);
    printf("FIXTURES n=%d bad=%d\n", n, bad);
    bad += constant_work<Sha1>("sha1");
    bad += constant_work<Sha256>("sha256");
    bad += constant_work<Sha384>("sha384");
    puts(bad ? "FAILED" : "OK");
    return bad ? 1 : 0;
}

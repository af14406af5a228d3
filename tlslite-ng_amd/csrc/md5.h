// md5.h -- the MD5 compression function (RFC 1321), one message block per
// call, with the interface of the hashes of sha.h.  The engine needs it for one
// thing: the TLS 1.0 / 1.1 PRF, P_MD5(S1, ...) xor P_SHA1(S2, ...)
// (tlslite/mathtls.py:701-714, tls10.hip).  No record is authenticated with it.
//
// MD5 is the only little-endian hash here (kBigEndian == false): compress
// takes the sixteen LITTLE-endian words of a block, the 64-bit bit length is
// little-endian in words 14 and 15, and the digest is the state's four words
// in little-endian byte order.  The helpers of prf_dev.h honour the trait.
//
// __host__ __device__ and no builtin, as sha.h: tests/native/md5_check.cpp
// runs this text on the CPU.  The 64 constants and the shift amounts are
// compile-time values of a fully unrolled round sequence -- no table is
// indexed at run time, so a kernel that hashes with it has no private segment.
#pragma once
#include "sha.h"

namespace tg {
namespace {

// floor(2^32 * abs(sin(i + 1))), RFC 1321 section 3.4
constexpr uint32_t c_kmd5[64] = {
    0xd76aa478, 0xe8c7b756, 0x242070db, 0xc1bdceee, 0xf57c0faf, 0x4787c62a, 0xa8304613,
    0xfd469501, 0x698098d8, 0x8b44f7af, 0xffff5bb1, 0x895cd7be, 0x6b901122, 0xfd987193,
    0xa679438e, 0x49b40821, 0xf61e2562, 0xc040b340, 0x265e5a51, 0xe9b6c7aa, 0xd62f105d,
    0x02441453, 0xd8a1e681, 0xe7d3fbc8, 0x21e1cde6, 0xc33707d6, 0xf4d50d87, 0x455a14ed,
    0xa9e3e905, 0xfcefa3f8, 0x676f02d9, 0x8d2a4c8a, 0xfffa3942, 0x8771f681, 0x6d9d6122,
    0xfde5380c, 0xa4beea44, 0x4bdecfa9, 0xf6bb4b60, 0xbebfbc70, 0x289b7ec6, 0xeaa127fa,
    0xd4ef3085, 0x04881d05, 0xd9d4d039, 0xe6db99e5, 0x1fa27cf8, 0xc4ac5665, 0xf4292244,
    0x432aff97, 0xab9423a7, 0xfc93a039, 0x655b59c3, 0x8f0ccc92, 0xffeff47d, 0x85845dd1,
    0x6fa87e4f, 0xfe2ce6e0, 0xa3014314, 0x4e0811a1, 0xf7537e82, 0xbd3af235, 0x2ad7d2bb,
    0xeb86d391};
constexpr int c_smd5[4][4] = {{7, 12, 17, 22}, {5, 9, 14, 20}, {4, 11, 16, 23}, {6, 10, 15, 21}};

// The reference hashes through hashlib (compatHMAC, mathtls.py:679-698).
struct Md5 {
    using word = uint32_t;
    static constexpr int kHash = 16, kStateOut = 4, kBlock = 64, kLenBytes = 8;
    static constexpr bool kBigEndian = false;
    TG_HD static void init(word s[8]) {
        s[0] = 0x67452301u; s[1] = 0xefcdab89u; s[2] = 0x98badcfeu; s[3] = 0x10325476u;
        s[4] = 0; s[5] = 0; s[6] = 0; s[7] = 0;
    }
    // m: the sixteen little-endian words of one block
    TG_HD static void compress(word s[8], const word m[16]) {
        word a = s[0], b = s[1], c = s[2], d = s[3];
#pragma unroll
        for (int t = 0; t < 64; ++t) {
            word f;
            int g;
            if (t < 16) {
                f = d ^ (b & (c ^ d)); g = t;
            } else if (t < 32) {
                f = c ^ (d & (b ^ c)); g = (5 * t + 1) & 15;
            } else if (t < 48) {
                f = b ^ c ^ d; g = (3 * t + 5) & 15;
            } else {
                f = c ^ (b | ~d); g = (7 * t) & 15;
            }
            const int r = c_smd5[t >> 4][t & 3];
            const word x = a + f + c_kmd5[t] + m[g];
            a = d; d = c; c = b; b = b + ((x << r) | (x >> (32 - r)));
        }
        s[0] += a; s[1] += b; s[2] += c; s[3] += d;
    }
};

}  // namespace
}  // namespace tg

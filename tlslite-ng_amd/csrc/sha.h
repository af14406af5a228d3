// sha.h -- the SHA-1 / SHA-256 / SHA-384 compression functions, one message
// block per call, shared by the key-setup kernels (keysetup.hip: HKDF,
// rekey) and the AES-CBC + HMAC record kernels (aes_cbc.hip, cbc_record.h).
//
// Every function is __host__ __device__ and uses no builtin, so the same code
// also builds with a plain C++ compiler: the HMAC midstates of a CBC key are
// computed on the host with it, and tests/native/cbc_verdict_check.cpp runs
// the record verdict code on the CPU.
//
// A hash H has: word (uint32_t / uint64_t), kHash (digest bytes), kStateOut
// (digest words), kBlock (message block bytes), kLenBytes (bytes of the
// trailing bit-length field), kBigEndian (the byte order of message words,
// length field and digest: true for all of these, false for the MD5 of md5.h),
// init(s) and compress(s, m) with m the sixteen big-endian words of one block.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define TG_HD __host__ __device__
#define TG_HDI __host__ __device__ __forceinline__
#else
#define TG_HD
#define TG_HDI inline __attribute__((always_inline))
#endif

// Host builds of the verdict test count compression calls (the constant-work
// check of tests/native/cbc_verdict_check.cpp).
#if defined(TG_SHA_COUNT) && !defined(__HIP_DEVICE_COMPILE__)
extern unsigned long tg_sha_count;
#define TG_SHA_TICK() (++tg_sha_count)
#else
#define TG_SHA_TICK() ((void)0)
#endif

namespace tg {
namespace {

#define TG_K256_INIT                                                                               \
    {0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4,           \
     0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe,           \
     0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f,           \
     0x4a7484aa, 0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7,           \
     0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc,           \
     0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b,           \
     0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116,           \
     0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3,           \
     0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7,           \
     0xc67178f2}

#define TG_K512_INIT                                                                               \
    {0x428a2f98d728ae22ull, 0x7137449123ef65cdull, 0xb5c0fbcfec4d3b2full, 0xe9b5dba58189dbbcull,   \
     0x3956c25bf348b538ull, 0x59f111f1b605d019ull, 0x923f82a4af194f9bull, 0xab1c5ed5da6d8118ull,   \
     0xd807aa98a3030242ull, 0x12835b0145706fbeull, 0x243185be4ee4b28cull, 0x550c7dc3d5ffb4e2ull,   \
     0x72be5d74f27b896full, 0x80deb1fe3b1696b1ull, 0x9bdc06a725c71235ull, 0xc19bf174cf692694ull,   \
     0xe49b69c19ef14ad2ull, 0xefbe4786384f25e3ull, 0x0fc19dc68b8cd5b5ull, 0x240ca1cc77ac9c65ull,   \
     0x2de92c6f592b0275ull, 0x4a7484aa6ea6e483ull, 0x5cb0a9dcbd41fbd4ull, 0x76f988da831153b5ull,   \
     0x983e5152ee66dfabull, 0xa831c66d2db43210ull, 0xb00327c898fb213full, 0xbf597fc7beef0ee4ull,   \
     0xc6e00bf33da88fc2ull, 0xd5a79147930aa725ull, 0x06ca6351e003826full, 0x142929670a0e6e70ull,   \
     0x27b70a8546d22ffcull, 0x2e1b21385c26c926ull, 0x4d2c6dfc5ac42aedull, 0x53380d139d95b3dfull,   \
     0x650a73548baf63deull, 0x766a0abb3c77b2a8ull, 0x81c2c92e47edaee6ull, 0x92722c851482353bull,   \
     0xa2bfe8a14cf10364ull, 0xa81a664bbc423001ull, 0xc24b8b70d0f89791ull, 0xc76c51a30654be30ull,   \
     0xd192e819d6ef5218ull, 0xd69906245565a910ull, 0xf40e35855771202aull, 0x106aa07032bbd1b8ull,   \
     0x19a4c116b8d2d0c8ull, 0x1e376c085141ab53ull, 0x2748774cdf8eeb99ull, 0x34b0bcb5e19b48a8ull,   \
     0x391c0cb3c5c95a63ull, 0x4ed8aa4ae3418acbull, 0x5b9cca4f7763e373ull, 0x682e6ff3d6b2b8a3ull,   \
     0x748f82ee5defb2fcull, 0x78a5636f43172f60ull, 0x84c87814a1f0ab72ull, 0x8cc702081a6439ecull,   \
     0x90befffa23631e28ull, 0xa4506cebde82bde9ull, 0xbef9a3f7b2c67915ull, 0xc67178f2e372532bull,   \
     0xca273eceea26619cull, 0xd186b8c721c0c207ull, 0xeada7dd6cde0eb1eull, 0xf57d4f7fee6ed178ull,   \
     0x06f067aa72176fbaull, 0x0a637dc5a2c898a6ull, 0x113f9804bef90daeull, 0x1b710b35131c471bull,   \
     0x28db77f523047d84ull, 0x32caab7b40c72493ull, 0x3c9ebe0a15c9bebcull, 0x431d67c49c100d4cull,   \
     0x4cc5d4becb3e42b6ull, 0x597f299cfc657e2aull, 0x5fcb6fab3ad6faecull, 0x6c44198c4a475817ull}

// constexpr, not __constant__: every use has a compile-time index (the round
// loops are fully unrolled), so the constants become immediates in device
// code as well, and host-device functions may name them.
constexpr uint32_t c_k256[64] = TG_K256_INIT;
constexpr uint64_t c_k512[80] = TG_K512_INIT;
#undef TG_K256_INIT
#undef TG_K512_INIT

TG_HD inline uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
TG_HD inline uint64_t rotr64(uint64_t x, int n) { return (x >> n) | (x << (64 - n)); }

// FIPS 180-4 section 6.1; the reference hashes through hashlib (compatHMAC).
struct Sha1 {
    using word = uint32_t;
    static constexpr int kHash = 20, kStateOut = 5, kBlock = 64, kLenBytes = 8;
    static constexpr bool kBigEndian = true;
    TG_HD static void init(word s[8]) {
        s[0] = 0x67452301u; s[1] = 0xefcdab89u; s[2] = 0x98badcfeu; s[3] = 0x10325476u;
        s[4] = 0xc3d2e1f0u; s[5] = 0; s[6] = 0; s[7] = 0;
    }
    TG_HD static void compress(word s[8], const word m[16]) {
        TG_SHA_TICK();
        word w[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) w[k] = m[k];
        word a = s[0], b = s[1], c = s[2], d = s[3], e = s[4];
#pragma unroll
        for (int t = 0; t < 80; ++t) {
            if (t >= 16) {
                const word x = w[(t - 3) & 15] ^ w[(t - 8) & 15] ^ w[(t - 14) & 15] ^ w[t & 15];
                w[t & 15] = (x << 1) | (x >> 31);
            }
            word f, k;
            if (t < 20) {
                f = (b & c) | (~b & d); k = 0x5a827999u;
            } else if (t < 40) {
                f = b ^ c ^ d; k = 0x6ed9eba1u;
            } else if (t < 60) {
                f = (b & c) | (b & d) | (c & d); k = 0x8f1bbcdcu;
            } else {
                f = b ^ c ^ d; k = 0xca62c1d6u;
            }
            const word tmp = ((a << 5) | (a >> 27)) + f + e + k + w[t & 15];
            e = d; d = c; c = (b << 30) | (b >> 2); b = a; a = tmp;
        }
        s[0] += a; s[1] += b; s[2] += c; s[3] += d; s[4] += e;
    }
};

struct Sha256 {
    using word = uint32_t;
    static constexpr int kHash = 32, kStateOut = 8, kBlock = 64, kLenBytes = 8;
    static constexpr bool kBigEndian = true;
    TG_HD static void init(word s[8]) {
        const word iv[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a,
                            0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
#pragma unroll
        for (int k = 0; k < 8; ++k) s[k] = iv[k];
    }
    TG_HD static void compress(word s[8], const word m[16]) {
        TG_SHA_TICK();
        word w[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) w[k] = m[k];
        word a = s[0], b = s[1], c = s[2], d = s[3], e = s[4], f = s[5], g = s[6], h = s[7];
#pragma unroll
        for (int t = 0; t < 64; ++t) {
            if (t >= 16) {
                const word w15 = w[(t - 15) & 15], w2 = w[(t - 2) & 15];
                w[t & 15] += (rotr(w15, 7) ^ rotr(w15, 18) ^ (w15 >> 3)) + w[(t - 7) & 15] +
                             (rotr(w2, 17) ^ rotr(w2, 19) ^ (w2 >> 10));
            }
            const word t1 = h + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) +
                            c_k256[t] + w[t & 15];
            const word t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
            h = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
        }
        s[0] += a; s[1] += b; s[2] += c; s[3] += d; s[4] += e; s[5] += f; s[6] += g; s[7] += h;
    }
};

struct Sha384 {
    using word = uint64_t;
    static constexpr int kHash = 48, kStateOut = 6, kBlock = 128, kLenBytes = 16;
    static constexpr bool kBigEndian = true;
    TG_HD static void init(word s[8]) {
        const word iv[8] = {0xcbbb9d5dc1059ed8ull, 0x629a292a367cd507ull, 0x9159015a3070dd17ull,
                            0x152fecd8f70e5939ull, 0x67332667ffc00b31ull, 0x8eb44a8768581511ull,
                            0xdb0c2e0d64f98fa7ull, 0x47b5481dbefa4fa4ull};
#pragma unroll
        for (int k = 0; k < 8; ++k) s[k] = iv[k];
    }
    TG_HD static void compress(word s[8], const word m[16]) {
        TG_SHA_TICK();
        word w[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) w[k] = m[k];
        word a = s[0], b = s[1], c = s[2], d = s[3], e = s[4], f = s[5], g = s[6], h = s[7];
#pragma unroll
        for (int t = 0; t < 80; ++t) {
            if (t >= 16) {
                const word w15 = w[(t - 15) & 15], w2 = w[(t - 2) & 15];
                w[t & 15] += (rotr64(w15, 1) ^ rotr64(w15, 8) ^ (w15 >> 7)) + w[(t - 7) & 15] +
                             (rotr64(w2, 19) ^ rotr64(w2, 61) ^ (w2 >> 6));
            }
            const word t1 = h + (rotr64(e, 14) ^ rotr64(e, 18) ^ rotr64(e, 41)) +
                            ((e & f) ^ (~e & g)) + c_k512[t] + w[t & 15];
            const word t2 = (rotr64(a, 28) ^ rotr64(a, 34) ^ rotr64(a, 39)) +
                            ((a & b) ^ (a & c) ^ (b & c));
            h = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
        }
        s[0] += a; s[1] += b; s[2] += c; s[3] += d; s[4] += e; s[5] += f; s[6] += g; s[7] += h;
    }
};

}  // namespace
}  // namespace tg

// cbc_dev.h -- what the AES-CBC + HMAC translation units share: the key
// handle and its device rows, the argument checks of every entry point that
// makes or refills a handle (aes_cbc.hip from host keys, tls12.hip from device
// keys and master secrets), the inverse-cipher tables and the equivalent
// inverse cipher (templated on the round-key provider, like aes_round.h's
// aes_block), and the global-memory helpers that cbc_record.h reads through.
// aes_cbc.hip (one connection per call, round keys wave-uniform) and
// aes_cbc_table.hip (a session per record, round keys per lane) each keep
// their own kernels around them.
//
// LDS as aes_cbc.hip describes it: a seal kernel stages the 64 KiB Te0 / Te2
// block at 0, an open kernel Td0 / Td2 there and the inverse S-box copies
// behind it.
#pragma once
#include <stdio.h>

#include "aes_round.h"
#include "api.h"
#include "cbc_record.h"

namespace tg {

// One CBC + HMAC key in device memory: a row of a handle's table.
struct CbcKeyDev {
    uint32_t ek[60];       // round keys, LE words of the key-schedule bytes
    uint32_t dk[60];       // equivalent inverse cipher: dk[r] = ek[Nr - r], InvMixColumns for 0 < r < Nr
    cbc::Mid mid;          // HMAC midstates (32-bit hashes in the low halves)
    uint32_t rounds;
    uint32_t mac;
    uint32_t pad[2];
};
static_assert(sizeof(CbcKeyDev) % 16 == 0, "rows keep ek / dk at 16-byte alignment");

}  // namespace tg

struct tg_cbc_key {
    int device;
    int rounds;
    int mac;
    size_t nkeys;
    tg::CbcKeyDev* dev_key;        // nkeys rows
    // tg_cbc_key_replace: pinned staging for the rows on their way to the
    // device, and the event behind the last copy out of it
    tg::CbcKeyDev* stage;
    hipEvent_t stage_done;
};

namespace tg {
namespace {

// ---- host side: what every entry point that takes or makes a handle checks --
inline int mac_block(int mac) {
    return mac == TG_MAC_SHA1 || mac == TG_MAC_SHA256 ? 64 : mac == TG_MAC_SHA384 ? 128 : 0;
}

// The text of what is wrong with a (cipher key length, MAC key length, MAC)
// triple, or nullptr.
inline const char* key_error(size_t keylen, size_t mackeylen, int mac, char (&buf)[80]) {
    if (keylen != 16 && keylen != 32) {
        snprintf(buf, sizeof(buf), "enc key length must be 16 or 32, got %zu", keylen);
        return buf;
    }
    const int block = mac_block(mac);
    if (!block) {
        snprintf(buf, sizeof(buf), "unknown mac %d", mac);
        return buf;
    }
    if (mackeylen == 0 || mackeylen > (size_t)block) {
        snprintf(buf, sizeof(buf), "mac key length must be 1..%d, got %zu", block, mackeylen);
        return buf;
    }
    return nullptr;
}

// key_error, then the row count of a new table.
inline const char* table_error(size_t keylen, size_t mackeylen, int mac, size_t nkeys, char (&buf)[80]) {
    if (const char* msg = key_error(keylen, mackeylen, mac, buf)) return msg;
    if (nkeys == 0 || nkeys > 0xffffffffull) {
        snprintf(buf, sizeof(buf), "nkeys must be 1 .. 2^32 - 1, got %zu", nkeys);
        return buf;
    }
    return nullptr;
}

// Makes the handle's device the current one.
inline int cbc_select_device(const tg_cbc_key* k) {
    int cur = -1;
    HIP_TRY(hipGetDevice(&cur));
    if (cur != k->device) HIP_TRY(hipSetDevice(k->device));
    return TG_OK;
}

static_assert(cbc::kRecOk == TG_REC_OK && cbc::kRecBadMac == TG_REC_BAD_MAC && cbc::kRecOverflow == TG_REC_OVERFLOW &&
                  cbc::kRecDecryptFailed == TG_REC_DECRYPT_FAILED,
              "cbc_record.h status codes");

constexpr int kCbcThreads = 512;
constexpr uint32_t kSiBase = 65536;                 // inverse S-box copies behind the Td block
constexpr size_t kSealLds = 65536;
constexpr size_t kOpenLds = 65536 + 256 * 16 * 4;

extern __shared__ __attribute__((aligned(16))) uint4 g_lds_cbc[];

// ---- Td0 and the inverse S-box, generated at compile time ----------------
struct TdTable {
    uint32_t td0[256];
    uint32_t si[256];
};

constexpr uint8_t gf_mul(uint8_t a, uint8_t b) {
    uint8_t p = 0;
    for (int k = 0; k < 8; ++k) {
        if (b & 1) p = (uint8_t)(p ^ a);
        a = xtime(a);
        b = (uint8_t)(b >> 1);
    }
    return p;
}

constexpr TdTable make_td() {
    const TeTable te = make_te();
    TdTable t = {};
    for (int v = 0; v < 256; ++v) t.si[(te.te0[v] >> 8) & 0xff] = (uint32_t)v;   // byte 1 of Te0[v] = S[v]
    for (int v = 0; v < 256; ++v) {
        const uint8_t s = (uint8_t)t.si[v];
        // column contribution of a row-0 byte: rows (0e s, 09 s, 0d s, 0b s), LE word
        t.td0[v] = (uint32_t)gf_mul(s, 0x0e) | ((uint32_t)gf_mul(s, 0x09) << 8) |
                   ((uint32_t)gf_mul(s, 0x0d) << 16) | ((uint32_t)gf_mul(s, 0x0b) << 24);
    }
    return t;
}

__constant__ TdTable c_td = make_td();

// InvMixColumns of one column (LE word of its bytes): the host's inverse schedule.
constexpr uint32_t inv_mix_column(uint32_t w) {
    const uint8_t a0 = (uint8_t)w, a1 = (uint8_t)(w >> 8), a2 = (uint8_t)(w >> 16), a3 = (uint8_t)(w >> 24);
    const uint8_t b0 = (uint8_t)(gf_mul(a0, 0x0e) ^ gf_mul(a1, 0x0b) ^ gf_mul(a2, 0x0d) ^ gf_mul(a3, 0x09));
    const uint8_t b1 = (uint8_t)(gf_mul(a0, 0x09) ^ gf_mul(a1, 0x0e) ^ gf_mul(a2, 0x0b) ^ gf_mul(a3, 0x0d));
    const uint8_t b2 = (uint8_t)(gf_mul(a0, 0x0d) ^ gf_mul(a1, 0x09) ^ gf_mul(a2, 0x0e) ^ gf_mul(a3, 0x0b));
    const uint8_t b3 = (uint8_t)(gf_mul(a0, 0x0b) ^ gf_mul(a1, 0x0d) ^ gf_mul(a2, 0x09) ^ gf_mul(a3, 0x0e));
    return (uint32_t)b0 | ((uint32_t)b1 << 8) | ((uint32_t)b2 << 16) | ((uint32_t)b3 << 24);
}

// The Td0 / Td2 copy block in stage_te's layout, then row x = 16 copies of Si[x].
__device__ __forceinline__ void stage_td(uint4* lds) {
#pragma unroll 4
    for (int e = threadIdx.x; e < 256 * 16; e += blockDim.x) {
        const uint32_t v = c_td.td0[e >> 4];
        const uint32_t w = (e & 8) ? rotl32(v, 16) : v;
        lds[e] = make_uint4(w, w, w, w);
    }
    for (int e = threadIdx.x; e < 256 * 4; e += blockDim.x) {
        const uint32_t v = c_td.si[e >> 2];
        lds[kSiBase / 16 + e] = make_uint4(v, v, v, v);
    }
}

template <int K>
__device__ __forceinline__ uint32_t Si(uint32_t x, uint32_t si4) {
    return lds_u32(kSiBase + (((x >> (8 * K)) & 0xffu) << 6) + si4);
}

// Last round of the inverse cipher: InvSubBytes of the InvShiftRows bytes.
__device__ __forceinline__ uint32_t inv_last(uint32_t sa, uint32_t sb, uint32_t sc, uint32_t sd, uint32_t rk,
                                             uint32_t si4) {
    return (Si<0>(sa, si4) | (Si<1>(sb, si4) << 8) | (Si<2>(sc, si4) << 16) | (Si<3>(sd, si4) << 24)) ^ rk;
}

// D_K(in) by the equivalent inverse cipher (FIPS-197 5.3.5; the reference's
// Rijndael.decrypt, rijndael.py:1040-1083): column c of a round reads row r
// from column c - r.
template <int NR, class RK>
__device__ __forceinline__ uint4 aes_dec_block(uint32_t lane4, uint32_t si4, const RK& dk, uint4 in) {
    const uint4 k0 = dk.get(0);
    uint32_t s0 = in.x ^ k0.x, s1 = in.y ^ k0.y, s2 = in.z ^ k0.z, s3 = in.w ^ k0.w;
#pragma unroll
    for (int r = 1; r < NR; ++r) {
        const uint4 k = dk.get(r);
        const uint32_t t0 = col(s0, s3, s2, s1, k.x, lane4);
        const uint32_t t1 = col(s1, s0, s3, s2, k.y, lane4);
        const uint32_t t2 = col(s2, s1, s0, s3, k.z, lane4);
        const uint32_t t3 = col(s3, s2, s1, s0, k.w, lane4);
        s0 = t0; s1 = t1; s2 = t2; s3 = t3;
    }
    const uint4 k = dk.get(NR);
    return make_uint4(inv_last(s0, s3, s2, s1, k.x, si4), inv_last(s1, s0, s3, s2, k.y, si4),
                      inv_last(s2, s1, s0, s3, k.z, si4), inv_last(s3, s2, s1, s0, k.w, si4));
}

// ---- global memory as cbc_record.h reads it -------------------------------
typedef uint32_t u32_a1 __attribute__((aligned(1)));

struct GMem {
    __device__ static __forceinline__ cbc::W4 ld16(const uint8_t* p) {
        const uint4 v = gload16u(p);
        return cbc::W4{v.x, v.y, v.z, v.w};
    }
    __device__ static __forceinline__ cbc::W4 ldn(const uint8_t* p, uint32_t n) {
        const uint4 v = load_partial(p, n);
        return cbc::W4{v.x, v.y, v.z, v.w};
    }
    __device__ static __forceinline__ uint32_t ld4(const uint8_t* p) {
#if defined(__HIP_DEVICE_COMPILE__)
        return *(const __attribute__((address_space(1))) u32_a1*)p;
#else
        return 0;
#endif
    }
    __device__ static __forceinline__ uint32_t ld1(const uint8_t* p) { return ((gptr_c)p)[0]; }
};

__device__ __forceinline__ void st4(uint8_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    *(__attribute__((address_space(1))) u32_a1*)p = v;
#endif
}

template <class H>
__device__ __forceinline__ void store_mac(uint8_t* p, const uint32_t dig[12]) {
#pragma unroll
    for (int k = 0; k < H::kHash / 4; ++k) st4(p + 4 * k, bswap32(dig[k]));
}

__device__ __forceinline__ void zero_bytes(uint8_t* p, uint32_t n, bool aligned) {   // n: multiple of 16
    const uint4 z = make_uint4(0, 0, 0, 0);
    for (uint32_t k = 0; k < n; k += 16) store16(p + k, z, aligned);
}

}  // namespace
}  // namespace tg

// keysetup.hip -- bulk TLS 1.3 key setup on the device (SURVEY.md section 8(f)
// row 4): many sessions' traffic keys and IVs derived and expanded in one
// pass, so a key table never round-trips through the host.
//
//   hkdf_kernel      HKDF-Expand-Label (tlslite/utils/cryptomath.py:155-173,
//                    HKDF_expand :146-153 with secureHMAC :128-132) of one
//                    secret per lane, SHA-256 or SHA-384, output <= one hash
//                    block (every record-layer use: "key", "iv",
//                    "traffic upd", "finished"; recordlayer.py:1268-1344).
//                    The HkdfLabel message (info || 0x01 and its SHA padding)
//                    is the same for every session, so the host lays it out
//                    once and each lane only hashes its own key blocks.
//   aes_setup_kernel AES key expansion (rijndael.py:922-993) per key, plus
//                    H = E_K(0^128) for GCM (aesgcm.py:45) in the layout the
//                    GCM kernels read (GcmKeyDev / GcmTableKey) or the CCM
//                    layout (AesKeyDev).
//   ghash_table_kernel  the 64 KiB single-key GHASH tables from H (the same
//                    tables host.cpp builds on the host).
//   rekey_kernel     entries of a LIVE key allocation rebuilt in place, from
//                    raw keys or through the TLS 1.3 derivation (install /
//                    KeyUpdate), fused: HKDF, key expansion, H and the
//                    entry's store in one lane (tg_key_replace_device,
//                    tg_sessions_rekey).
// The AES schedule, the entry store, the word helpers, the key loads, the
// digest stores and HKDF's T(1) (hkdf_t1, on the one HMAC core) are
// keysetup_dev.h's, shared with the TLS 1.0 - 1.2 key setup of tls12.hip and
// tls10.hip and the TLS 1.3 key schedule of tls13.hip.
#include "keysetup_dev.h"

namespace tg {
namespace {

template <class H>
__global__ __launch_bounds__(256) void hkdf_kernel(tg::HkdfMsg msg, const uint8_t* __restrict__ secrets, uint64_t n,
                            uint8_t* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    typename H::word key[16], st[8];
    key_from_row<H, H::kHash>(secrets + (uint64_t)H::kHash * i, key);
    hkdf_t1<H>(msg, key, st);
    store_digest_bytes<H>(st, out + (uint64_t)msg.outlen * i, msg.outlen);
}

template <int NK, int LAYOUT>
__global__ void aes_setup_kernel(const uint8_t* __restrict__ keys, uint64_t n, void* out) {
    __shared__ uint8_t sb[256];
    for (int k = threadIdx.x; k < 256; k += blockDim.x) sb[k] = c_sbox.s[k];
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t rk[60];
    expand_key<NK>(sb, keys + 4 * NK * i, rk);
    store_aes_entry<NK, LAYOUT>(sb, rk, out, i);
}

// ------------------------------------------------------- rekey in place --
// tg_key_replace_device / tg_sessions_rekey: lane j rebuilds entry slot[j]
// of a live key table (slot NULL: entry j); a slot that is not below nkeys is
// skipped, nothing read or written for it.
//   H = NoHash      the new raw key is row j of ``src`` (tg_key_replace_device)
//   H = Sha256/384  TLS 1.3 (recordlayer.py:1291-1316, :1325-1349): the
//       slot's secret is row j of ``src`` (install; copied to row s of
//       ``secrets`` when that is given) or row s of ``secrets`` advanced with
//       "traffic upd" and written back (update, src NULL); key and IV are
//       Expand-Label(secret, "key" / "iv"), the IV goes to row s of iv_table,
//       seq_next[s] = 0.  The raw key lives in registers only.
// NK = 4 / 8: AES-128 / -256 into layout 0 / 1 / 2 (aes_setup_kernel's);
// NK = 0: ChaCha20-Poly1305, the 32 key bytes as ChachaKeyDev (layout 3).
struct NoHash {
    using word = uint32_t;
    static constexpr int kHash = 0;
};

struct RekeyMsgs {
    tg::HkdfMsg upd, key, iv;
};

template <class H, int NK, int LAYOUT>
__global__ __launch_bounds__(256) void rekey_kernel(RekeyMsgs msgs, const uint32_t* __restrict__ slot,
                                                    const uint8_t* __restrict__ src, uint8_t* __restrict__ secrets,
                                                    uint8_t* __restrict__ iv_table, uint64_t* __restrict__ seq_next,
                                                    uint64_t n, uint64_t nkeys, void* out) {
    constexpr int KW = NK ? NK : 8;   // key words
    __shared__ uint8_t sb[256];
    if (NK) {
        for (int k = threadIdx.x; k < 256; k += blockDim.x) sb[k] = c_sbox.s[k];
        __syncthreads();
    }
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint64_t s = slot ? (uint64_t)slot[j] : j;
    if (s >= nkeys) return;
    uint32_t rk[60];   // rk[0 .. KW): the key as LE words of its bytes
    if constexpr (H::kHash == 0) {
#pragma unroll
        for (int k = 0; k < KW; ++k) rk[k] = load_u32u(src + 4 * KW * j + 4 * k);
    } else {
        using W = typename H::word;
        const uint8_t* from = src ? src + (uint64_t)H::kHash * j : secrets + (uint64_t)H::kHash * s;
        W sec[16], st[8];
        uint32_t d[12];
        key_from_row<H, H::kHash>(from, sec);
        if (!src) {   // KeyUpdate: the secret advances (uniform branch)
            hkdf_t1<H>(msgs.upd, sec, st);
#pragma unroll
            for (int k = 0; k < H::kStateOut; ++k) sec[k] = st[k];
        }
        if (secrets) store_digest<H>(sec, secrets + (uint64_t)H::kHash * s);
        hkdf_t1<H>(msgs.iv, sec, st);
        digest_words<H>(st, d);
        store_words<3>(d, iv_table + 12 * s);
        hkdf_t1<H>(msgs.key, sec, st);
        digest_words<H>(st, d);
#pragma unroll
        for (int k = 0; k < KW; ++k) rk[k] = bswap32(d[k]);
        if (seq_next) seq_next[s] = 0;
    }
    if constexpr (NK == 0) {
        ChachaKeyDev* o = static_cast<ChachaKeyDev*>(out) + s;
#pragma unroll
        for (int k = 0; k < 8; ++k) o->k[k] = rk[k];
    } else {
        expand_words<NK>(sb, rk);
        store_aes_entry<NK, LAYOUT>(sb, rk, out, s);
    }
}

// M_j[b] = XOR of H * x^(8j + t) over the bits t (MSB first) of b, in the
// block byte layout (host.cpp ghash_tables; aesgcm.py:8-14 bit order).
// Entry (0, 0) = 0 holds H on entry and is left alone here (every thread reads
// it); the launcher zeroes it afterwards, stream-ordered.
//
// The five kernels of this chain also rebuild a live single-key handle
// (rekey_kernel, layout 0).  GUARD: the rebuild's one-entry slot list; when it
// names another entry than 0 rekey_kernel wrote nothing, so the chain leaves
// the key alone too.  Key creation runs them with GUARD false.
template <bool GUARD>
__device__ __forceinline__ bool slot_skipped(const uint32_t* slot) {
    return GUARD && slot && *slot != 0;
}

template <bool GUARD>
__global__ void ghash_table_kernel(GcmKeyDev* key, const uint32_t* slot) {
    if (slot_skipped<GUARD>(slot)) return;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;   // entry j * 256 + b
    if (e == 0 || e >= kGhashEntries) return;
    const uint4 hw = key->ghash[0];                         // H as LE words of its bytes
    const uint32_t hv[4] = {hw.x, hw.y, hw.z, hw.w};
    key->ghash[e] = ghash_table_entry(hv, e);
}

// GcmKeyDev::ghash64: the same tables for H^64 (after hpow_kernel).
template <bool GUARD>
__global__ void ghash64_table_kernel(GcmKeyDev* key, const uint32_t* slot) {
    if (slot_skipped<GUARD>(slot)) return;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= kGhashEntries) return;
    const uint4 p = key->hpow[63];                          // normal order -> byte layout
    const uint32_t hv[4] = {gcm_word_to_norm(p.x), gcm_word_to_norm(p.y), gcm_word_to_norm(p.z),
                            gcm_word_to_norm(p.w)};
    key->ghash64[e] = ghash_table_entry(hv, e);
}

// GcmKeyDev::ghash8: the same tables for H^8 (after hpow_kernel).
template <bool GUARD>
__global__ void ghash8_table_kernel(GcmKeyDev* key, const uint32_t* slot) {
    if (slot_skipped<GUARD>(slot)) return;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= kGhashEntries) return;
    const uint4 p = key->hpow[7];
    const uint32_t hv[4] = {gcm_word_to_norm(p.x), gcm_word_to_norm(p.y), gcm_word_to_norm(p.z),
                            gcm_word_to_norm(p.w)};
    key->ghash8[e] = ghash_table_entry(hv, e);
}

// GcmKeyDev::hpow: thread e computes H^(e+1) by square and multiply from H,
// which aes_setup_kernel parked in ghash[0] (the table kernel leaves entry 0
// alone and the launcher zeroes it after this kernel, stream-ordered).
template <bool GUARD>
__global__ void hpow_kernel(GcmKeyDev* key, const uint32_t* slot) {
    if (slot_skipped<GUARD>(slot)) return;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= kHPow) return;
    const uint4 hw = key->ghash[0];
    const uint32_t hn[4] = {gcm_word_to_norm(hw.x), gcm_word_to_norm(hw.y), gcm_word_to_norm(hw.z),
                            gcm_word_to_norm(hw.w)};
    uint32_t r[4] = {1, 0, 0, 0}, x[4] = {hn[0], hn[1], hn[2], hn[3]};
    for (uint32_t n = (uint32_t)e + 1; n; n >>= 1) {
        if (n & 1) gf_mul_norm(r, x, r);
        if (n > 1) gf_mul_norm(x, x, x);
    }
    key->hpow[e] = make_uint4(r[0], r[1], r[2], r[3]);
}

// GcmKeyDev::bs8mask from the round keys (after aes_setup_kernel, layout 0):
// 32 (NR + 1) <= 480 planes.
template <bool GUARD>
__global__ void bs_mask_kernel(GcmKeyDev* key, const uint32_t* slot) {
    if (slot_skipped<GUARD>(slot)) return;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    const int nr = (int)key->rounds;
    if (e < 32 * (nr + 1)) key->bs8mask[e] = bs8::mask_word(key->rk, e);
    if (e < 15 * 32) key->bs8rows[e] = bs8_row_word(key->rk, nr, e);   // the hybrid's key rows
    if (e < 64) key->rkrot[e] = rkrot_word(key->rk, nr, e);
    // the rebuild's last kernel un-parks H itself (creation: the launcher's memset)
    if (GUARD && e == 0) key->ghash[0] = make_uint4(0, 0, 0, 0);
}

// Everything of a GcmKeyDev behind rk and H (parked in ghash[0]).
template <bool GUARD>
int launch_single_chain(GcmKeyDev* k, const uint32_t* slot, hipStream_t s) {
    hipLaunchKernelGGL(ghash_table_kernel<GUARD>, dim3(kGhashEntries / 256), dim3(256), 0, s, k, slot);
    if (hipGetLastError() != hipSuccess) return TG_EHIP;
    hipLaunchKernelGGL(hpow_kernel<GUARD>, dim3((kHPow + 255) / 256), dim3(256), 0, s, k, slot);
    if (hipGetLastError() != hipSuccess) return TG_EHIP;
    hipLaunchKernelGGL(ghash64_table_kernel<GUARD>, dim3(kGhashEntries / 256), dim3(256), 0, s, k, slot);
    if (hipGetLastError() != hipSuccess) return TG_EHIP;
    hipLaunchKernelGGL(ghash8_table_kernel<GUARD>, dim3(kGhashEntries / 256), dim3(256), 0, s, k, slot);
    if (hipGetLastError() != hipSuccess) return TG_EHIP;
    hipLaunchKernelGGL(bs_mask_kernel<GUARD>, dim3((15 * 32 + 255) / 256), dim3(256), 0, s, k, slot);
    return hipGetLastError() == hipSuccess ? TG_OK : TG_EHIP;
}

}  // namespace
}  // namespace tg

int tg_launch_hkdf(int hashlen, const tg::HkdfMsg& msg, const uint8_t* secrets, uint64_t n,
                   uint8_t* out, hipStream_t s) {
    const unsigned blocks = (unsigned)((n + 255) / 256);
    if (hashlen == 32)
        hipLaunchKernelGGL(tg::hkdf_kernel<tg::Sha256>, dim3(blocks), dim3(256), 0, s, msg, secrets,
                           n, out);
    else if (hashlen == 48)
        hipLaunchKernelGGL(tg::hkdf_kernel<tg::Sha384>, dim3(blocks), dim3(256), 0, s, msg, secrets,
                           n, out);
    else
        return TG_EINVAL;
    return hipGetLastError() == hipSuccess ? TG_OK : TG_EHIP;
}

// layout: 0 = GcmKeyDev (n == 1, GHASH tables built too), 1 = GcmTableKey, 2 = AesKeyDev
int tg_launch_aes_setup(int keylen, int layout, const uint8_t* keys, uint64_t n, void* out,
                        hipStream_t s) {
    const unsigned blocks = (unsigned)((n + 255) / 256);
#define TG_AES_SETUP(NK, L)                                                                        \
    hipLaunchKernelGGL((tg::aes_setup_kernel<NK, L>), dim3(blocks), dim3(256), 0, s, keys, n, out)
    if (keylen == 16) {
        if (layout == 0) TG_AES_SETUP(4, 0);
        else if (layout == 1) TG_AES_SETUP(4, 1);
        else TG_AES_SETUP(4, 2);
    } else if (keylen == 32) {
        if (layout == 0) TG_AES_SETUP(8, 0);
        else if (layout == 1) TG_AES_SETUP(8, 1);
        else TG_AES_SETUP(8, 2);
    } else {
        return TG_EINVAL;
    }
#undef TG_AES_SETUP
    if (hipGetLastError() != hipSuccess) return TG_EHIP;
    if (layout == 0) {
        tg::GcmKeyDev* k = static_cast<tg::GcmKeyDev*>(out);
        if (int rc = tg::launch_single_chain<false>(k, nullptr, s)) return rc;
        if (hipMemsetAsync(&k->ghash[0], 0, sizeof(uint4), s) != hipSuccess) return TG_EHIP;
    }
    return TG_OK;
}

int tg_launch_rekey(int hashlen, int alg_keylen, int layout, const tg::HkdfMsg* msgs, const uint32_t* slot,
                    const uint8_t* src, uint8_t* secrets, uint8_t* iv_table, uint64_t* seq_next, uint64_t n,
                    uint64_t nkeys, void* out, hipStream_t s) {
    using namespace tg;
    const unsigned blocks = (unsigned)((n + 255) / 256);
    RekeyMsgs m{};
    if (hashlen) {
        m.upd = msgs[0];
        m.key = msgs[1];
        m.iv = msgs[2];
    }
#define TG_REKEY(H, NK, L)                                                                          \
    hipLaunchKernelGGL((rekey_kernel<H, NK, L>), dim3(blocks), dim3(256), 0, s, m, slot, src, secrets, \
                       iv_table, seq_next, n, nkeys, out)
#define TG_REKEY_HASH(NK, L)                  \
    do {                                      \
        if (hashlen == 0) TG_REKEY(NoHash, NK, L);      \
        else if (hashlen == 32) TG_REKEY(Sha256, NK, L); \
        else if (hashlen == 48) TG_REKEY(Sha384, NK, L); \
        else return TG_EINVAL;                \
    } while (0)
    if (layout == 3) {   // ChaCha20-Poly1305
        TG_REKEY_HASH(0, 3);
    } else if (alg_keylen == 16) {
        if (layout == 0) TG_REKEY_HASH(4, 0);
        else if (layout == 1) TG_REKEY_HASH(4, 1);
        else TG_REKEY_HASH(4, 2);
    } else if (alg_keylen == 32) {
        if (layout == 0) TG_REKEY_HASH(8, 0);
        else if (layout == 1) TG_REKEY_HASH(8, 1);
        else TG_REKEY_HASH(8, 2);
    } else {
        return TG_EINVAL;
    }
#undef TG_REKEY_HASH
#undef TG_REKEY
    if (hipGetLastError() != hipSuccess) return TG_EHIP;
    if (layout == 0) return launch_single_chain<true>(static_cast<GcmKeyDev*>(out), slot, s);
    return TG_OK;
}

int tg_launch_single_rebuild(void* key, const uint32_t* slot, hipStream_t s) {
    return tg::launch_single_chain<true>(static_cast<tg::GcmKeyDev*>(key), slot, s);
}


// bs8_win_check.cpp -- CPU check of the bitsliced cipher's 256-counter window
// path (tlslite-ng_amd/csrc/aes_bs8.h: v_word, win_words, a_plane, win_sel7,
// win_rounds, rounds_from) against bs8::encrypt and the C oracle's AES block
// cipher (oracle/aead_oracle.c, rijndael.py restated).  TEST INFRASTRUCTURE
// ONLY.  Built and run by tests/test_bs8_win_host.py:
//   g++ -O2 -I tlslite-ng_amd/csrc -I oracle tests/native/bs8_win_check.cpp oracle/aead_oracle.c
// For AES-128 and AES-256, plain and folded key planes, every rho 0..7 and
// every batch beta 0..1022 in order (so the two B buffers are filled and
// swapped as the kernel does it: the next window's constants computed at
// beta % 4 = 3, selected into block 7 of the lanes that cross, current from
// beta + 1 on), the eight keystream blocks nonce || be32(2 + rho + 64 beta +
// 8 j) must equal both; then batches at and above the 2^16 limit through the
// full-round fallback (first_state + round1 + rounds_from).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "aead_oracle.h"
#include "aes_bs8.h"

static uint8_t S[256];
static uint8_t xt(uint8_t a) { return (uint8_t)((a << 1) ^ ((a & 0x80) ? 0x1b : 0)); }
static void make_sbox() {
    uint8_t p = 1, q = 1;
    S[0] = 0x63;
    do {
        p = p ^ (uint8_t)(p << 1) ^ (p & 0x80 ? 0x1b : 0);
        q ^= q << 1; q ^= q << 2; q ^= q << 4;
        if (q & 0x80) q ^= 0x09;
        const uint8_t x = q ^ (uint8_t)((q << 1) | (q >> 7)) ^ (uint8_t)((q << 2) | (q >> 6)) ^
                          (uint8_t)((q << 3) | (q >> 5)) ^ (uint8_t)((q << 4) | (q >> 4));
        S[p] = x ^ 0x63;
    } while (p != 1);
}
static void expand(const uint8_t* key, int nk, uint8_t* rk) {   // FIPS-197 key expansion
    const int nr = nk + 6, tot = 4 * (nr + 1);
    memcpy(rk, key, 4 * nk);
    uint8_t rc = 1;
    for (int i = nk; i < tot; ++i) {
        uint8_t t[4];
        memcpy(t, rk + 4 * (i - 1), 4);
        if (i % nk == 0) {
            const uint8_t u = t[0];
            t[0] = S[t[1]] ^ rc; t[1] = S[t[2]]; t[2] = S[t[3]]; t[3] = S[u];
            rc = xt(rc);
        } else if (nk > 6 && i % nk == 4) {
            for (int k = 0; k < 4; ++k) t[k] = S[t[k]];
        }
        for (int k = 0; k < 4; ++k) rk[4 * i + k] = rk[4 * (i - nk) + k] ^ t[k];
    }
}
static uint32_t le(const uint8_t* p) { return p[0] | p[1] << 8 | p[2] << 16 | (uint32_t)p[3] << 24; }

struct SboxTab {
    uint32_t operator()(uint32_t x) const { return S[x & 0xff]; }
};

struct FoldedRows {   // the device's KeyPlanesVmemFolded, read from bs8mask order
    static constexpr bool kFolded = true;
    const uint32_t* w;
    tg::bs8::Word4 row4(int r, int b) const {
        return tg::bs8::word4(w[(4 * r) * 8 + b], w[(4 * r + 1) * 8 + b], w[(4 * r + 2) * 8 + b],
                              w[(4 * r + 3) * 8 + b]);
    }
};

struct WinBuf {   // one record's B planes, as a wave keeps them in LDS
    uint32_t b[4][8];
};

struct WinPlanes {   // the kernel's provider: rows 0..3 of bit b, block 7 of a crossing lane from the next window
    const WinBuf *cur, *nxt;
    uint32_t m7;
    bool cross;
    tg::bs8::Word4 operator()(int b) const {
        uint32_t v[4];
        for (int i = 0; i < 4; ++i)
            v[i] = cross ? tg::bs8::win_sel7(cur->b[i][b], nxt->b[i][b], m7) : cur->b[i][b];
        return tg::bs8::word4(v[0], v[1], v[2], v[3]);
    }
};

static void fill(WinBuf* dst, const uint32_t* rkw, const uint32_t n[3], uint32_t win, uint32_t* a) {
    uint32_t A, B[4];
    tg::bs8::win_words(rkw, n[0], n[1], n[2], win, SboxTab(), A, B);
    for (int e = 0; e < 32; ++e) dst->b[e >> 3][e & 7] = tg::bs8::rec_plane(B, e);
    for (uint32_t b = 0; b < 8; ++b) a[b] = tg::bs8::a_plane(A, b);
}

template <int NR, bool FOLD>
static int run(int klen, unsigned seed) {
    srand(seed);
    uint8_t key[32], rk[16 * 15], nonce[12];
    for (int i = 0; i < klen; ++i) key[i] = (uint8_t)rand();
    for (int i = 0; i < 12; ++i) nonce[i] = (uint8_t)rand();
    expand(key, klen / 4, rk);
    uint32_t rkw[60];
    for (int q = 0; q < 4 * (NR + 1); ++q) rkw[q] = le(rk + 4 * q);
    // heap copies, exactly sized: the sanitizer build sees any read past them
    uint32_t* planes = (uint32_t*)malloc(sizeof(uint32_t) * 32 * (NR + 1));
    uint32_t* folded = (uint32_t*)malloc(sizeof(uint32_t) * 32 * (NR + 1));
    uint32_t* V = (uint32_t*)malloc(sizeof(uint32_t) * 256);
    for (int e = 0; e < 32 * (NR + 1); ++e) planes[e] = tg::bs8::mask_word(rkw, e);
    for (int e = 0; e < 32 * (NR + 1); ++e)
        folded[e] = (e >> 5) >= 1 && (e >> 5) < NR ? tg::bs8_fold_word(rkw, e) : planes[e];
    for (uint32_t e = 0; e < 256; ++e)   // V[rho][bm] word b at index 32 rho + 8 bm + b
        V[e] = tg::bs8::v_word(rkw[3] >> 24, e >> 5, (e >> 3) & 3, e & 7, SboxTab());
    const tg::bs8::KeyPlanes km{planes};
    const FoldedRows kf{folded};
    const uint32_t n[3] = {le(nonce), le(nonce + 4), le(nonce + 8)};
    const uint32_t u[4] = {n[0] ^ rkw[0], n[1] ^ rkw[1], n[2] ^ rkw[2], rkw[3]};
    int bad = 0, checked = 0, crossed = 0, refreshed = 0;
    auto check = [&](uint32_t rho, uint32_t beta, uint32_t (*w)[8], const char* what) {
        for (int j = 0; j < 8; ++j) {
            const uint32_t ctr = 2 + rho + 64 * beta + 8 * (uint32_t)j;
            uint8_t blk[16], want[16];
            memcpy(blk, nonce, 12);
            blk[12] = (uint8_t)(ctr >> 24); blk[13] = (uint8_t)(ctr >> 16);
            blk[14] = (uint8_t)(ctr >> 8); blk[15] = (uint8_t)ctr;
            oracle_aes_encrypt_block(key, (size_t)klen, blk, want);
            for (int q = 0; q < 4; ++q) {
                const uint32_t got = w[q][j] ^ rkw[4 * NR + q] ^ 0x63636363u;
                if (got != le(want + 4 * q)) {
                    if (bad < 5)
                        fprintf(stderr, "%s NR=%d rho=%u beta=%u j=%d q=%d got %08x want %08x\n", what, NR, rho,
                                beta, j, q, got, le(want + 4 * q));
                    ++bad;
                }
            }
            ++checked;
        }
    };
    for (uint32_t rho = 0; rho < 8; ++rho) {
        const uint32_t c0 = 2 + rho;
        uint32_t lanec[6], kmask;
        tg::bs8::lane_consts<3>(c0, lanec, kmask);
        WinBuf buf[2];
        uint32_t a[8];
        for (uint32_t beta = 0; beta <= 1022; ++beta) {
            const bool cross = (beta & 3u) == 3u;
            if (beta == 0) { fill(&buf[0], rkw, n, 0, a); ++refreshed; }
            if (cross) { fill(&buf[((beta >> 2) + 1) & 1], rkw, n, (beta >> 2) + 1, a); ++refreshed; }
            const WinBuf& cur = buf[(beta >> 2) & 1];
            const WinBuf& nxt = buf[((beta >> 2) + 1) & 1];
            uint32_t s[4][8], w[4][8], x[8];
            const uint32_t m7 = tg::bs8::win_m7(kmask);
            if (cross && m7) ++crossed;
            for (int b = 0; b < 8; ++b) x[b] = a[b] ^ V[32 * rho + 8 * (beta & 3u) + b];
            tg::bs8::win_rounds(x, WinPlanes{&cur, &nxt, m7, cross}, s);
            if (FOLD)
                tg::bs8::rounds_from<NR>(s, kf, w, 3);
            else
                tg::bs8::rounds_from<NR>(s, km, w, 3);
            check(rho, beta, w, "window");
            // and the same blocks by encrypt() on the first state
            uint32_t s2[4][8], w2[4][8];
            tg::bs8::first_state(u, c0, beta, false, s2);
            if (FOLD)
                tg::bs8::encrypt<NR>(s2, kf, w2);
            else
                tg::bs8::encrypt<NR>(s2, km, w2);
            if (memcmp(w, w2, sizeof(w)) != 0) {
                if (bad < 5) fprintf(stderr, "window != encrypt NR=%d rho=%u beta=%u\n", NR, rho, beta);
                ++bad;
            }
        }
        // at and above the 2^16 limit: the kernel's full-round fallback
        const uint32_t his[] = {1023, 1024, 1025, 2047, 65535, 65536, 0x3ffffe};
        for (uint32_t beta : his) {
            uint32_t s[4][8], w[4][8];
            tg::bs8::first_state(u, c0, beta, true, s);
            if (FOLD) {
                tg::bs8::round1(s, kf);
                tg::bs8::rounds_from<NR>(s, kf, w, 2);
            } else {
                tg::bs8::round1(s, km);
                tg::bs8::rounds_from<NR>(s, km, w, 2);
            }
            check(rho, beta, w, "fallback");
        }
    }
    free(planes);
    free(folded);
    free(V);
    printf("NR=%d fold=%d seed=%u blocks=%d crossing_batches=%d refreshes=%d bad=%d\n", NR, (int)FOLD, seed,
           checked, crossed, refreshed, bad);
    return bad;
}

int main() {
    make_sbox();
    int bad = 0;
    bad += run<10, false>(16, 1);
    bad += run<10, true>(16, 2);
    bad += run<14, false>(32, 101);
    bad += run<14, true>(32, 102);
    printf(bad ? "FAIL\n" : "OK\n");
    return bad != 0;
}

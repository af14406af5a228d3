// framing.hip -- host orchestration of the record-framing calls (kernels:
// records.hip, sessions.hip): per-call scratch, the prep kernel, the AEAD
// batch over what it laid out, and the finish kernel.
#include <cstring>

#include "api.h"
#include "common.h"
#include "dispatch.h"
#include "keys.h"
#include "runtime.h"

namespace tg {
namespace {

// Stream-ordered scratch for the record-framing calls.
int records_scratch(uint64_t n, hipStream_t st, Scratch& a, RecScratch& s) {
    const size_t per = 8 + 8 + 4 + 12 + 16 + 4 + 1 + 1;
    if (a.alloc(per * n + 64 + 64 + 64)) return fail(TG_EHIP, "scratch allocation failed");
    s.in_abs = a.take<uint64_t>(8 * n, 8);
    s.out_abs = a.take<uint64_t>(8 * n, 8);
    s.aad = a.take<uint8_t>(16 * n, 16);
    s.len = a.take<uint32_t>(4 * n, 4);
    s.aad_len = a.take<uint32_t>(4 * n, 4);
    s.nonce = a.take<uint8_t>(12 * n, 1);
    s.st = a.take<uint8_t>(n, 1);
    s.aead_st = a.take<uint8_t>(n, 1);
    s.dummy = a.take<uint8_t>(64, 64);
    s.sink = a.take<uint8_t>(64, 64);
    HIP_TRY(hipMemsetAsync(s.dummy, 0, 32, st));
    return TG_OK;
}

// _getNonce (recordlayer.py:522-534) then asserts a 12-byte nonce (:556):
// TLS 1.3 XORs a 12-byte IV; TLS 1.2 AES-GCM / AES-CCM append the 8-byte
// sequence number to a 4-byte IV; TLS 1.2 ChaCha XORs a 12-byte IV (RFC
// 7905) or appends to a 4-byte one (draft-00).
int check_framing(const tg_key* k, uint32_t version, uint32_t ivl) {
    if (version != TG_TLS12 && version != TG_TLS13)
        return fail(TG_EINVAL, "version must be TG_TLS12 or TG_TLS13");
    const bool chacha = k->alg == TG_CHACHA20_POLY1305;
    const bool ok = version == TG_TLS13 ? ivl == 12 : chacha ? (ivl == 12 || ivl == 4) : ivl == 4;
    if (!ok)
        return fail(TG_EINVAL, "fixed IV of %u bytes gives no 12-byte nonce for this suite "
                    "(TLS 1.3: 12; TLS 1.2 AES: 4; TLS 1.2 ChaCha: 12 or 4)", ivl);
    return TG_OK;
}

// The device arrays tg_records and tg_session_records have in common.
template <class R>
bool null_array(const R& r, bool seal) {
    return !r.data || !r.data_off || !r.data_len || !r.ctype || !r.wire || !r.wire_off || !r.wire_len ||
           (!seal && !r.status);
}

// The prep kernel, the AEAD batch between the framing kernels -- payloads,
// nonces and AAD rows as the prep kernel laid them out -- and, on open, the
// finish kernel.  prep(aes) and finish() launch the call's own kernels.
template <class R, class Prep, class Finish>
int frame(tg_key* k, const R& r, const uint32_t* key_idx, bool seal, const RecScratch& s, hipStream_t st,
          Prep prep, Finish finish) {
    int rc;
    const bool aes = k->alg != TG_CHACHA20_POLY1305;   // "aes" in name (recordlayer.py:561, :783)
    if ((rc = prep(aes))) return fail(rc, "framing launch failed");
    tg_batch b;
    memset(&b, 0, sizeof(b));
    b.n = r.n;
    b.len = s.len;
    b.nonce = s.nonce;
    b.aad = s.aad;
    b.aad_stride = 16;
    b.aad_len = s.aad_len;
    b.out_off = s.out_abs;          // absolute addresses: out base NULL
    b.key_idx = key_idx;
    if (seal) {
        b.in = r.data;
        b.in_off = r.data_off;
    } else {
        b.in_off = s.in_abs;
        b.status = s.aead_st;
    }
    if ((rc = launch(k, b, !seal, st))) return fail(rc, "AEAD launch failed");
    if (!seal && (rc = finish())) return fail(rc, "finish launch failed");
    return TG_OK;
}

// The scratch goes back behind the launches; a failed release is the call's
// error when nothing failed before it.
int released(int rc, Scratch& a) {
    return a.release() && !rc ? fail(TG_EHIP, "scratch release failed") : rc;
}

}  // namespace

int records(tg_key* k, const tg_records* r, void* stream, bool seal) {
    if (!k || !r) return fail(TG_EINVAL, "null argument");
    if (r->n == 0) return TG_OK;
    if (k->nkeys != 1) return fail(TG_EINVAL, "record framing needs a single-key handle");
    int rc = check_framing(k, r->version, r->fixed_iv_len);
    if (rc) return rc;
    if (null_array(*r, seal)) return fail(TG_EINVAL, "null device array");
    if ((rc = select_device(k))) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    Scratch scratch(st);
    RecScratch s;
    if ((rc = records_scratch(r->n, st, scratch, s))) return rc;
    rc = frame(k, *r, nullptr, seal, s, st,
               [&](bool aes) { return tg_launch_records_prep(*r, seal, aes, k->taglen, s, st); },
               [&] { return tg_launch_records_finish(*r, s, st); });
    return released(rc, scratch);
}

// tg_seal_session_records / tg_open_session_records: the framing of
// records() with a session per record.  Argument errors come first, before
// any HIP call.  Counter mode runs the rank pass (sessions.hip) into a
// per-call array of sequence numbers; explicit mode reads the caller's.
int session_records(tg_key* k, const tg_session_records* r, void* stream, bool seal) {
    if (!r) return fail(TG_EINVAL, "null argument");
    if ((r->seq != nullptr) == (r->seq_next != nullptr))
        return fail(TG_EINVAL, "exactly one of seq (explicit numbers) and seq_next (per-session "
                    "counters) must be given, got %s", r->seq ? "both" : "neither");
    // one limit for both modes, checked before anything is launched: the
    // rank pass and the key-table plans index records with 32 bits
    if (r->n > 0xfffffffeull) return fail(TG_EINVAL, "at most 2^32 - 2 records per call");
    if (!k) return fail(TG_EINVAL, "null argument");
    if (r->n == 0) return TG_OK;
    if (!r->iv_table || !r->session || null_array(*r, seal)) return fail(TG_EINVAL, "null device array");
    if (r->nsessions != k->nkeys)
        return fail(TG_EINVAL, "nsessions (%llu) must equal the key handle's nkeys (%llu)",
                    (unsigned long long)r->nsessions, (unsigned long long)k->nkeys);
    int rc = check_framing(k, r->version, r->fixed_iv_len);
    if (rc) return rc;
    if ((rc = select_device(k))) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    Scratch scratch(st), seq_scratch(st);
    RecScratch s;
    if ((rc = records_scratch(r->n, st, scratch, s))) return rc;
    const uint64_t* seq = r->seq;
    if (r->seq_next) {
        size_t rank_bytes = 0;
        if ((rc = tg_session_rank(nullptr, r->n, r->nsessions, nullptr, nullptr, nullptr, &rank_bytes, st)))
            return fail(rc, "rank pass sizing failed");
        if (seq_scratch.alloc(align_up(r->n * sizeof(uint64_t), 256) + rank_bytes))
            return fail(TG_EHIP, "scratch allocation failed");
        uint64_t* ranked = seq_scratch.take<uint64_t>(r->n * sizeof(uint64_t), 256);
        if ((rc = tg_session_rank(r->session, r->n, r->nsessions, r->seq_next, ranked,
                                  seq_scratch.take<uint8_t>(rank_bytes, 256), &rank_bytes, st)))
            return fail(rc, "rank pass launch failed");
        seq = ranked;
    }
    // launch() takes no key index for a single key; the prep kernel has
    // already emptied the records whose session is out of range
    rc = frame(k, *r, k->nkeys > 1 ? r->session : nullptr, seal, s, st,
               [&](bool aes) { return tg_launch_session_records_prep(*r, seq, seal, aes, k->taglen, s, st); },
               [&] { return tg_launch_session_records_finish(*r, s, st); });
    return released(released(rc, seq_scratch), scratch);
}

}  // namespace tg

// api.h -- what the files behind the C ABI share with api.hip: the error
// text of tg_last_error() and the calls behind the AEAD entry points.
#pragma once
#include <hip/hip_runtime.h>

#include "tlsgpu.h"

namespace tg {

// Records the calling thread's tg_last_error() text and returns ``code``.
int fail(int code, const char* fmt, ...);

#define HIP_TRY(expr)                                                                 \
    do {                                                                              \
        hipError_t e_ = (expr);                                                       \
        if (e_ != hipSuccess)                                                         \
            return tg::fail(TG_EHIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_),  \
                            __FILE__, __LINE__);                                      \
    } while (0)

// tg_seal / tg_open and tg_seal_batch / tg_open_batch (aead.hip).
int single(tg_key* k, const uint8_t* nonce, size_t noncelen, const uint8_t* aad, size_t aadlen,
           const uint8_t* in, size_t inlen, uint8_t* out, bool open);
int batch(tg_key* k, const tg_batch* b, void* stream, bool open);
// tg_*_records and tg_*_session_records (framing.hip).
int records(tg_key* k, const tg_records* r, void* stream, bool seal);
int session_records(tg_key* k, const tg_session_records* r, void* stream, bool seal);

}  // namespace tg

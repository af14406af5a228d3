// dispatch.h -- kernel selection (dispatch.hip): the AEAD kernels for batch
// ``b`` under key ``k`` on stream ``s``.
#pragma once
#include <hip/hip_runtime.h>

#include "tlsgpu.h"

namespace tg {

int launch(tg_key* k, const tg_batch& b, bool open, hipStream_t s);

}  // namespace tg

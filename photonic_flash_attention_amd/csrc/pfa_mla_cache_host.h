// pfa_mla_cache_host.h -- what the two units of include/pfa_hip_mla_cache.h share (pfa_mla_decode_fp8_capi.hip, pfa_mla_append_capi.hip):
// the field rules of pfa_mla_kv_quant.  Internal.
#pragma once
#include "pfa_hip_mla_cache.h"
#include "pfa_host.h"

namespace pfa {
namespace mla {

// include/pfa_hip_mla_cache.h, pfa_mla_kv_quant, in the order the errors are reported.  pointers = false stops in front of the rules about
// the descale pointer (the workspace query takes none).
inline int check_kv_quant(const pfa_mla_kv_quant* q, bool pointers = true) {
    if (!q) return PFA_ERR_NULL;
    if (q->size != sizeof(pfa_mla_kv_quant)) return PFA_ERR_STRUCT_SIZE;
    if (q->flags != 0 || q->reserved != 0) return PFA_ERR_FLAGS;
    if (q->kv_dtype != PFA_DTYPE_FP8_E4M3) return PFA_ERR_DTYPE;
    if (!pointers) return PFA_OK;
    if (!q->kv_descale) return PFA_ERR_NULL;
    if (!aligned4(q->kv_descale)) return PFA_ERR_ALIGN;
    if (q->descale_stride_b < 0) return PFA_ERR_STRIDE;
    return PFA_OK;
}

}  // namespace mla
}  // namespace pfa

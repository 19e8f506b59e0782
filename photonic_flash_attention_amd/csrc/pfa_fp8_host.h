// pfa_fp8_host.h -- what the entry-point files of the FP8 KV cache share (pfa_kv_append_fp8_capi.hip and, through
// pfa_cache_modes.h, pfa_decode_fp8_capi.hip and the two pfa_prefill*_fp8_capi.hip): the field rules of pfa_fa3_kv_quant and of an argument block's cache tensors
// when they hold one-byte elements, and the refusal of a window.  Internal.
#pragma once
#include "pfa_host.h"

namespace pfa {

// include/pfa_hip.h, pfa_fa3_kv_quant, in the order the errors are reported; the caller has checked `a` and a->size.  pointers = false
// stops in front of the rules about pointers and strides (the workspace query takes none).
template <typename Args>
inline int check_kv_quant(const pfa_fa3_kv_quant* q, const Args* a, bool pointers = true) {
    if (!q) return PFA_ERR_NULL;
    if (q->size != sizeof(pfa_fa3_kv_quant)) return PFA_ERR_STRUCT_SIZE;
    if (q->flags != 0 || q->reserved != 0) return PFA_ERR_FLAGS;
    if (q->kv_dtype != PFA_DTYPE_FP8_E4M3) return PFA_ERR_DTYPE;
    if (!pointers) return PFA_OK;
    if (!q->k_descale || !q->v_descale) return PFA_ERR_NULL;
    if (!aligned4(q->k_descale) || !aligned4(q->v_descale)) return PFA_ERR_ALIGN;
    if (q->descale_stride_b != 0 && q->descale_stride_b < a->Hkv) return PFA_ERR_STRIDE;
    // one-byte elements: a 16-byte load or store needs strides of 16
    if (!multiples_of(16, {a->k_stride_b, a->k_stride_h, a->k_stride_s, a->v_stride_b, a->v_stride_h, a->v_stride_s}) || !kv_rows_forward(a))
        return PFA_ERR_STRIDE;
    if (!aligned16(a->k_cache) || !aligned16(a->v_cache)) return PFA_ERR_ALIGN;
    return PFA_OK;
}

// An FP8 cache takes no window (PFA_ERR_FLAGS; the workspace query answers 0): asked in front of the 16-bit call's own rules, so only
// of a block whose size says that `window` is where this library reads it.
inline bool fp8_refuses_window(const pfa_fa3_cache_ext* ext) { return ext && ext->size == sizeof(pfa_fa3_cache_ext) && ext->window > 0; }

}  // namespace pfa

// pfa_host.h -- host-side glue the entry points of libpfa_hip.so share (internal: nothing here is exported).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "pfa_hip.h"

namespace pfa {

void set_last_hip_error(int e);   // pfa_capi.hip: what pfa_last_hip_error() reports

// A failed HIP call: keep its code (in *sink if given, else for pfa_last_hip_error) and clear HIP's sticky error.
inline bool hip_failed(hipError_t e, int* sink = nullptr) {
    if (e == hipSuccess) return false;
    if (sink) *sink = (int)e;
    else set_last_hip_error((int)e);
    (void)hipGetLastError();
    return true;
}

// Makes `dev` the current device for the scope and puts the caller's device back on every way out.
class DeviceScope {
    int prev_ = -1;
    bool switched_ = false;
    hipError_t err_;

public:
    explicit DeviceScope(int dev) {
        err_ = hipGetDevice(&prev_);
        if (err_ == hipSuccess && prev_ != dev) {
            err_ = hipSetDevice(dev);
            switched_ = err_ == hipSuccess;
        }
    }
    ~DeviceScope() {
        if (switched_) (void)hipSetDevice(prev_);
    }
    DeviceScope(const DeviceScope&) = delete;
    DeviceScope& operator=(const DeviceScope&) = delete;
    hipError_t error() const { return err_; }   // of the switch; a launch behind a failed one is PFA_ERR_DEVICE
};

// The mask fields of a kernel parameter block (FwdParams, F32Params, WeightsParams): the element mask with its four byte
// strides, or the [B, Sk] key mask as (stride, 0, 0, 1), or null.
template <typename Params>
inline void fill_mask(Params& p, const pfa_fa3_args* a) {
    if (a->mask) {
        p.mask = a->mask; p.m_sb = a->mask_stride_b; p.m_sh = a->mask_stride_h; p.m_sq = a->mask_stride_q; p.m_sk = a->mask_stride_k;
    } else {
        p.mask = a->key_mask; p.m_sb = a->key_mask_stride_b; p.m_sh = 0; p.m_sq = 0; p.m_sk = 1;
    }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// The paging fields every call over a KV cache carries (include/pfa_hip.h, pfa_fa3_decode_args): all set, or all zero.
inline int check_paging(const int32_t* block_table, int64_t block_table_stride_b, int32_t page_size, int32_t num_pages, int32_t Smax) {
    if (block_table) {
        // Smax is the logical capacity max_pages * page_size; a 64-key tile must lie inside one page
        if (page_size <= 0 || page_size % 64 != 0 || num_pages <= 0) return PFA_ERR_SHAPE;
        if (Smax % page_size != 0 || block_table_stride_b < Smax / page_size) return PFA_ERR_SHAPE;
        if (reinterpret_cast<uintptr_t>(block_table) & 3u) return PFA_ERR_ALIGN;
    } else if (page_size != 0 || num_pages != 0 || block_table_stride_b != 0) {
        return PFA_ERR_FLAGS;
    }
    return PFA_OK;
}

// The field rules pfa_fa3_decode and pfa_fa3_prefill share (include/pfa_hip.h, pfa_fa3_decode_args), in the order their errors are
// reported: everything but the limits that depend on the kernel (key mask, grid, workspace).  max_sq: the most query rows the caller takes.
inline int check_cache_args(const pfa_fa3_decode_args* a, int max_sq) {
    if (!a) return PFA_ERR_NULL;
    if (a->size != sizeof(pfa_fa3_decode_args)) return PFA_ERR_STRUCT_SIZE;
    if (a->flags != 0 || a->reserved0 != 0) return PFA_ERR_FLAGS;
    if (!a->q || !a->k_cache || !a->v_cache || !a->o) return PFA_ERR_NULL;
    if (a->B <= 0 || a->H <= 0 || a->Hkv <= 0 || a->Smax <= 0 || a->Sq < 1 || a->Sq > max_sq) return PFA_ERR_SHAPE;
    if (a->H % a->Hkv != 0) return PFA_ERR_SHAPE;
    if (a->D != 64 && a->D != 128) return PFA_ERR_HEAD_DIM;
    if (a->dtype_in != PFA_DTYPE_BF16 && a->dtype_in != PFA_DTYPE_FP16) return PFA_ERR_DTYPE;
    if (a->dtype_out != a->dtype_in && a->dtype_out != PFA_DTYPE_FP32) return PFA_ERR_DTYPE;
    if (!(a->softmax_scale > 0.f) || !isfinite(a->softmax_scale)) return PFA_ERR_SHAPE;
    const int64_t st8[] = {a->q_stride_b, a->q_stride_h, a->q_stride_s, a->k_stride_b, a->k_stride_h, a->k_stride_s,
                           a->v_stride_b, a->v_stride_h, a->v_stride_s};
    for (int64_t s : st8)
        if (s % 8 != 0) return PFA_ERR_STRIDE;
    const int64_t st4[] = {a->o_stride_b, a->o_stride_h, a->o_stride_s};
    for (int64_t s : st4)
        if (s % 4 != 0) return PFA_ERR_STRIDE;
    if (!aligned16(a->q) || !aligned16(a->k_cache) || !aligned16(a->v_cache) || !aligned16(a->o)) return PFA_ERR_ALIGN;
    if (a->lse && (reinterpret_cast<uintptr_t>(a->lse) & 3u)) return PFA_ERR_ALIGN;
    if (a->cache_seqlens && (reinterpret_cast<uintptr_t>(a->cache_seqlens) & 3u)) return PFA_ERR_ALIGN;
    // a tile's K / V rows are addressed by 32-bit offsets from a per-tile buffer descriptor
    if (a->k_stride_s < 0 || a->v_stride_s < 0 || a->k_stride_s * 2 * 64 + 256 > 0x7fffffffLL || a->v_stride_s * 2 * 64 + 256 > 0x7fffffffLL)
        return PFA_ERR_STRIDE;
    return check_paging(a->block_table, a->block_table_stride_b, a->page_size, a->num_pages, a->Smax);
}

// The extension block of the *_ex calls over a KV cache (include/pfa_hip.h, pfa_fa3_cache_ext), checked after the argument block's own
// rules.  -> PFA_OK and the window the kernels take in *window: 0 for none, else min(W, Smax) -- a window of Smax keys or more hides
// nothing, and the clamp keeps the kernels' row bounds inside 32 bits.
inline int check_cache_ext(const pfa_fa3_cache_ext* e, int causal, int Smax, int* window) {
    *window = 0;
    if (!e) return PFA_OK;
    if (e->size != sizeof(pfa_fa3_cache_ext)) return PFA_ERR_STRUCT_SIZE;
    if (e->flags != 0 || e->reserved != 0) return PFA_ERR_FLAGS;
    if (e->window < 0) return PFA_ERR_SHAPE;
    if (e->window > 0 && causal == 0) return PFA_ERR_FLAGS;
    *window = e->window < Smax ? e->window : Smax;
    return PFA_OK;
}

}  // namespace pfa

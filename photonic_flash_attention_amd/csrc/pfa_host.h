// pfa_host.h -- host-side glue the entry points of libpfa_hip.so share (internal: nothing here is exported).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <initializer_list>
#include <type_traits>

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

// A kernel of this library: one parameter block, by value.  Every kernel table hands out this type, so a table's rungs agree on the block.
template <typename Params>
using KernelFn = void (*)(Params);
template <typename T>
struct same_type { using type = T; };       // keeps a function parameter out of template argument deduction

// The tail of a launch: opt in to more than 64 KiB of dynamic LDS where the kernel asks for it (idempotent, per function), enqueue with
// the parameter block as the one kernel argument, and map a failure to PFA_ERR_LAUNCH (its code kept for pfa_last_hip_error).
// Params comes from the kernel alone; the block converts to it, so a block of another type does not compile and a derived block
// (a decode block with mode parts for the combine kernel's DecodeParams) is passed as its base, which is what the kernel copies.
template <typename Params>
inline int launch(KernelFn<Params> fn, dim3 grid, unsigned threads, const typename same_type<Params>::type& p, size_t lds, void* stream) {
    const void* f = reinterpret_cast<const void*>(fn);
    if (lds > 64 * 1024) (void)hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    void* kargs[] = {const_cast<Params*>(&p)};
    return hip_failed(hipLaunchKernel(f, grid, dim3(threads), kargs, lds, (hipStream_t)stream)) ? PFA_ERR_LAUNCH : PFA_OK;
}

// One tensor's strides from an argument block into a kernel parameter block: p.x_sb / x_sh / x_ss = a->x_stride_b / _h / _s.  Every
// parameter block names them so; the templates below copy the sets the kernels take.
#define PFA_FILL_STRIDES(p, a, x) ((p).x##_sb = (a)->x##_stride_b, (p).x##_sh = (a)->x##_stride_h, (p).x##_ss = (a)->x##_stride_s)
template <typename Params, typename Args>
inline void fill_qk_strides(Params& p, const Args* a) {         // WeightsParams
    PFA_FILL_STRIDES(p, a, q); PFA_FILL_STRIDES(p, a, k);
}
template <typename Params, typename Args>
inline void fill_qkvo_strides(Params& p, const Args* a) {       // FwdParams, F32Params
    fill_qk_strides(p, a);
    PFA_FILL_STRIDES(p, a, v); PFA_FILL_STRIDES(p, a, o);
}
template <typename Params>
inline void fill_bwd_strides(Params& p, const pfa_fa3_bwd_args* a) {      // BwdParams, F32BwdParams: the gradients too, and the element mask
    fill_qkvo_strides(p, a);
    PFA_FILL_STRIDES(p, a, do); PFA_FILL_STRIDES(p, a, dq); PFA_FILL_STRIDES(p, a, dk); PFA_FILL_STRIDES(p, a, dv);
    p.m_sb = a->mask_stride_b; p.m_sh = a->mask_stride_h; p.m_sq = a->mask_stride_q; p.m_sk = a->mask_stride_k;
}
// query heads per K/V head as the kernels take it: the argument blocks' 0 means 1
template <typename Args>
inline int kv_group_of(const Args* a) { return a->kv_group > 1 ? a->kv_group : 1; }

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

constexpr float LOG2E = 1.4426950408889634f;   // exp(x) = exp2(x * LOG2E): softmax_scale * LOG2E is every kernel's scale_log2

// The pointer and stride rules of the 16-bit tensors: 16-byte data pointers, 4-byte int32 / fp32 arrays (NULL passes both), element
// strides that keep every row of 8 (fp32 output: of 4) elements aligned.
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }
inline bool multiples_of(int m, std::initializer_list<int64_t> strides) {
    for (int64_t s : strides)
        if (s % m != 0) return false;
    return true;
}
template <typename Args>
inline bool qkv_strides_multiples_of(int m, const Args* a) {
    return multiples_of(m, {a->q_stride_b, a->q_stride_h, a->q_stride_s, a->k_stride_b, a->k_stride_h, a->k_stride_s, a->v_stride_b, a->v_stride_h,
                            a->v_stride_s});
}
inline bool scale_ok(float softmax_scale) { return softmax_scale > 0.f && isfinite(softmax_scale); }     // finite and positive
// The S rows of one (batch, head), `stride` elements apart and D wide, are addressed by 32-bit byte offsets (buffer descriptors, DMA).
inline int64_t slab_bytes(int32_t S, int64_t stride, int32_t D, int elem_bytes) { return ((int64_t)(S - 1) * stride + D) * elem_bytes; }
inline bool slab_fits32(int32_t S, int64_t stride, int32_t D, int elem_bytes) { return slab_bytes(S, stride, D, elem_bytes) <= 0x7fffffffLL; }
// cache rows run forward: k_stride_s / v_stride_s >= 0, for the calls that read the cache and the one that writes it
template <typename Args>
inline bool kv_rows_forward(const Args* a) { return a->k_stride_s >= 0 && a->v_stride_s >= 0; }

// Calls f with a tag of the 16-bit element type and the head dim (validated before: bf16 / fp16, D 64 / 128): the one dtype x D ladder.
template <typename T, int HEAD_DIM>
struct ElemDim {
    using type = T;
    static constexpr int D = HEAD_DIM;
};
template <typename F>
inline auto dispatch_elem_dim(int dtype, int D, F&& f) {
    return dtype == PFA_DTYPE_BF16 ? (D == 128 ? f(ElemDim<__bf16, 128>{}) : f(ElemDim<__bf16, 64>{}))
                                   : (D == 128 ? f(ElemDim<_Float16, 128>{}) : f(ElemDim<_Float16, 64>{}));
}
// ... with the head dim alone (the fp32 kernels), as a std::integral_constant
template <typename F>
inline auto dispatch_dim(int D, F&& f) {
    return D == 128 ? f(std::integral_constant<int, 128>{}) : f(std::integral_constant<int, 64>{});
}
// Calls f with a std::bool_constant tag for every run-time flag, true before false: the flags' half of a kernel ladder.
template <bool... Bs, typename F>
inline auto dispatch_bools(F&& f) { return f(std::bool_constant<Bs>{}...); }
template <bool... Bs, typename F, typename... Rest>
inline auto dispatch_bools(F&& f, bool b, Rest... rest) {
    return b ? dispatch_bools<Bs..., true>(f, rest...) : dispatch_bools<Bs..., false>(f, rest...);
}
template <bool FP32, typename T>
using out_t = std::conditional_t<FP32, float, T>;      // what a kernel stores: fp32 where the flag asks for it, else the element type

// The paging fields every call over a KV cache carries (include/pfa_hip.h, pfa_fa3_decode_args): all set, or all zero.
inline int check_paging(const int32_t* block_table, int64_t block_table_stride_b, int32_t page_size, int32_t num_pages, int32_t Smax) {
    if (block_table) {
        // Smax is the logical capacity max_pages * page_size; a 64-key tile must lie inside one page
        if (page_size <= 0 || page_size % 64 != 0 || num_pages <= 0) return PFA_ERR_SHAPE;
        if (Smax % page_size != 0 || block_table_stride_b < Smax / page_size) return PFA_ERR_SHAPE;
        if (!aligned4(block_table)) return PFA_ERR_ALIGN;
    } else if (page_size != 0 || num_pages != 0 || block_table_stride_b != 0) {
        return PFA_ERR_FLAGS;
    }
    return PFA_OK;
}

// What the two argument blocks of the attention calls over a cache name differently: the query rows of one sequence and the q / o
// batch strides.  The packed tensors of the ragged call have no batch stride (0 passes every stride rule) and max_seqlen_q stands
// where Sq does.  Every other field the templates below touch has one name in both blocks.
struct QueryRows {
    int32_t Sq;
    int64_t q_sb, o_sb;
};
inline QueryRows query_rows(const pfa_fa3_decode_args* a) { return {a->Sq, a->q_stride_b, a->o_stride_b}; }
inline QueryRows query_rows(const pfa_fa3_prefill_varlen_args* a) { return {a->max_seqlen_q, 0, 0}; }

// The shape rules a plan can be made from (pfa_fa3_decode_workspace_bytes stops here: it takes no pointers and no strides).
template <typename Args>
inline int check_cache_shape(const Args* a) {
    if (a->B <= 0 || a->H <= 0 || a->Hkv <= 0 || a->Smax <= 0 || query_rows(a).Sq < 1 || a->H % a->Hkv != 0) return PFA_ERR_SHAPE;
    if (a->D != 64 && a->D != 128) return PFA_ERR_HEAD_DIM;
    return PFA_OK;
}

// The field rules pfa_fa3_decode, pfa_fa3_prefill and pfa_fa3_prefill_varlen share (include/pfa_hip.h, pfa_fa3_decode_args), in the
// order their errors are reported: everything but the limits that depend on the kernel (key mask, cu_seqlens_q, grid, workspace).
// max_sq: the most query rows the caller takes.
template <typename Args>
inline int check_cache_args(const Args* a, int max_sq) {
    if (!a) return PFA_ERR_NULL;
    if (a->size != sizeof(Args)) return PFA_ERR_STRUCT_SIZE;
    if (a->flags != 0 || a->reserved0 != 0) return PFA_ERR_FLAGS;
    if (!a->q || !a->k_cache || !a->v_cache || !a->o) return PFA_ERR_NULL;
    const QueryRows g = query_rows(a);
    if (g.Sq > max_sq) return PFA_ERR_SHAPE;
    const int st = check_cache_shape(a);
    if (st != PFA_OK) return st;
    if (a->dtype_in != PFA_DTYPE_BF16 && a->dtype_in != PFA_DTYPE_FP16) return PFA_ERR_DTYPE;
    if (a->dtype_out != a->dtype_in && a->dtype_out != PFA_DTYPE_FP32) return PFA_ERR_DTYPE;
    if (!scale_ok(a->softmax_scale)) return PFA_ERR_SHAPE;
    if (!multiples_of(8, {g.q_sb, a->q_stride_h, a->q_stride_s, a->k_stride_b, a->k_stride_h, a->k_stride_s, a->v_stride_b, a->v_stride_h,
                          a->v_stride_s}))
        return PFA_ERR_STRIDE;
    if (!multiples_of(4, {g.o_sb, a->o_stride_h, a->o_stride_s})) return PFA_ERR_STRIDE;
    if (!aligned16(a->q) || !aligned16(a->k_cache) || !aligned16(a->v_cache) || !aligned16(a->o)) return PFA_ERR_ALIGN;
    if (!aligned4(a->lse) || !aligned4(a->cache_seqlens)) return PFA_ERR_ALIGN;
    // a tile's K / V rows are addressed by 32-bit offsets from a per-tile buffer descriptor
    if (!kv_rows_forward(a) || a->k_stride_s * 2 * 64 + 256 > 0x7fffffffLL || a->v_stride_s * 2 * 64 + 256 > 0x7fffffffLL)
        return PFA_ERR_STRIDE;
    return check_paging(a->block_table, a->block_table_stride_b, a->page_size, a->num_pages, a->Smax);
}

// What every kernel parameter block over a cache carries (DecodeParams, PrefillParams, KvAppendParams name these members alike):
// the cache strides, the lengths and the paging fields.
template <typename Params, typename Args>
inline void fill_cache_params(Params& p, const Args* a) {
    p.seqlens = a->cache_seqlens; p.Smax = a->Smax;
    PFA_FILL_STRIDES(p, a, k); PFA_FILL_STRIDES(p, a, v);
    p.block_table = a->block_table; p.bt_sb = a->block_table_stride_b; p.page_size = a->page_size; p.num_pages = a->num_pages;
}
// ... and on top of them what the attention kernels' blocks (DecodeParams, PrefillParams) share: the tensors, q / o strides, scale.
template <typename Params, typename Args>
inline void fill_attention_params(Params& p, const Args* a) {
    fill_cache_params(p, a);
    const QueryRows g = query_rows(a);
    p.q = a->q; p.k = a->k_cache; p.v = a->v_cache; p.o = a->o; p.lse = a->lse;
    p.q_sb = g.q_sb; p.q_sh = a->q_stride_h; p.q_ss = a->q_stride_s;
    p.o_sb = g.o_sb; p.o_sh = a->o_stride_h; p.o_ss = a->o_stride_s;
    p.B = a->B; p.H = a->H; p.Sq = g.Sq;
    p.scale_log2 = a->softmax_scale * LOG2E;
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

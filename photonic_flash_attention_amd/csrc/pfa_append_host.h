// pfa_append_host.h -- what the three calls that write new rows into a KV cache share (internal): pfa_kv_append_capi.hip,
// pfa_kv_append_fp8_capi.hip and pfa_rope_append_capi.hip.  The field rules and the parameter fill the argument blocks have in common
// (pfa_kv_append_args and pfa_rope_append_args name those fields alike), the grid, and the kernel tables.  The tables are templates, so
// a unit instantiates the kernels of the table it calls and no others.
#pragma once
#include "kv_append_kernel.h"
#include "pfa_host.h"
#include "rope_append_kernel.h"

namespace pfa {
namespace append {

static_assert(KV_APPEND_THREADS == ROPE_APPEND_THREADS, "one grid rule");
// Work items of one sequence, at most: max_seqlen_q rows of `heads` heads of D / piece pieces (piece: 8 elements, 16 where the kernel
// quantises or rotates; heads: Hkv, the rotary call H + 2 * Hkv) ...
template <typename Args>
int64_t items(const Args* a, int64_t heads, int piece) { return (int64_t)a->max_seqlen_q * heads * (a->D / piece); }
// ... and the workgroups: from host shapes only (max_seqlen_q, never cu_seqlens_q), so a captured graph stays valid while the device data changes
template <typename Args>
int64_t workgroups(const Args* a, int64_t heads, int piece) {
    return (int64_t)a->B * ((items(a, heads, piece) + KV_APPEND_THREADS - 1) / KV_APPEND_THREADS);
}
// the grid, and a sequence's item index inside 32 bits
template <typename Args>
bool grid_fits(const Args* a, int64_t heads, int piece) {
    return workgroups(a, heads, piece) <= 0x7fffffffLL && items(a, heads, piece) + KV_APPEND_THREADS <= 0x7fffffffLL;
}

// The field rules of pfa_kv_append (include/pfa_hip.h, pfa_kv_append_args), in the order their errors are reported, up to the grid; the
// rotary call's block begins with the same rules.  no_flags: the call defines no flag bit, so a set one is refused with the reserved
// fields, in front of the NULL checks; a call with bits of its own checks them among its own rules, behind these.
template <typename Args>
int check_args(const Args* a, bool no_flags) {
    if (!a) return PFA_ERR_NULL;
    if (a->size != sizeof(Args)) return PFA_ERR_STRUCT_SIZE;
    if ((no_flags && a->flags != 0) || a->reserved0 != 0 || a->reserved1 != 0) return PFA_ERR_FLAGS;
    if (!a->k_new || !a->v_new || !a->k_cache || !a->v_cache || !a->cache_seqlens) return PFA_ERR_NULL;
    if (a->B <= 0 || a->Hkv <= 0 || a->Smax <= 0 || a->total_new < 1 || a->max_seqlen_q < 1) return PFA_ERR_SHAPE;
    if (a->D < 8 || a->D % 8 != 0 || a->D > 256) return PFA_ERR_HEAD_DIM;
    if (a->dtype != PFA_DTYPE_BF16 && a->dtype != PFA_DTYPE_FP16) return PFA_ERR_DTYPE;
    if (!multiples_of(8, {a->kn_stride_b, a->kn_stride_s, a->kn_stride_h, a->vn_stride_b, a->vn_stride_s, a->vn_stride_h,
                          a->k_stride_b, a->k_stride_h, a->k_stride_s, a->v_stride_b, a->v_stride_h, a->v_stride_s}))
        return PFA_ERR_STRIDE;
    if (!kv_rows_forward(a)) return PFA_ERR_STRIDE;      // as the calls that read the cache
    if (!aligned16(a->k_new) || !aligned16(a->v_new) || !aligned16(a->k_cache) || !aligned16(a->v_cache)) return PFA_ERR_ALIGN;
    if (!aligned4(a->cache_seqlens)) return PFA_ERR_ALIGN;
    const int st = check_paging(a->block_table, a->block_table_stride_b, a->page_size, a->num_pages, a->Smax);
    if (st != PFA_OK) return st;
    if (a->cu_seqlens_q) {
        if (!aligned4(a->cu_seqlens_q)) return PFA_ERR_ALIGN;
        if (a->kn_stride_b != 0 || a->vn_stride_b != 0) return PFA_ERR_FLAGS;      // packed rows have no batch stride
        if (a->max_seqlen_q > a->total_new) return PFA_ERR_SHAPE;
    } else if ((int64_t)a->B * a->max_seqlen_q > a->total_new) {
        return PFA_ERR_SHAPE;
    }
    return PFA_OK;
}

// What KvAppendParams, KvAppendQ8Params and RopeAppendParams hold alike, of checked arguments: the new rows, the cache, the grid.
template <typename Params, typename Args>
void fill_params(Params& p, const Args* a, int64_t heads, int piece) {
    p.k_new = a->k_new; p.v_new = a->v_new; p.k_cache = a->k_cache; p.v_cache = a->v_cache;
    p.cu_seqlens_q = a->cu_seqlens_q;
    p.kn_sb = a->kn_stride_b; p.kn_ss = a->kn_stride_s; p.kn_sh = a->kn_stride_h;
    p.vn_sb = a->vn_stride_b; p.vn_ss = a->vn_stride_s; p.vn_sh = a->vn_stride_h;
    fill_cache_params(p, a);
    p.nchunk = (int32_t)(workgroups(a, heads, piece) / a->B);
    p.Sq = a->max_seqlen_q; p.total_new = a->total_new;
    p.units = (int32_t)(heads * (a->D / piece));
}

// kv_append_kernel: the 16-bit copy (QUANT false: the element type plays no part) or the quantising one of element type T
template <bool QUANT, typename T = void>
KernelFn<typename KvAppendParamsOf<QUANT>::type> kv_kernel(bool varlen, bool paged) {
    return dispatch_bools([](auto v, auto pg) -> KernelFn<typename KvAppendParamsOf<QUANT>::type> {
        return &kv_append_kernel<v.value, pg.value, QUANT, T>;
    }, varlen, paged);
}
template <typename T>
KernelFn<RopeAppendParams> rope_kernel(bool varlen, bool paged, bool interleaved) {
    return dispatch_bools([](auto v, auto pg, auto il) -> KernelFn<RopeAppendParams> { return &rope_append_kernel<T, v.value, pg.value, il.value>; },
                          varlen, paged, interleaved);
}

}  // namespace append
}  // namespace pfa

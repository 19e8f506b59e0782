// pfa_kv_append_capi.hip -- C ABI of the device-side KV-cache append (include/pfa_hip.h, pfa_kv_append*): validation and the launch of
// kv_append_kernel.  No allocation, no synchronisation, no process-wide state, no workspace.
#include "pfa_hip.h"

#include <hip/hip_runtime.h>
#include <stdio.h>

#include "kv_append_kernel.h"
#include "pfa_host.h"

namespace {

// 16-byte work items of one sequence, at most: max_seqlen_q rows of Hkv heads of D / 8 pieces
int64_t items(const pfa_kv_append_args* a) { return (int64_t)a->max_seqlen_q * a->Hkv * (a->D / 8); }

// workgroups: from host shapes only (max_seqlen_q, never cu_seqlens_q), so a captured graph stays valid while the device data changes
int64_t workgroups(const pfa_kv_append_args* a) {
    return (int64_t)a->B * ((items(a) + pfa::KV_APPEND_THREADS - 1) / pfa::KV_APPEND_THREADS);
}

int check(const pfa_kv_append_args* a) {
    if (!a) return PFA_ERR_NULL;
    if (a->size != sizeof(pfa_kv_append_args)) return PFA_ERR_STRUCT_SIZE;
    if (a->flags != 0 || a->reserved0 != 0 || a->reserved1 != 0) return PFA_ERR_FLAGS;
    if (!a->k_new || !a->v_new || !a->k_cache || !a->v_cache || !a->cache_seqlens) return PFA_ERR_NULL;
    if (a->B <= 0 || a->Hkv <= 0 || a->Smax <= 0 || a->total_new < 1 || a->max_seqlen_q < 1) return PFA_ERR_SHAPE;
    if (a->D < 8 || a->D % 8 != 0 || a->D > 256) return PFA_ERR_HEAD_DIM;
    if (a->dtype != PFA_DTYPE_BF16 && a->dtype != PFA_DTYPE_FP16) return PFA_ERR_DTYPE;
    if (!pfa::multiples_of(8, {a->kn_stride_b, a->kn_stride_s, a->kn_stride_h, a->vn_stride_b, a->vn_stride_s, a->vn_stride_h,
                               a->k_stride_b, a->k_stride_h, a->k_stride_s, a->v_stride_b, a->v_stride_h, a->v_stride_s}))
        return PFA_ERR_STRIDE;
    if (!pfa::kv_rows_forward(a)) return PFA_ERR_STRIDE;      // as the calls that read the cache
    if (!pfa::aligned16(a->k_new) || !pfa::aligned16(a->v_new) || !pfa::aligned16(a->k_cache) || !pfa::aligned16(a->v_cache)) return PFA_ERR_ALIGN;
    if (!pfa::aligned4(a->cache_seqlens)) return PFA_ERR_ALIGN;
    const int st = pfa::check_paging(a->block_table, a->block_table_stride_b, a->page_size, a->num_pages, a->Smax);
    if (st != PFA_OK) return st;
    if (a->cu_seqlens_q) {
        if (!pfa::aligned4(a->cu_seqlens_q)) return PFA_ERR_ALIGN;
        if (a->kn_stride_b != 0 || a->vn_stride_b != 0) return PFA_ERR_FLAGS;      // packed rows have no batch stride
        if (a->max_seqlen_q > a->total_new) return PFA_ERR_SHAPE;
    } else if ((int64_t)a->B * a->max_seqlen_q > a->total_new) {
        return PFA_ERR_SHAPE;
    }
    // the grid, and a sequence's item index inside 32 bits
    if (workgroups(a) > 0x7fffffffLL || items(a) + pfa::KV_APPEND_THREADS > 0x7fffffffLL) return PFA_ERR_SHAPE;
    return PFA_OK;
}

}  // namespace

extern "C" {

int pfa_kv_append_check(const pfa_kv_append_args* a) { return check(a); }

int pfa_kv_append_describe(const pfa_kv_append_args* a, char* buf, size_t n) {
    const int st = check(a);
    if (st != PFA_OK) return st;
    if (buf && n)
        snprintf(buf, n, "kv_append_%s_d%d%s%s", a->dtype == PFA_DTYPE_BF16 ? "bf16" : "fp16", a->D, a->cu_seqlens_q ? "_varlen" : "",
                 a->block_table ? "_paged" : "");
    return (int)workgroups(a);
}

int pfa_kv_append(const pfa_kv_append_args* a, void* stream) {
    const int st = check(a);
    if (st != PFA_OK) return st;
    pfa::KvAppendParams p;
    p.k_new = a->k_new; p.v_new = a->v_new; p.k_cache = a->k_cache; p.v_cache = a->v_cache;
    p.cu_seqlens_q = a->cu_seqlens_q;
    p.kn_sb = a->kn_stride_b; p.kn_ss = a->kn_stride_s; p.kn_sh = a->kn_stride_h;
    p.vn_sb = a->vn_stride_b; p.vn_ss = a->vn_stride_s; p.vn_sh = a->vn_stride_h;
    pfa::fill_cache_params(p, a);
    p.nchunk = (int32_t)(workgroups(a) / a->B);
    p.Sq = a->max_seqlen_q; p.total_new = a->total_new;
    p.dchunks = a->D / 8; p.units = a->Hkv * (a->D / 8);

    const bool varlen = a->cu_seqlens_q != nullptr, paged = a->block_table != nullptr;
    const void* fn = varlen ? (paged ? (const void*)&pfa::kv_append_kernel<true, true> : (const void*)&pfa::kv_append_kernel<true, false>)
                            : (paged ? (const void*)&pfa::kv_append_kernel<false, true> : (const void*)&pfa::kv_append_kernel<false, false>);
    const pfa::DeviceScope dev(a->device_id);
    if (pfa::hip_failed(dev.error())) return PFA_ERR_DEVICE;
    return pfa::launch(fn, dim3((unsigned)workgroups(a)), pfa::KV_APPEND_THREADS, p, 0, stream);
}

}  // extern "C"

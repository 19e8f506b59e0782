// pfa_mla_append_capi.hip -- C ABI of the latent-cache append at width 576 (include/pfa_hip_mla_cache.h, pfa_mla_append*): the field
// rules, and the launch of mla_append_kernel's 12 instantiations (ragged x paged x {16-bit copy, quantising from bf16, from fp16}).
// Built with -ffp-contract=off (csrc/Makefile), as pfa_kv_append_fp8_capi is: the plain-torch model of the quantising store is byte-equal.
// No allocation, no synchronisation, no process-wide state, no workspace; the grid from host shapes only.
#include <stdio.h>

#include "mla_append_kernel.h"
#include "pfa_mla_cache_host.h"

namespace {

using pfa::MlaAppendParams;

// work items of one sequence at most, and the workgroups: from max_seqlen_q, never from cu_seqlens_q
int64_t items(const pfa_mla_append_args* a, bool q8) { return (int64_t)a->max_seqlen_q * (pfa::MLA_APPEND_D / (q8 ? 16 : 8)); }
int64_t workgroups(const pfa_mla_append_args* a, bool q8) {
    return (int64_t)a->B * ((items(a, q8) + pfa::KV_APPEND_THREADS - 1) / pfa::KV_APPEND_THREADS);
}

// include/pfa_hip_mla_cache.h, pfa_mla_append, in the order the errors are reported
int check(const pfa_mla_append_args* a, const pfa_mla_kv_quant* quant) {
    if (!a) return PFA_ERR_NULL;
    if (a->size != sizeof(pfa_mla_append_args)) return PFA_ERR_STRUCT_SIZE;
    if (quant) {
        const int st = pfa::mla::check_kv_quant(quant);
        if (st != PFA_OK) return st;
    }
    if (a->flags != 0 || a->reserved != 0 || a->reserved1 != 0) return PFA_ERR_FLAGS;
    if (!a->kv_c || !a->k_pe || !a->kv_cache || !a->cache_seqlens) return PFA_ERR_NULL;
    if (a->B <= 0 || a->Smax <= 0 || a->total_new < 1 || a->max_seqlen_q < 1) return PFA_ERR_SHAPE;
    if (a->dtype != PFA_DTYPE_BF16 && a->dtype != PFA_DTYPE_FP16) return PFA_ERR_DTYPE;
    if (!pfa::multiples_of(8, {a->kvc_stride_b, a->kvc_stride_s, a->kpe_stride_b, a->kpe_stride_s})) return PFA_ERR_STRIDE;
    if (!pfa::multiples_of(quant ? 16 : 8, {a->kv_stride_b, a->kv_stride_s}) || a->kv_stride_s < pfa::MLA_APPEND_D) return PFA_ERR_STRIDE;
    if (!pfa::aligned16(a->kv_c) || !pfa::aligned16(a->k_pe) || !pfa::aligned16(a->kv_cache)) return PFA_ERR_ALIGN;
    if (!pfa::aligned4(a->cache_seqlens) || !pfa::aligned4(a->cu_seqlens_q)) return PFA_ERR_ALIGN;
    const int st = pfa::check_paging(a->block_table, a->block_table_stride_b, a->page_size, a->num_pages, a->Smax);
    if (st != PFA_OK) return st;
    if (a->cu_seqlens_q) {
        if (a->kvc_stride_b != 0 || a->kpe_stride_b != 0) return PFA_ERR_FLAGS;      // packed rows have no batch stride
        if (a->max_seqlen_q > a->total_new) return PFA_ERR_SHAPE;
    } else if ((int64_t)a->B * a->max_seqlen_q > a->total_new) {
        return PFA_ERR_SHAPE;
    }
    // the grid, and a sequence's item index inside 32 bits
    if (workgroups(a, quant != nullptr) > 0x7fffffffLL || items(a, quant != nullptr) + pfa::KV_APPEND_THREADS > 0x7fffffffLL) return PFA_ERR_SHAPE;
    return PFA_OK;
}

// the 16-bit copy (the element type plays no part) or the quantising store from T
template <bool QUANT, typename T = void>
pfa::KernelFn<MlaAppendParams> kernel(bool varlen, bool paged) {
    return pfa::dispatch_bools([](auto v, auto pg) -> pfa::KernelFn<MlaAppendParams> { return &pfa::mla_append_kernel<v.value, pg.value, QUANT, T>; },
                               varlen, paged);
}

}  // namespace

extern "C" {

int pfa_mla_append_check(const pfa_mla_append_args* a, const pfa_mla_kv_quant* quant) { return check(a, quant); }

int pfa_mla_append_describe(const pfa_mla_append_args* a, const pfa_mla_kv_quant* quant, char* buf, size_t n) {
    const int st = check(a, quant);
    if (st != PFA_OK) return st;
    if (buf && n)
        snprintf(buf, n, "mla_append%s%s%s", !quant ? "" : a->dtype == PFA_DTYPE_BF16 ? "_q8_bf16" : "_q8_fp16", a->cu_seqlens_q ? "_varlen" : "",
                 a->block_table ? "_paged" : "");
    return (int)workgroups(a, quant != nullptr);
}

int pfa_mla_append(const pfa_mla_append_args* a, const pfa_mla_kv_quant* quant, void* stream) {
    const int st = check(a, quant);
    if (st != PFA_OK) return st;
    const bool q8 = quant != nullptr, varlen = a->cu_seqlens_q != nullptr, paged = a->block_table != nullptr;
    MlaAppendParams p = {};
    p.kv_c = a->kv_c; p.k_pe = a->k_pe; p.kv_cache = a->kv_cache;
    p.cu_seqlens_q = a->cu_seqlens_q; p.seqlens = a->cache_seqlens; p.block_table = a->block_table;
    p.kvc_sb = a->kvc_stride_b; p.kvc_ss = a->kvc_stride_s; p.kpe_sb = a->kpe_stride_b; p.kpe_ss = a->kpe_stride_s;
    p.k_sb = a->kv_stride_b; p.k_ss = a->kv_stride_s; p.bt_sb = a->block_table_stride_b;
    p.nchunk = (int32_t)(workgroups(a, q8) / a->B);
    p.Sq = a->max_seqlen_q; p.Smax = a->Smax; p.total_new = a->total_new; p.page_size = a->page_size; p.num_pages = a->num_pages;
    if (q8) { p.kv_descale = quant->kv_descale; p.ds_sb = quant->descale_stride_b; }
    const auto fn = !q8 ? kernel<false>(varlen, paged) : a->dtype == PFA_DTYPE_BF16 ? kernel<true, __bf16>(varlen, paged) : kernel<true, _Float16>(varlen, paged);
    const pfa::DeviceScope dev(a->device_id);
    if (pfa::hip_failed(dev.error())) return PFA_ERR_DEVICE;
    return pfa::launch(fn, dim3((unsigned)workgroups(a, q8)), pfa::KV_APPEND_THREADS, p, 0, stream);
}

}  // extern "C"

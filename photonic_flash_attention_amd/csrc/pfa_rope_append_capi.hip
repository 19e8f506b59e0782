// pfa_rope_append_capi.hip -- C ABI of the rotary embedding fused into the KV-cache append (include/pfa_hip.h, pfa_rope_append*):
// validation and the launch of rope_append_kernel.  No allocation, no synchronisation, no process-wide state, no workspace.
// This object alone is compiled with -ffp-contract=off (csrc/Makefile): the kernel's products and sums round separately.
#include "pfa_hip.h"

#include <hip/hip_runtime.h>
#include <stdio.h>

#include "pfa_host.h"
#include "rope_append_kernel.h"

namespace {

// 16-element work items of one sequence, at most: max_seqlen_q rows of H + 2 * Hkv heads of D / 16 units
int64_t items(const pfa_rope_append_args* a) { return (int64_t)a->max_seqlen_q * ((int64_t)a->H + 2 * (int64_t)a->Hkv) * (a->D / 16); }

// workgroups: from host shapes only (max_seqlen_q, never cu_seqlens_q), so a captured graph stays valid while the device data changes
int64_t workgroups(const pfa_rope_append_args* a) {
    return (int64_t)a->B * ((items(a) + pfa::ROPE_APPEND_THREADS - 1) / pfa::ROPE_APPEND_THREADS);
}

int check(const pfa_rope_append_args* a) {
    // pfa_kv_append's rules, in its order, where the fields coincide
    if (!a) return PFA_ERR_NULL;
    if (a->size != sizeof(pfa_rope_append_args)) return PFA_ERR_STRUCT_SIZE;
    if (a->reserved0 != 0 || a->reserved1 != 0) return PFA_ERR_FLAGS;
    if (!a->k_new || !a->v_new || !a->k_cache || !a->v_cache || !a->cache_seqlens) return PFA_ERR_NULL;
    if (a->B <= 0 || a->Hkv <= 0 || a->Smax <= 0 || a->total_new < 1 || a->max_seqlen_q < 1) return PFA_ERR_SHAPE;
    if (a->D < 8 || a->D % 8 != 0 || a->D > 256) return PFA_ERR_HEAD_DIM;
    if (a->dtype != PFA_DTYPE_BF16 && a->dtype != PFA_DTYPE_FP16) return PFA_ERR_DTYPE;
    if (!pfa::multiples_of(8, {a->kn_stride_b, a->kn_stride_s, a->kn_stride_h, a->vn_stride_b, a->vn_stride_s, a->vn_stride_h,
                               a->k_stride_b, a->k_stride_h, a->k_stride_s, a->v_stride_b, a->v_stride_h, a->v_stride_s}))
        return PFA_ERR_STRIDE;
    if (!pfa::kv_rows_forward(a)) return PFA_ERR_STRIDE;
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
    // the rotary rules
    if (a->flags & ~PFA_ROPE_INTERLEAVED) return PFA_ERR_FLAGS;
    if (!a->cos || !a->sin) return PFA_ERR_NULL;
    if ((a->q == nullptr) != (a->q_out == nullptr)) return PFA_ERR_NULL;
    if (a->q && a->H < 1) return PFA_ERR_SHAPE;
    if (!a->q && a->H != 0) return PFA_ERR_FLAGS;
    if (a->max_pos < 1) return PFA_ERR_SHAPE;
    if (a->D % 16 != 0 || a->rot_dim < 16 || a->rot_dim % 16 != 0 || a->rot_dim > a->D) return PFA_ERR_HEAD_DIM;
    if (!pfa::multiples_of(8, {a->q_stride_b, a->q_stride_s, a->q_stride_h, a->qo_stride_b, a->qo_stride_s, a->qo_stride_h}))
        return PFA_ERR_STRIDE;
    if (a->cs_stride % 4 != 0 || a->cs_stride < a->rot_dim / 2) return PFA_ERR_STRIDE;
    if (!pfa::aligned16(a->q) || !pfa::aligned16(a->q_out) || !pfa::aligned16(a->cos) || !pfa::aligned16(a->sin)) return PFA_ERR_ALIGN;
    if (!pfa::aligned4(a->pos_offsets)) return PFA_ERR_ALIGN;
    if (a->cu_seqlens_q && (a->q_stride_b != 0 || a->qo_stride_b != 0)) return PFA_ERR_FLAGS;
    // the grid, and a sequence's item index inside 32 bits
    if (workgroups(a) > 0x7fffffffLL || items(a) + pfa::ROPE_APPEND_THREADS > 0x7fffffffLL) return PFA_ERR_SHAPE;
    return PFA_OK;
}

template <typename T>
const void* kernel_of(bool varlen, bool paged, bool il) {
    const void* fns[8] = {
        (const void*)&pfa::rope_append_kernel<T, false, false, false>, (const void*)&pfa::rope_append_kernel<T, false, false, true>,
        (const void*)&pfa::rope_append_kernel<T, false, true, false>,  (const void*)&pfa::rope_append_kernel<T, false, true, true>,
        (const void*)&pfa::rope_append_kernel<T, true, false, false>,  (const void*)&pfa::rope_append_kernel<T, true, false, true>,
        (const void*)&pfa::rope_append_kernel<T, true, true, false>,   (const void*)&pfa::rope_append_kernel<T, true, true, true>};
    return fns[(varlen ? 4 : 0) + (paged ? 2 : 0) + (il ? 1 : 0)];
}

}  // namespace

extern "C" {

int pfa_rope_append_check(const pfa_rope_append_args* a) { return check(a); }

int pfa_rope_append_describe(const pfa_rope_append_args* a, char* buf, size_t n) {
    const int st = check(a);
    if (st != PFA_OK) return st;
    if (buf && n)
        snprintf(buf, n, "rope_append_%s_d%d_r%d%s%s%s", a->dtype == PFA_DTYPE_BF16 ? "bf16" : "fp16", a->D, a->rot_dim,
                 (a->flags & PFA_ROPE_INTERLEAVED) ? "_il" : "", a->cu_seqlens_q ? "_varlen" : "", a->block_table ? "_paged" : "");
    return (int)workgroups(a);
}

int pfa_rope_append(const pfa_rope_append_args* a, void* stream) {
    const int st = check(a);
    if (st != PFA_OK) return st;
    pfa::RopeAppendParams p;
    p.q = a->q; p.q_out = a->q_out; p.k_new = a->k_new; p.v_new = a->v_new; p.k_cache = a->k_cache; p.v_cache = a->v_cache;
    p.cos = a->cos; p.sin = a->sin; p.cu_seqlens_q = a->cu_seqlens_q; p.pos_offsets = a->pos_offsets;
    p.q_sb = a->q_stride_b; p.q_ss = a->q_stride_s; p.q_sh = a->q_stride_h;
    p.qo_sb = a->qo_stride_b; p.qo_ss = a->qo_stride_s; p.qo_sh = a->qo_stride_h;
    p.kn_sb = a->kn_stride_b; p.kn_ss = a->kn_stride_s; p.kn_sh = a->kn_stride_h;
    p.vn_sb = a->vn_stride_b; p.vn_ss = a->vn_stride_s; p.vn_sh = a->vn_stride_h;
    pfa::fill_cache_params(p, a);
    p.cs_stride = a->cs_stride;
    p.nchunk = (int32_t)(workgroups(a) / a->B);
    p.Sq = a->max_seqlen_q; p.total_new = a->total_new;
    p.H = a->H; p.Hkv = a->Hkv;
    p.dunits = a->D / 16; p.runits = a->rot_dim / 16; p.units = (a->H + 2 * a->Hkv) * (a->D / 16);
    p.max_pos = a->max_pos;

    const bool varlen = a->cu_seqlens_q != nullptr, paged = a->block_table != nullptr, il = (a->flags & PFA_ROPE_INTERLEAVED) != 0;
    const void* fn = a->dtype == PFA_DTYPE_BF16 ? kernel_of<__bf16>(varlen, paged, il) : kernel_of<_Float16>(varlen, paged, il);
    const pfa::DeviceScope dev(a->device_id);
    if (pfa::hip_failed(dev.error())) return PFA_ERR_DEVICE;
    return pfa::launch(fn, dim3((unsigned)workgroups(a)), pfa::ROPE_APPEND_THREADS, p, 0, stream);
}

}  // extern "C"

// pfa_norm_rope_append_capi.hip -- C ABI of QK-norm, rotary embedding and the FP8 store fused into the KV-cache append
// (include/pfa_hip_norm_rope_append.h, pfa_norm_rope_append*): validation and the launch of norm_rope_append_kernel.  No allocation, no
// synchronisation, no process-wide state, no workspace.
// Compiled with -ffp-contract=off (csrc/Makefile), as pfa_rope_append_capi and pfa_qk_norm_capi are: the kernel's products and sums
// round separately.
#include "pfa_hip_norm_rope_append.h"

#include <math.h>
#include <stdio.h>

#include "norm_rope_append_kernel.h"
#include "pfa_append_host.h"
#include "pfa_rows_host.h"

namespace {

namespace rows = pfa::rows;
using rows::kPiece;            // a work item is 16 elements of a row: a rotation's pairs lie inside it
using A = pfa_norm_rope_append_args;
constexpr uint32_t kFlags = PFA_NRA_INTERLEAVED | PFA_NRA_UNIT_OFFSET;

int64_t heads(const A* a) { return (int64_t)a->H + 2 * (int64_t)a->Hkv; }                       // of a row: q, k_new and v_new
int64_t workgroups(const A* a) { return pfa::append::workgroups(a, heads(a), kPiece); }
bool fp8(const A* a) { return a->kv_dtype == PFA_DTYPE_FP8_E4M3; }

// One rung per status, in the order of the header: which of two broken rules wins is part of the ABI.
int check(const A* a) {
    using pfa::aligned4;
    using pfa::multiples_of;
    if (!a) return PFA_ERR_NULL;
    if (a->size != sizeof(A)) return PFA_ERR_STRUCT_SIZE;
    // flags
    if ((a->flags & ~kFlags) || a->reserved0 != 0 || a->reserved1 != 0) return PFA_ERR_FLAGS;
    if (!a->q && (a->H != 0 || a->q_weight)) return PFA_ERR_FLAGS;
    if ((a->flags & PFA_NRA_UNIT_OFFSET) && !a->q_weight && !a->k_weight) return PFA_ERR_FLAGS;
    if (a->rot_dim == 0 && !a->q_weight && !a->k_weight) return PFA_ERR_FLAGS;               // nothing to do: that call is pfa_kv_append
    if (!a->block_table && (a->page_size != 0 || a->num_pages != 0 || a->block_table_stride_b != 0)) return PFA_ERR_FLAGS;
    if (a->cu_seqlens_q && (a->q_stride_b != 0 || a->qo_stride_b != 0 || a->kn_stride_b != 0 || a->vn_stride_b != 0)) return PFA_ERR_FLAGS;
    // NULL
    if (!a->k_new || !a->v_new || !a->k_cache || !a->v_cache || !a->cache_seqlens) return PFA_ERR_NULL;
    if ((a->q == nullptr) != (a->q_out == nullptr) || (a->k_descale == nullptr) != (a->v_descale == nullptr)) return PFA_ERR_NULL;
    if (!rows::null_iff(a->rot_dim == 0, {a->cos, a->sin})) return PFA_ERR_NULL;
    // shape
    if (a->B < 1 || a->Hkv < 1 || a->Smax < 1 || a->total_new < 1 || a->max_seqlen_q < 1 || (a->q && a->H < 1)) return PFA_ERR_SHAPE;
    if ((a->rot_dim != 0 && a->max_pos < 1) || !(a->eps >= 0.f) || !isfinite(a->eps)) return PFA_ERR_SHAPE;
    if (a->block_table && (a->page_size <= 0 || a->page_size % 64 != 0 || a->num_pages <= 0 || a->Smax % a->page_size != 0 ||
                           a->block_table_stride_b < a->Smax / a->page_size))
        return PFA_ERR_SHAPE;
    if (a->cu_seqlens_q ? a->max_seqlen_q > a->total_new : (int64_t)a->B * a->max_seqlen_q > a->total_new) return PFA_ERR_SHAPE;
    // head dim
    if (a->D != 64 && a->D != 128) return PFA_ERR_HEAD_DIM;
    if (a->rot_dim != 0 && (a->rot_dim < kPiece || a->rot_dim % kPiece != 0 || a->rot_dim > a->D)) return PFA_ERR_HEAD_DIM;
    // dtype
    if (a->dtype != PFA_DTYPE_BF16 && a->dtype != PFA_DTYPE_FP16) return PFA_ERR_DTYPE;
    if ((a->q_weight || a->k_weight) && a->weight_dtype != a->dtype && a->weight_dtype != PFA_DTYPE_FP32) return PFA_ERR_DTYPE;
    if (a->kv_dtype != a->dtype && !fp8(a)) return PFA_ERR_DTYPE;
    if (fp8(a) != (a->k_descale != nullptr)) return PFA_ERR_DTYPE;      // a descale with a 16-bit cache, an FP8 cache without descales
    // stride
    if (!multiples_of(8, {a->q_stride_b, a->q_stride_s, a->q_stride_h, a->qo_stride_b, a->qo_stride_s, a->qo_stride_h, a->kn_stride_b,
                          a->kn_stride_s, a->kn_stride_h, a->vn_stride_b, a->vn_stride_s, a->vn_stride_h}))
        return PFA_ERR_STRIDE;
    // a 16-byte store of 16-bit elements needs strides of 8, of one-byte elements strides of 16
    if (!multiples_of(fp8(a) ? 16 : 8, {a->k_stride_b, a->k_stride_h, a->k_stride_s, a->v_stride_b, a->v_stride_h, a->v_stride_s}) ||
        !pfa::kv_rows_forward(a))
        return PFA_ERR_STRIDE;
    if (a->rot_dim != 0 && (a->cs_stride % 4 != 0 || a->cs_stride < a->rot_dim / 2)) return PFA_ERR_STRIDE;
    if (fp8(a) && a->ds_sb != 0 && a->ds_sb < a->Hkv) return PFA_ERR_STRIDE;
    // alignment
    if (!rows::all_aligned16({a->q, a->q_out, a->k_new, a->v_new, a->k_cache, a->v_cache, a->q_weight, a->k_weight, a->cos, a->sin}))
        return PFA_ERR_ALIGN;
    if (!aligned4(a->cu_seqlens_q) || !aligned4(a->cache_seqlens) || !aligned4(a->pos_offsets) || !aligned4(a->block_table) ||
        !aligned4(a->k_descale) || !aligned4(a->v_descale))
        return PFA_ERR_ALIGN;
    // grid: the workgroups and a sequence's item index inside 32 bits
    return pfa::append::grid_fits(a, heads(a), kPiece) ? PFA_OK : PFA_ERR_SHAPE;
}

// the kernel table: 16-bit type x G x ragged x paged x pairing x quantising store
template <typename T, int G>
pfa::KernelFn<pfa::NormRopeAppendParams> kernel_of(bool varlen, bool paged, bool interleaved, bool quant) {
    return pfa::dispatch_bools(
        [](auto v, auto pg, auto il, auto q8) -> pfa::KernelFn<pfa::NormRopeAppendParams> {
            return &pfa::norm_rope_append_kernel<T, G, v.value, pg.value, il.value, q8.value>;
        },
        varlen, paged, interleaved, quant);
}

}  // namespace

extern "C" {

int pfa_norm_rope_append_check(const pfa_norm_rope_append_args* a) { return check(a); }

int pfa_norm_rope_append_describe(const pfa_norm_rope_append_args* a, char* buf, size_t n) {
    const int st = check(a);
    if (st != PFA_OK) return st;
    const bool normed = a->q_weight || a->k_weight;
    if (buf && n)
        snprintf(buf, n, "norm_rope_append_%s_d%d%s%s%s%s%s%s%s%s%s", a->dtype == PFA_DTYPE_BF16 ? "bf16" : "fp16", a->D,
                 a->cu_seqlens_q ? "_varlen" : "", a->block_table ? "_paged" : "", (a->flags & PFA_NRA_INTERLEAVED) ? "_il" : "",
                 a->rot_dim ? "_rot" : "", a->q_weight ? "_qn" : "", a->k_weight ? "_kn" : "", (a->flags & PFA_NRA_UNIT_OFFSET) ? "_unit" : "",
                 normed && a->weight_dtype == PFA_DTYPE_FP32 ? "_w32" : "", fp8(a) ? "_q8" : "");
    return (int)workgroups(a);
}

int pfa_norm_rope_append(const pfa_norm_rope_append_args* a, void* stream) {
    const int st = check(a);
    if (st != PFA_OK) return st;
    pfa::NormRopeAppendParams p;
    pfa::append::fill_params(p, a, heads(a), kPiece);
    p.q = a->q; p.q_out = a->q_out; p.cos = a->cos; p.sin = a->sin; p.pos_offsets = a->pos_offsets;
    p.q_sb = a->q_stride_b; p.q_ss = a->q_stride_s; p.q_sh = a->q_stride_h;
    p.qo_sb = a->qo_stride_b; p.qo_ss = a->qo_stride_s; p.qo_sh = a->qo_stride_h;
    p.cs_stride = a->cs_stride;
    p.H = a->H; p.Hkv = a->Hkv;
    p.dunits = a->D / kPiece; p.runits = a->rot_dim / kPiece;
    p.max_pos = a->max_pos;
    p.q_weight = a->q_weight; p.k_weight = a->k_weight;
    p.k_descale = a->k_descale; p.v_descale = a->v_descale; p.ds_sb = a->ds_sb;
    p.eps = a->eps; p.inv_d = 1.0f / (float)a->D;
    p.w_fp32 = a->weight_dtype == PFA_DTYPE_FP32;
    p.unit_offset = (a->flags & PFA_NRA_UNIT_OFFSET) ? 1 : 0;

    const bool varlen = a->cu_seqlens_q != nullptr, paged = a->block_table != nullptr, il = (a->flags & PFA_NRA_INTERLEAVED) != 0;
    const bool quant = fp8(a);
    const auto fn = pfa::dispatch_elem_dim(a->dtype, a->D, [&](auto tag) {
        using Tag = decltype(tag);
        return kernel_of<typename Tag::type, Tag::D / kPiece>(varlen, paged, il, quant);
    });
    const pfa::DeviceScope dev(a->device_id);
    if (pfa::hip_failed(dev.error())) return PFA_ERR_DEVICE;
    return pfa::launch(fn, dim3((unsigned)workgroups(a)), pfa::NORM_ROPE_APPEND_THREADS, p, 0, stream);
}

}  // extern "C"

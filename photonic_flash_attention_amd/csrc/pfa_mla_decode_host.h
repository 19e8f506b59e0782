// pfa_mla_decode_host.h -- what pfa_mla_decode_capi.hip and pfa_mla_decode_fp8_capi.hip share behind pfa_mla_decode_args (internal): the
// field rules, the block restated as the pfa_fa3_decode_args of one K/V head at D = 512 -- so that the split rule, the workspace layout and
// the parameter fill are pfa_decode_host.h's, which every decode unit shares -- and the describe.  Nothing here looks at the cache's
// element type: the FP8 call plans, splits and sizes its workspace as the 16-bit call does.  No kernel is named here, so a unit
// instantiates its own only.
#pragma once
#include "fa3_mla_decode_kernel.h"
#include "pfa_decode_host.h"
#include "pfa_hip_mla.h"

namespace pfa {
namespace mla {

using decode::Plan;
using dec::GeoMla;

constexpr int kMaxSq = 64;

// the shape rules a plan can be made from (the workspace query stops here: it takes no pointers and no strides)
inline int check_shape(const pfa_mla_decode_args* a) {
    if (!a) return PFA_ERR_NULL;
    if (a->size != sizeof(pfa_mla_decode_args)) return PFA_ERR_STRUCT_SIZE;
    if (a->B <= 0 || a->H <= 0 || a->Smax <= 0 || a->Sq < 1 || a->Sq > kMaxSq) return PFA_ERR_SHAPE;
    return PFA_OK;
}

// the call as the decode of one K/V head at D = 512 whose K and V are the latent cache: what plan() and fill_params() read
inline pfa_fa3_decode_args as_decode(const pfa_mla_decode_args* a) {
    pfa_fa3_decode_args d = {};
    d.size = sizeof(d);
    d.q = a->q; d.k_cache = a->kv_cache; d.v_cache = a->kv_cache; d.o = a->o; d.lse = a->lse; d.cache_seqlens = a->cache_seqlens;
    d.q_stride_b = a->q_stride_b; d.q_stride_h = a->q_stride_h; d.q_stride_s = a->q_stride_s;
    d.o_stride_b = a->o_stride_b; d.o_stride_h = a->o_stride_h; d.o_stride_s = a->o_stride_s;
    d.k_stride_b = d.v_stride_b = a->kv_stride_b;
    d.k_stride_s = d.v_stride_s = a->kv_stride_s;
    d.B = a->B; d.H = a->H; d.Hkv = 1; d.Sq = a->Sq; d.Smax = a->Smax; d.D = GeoMla::DV;
    d.dtype_in = a->dtype_in; d.dtype_out = a->dtype_out; d.causal = a->causal; d.softmax_scale = a->softmax_scale;
    d.device_id = a->device_id; d.workspace = a->workspace; d.workspace_bytes = a->workspace_bytes;
    d.block_table = a->block_table; d.block_table_stride_b = a->block_table_stride_b; d.page_size = a->page_size; d.num_pages = a->num_pages;
    return d;
}

// the field rules of include/pfa_hip_mla.h in the order their errors are reported -> PFA_OK, the restated block in *d, its plan in *pl and
// the workgroups of the main launch in *grid
inline int check(const pfa_mla_decode_args* a, pfa_fa3_decode_args* d, Plan* pl, int64_t* grid) {
    if (!a) return PFA_ERR_NULL;
    if (a->size != sizeof(pfa_mla_decode_args)) return PFA_ERR_STRUCT_SIZE;
    if (a->flags != 0 || a->reserved != 0) return PFA_ERR_FLAGS;
    if (!a->q || !a->kv_cache || !a->o || !a->cache_seqlens) return PFA_ERR_NULL;
    int st = check_shape(a);
    if (st != PFA_OK) return st;
    if (!pfa::scale_ok(a->softmax_scale)) return PFA_ERR_SHAPE;
    if (a->dtype_in != PFA_DTYPE_BF16 && a->dtype_in != PFA_DTYPE_FP16) return PFA_ERR_DTYPE;
    if (a->dtype_out != a->dtype_in && a->dtype_out != PFA_DTYPE_FP32) return PFA_ERR_DTYPE;
    if (!pfa::multiples_of(8, {a->q_stride_b, a->q_stride_h, a->q_stride_s, a->kv_stride_b, a->kv_stride_s})) return PFA_ERR_STRIDE;
    if (!pfa::multiples_of(4, {a->o_stride_b, a->o_stride_h, a->o_stride_s})) return PFA_ERR_STRIDE;
    // a tile's rows are addressed by 32-bit offsets from a per-tile buffer descriptor
    if (a->kv_stride_s < GeoMla::DQK || a->kv_stride_s * 2 * GeoMla::KT + GeoMla::DQK * 2 > 0x7fffffffLL) return PFA_ERR_STRIDE;
    if (!pfa::aligned16(a->q) || !pfa::aligned16(a->kv_cache) || !pfa::aligned16(a->o)) return PFA_ERR_ALIGN;
    if (!pfa::aligned4(a->lse) || !pfa::aligned4(a->cache_seqlens)) return PFA_ERR_ALIGN;
    st = pfa::check_paging(a->block_table, a->block_table_stride_b, a->page_size, a->num_pages, a->Smax);
    if (st != PFA_OK) return st;
    *d = as_decode(a);
    *pl = decode::plan(d, 0);
    *grid = pfa::dec::mla_grid(a->B, pl->nsplit, pl->nrb);
    return decode::check_launch(d, *pl, *grid);
}

// of arguments that passed check(): "mla_decode<tag>_{bf16|fp16}_{o16|o32}[+combine][_paged]" into buf, the splits into *nsplit -> workgroups
inline int describe(const pfa_mla_decode_args* a, const Plan& pl, int64_t grid, const char* tag, char* buf, size_t n, int32_t* nsplit) {
    if (buf && n)
        snprintf(buf, n, "mla_decode%s_%s_%s%s%s", tag, a->dtype_in == PFA_DTYPE_BF16 ? "bf16" : "fp16", a->dtype_out == PFA_DTYPE_FP32 ? "o32" : "o16",
                 pl.nsplit > 1 ? "+combine" : "", a->block_table ? "_paged" : "");
    if (nsplit) *nsplit = pl.nsplit;
    return (int)grid;
}

}  // namespace mla
}  // namespace pfa

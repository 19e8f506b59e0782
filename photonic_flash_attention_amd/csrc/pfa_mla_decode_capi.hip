// pfa_mla_decode_capi.hip -- C ABI of the MLA decode over a latent KV cache (include/pfa_hip_mla.h, ABI v9 additive): the entry points
// and the 8 instantiations of fa3_mla_decode_kernel (bf16 / fp16 x output x paged) with the 4 of the combine kernel at D = 512.  The
// argument block is this call's own; behind its check it is restated as the pfa_fa3_decode_args of one K/V head at D = 512, so that the
// split rule, the workspace layout and the parameter fill are pfa_decode_host.h's, which every decode unit shares.  A file of its own:
// the other decode objects are built from what they were built from.
// No allocation, no synchronisation, no process-wide state, a grid from host shapes only.
#include "fa3_mla_decode_kernel.h"
#include "pfa_decode_host.h"
#include "pfa_hip_mla.h"

using namespace pfa::decode;
using pfa::dec::DecodeParams;
using pfa::dec::GeoMla;

namespace {

constexpr int kMaxSq = 64;

pfa::KernelFn<DecodeParams> kernel_mla(int dtype, bool out32, bool paged) {
    return pfa::dispatch_bools([](auto bf, auto o32, auto pg) -> pfa::KernelFn<DecodeParams> {
        using T = std::conditional_t<bf.value, __bf16, _Float16>;
        return &pfa::dec::fa3_mla_decode_kernel<T, pfa::out_t<o32.value, T>, pg.value>;
    }, dtype == PFA_DTYPE_BF16, out32, paged);
}
// the shape rules a plan can be made from (the workspace query stops here: it takes no pointers and no strides)
int check_shape(const pfa_mla_decode_args* a) {
    if (!a) return PFA_ERR_NULL;
    if (a->size != sizeof(pfa_mla_decode_args)) return PFA_ERR_STRUCT_SIZE;
    if (a->B <= 0 || a->H <= 0 || a->Smax <= 0 || a->Sq < 1 || a->Sq > kMaxSq) return PFA_ERR_SHAPE;
    return PFA_OK;
}

// the call as the decode of one K/V head at D = 512 whose K and V are the latent cache: what plan() and fill_params() read
pfa_fa3_decode_args as_decode(const pfa_mla_decode_args* a) {
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
int check(const pfa_mla_decode_args* a, pfa_fa3_decode_args* d, Plan* pl, int64_t* grid) {
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
    *pl = plan(d, 0);
    *grid = pfa::dec::mla_grid(a->B, pl->nsplit, pl->nrb);
    return check_launch(d, *pl, *grid);
}

}  // namespace

extern "C" {

size_t pfa_mla_decode_workspace_bytes(const pfa_mla_decode_args* a) {
    if (check_shape(a) != PFA_OK) return 0;
    const pfa_fa3_decode_args d = as_decode(a);
    return plan(&d, 0).ws_bytes;
}

int pfa_mla_decode_check(const pfa_mla_decode_args* a) {
    pfa_fa3_decode_args d;
    Plan pl;
    int64_t grid;
    return check(a, &d, &pl, &grid);
}

int pfa_mla_decode_describe(const pfa_mla_decode_args* a, char* buf, size_t n, int32_t* nsplit) {
    pfa_fa3_decode_args d;
    Plan pl;
    int64_t grid;
    const int st = check(a, &d, &pl, &grid);
    if (st != PFA_OK) return st;
    if (buf && n)
        snprintf(buf, n, "mla_decode_%s_%s%s%s", a->dtype_in == PFA_DTYPE_BF16 ? "bf16" : "fp16", a->dtype_out == PFA_DTYPE_FP32 ? "o32" : "o16",
                 pl.nsplit > 1 ? "+combine" : "", a->block_table ? "_paged" : "");
    if (nsplit) *nsplit = pl.nsplit;
    return (int)grid;
}

int pfa_mla_decode(const pfa_mla_decode_args* a, void* stream) {
    pfa_fa3_decode_args d;
    Plan pl;
    int64_t grid;
    const int st = check(a, &d, &pl, &grid);
    if (st != PFA_OK) return st;
    DecodeParams p;
    fill_params(p, &d, pl);
    const bool out32 = a->dtype_out == PFA_DTYPE_FP32;
    const auto fn = kernel_mla(a->dtype_in, out32, a->block_table != nullptr);
    const auto cfn = combine_at<GeoMla::DV>(a->dtype_in, out32);
    return launch_with_combine(fn, cfn, p, &d, pl, grid, GeoMla::LDS, stream);
}

}  // extern "C"

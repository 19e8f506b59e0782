// pfa_decode_capi.hip -- C ABI of the split-KV decode path (include/pfa_hip.h, ABI v9): validation, the split rule, launches.
// No allocation, no synchronisation, no process-wide state.
#include "pfa_hip.h"

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "fa3_decode_kernel.h"
#include "pfa_host.h"

namespace {

constexpr int kTargetWorkgroups = 512;   // two 4-wave workgroups per CU of the 256-CU part
constexpr int kMinSplitKeys = 256;       // every split covers at least four 64-key tiles
constexpr int kMaxSplits = 128;

struct Plan {
    int G = 1, nrb = 0, nsplit = 1;
    int64_t items = 0;           // workgroups of the main kernel
    size_t ws_bytes = 0;
};

// Everything here depends on shapes only (never on cache_seqlens / key_mask / the block table or the page size), so a captured graph
// stays valid while they change, and a paged call splits exactly as the contiguous call of the same (B, H, Hkv, Sq, Smax, D).
Plan plan(const pfa_fa3_decode_args* a) {
    Plan pl;
    pl.G = a->H / a->Hkv;
    pl.nrb = (int)(((int64_t)a->Sq * pl.G + pfa::dec::ROWS - 1) / pfa::dec::ROWS);
    const int64_t base = (int64_t)a->B * a->Hkv * pl.nrb;
    int64_t ns = (kTargetWorkgroups + base - 1) / base;
    const int64_t max_by_len = a->Smax / kMinSplitKeys > 1 ? a->Smax / kMinSplitKeys : 1;
    if (ns > max_by_len) ns = max_by_len;
    if (ns > kMaxSplits) ns = kMaxSplits;
    if (ns < 1) ns = 1;
    pl.nsplit = (int)ns;
    pl.items = base * ns;
    if (ns > 1) pl.ws_bytes = (size_t)ns * a->B * a->H * a->Sq * (size_t)(a->D + 2) * sizeof(float);
    return pl;
}

int check(const pfa_fa3_decode_args* a) {
    const int st = pfa::check_cache_args(a, 64);
    if (st != PFA_OK) return st;
    const Plan pl = plan(a);
    if (pl.items > 0x7fffffffLL || (int64_t)a->B * a->H * a->Sq * (a->D / 4) / 256 + 1 > 0x7fffffffLL) return PFA_ERR_SHAPE;
    if (pl.ws_bytes) {
        if (!a->workspace || a->workspace_bytes < pl.ws_bytes) return PFA_ERR_NULL;
        if (!pfa::aligned16(a->workspace)) return PFA_ERR_ALIGN;
    }
    return PFA_OK;
}

template <typename T, int D>
const void* main_fn(bool out32, bool paged) {
    if (paged)
        return out32 ? (const void*)&pfa::dec::fa3_decode_kernel<T, D, float, true> : (const void*)&pfa::dec::fa3_decode_kernel<T, D, T, true>;
    return out32 ? (const void*)&pfa::dec::fa3_decode_kernel<T, D, float> : (const void*)&pfa::dec::fa3_decode_kernel<T, D, T>;
}
template <typename T, int D>
const void* combine_fn(bool out32) {
    return out32 ? (const void*)&pfa::dec::fa3_decode_combine_kernel<D, float> : (const void*)&pfa::dec::fa3_decode_combine_kernel<D, T>;
}

}  // namespace

extern "C" {

size_t pfa_fa3_decode_workspace_bytes(const pfa_fa3_decode_args* a) {
    if (!a || a->size != sizeof(pfa_fa3_decode_args) || a->B <= 0 || a->H <= 0 || a->Hkv <= 0 || a->H % a->Hkv != 0 || a->Sq < 1 ||
        a->Smax <= 0 || (a->D != 64 && a->D != 128))
        return 0;
    return plan(a).ws_bytes;
}

int pfa_fa3_decode_check(const pfa_fa3_decode_args* a) { return check(a); }

int pfa_fa3_decode_describe(const pfa_fa3_decode_args* a, char* buf, size_t n, int32_t* nsplit) {
    const int st = check(a);
    if (st != PFA_OK) return st;
    const Plan pl = plan(a);
    if (buf && n)
        snprintf(buf, n, "fa3_decode_%s_d%d_%s%s%s", a->dtype_in == PFA_DTYPE_BF16 ? "bf16" : "fp16", a->D,
                 a->dtype_out == PFA_DTYPE_FP32 ? "o32" : "o16", pl.nsplit > 1 ? "+combine" : "", a->block_table ? "_paged" : "");
    if (nsplit) *nsplit = pl.nsplit;
    return (int)pl.items;
}

int pfa_fa3_decode(const pfa_fa3_decode_args* a, void* stream) {
    const int st = check(a);
    if (st != PFA_OK) return st;
    const Plan pl = plan(a);
    pfa::dec::DecodeParams p;
    p.q = a->q; p.k = a->k_cache; p.v = a->v_cache; p.o = a->o;
    p.lse = a->lse; p.seqlens = a->cache_seqlens; p.key_mask = a->key_mask;
    p.q_sb = a->q_stride_b; p.q_sh = a->q_stride_h; p.q_ss = a->q_stride_s;
    p.k_sb = a->k_stride_b; p.k_sh = a->k_stride_h; p.k_ss = a->k_stride_s;
    p.v_sb = a->v_stride_b; p.v_sh = a->v_stride_h; p.v_ss = a->v_stride_s;
    p.o_sb = a->o_stride_b; p.o_sh = a->o_stride_h; p.o_ss = a->o_stride_s;
    p.km_sb = a->key_mask_stride_b;
    p.part_o = pl.nsplit > 1 ? (float*)a->workspace : nullptr;
    p.part_ml = pl.nsplit > 1 ? (float*)((char*)a->workspace + (size_t)pl.nsplit * a->B * a->H * a->Sq * a->D * sizeof(float)) : nullptr;
    p.B = a->B; p.H = a->H; p.Hkv = a->Hkv; p.G = pl.G; p.Sq = a->Sq; p.Smax = a->Smax; p.nrb = pl.nrb; p.nsplit = pl.nsplit;
    p.causal = a->causal != 0;
    p.scale_log2 = a->softmax_scale * 1.4426950408889634f;
    p.block_table = a->block_table; p.bt_sb = a->block_table_stride_b; p.page_size = a->page_size; p.num_pages = a->num_pages;

    const bool bf = a->dtype_in == PFA_DTYPE_BF16, out32 = a->dtype_out == PFA_DTYPE_FP32, paged = a->block_table != nullptr;
    const void* fn = bf ? (a->D == 128 ? main_fn<__bf16, 128>(out32, paged) : main_fn<__bf16, 64>(out32, paged))
                        : (a->D == 128 ? main_fn<_Float16, 128>(out32, paged) : main_fn<_Float16, 64>(out32, paged));
    const void* cfn = bf ? (a->D == 128 ? combine_fn<__bf16, 128>(out32) : combine_fn<__bf16, 64>(out32))
                         : (a->D == 128 ? combine_fn<_Float16, 128>(out32) : combine_fn<_Float16, 64>(out32));
    const pfa::DeviceScope dev(a->device_id);
    if (pfa::hip_failed(dev.error())) return PFA_ERR_DEVICE;
    void* kargs[] = {&p};
    hipError_t e = hipLaunchKernel(fn, dim3((unsigned)pl.items), dim3(pfa::dec::THREADS), kargs, 0, (hipStream_t)stream);
    if (e == hipSuccess && pl.nsplit > 1) {
        const int64_t threads = (int64_t)a->B * a->H * a->Sq * (a->D / 4);
        e = hipLaunchKernel(cfn, dim3((unsigned)((threads + 255) / 256)), dim3(256), kargs, 0, (hipStream_t)stream);
    }
    return pfa::hip_failed(e) ? PFA_ERR_LAUNCH : PFA_OK;
}

}  // extern "C"

// pfa_decode_fp8_capi.hip -- C ABI of the split-KV decode over an FP8 (e4m3fn) KV cache (include/pfa_hip.h, pfa_fa3_decode_q8*): the
// rules of pfa_fa3_kv_quant, then everything pfa_fa3_decode_ex says of the same argument block, and the launch of the KV8 instantiations of
// fa3_decode_kernel.  The split count, the workgroups and the workspace are asked of the 16-bit call (its plan never sees the cache's
// element type), so the two cannot drift apart.  A file of its own: the 16-bit decode's object is built from what it was built from.
// No allocation, no synchronisation, no process-wide state.
#include "pfa_hip.h"

#include <hip/hip_runtime.h>
#include <stdio.h>

#include "fa3_decode_kernel.h"
#include "pfa_fp8_host.h"

namespace {

// -> PFA_OK, with the 16-bit call's workgroups and split count
int check(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_kv_quant* quant, int* items, int32_t* nsplit) {
    if (!a) return PFA_ERR_NULL;
    if (a->size != sizeof(pfa_fa3_decode_args)) return PFA_ERR_STRUCT_SIZE;
    int st = pfa::check_kv_quant(quant, a);
    if (st != PFA_OK) return st;
    if (ext && ext->size == sizeof(pfa_fa3_cache_ext) && ext->window > 0) return PFA_ERR_FLAGS;
    st = pfa_fa3_decode_describe_ex(a, ext, nullptr, 0, nsplit);
    if (st < 0) return st;
    *items = st;
    return PFA_OK;
}

template <typename T, int D>
const void* main_fn(bool out32, bool paged) {
    if (paged)
        return out32 ? (const void*)&pfa::dec::fa3_decode_kernel<T, D, float, true, false, false, true>
                     : (const void*)&pfa::dec::fa3_decode_kernel<T, D, T, true, false, false, true>;
    return out32 ? (const void*)&pfa::dec::fa3_decode_kernel<T, D, float, false, false, false, true>
                 : (const void*)&pfa::dec::fa3_decode_kernel<T, D, T, false, false, false, true>;
}
template <typename T, int D>
const void* combine_fn(bool out32) {
    return out32 ? (const void*)&pfa::dec::fa3_decode_combine_kernel<D, float> : (const void*)&pfa::dec::fa3_decode_combine_kernel<D, T>;
}

}  // namespace

extern "C" {

size_t pfa_fa3_decode_q8_workspace_bytes(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_kv_quant* quant) {
    if (!a || a->size != sizeof(pfa_fa3_decode_args) || pfa::check_kv_quant(quant, a, false) != PFA_OK) return 0;
    if (ext && ext->size == sizeof(pfa_fa3_cache_ext) && ext->window > 0) return 0;
    return pfa_fa3_decode_workspace_bytes_ex(a, ext);
}

int pfa_fa3_decode_q8_check(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_kv_quant* quant) {
    int items;
    int32_t nsplit;
    return check(a, ext, quant, &items, &nsplit);
}

int pfa_fa3_decode_q8_describe(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_kv_quant* quant, char* buf, size_t n,
                               int32_t* nsplit) {
    int items;
    int32_t ns;
    const int st = check(a, ext, quant, &items, &ns);
    if (st != PFA_OK) return st;
    if (buf && n)
        snprintf(buf, n, "fa3_decode_%s_d%d_%s_kv8%s%s", a->dtype_in == PFA_DTYPE_BF16 ? "bf16" : "fp16", a->D,
                 a->dtype_out == PFA_DTYPE_FP32 ? "o32" : "o16", ns > 1 ? "+combine" : "", a->block_table ? "_paged" : "");
    if (nsplit) *nsplit = ns;
    return items;
}

int pfa_fa3_decode_q8(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_kv_quant* quant, void* stream) {
    int items;
    int32_t nsplit;
    const int st = check(a, ext, quant, &items, &nsplit);
    if (st != PFA_OK) return st;
    pfa::dec::DecodeQ8Params p;
    pfa::fill_attention_params(p, a);
    p.key_mask = a->key_mask; p.km_sb = a->key_mask_stride_b;
    p.part_o = nsplit > 1 ? (float*)a->workspace : nullptr;
    p.part_ml = nsplit > 1 ? (float*)((char*)a->workspace + (size_t)nsplit * a->B * a->H * a->Sq * a->D * sizeof(float)) : nullptr;
    p.Hkv = a->Hkv; p.G = a->H / a->Hkv; p.nrb = (int)(((int64_t)a->Sq * p.G + pfa::dec::ROWS - 1) / pfa::dec::ROWS); p.nsplit = nsplit;
    p.causal = a->causal != 0;
    p.k_descale = quant->k_descale; p.v_descale = quant->v_descale; p.ds_sb = quant->descale_stride_b;

    const bool out32 = a->dtype_out == PFA_DTYPE_FP32, paged = a->block_table != nullptr;
    const void* fn = pfa::dispatch_elem_dim(a->dtype_in, a->D, [&](auto t) { return main_fn<typename decltype(t)::type, decltype(t)::D>(out32, paged); });
    const void* cfn = pfa::dispatch_elem_dim(a->dtype_in, a->D, [&](auto t) { return combine_fn<typename decltype(t)::type, decltype(t)::D>(out32); });
    const pfa::DeviceScope dev(a->device_id);
    if (pfa::hip_failed(dev.error())) return PFA_ERR_DEVICE;
    const int st_main = pfa::launch(fn, dim3((unsigned)items), pfa::dec::THREADS, p, 0, stream);
    if (st_main != PFA_OK || nsplit <= 1) return st_main;
    const int64_t threads = (int64_t)a->B * a->H * a->Sq * (a->D / 4);
    return pfa::launch(cfn, dim3((unsigned)((threads + 255) / 256)), 256, p, 0, stream);
}

}  // extern "C"

// pfa_prefill_host.h -- what pfa_fa3_prefill and pfa_fa3_prefill_varlen share behind their argument blocks (internal): the grid, the
// kernel table, the parameter fill and the launch of fa3_prefill_kernel.  VARLEN picks the ragged instantiations; each of the two
// translation units instantiates one side only, so they still compile side by side.
#pragma once
#include <limits.h>
#include <stdio.h>
#include <string.h>

#include "fa3_prefill_kernel.h"
#include "pfa_fp8_host.h"
#include "pfa_host.h"

namespace pfa {
namespace prefill {

// workgroups: from host shapes only (Sq or max_seqlen_q, never device data), so a captured graph stays valid while cache_seqlens,
// cu_seqlens_q, the block table and the cache change
template <typename Args>
int64_t workgroups(const Args* a) {
    return (int64_t)a->B * a->H * (((int64_t)query_rows(a).Sq + FWD_BLOCK_M - 1) / FWD_BLOCK_M);
}

// The tail of both calls' checks, behind check_cache_args and the call's own rules: the grid, then the extension block.
// -> PFA_OK and the kernel's window (0: none) in *window
template <typename Args>
int check_grid_and_ext(const Args* a, const pfa_fa3_cache_ext* ext, int* window) {
    if (workgroups(a) > 0x7fffffffLL) return PFA_ERR_SHAPE;
    return check_cache_ext(ext, a->causal, a->Smax, window);
}

// fp32 output: P carried as a 16-bit hi + lo pair (SPLITP), as the forward does for its <= 1e-3 mode
template <typename T, int D, bool VARLEN, bool CAUSAL, bool PAGED, bool WINDOW = false>
const void* fn_out(bool out32) {
    return out32 ? (const void*)&fa3_prefill_kernel<T, D, CAUSAL, true, PAGED, float, VARLEN, WINDOW>
                 : (const void*)&fa3_prefill_kernel<T, D, CAUSAL, false, PAGED, T, VARLEN, WINDOW>;
}
// the windowed instantiations exist under the causal flag only
template <typename T, int D, bool VARLEN>
const void* fn_td(bool causal, bool paged, bool out32, bool window) {
    if (window) return paged ? fn_out<T, D, VARLEN, true, true, true>(out32) : fn_out<T, D, VARLEN, true, false, true>(out32);
    if (causal) return paged ? fn_out<T, D, VARLEN, true, true>(out32) : fn_out<T, D, VARLEN, true, false>(out32);
    return paged ? fn_out<T, D, VARLEN, false, true>(out32) : fn_out<T, D, VARLEN, false, false>(out32);
}

// KV8 (pfa_fa3_prefill_q8 / pfa_fa3_prefill_varlen_q8): the instantiations over an FP8 cache, no window
template <typename T, int D, bool VARLEN, bool CAUSAL, bool PAGED>
const void* fn_out_q8(bool out32) {
    return out32 ? (const void*)&fa3_prefill_kernel<T, D, CAUSAL, true, PAGED, float, VARLEN, false, false, true>
                 : (const void*)&fa3_prefill_kernel<T, D, CAUSAL, false, PAGED, T, VARLEN, false, false, true>;
}
template <typename T, int D, bool VARLEN>
const void* fn_td_q8(bool causal, bool paged, bool out32) {
    if (causal) return paged ? fn_out_q8<T, D, VARLEN, true, true>(out32) : fn_out_q8<T, D, VARLEN, true, false>(out32);
    return paged ? fn_out_q8<T, D, VARLEN, false, true>(out32) : fn_out_q8<T, D, VARLEN, false, false>(out32);
}

// of checked arguments: the kernel's name into buf -> workgroups.  `mode` (pfa_fa3_prefill_split: "_split{N}+merge") goes in front of "_paged"
template <bool VARLEN, typename Args>
int describe(const Args* a, int window, char* buf, size_t n, const char* mode = "") {
    if (buf && n)
        snprintf(buf, n, "fa3_prefill_%s_d%d_%s%s%s%s%s%s", a->dtype_in == PFA_DTYPE_BF16 ? "bf16" : "fp16", a->D,
                 a->dtype_out == PFA_DTYPE_FP32 ? "o32" : "o16", a->causal ? "_causal" : "", window ? "_win" : "", VARLEN ? "_varlen" : "",
                 mode, a->block_table ? "_paged" : "");
    return (int)workgroups(a);
}

// what every launch of the kernel fills behind fill_attention_params
template <bool VARLEN, typename Params, typename Args>
void fill_prefill_params(Params& p, const Args* a) {
    fill_attention_params(p, a);
    p.nqblk = (p.Sq + FWD_BLOCK_M - 1) / FWD_BLOCK_M;
    p.kv_group = a->H / a->Hkv;
    if constexpr (VARLEN) {
        p.cu_seqlens_q = a->cu_seqlens_q; p.total_q = a->total_q;
    }
}
// two buffers of a K and a V tile image (<= 64 KiB); the KV8 kernels stage through registers and build the same images
template <typename Args>
size_t lds_bytes(const Args* a) { return (size_t)(2 * 2 * BLOCK_N * a->D * 2); }

// of checked arguments: one launch on `stream`
template <bool VARLEN, typename Args>
int launch(const Args* a, int window, void* stream) {
    typename PrefillParamsOf<VARLEN, true>::type p;   // the window-less kernels take its base, unchanged
    fill_prefill_params<VARLEN>(p, a);
    p.window = window;

    const bool out32 = a->dtype_out == PFA_DTYPE_FP32, paged = a->block_table != nullptr, causal = a->causal != 0, win = window != 0;
    const void* fn = dispatch_elem_dim(a->dtype_in, a->D, [&](auto t) {
        return fn_td<typename decltype(t)::type, decltype(t)::D, VARLEN>(causal, paged, out32, win);
    });
    const DeviceScope dev(a->device_id);
    if (hip_failed(dev.error())) return PFA_ERR_DEVICE;
    return pfa::launch(fn, dim3((unsigned)workgroups(a)), FWD_THREADS, p, lds_bytes(a), stream);
}

// ... over an FP8 cache (a checked pfa_fa3_kv_quant): the KV8 instantiations, same grid, same LDS
template <bool VARLEN, typename Args>
int launch_q8(const Args* a, const pfa_fa3_kv_quant* quant, void* stream) {
    typename PrefillParamsOf<VARLEN, false, false, true>::type p;
    fill_prefill_params<VARLEN>(p, a);
    p.k_descale = quant->k_descale; p.v_descale = quant->v_descale; p.ds_sb = quant->descale_stride_b;

    const bool out32 = a->dtype_out == PFA_DTYPE_FP32, paged = a->block_table != nullptr, causal = a->causal != 0;
    const void* fn = dispatch_elem_dim(a->dtype_in, a->D, [&](auto t) {
        return fn_td_q8<typename decltype(t)::type, decltype(t)::D, VARLEN>(causal, paged, out32);
    });
    const DeviceScope dev(a->device_id);
    if (hip_failed(dev.error())) return PFA_ERR_DEVICE;
    return pfa::launch(fn, dim3((unsigned)workgroups(a)), FWD_THREADS, p, lds_bytes(a), stream);
}

// The checks both q8 calls make in front of the 16-bit call's: the block, the rules of pfa_fa3_kv_quant, no window
template <typename Args>
int check_q8_front(const Args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_kv_quant* quant) {
    if (!a) return PFA_ERR_NULL;
    if (a->size != sizeof(Args)) return PFA_ERR_STRUCT_SIZE;
    const int st = check_kv_quant(quant, a);
    if (st != PFA_OK) return st;
    if (ext && ext->size == sizeof(pfa_fa3_cache_ext) && ext->window > 0) return PFA_ERR_FLAGS;
    return PFA_OK;
}
// "fa3_prefill_..." of the 16-bit describe with "_kv8" behind the output type's part, in front of "_varlen" / "_paged"
inline void name_q8(const char* name16, char* buf, size_t n) {
    if (!buf || !n) return;
    const char* at = strstr(name16, "_varlen");
    if (!at) at = strstr(name16, "_paged");
    if (!at) at = name16 + strlen(name16);
    snprintf(buf, n, "%.*s_kv8%s", (int)(at - name16), name16, at);
}

}  // namespace prefill
}  // namespace pfa

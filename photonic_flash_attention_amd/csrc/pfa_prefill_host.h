// pfa_prefill_host.h -- what the pfa_prefill*_capi.hip units share behind their argument blocks (internal): the grid, the one
// kernel table, the parameter fill and the one launch of fa3_prefill_kernel.  VARLEN / WINDOW / SPLIT / KV8 / SINK are fixed by the unit
// that calls, so each unit instantiates its own kernels only and they still compile side by side.
#pragma once
#include <limits.h>
#include <stdio.h>
#include <string.h>

#include "fa3_prefill_kernel.h"
#include "pfa_fp8_host.h"
#include "pfa_host.h"
#include "pfa_sink_host.h"

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

template <bool VARLEN, bool WINDOW = false, bool SPLIT = false, bool KV8 = false, bool SINK = false>
using Params = typename PrefillParamsOf<VARLEN, WINDOW, SPLIT, KV8, SINK>::type;

// fa3_prefill_kernel for (dtype, D, causal, paged, out) in the mode the caller fixes.  fp32 output: P carried as a 16-bit hi + lo pair
// (SPLITP), as the forward does for its <= 1e-3 mode.  The windowed instantiations exist under the causal flag only and the split
// ones with fp32 output only: validation refuses the rest, and the table has nullptr there, which no launch accepts.
template <bool VARLEN, bool WINDOW = false, bool SPLIT = false, bool KV8 = false, bool SINK = false>
KernelFn<Params<VARLEN, WINDOW, SPLIT, KV8, SINK>> kernel(int dtype, int D, bool causal, bool paged, bool out32) {
    return dispatch_elem_dim(dtype, D, [&](auto t) {
        using T = typename decltype(t)::type;
        return dispatch_bools([](auto c, auto pg, auto o32) -> KernelFn<Params<VARLEN, WINDOW, SPLIT, KV8, SINK>> {
            if constexpr ((WINDOW && !c.value) || (SPLIT && !o32.value)) return nullptr;
            else return &fa3_prefill_kernel<T, decltype(t)::D, c.value, o32.value, pg.value, out_t<o32.value, T>, VARLEN, WINDOW, SPLIT, KV8, SINK>;
        }, causal, paged, out32);
    });
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
template <bool VARLEN, typename Block, typename Args>
void fill_prefill_params(Block& p, const Args* a) {
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

// of checked arguments and a block whose mode's own members (window; descales; split count and parts; sinks) the caller has set: the rest of
// the block and one launch on `stream`, of nsplit times the call's workgroups.  The split parts are fp32 whatever the call's output is.
template <bool VARLEN, bool WINDOW = false, bool SPLIT = false, bool KV8 = false, bool SINK = false, typename Args>
int launch(const Args* a, Params<VARLEN, WINDOW, SPLIT, KV8, SINK>& p, void* stream, int nsplit = 1) {
    fill_prefill_params<VARLEN>(p, a);
    const auto fn = kernel<VARLEN, WINDOW, SPLIT, KV8, SINK>(a->dtype_in, a->D, a->causal != 0, a->block_table != nullptr,
                                                       SPLIT || a->dtype_out == PFA_DTYPE_FP32);
    const DeviceScope dev(a->device_id);
    if (hip_failed(dev.error())) return PFA_ERR_DEVICE;
    return pfa::launch(fn, dim3((unsigned)(workgroups(a) * nsplit)), FWD_THREADS, p, lds_bytes(a), stream);
}
// ... of the 16-bit calls: with the window (0: none) check_grid_and_ext gave
template <bool VARLEN, typename Args>
int launch_windowed(const Args* a, int window, void* stream) {
    if (window) {
        Params<VARLEN, true> p;
        p.window = window;
        return launch<VARLEN, true>(a, p, stream);
    }
    Params<VARLEN> p;
    return launch<VARLEN>(a, p, stream);
}
// ... with sinks (a checked pfa_fa3_sinks): the SINK instantiations, same grid, same LDS
template <bool VARLEN, typename Args>
int launch_windowed_sink(const Args* a, int window, const pfa_fa3_sinks* sinks, void* stream) {
    if (window) {
        Params<VARLEN, true, false, false, true> p;
        p.window = window; p.sinks = sinks->sinks;
        return launch<VARLEN, true, false, false, true>(a, p, stream);
    }
    Params<VARLEN, false, false, false, true> p;
    p.sinks = sinks->sinks;
    return launch<VARLEN, false, false, false, true>(a, p, stream);
}
// ... over an FP8 cache (a checked pfa_fa3_kv_quant): the KV8 instantiations, same grid, same LDS
template <bool VARLEN, typename Args>
int launch_q8(const Args* a, const pfa_fa3_kv_quant* quant, void* stream) {
    Params<VARLEN, false, false, true> p;
    p.k_descale = quant->k_descale; p.v_descale = quant->v_descale; p.ds_sb = quant->descale_stride_b;
    return launch<VARLEN, false, false, true>(a, p, stream);
}

// The checks both q8 calls make in front of the 16-bit call's: the block, the rules of pfa_fa3_kv_quant, no window
template <typename Args>
int check_q8_front(const Args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_kv_quant* quant) {
    if (!a) return PFA_ERR_NULL;
    if (a->size != sizeof(Args)) return PFA_ERR_STRUCT_SIZE;
    const int st = check_kv_quant(quant, a);
    if (st != PFA_OK) return st;
    if (fp8_refuses_window(ext)) return PFA_ERR_FLAGS;
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

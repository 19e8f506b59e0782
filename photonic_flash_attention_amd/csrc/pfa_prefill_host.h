// pfa_prefill_host.h -- what the pfa_prefill*_capi.hip units share behind their argument blocks (internal): validation, the grid, the
// describe, the one kernel table, the parameter fill and the one launch of fa3_prefill_kernel.  VARLEN follows from the argument type; a
// unit names the other mode sets it instantiates (pfa_cache_modes.h: ON, MAY), so each unit instantiates its own kernels only and they
// still compile side by side.
#pragma once
#include <limits.h>
#include <stdio.h>

#include <type_traits>

#include "fa3_prefill_kernel.h"
#include "pfa_cache_modes.h"

static_assert(PFA_PREFILL_MAX_SPLITS == 8, "describe() names the counts 2 .. 8");

namespace pfa {
namespace prefill {

// the ragged call is the one whose argument block says so
template <typename Args>
constexpr bool kVarlen = std::is_same<Args, pfa_fa3_prefill_varlen_args>::value;

// workgroups: from host shapes only (Sq or max_seqlen_q, never device data), so a captured graph stays valid while cache_seqlens,
// cu_seqlens_q, the block table and the cache change
template <typename Args>
int64_t workgroups(const Args* a) {
    return (int64_t)a->B * a->H * (((int64_t)query_rows(a).Sq + FWD_BLOCK_M - 1) / FWD_BLOCK_M);
}

// the rules each call has of its own, behind check_cache_args
inline int check_own_rules(const pfa_fa3_decode_args* a) {
    return a->key_mask ? PFA_ERR_FLAGS : PFA_OK;           // key masks over the cache: pfa_fa3_decode only
}
inline int check_own_rules(const pfa_fa3_prefill_varlen_args* a) {      // (max_seqlen_q < 1 is check_cache_args' Sq < 1)
    if (!a->cu_seqlens_q) return PFA_ERR_NULL;
    if (!aligned4(a->cu_seqlens_q)) return PFA_ERR_ALIGN;
    if (a->total_q < 1 || a->max_seqlen_q > a->total_q) return PFA_ERR_SHAPE;
    return PFA_OK;
}

// The check of the uniform and the ragged call, with whichever blocks the export takes -> PFA_OK and the modes in *m.  KV8: the unit over
// an FP8 cache, whose quant block is not optional.  The grid, then the extension block, come last.
template <bool KV8 = false, typename Args>
int check(const Args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_kv_quant* quant, const pfa_fa3_sinks* sinks, CacheModes* m) {
    *m = CacheModes{};
    int st = check_blocks_front<KV8>(a, ext, quant, sinks);
    if (st != PFA_OK) return st;
    st = check_cache_args(a, INT_MAX);
    if (st != PFA_OK) return st;
    st = check_own_rules(a);
    if (st != PFA_OK) return st;
    if (workgroups(a) > 0x7fffffffLL) return PFA_ERR_SHAPE;
    st = check_cache_ext(ext, a->causal, a->Smax, &m->window);
    if (st != PFA_OK) return st;
    m->quant = quant; m->sinks = sinks;
    return PFA_OK;
}

template <bool VARLEN, bool WINDOW = false, bool SPLIT = false, bool KV8 = false, bool SINK = false>
using Params = typename PrefillParamsOf<VARLEN, WINDOW, SPLIT, KV8, SINK>::type;

// fa3_prefill_kernel for (dtype, D, causal, paged, out) in the mode set the caller fixes.  fp32 output: P carried as a 16-bit hi + lo pair
// (SPLITP), as the forward does for its <= 1e-3 mode.  Where prefill_kernel_exists says no (a window without the causal flag, split parts
// that are not fp32) validation refuses the call, and the table has nullptr, which no launch accepts.
template <bool VARLEN, bool WINDOW = false, bool SPLIT = false, bool KV8 = false, bool SINK = false>
KernelFn<Params<VARLEN, WINDOW, SPLIT, KV8, SINK>> kernel(int dtype, int D, bool causal, bool paged, bool out32) {
    return dispatch_elem_dim(dtype, D, [&](auto t) {
        using T = typename decltype(t)::type;
        return dispatch_bools([](auto c, auto pg, auto o32) -> KernelFn<Params<VARLEN, WINDOW, SPLIT, KV8, SINK>> {
            if constexpr (!prefill_kernel_exists(c.value, o32.value, o32.value ? 4 : 2, VARLEN, WINDOW, SPLIT, KV8, SINK)) return nullptr;
            else return &fa3_prefill_kernel<T, decltype(t)::D, c.value, o32.value, pg.value, out_t<o32.value, T>, VARLEN, WINDOW, SPLIT, KV8, SINK>;
        }, causal, paged, out32);
    });
}

// of checked arguments and their modes: the kernel's name into buf -> workgroups
template <typename Args>
int describe(const Args* a, const CacheModes& m, char* buf, size_t n) {
    static const char* const kSplit[PFA_PREFILL_MAX_SPLITS + 1] = {"", "", "_split2+merge", "_split3+merge", "_split4+merge", "_split5+merge",
                                                                   "_split6+merge", "_split7+merge", "_split8+merge"};
    if (buf && n)
        snprintf(buf, n, "fa3_prefill_%s_d%d_%s%s%s%s%s%s%s%s", a->dtype_in == PFA_DTYPE_BF16 ? "bf16" : "fp16", a->D,
                 a->dtype_out == PFA_DTYPE_FP32 ? "o32" : "o16", a->causal ? "_causal" : "", m.window ? "_win" : "", m.quant ? "_kv8" : "",
                 m.sinks ? "_sink" : "", kVarlen<Args> ? "_varlen" : "", kSplit[m.nsplit], a->block_table ? "_paged" : "");
    return (int)(workgroups(a) * m.nsplit);
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

// of checked arguments and their modes: the block of the call's mode set and one launch on `stream`, of nsplit times the call's workgroups.
// The run-time modes become the kernel's flags here; a set the unit does not name (ON, MAY) instantiates nothing.  The split parts are
// fp32 whatever the call's output is.
template <unsigned ON, unsigned MAY = 0, typename Args>
int launch(const Args* a, const CacheModes& m, void* stream) {
    constexpr bool VARLEN = kVarlen<Args>;
    return dispatch_bools([&](auto w, auto s, auto k8, auto sk) -> int {
        constexpr bool W = w.value, S = s.value, K8 = k8.value, SK = sk.value;
        if constexpr (!unit_has(ON, MAY, mode_bits(W, false, S, K8, SK)) || !prefill_kernel_exists(true, true, 4, VARLEN, W, S, K8, SK)) {
            return PFA_ERR_FLAGS;      // not this unit's: its check lets no such call through
        } else {
            Params<VARLEN, W, S, K8, SK> p;
            fill_prefill_params<VARLEN>(p, a);
            fill_modes<W, false, S, K8, SK>(p, m);
            const auto fn = kernel<VARLEN, W, S, K8, SK>(a->dtype_in, a->D, a->causal != 0, a->block_table != nullptr,
                                                         S || a->dtype_out == PFA_DTYPE_FP32);
            const DeviceScope dev(a->device_id);
            if (hip_failed(dev.error())) return PFA_ERR_DEVICE;
            return pfa::launch(fn, dim3((unsigned)(workgroups(a) * m.nsplit)), FWD_THREADS, p, lds_bytes(a), stream);
        }
    }, m.window != 0, m.nsplit > 1, m.quant != nullptr, m.sinks != nullptr);
}

// The bodies of the entry points of the uniform and the ragged call, written once over Args.  The 16-bit units pass no quant and no
// sinks, the FP8 units (ON has MODE_KV8) no sinks, the sink units no quant.
template <bool KV8 = false, typename Args>
int entry_check(const Args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_kv_quant* quant, const pfa_fa3_sinks* sinks) {
    CacheModes m;
    return check<KV8>(a, ext, quant, sinks, &m);
}
template <bool KV8 = false, typename Args>
int entry_describe(const Args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_kv_quant* quant, const pfa_fa3_sinks* sinks, char* buf, size_t n) {
    CacheModes m;
    const int st = check<KV8>(a, ext, quant, sinks, &m);
    return st != PFA_OK ? st : describe(a, m, buf, n);
}
// the sink-less call of the same arguments: the 16-bit unit's export, whose kernels a sink unit does not have
inline int sinkless(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, void* stream) { return pfa_fa3_prefill_ex(a, ext, stream); }
inline int sinkless(const pfa_fa3_prefill_varlen_args* a, const pfa_fa3_cache_ext* ext, void* stream) { return pfa_fa3_prefill_varlen_ex(a, ext, stream); }
template <unsigned ON, unsigned MAY = 0, typename Args>
int entry_run(const Args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_kv_quant* quant, const pfa_fa3_sinks* sinks, void* stream) {
    if constexpr ((ON & MODE_SINK) != 0)
        if (!sinks) return sinkless(a, ext, stream);       // a NULL block is the sink-less call itself
    CacheModes m;
    const int st = check<(ON & MODE_KV8) != 0>(a, ext, quant, sinks, &m);
    return st != PFA_OK ? st : launch<ON, MAY>(a, m, stream);
}

}  // namespace prefill
}  // namespace pfa

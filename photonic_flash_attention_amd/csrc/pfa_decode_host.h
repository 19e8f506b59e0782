// pfa_decode_host.h -- what pfa_decode_capi.hip, pfa_decode_fp8_capi.hip and pfa_decode_sink_capi.hip share behind pfa_fa3_decode_args (internal): the split rule,
// the kernel tables of fa3_decode_kernel and its combine, the parameter fill with the workspace layout, and the launch with its combine.
// WINDOW / TREE / KV8 / SINK are fixed by the unit that calls, so each unit instantiates its own kernels only.
#pragma once
#include "fa3_decode_kernel.h"
#include "pfa_host.h"

namespace pfa {
namespace decode {

constexpr int kTargetWorkgroups = 512;   // two 4-wave workgroups per CU of the 256-CU part
constexpr int kMinSplitKeys = 256;       // every split covers at least four 64-key tiles
constexpr int kMaxSplits = 128;

struct Plan {
    int G = 1, nrb = 0, nsplit = 1;
    int64_t items = 0;           // workgroups of the main kernel
    size_t ws_bytes = 0;
};

// Everything here depends on shapes and the host window only (never on cache_seqlens / key_mask / the block table or the page size), so a
// captured graph stays valid while they change, and a paged call splits exactly as the contiguous call of the same (B, H, Hkv, Sq, Smax,
// D, window).  window (0: none, else 1 .. Smax): the keys a batch's splits divide are at most window + Sq - 1 and the up to 63 below
// them in the first tile, so that span, rounded to tiles, stands where Smax does -- a 4096-key window over a 128K cache is not cut
// into 128 splits of a few tiles.  The cache's element type plays no part: the FP8 call plans as the 16-bit one.  Nor does a sink.
inline Plan plan(const pfa_fa3_decode_args* a, int window) {
    Plan pl;
    pl.G = a->H / a->Hkv;
    pl.nrb = (int)(((int64_t)a->Sq * pl.G + dec::ROWS - 1) / dec::ROWS);
    const int64_t base = (int64_t)a->B * a->Hkv * pl.nrb;
    int64_t ns = (kTargetWorkgroups + base - 1) / base;
    int64_t keys = a->Smax;
    if (window > 0) {
        const int64_t span = ((int64_t)window + a->Sq - 1 + dec::SPLIT_ALIGN - 1) / dec::SPLIT_ALIGN * dec::SPLIT_ALIGN;
        if (span < keys) keys = span;
    }
    const int64_t max_by_len = keys / kMinSplitKeys > 1 ? keys / kMinSplitKeys : 1;
    if (ns > max_by_len) ns = max_by_len;
    if (ns > kMaxSplits) ns = kMaxSplits;
    if (ns < 1) ns = 1;
    pl.nsplit = (int)ns;
    pl.items = base * ns;
    if (ns > 1) pl.ws_bytes = (size_t)ns * a->B * a->H * a->Sq * (size_t)(a->D + 2) * sizeof(float);
    return pl;
}

template <bool WINDOW, bool TREE = false, bool KV8 = false, bool SINK = false>
using Params = typename dec::DecodeParamsOf<WINDOW, TREE, KV8, SINK>::type;

// fa3_decode_kernel for (dtype, D, out, paged) in the mode the caller fixes
template <bool WINDOW, bool TREE = false, bool KV8 = false, bool SINK = false>
KernelFn<Params<WINDOW, TREE, KV8, SINK>> kernel(int dtype, int D, bool out32, bool paged) {
    return dispatch_elem_dim(dtype, D, [&](auto t) {
        using T = typename decltype(t)::type;
        return dispatch_bools([](auto o32, auto pg) -> KernelFn<Params<WINDOW, TREE, KV8, SINK>> {
            return &dec::fa3_decode_kernel<T, decltype(t)::D, out_t<o32.value, T>, pg.value, WINDOW, TREE, KV8, SINK>;
        }, out32, paged);
    });
}
// ... and the kernel that joins the splits: it reads the DecodeParams every mode's block begins with
inline KernelFn<dec::DecodeParams> combine(int dtype, int D, bool out32) {
    return dispatch_elem_dim(dtype, D, [&](auto t) {
        using T = typename decltype(t)::type;
        return dispatch_bools([](auto o32) -> KernelFn<dec::DecodeParams> { return &dec::fa3_decode_combine_kernel<decltype(t)::D, out_t<o32.value, T>>; },
                              out32);
    });
}

// What every mode's block holds of checked arguments and their plan; the mode's own members (window, tree, descales, sinks) are the caller's.
// The workspace of a split call is the partial O [nsplit][B][H][Sq][D] and behind it the partial (m, l) pairs, both fp32.
inline void fill_params(dec::DecodeParams& p, const pfa_fa3_decode_args* a, const Plan& pl) {
    fill_attention_params(p, a);
    p.key_mask = a->key_mask; p.km_sb = a->key_mask_stride_b;
    p.part_o = pl.nsplit > 1 ? (float*)a->workspace : nullptr;
    p.part_ml = pl.nsplit > 1 ? p.part_o + (size_t)pl.nsplit * a->B * a->H * a->Sq * a->D : nullptr;
    p.Hkv = a->Hkv; p.G = pl.G; p.nrb = pl.nrb; p.nsplit = pl.nsplit;
    p.causal = a->causal != 0;
}

// of checked arguments and a filled block: the main kernel on `stream` and, where the plan splits, the combine behind it
template <bool WINDOW, bool TREE = false, bool KV8 = false, bool SINK = false>
int launch(const pfa_fa3_decode_args* a, const Plan& pl, const Params<WINDOW, TREE, KV8, SINK>& p, void* stream) {
    const bool out32 = a->dtype_out == PFA_DTYPE_FP32;
    const auto fn = kernel<WINDOW, TREE, KV8, SINK>(a->dtype_in, a->D, out32, a->block_table != nullptr);
    const auto cfn = combine(a->dtype_in, a->D, out32);
    const DeviceScope dev(a->device_id);
    if (hip_failed(dev.error())) return PFA_ERR_DEVICE;
    const int st_main = pfa::launch(fn, dim3((unsigned)pl.items), dec::THREADS, p, 0, stream);
    if (st_main != PFA_OK || pl.nsplit <= 1) return st_main;
    const int64_t threads = (int64_t)a->B * a->H * a->Sq * (a->D / 4);
    return pfa::launch(cfn, dim3((unsigned)((threads + 255) / 256)), 256, p, 0, stream);
}

}  // namespace decode
}  // namespace pfa

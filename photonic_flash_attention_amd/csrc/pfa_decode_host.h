// pfa_decode_host.h -- what pfa_decode_capi.hip, pfa_decode_fp8_capi.hip and pfa_decode_sink_capi.hip share behind pfa_fa3_decode_args (internal): the split rule,
// validation, the describe, the kernel tables of fa3_decode_kernel and its combine, the parameter fill with the workspace layout, and the
// launch with its combine.  A unit names the mode sets it instantiates (pfa_cache_modes.h: ON, MAY), so each unit instantiates its own
// kernels only.
#pragma once
#include <stdio.h>

#include "fa3_decode_kernel.h"
#include "pfa_cache_modes.h"

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

// What every mode's block holds of checked arguments and their plan; the mode's own members are fill_modes'.
// The workspace of a split call is the partial O [nsplit][B][H][Sq][D] and behind it the partial (m, l) pairs, both fp32.
inline void fill_params(dec::DecodeParams& p, const pfa_fa3_decode_args* a, const Plan& pl) {
    fill_attention_params(p, a);
    p.key_mask = a->key_mask; p.km_sb = a->key_mask_stride_b;
    p.part_o = pl.nsplit > 1 ? (float*)a->workspace : nullptr;
    p.part_ml = pl.nsplit > 1 ? p.part_o + (size_t)pl.nsplit * a->B * a->H * a->Sq * a->D : nullptr;
    p.Hkv = a->Hkv; p.G = pl.G; p.nrb = pl.nrb; p.nsplit = pl.nsplit;
    p.causal = a->causal != 0;
}

// The tree block's field rules (include/pfa_hip.h, pfa_fa3_tree_mask), in the order their errors are reported; NULL is no tree.
// pointers = false leaves out the two rules about `words` (the workspace query takes no pointers).
inline int check_tree(const pfa_fa3_tree_mask* t, const pfa_fa3_decode_args* a, int window, bool pointers) {
    if (!t) return PFA_OK;
    if (t->size != sizeof(pfa_fa3_tree_mask)) return PFA_ERR_STRUCT_SIZE;
    if (t->flags != 0) return PFA_ERR_FLAGS;
    if (pointers) {
        if (!t->words) return PFA_ERR_NULL;
        if ((reinterpret_cast<uintptr_t>(t->words) & 7u) != 0) return PFA_ERR_ALIGN;
    }
    if (t->stride_b < a->Sq) return PFA_ERR_SHAPE;
    if (a->causal == 0) return PFA_ERR_FLAGS;     // the words replace the causal triangle
    if (window > 0) return PFA_ERR_FLAGS;         // a node's window would be by depth, not by row index
    return PFA_OK;
}

// The optional blocks of the decode calls; a unit passes the ones its exports take
struct Blocks {
    const pfa_fa3_cache_ext* ext = nullptr;
    const pfa_fa3_tree_mask* tree = nullptr;
    const pfa_fa3_kv_quant* quant = nullptr;
    const pfa_fa3_sinks* sinks = nullptr;
};

// Every decode call's check -> PFA_OK, the modes in *m and their plan in *pl.  KV8: the unit over an FP8 cache, whose quant block is
// not optional.  The split count and the workspace never depend on tree, quant or sinks, so a captured graph replays while they change.
template <bool KV8 = false>
int check(const pfa_fa3_decode_args* a, const Blocks& b, CacheModes* m, Plan* pl) {
    *m = CacheModes{};
    int st = check_blocks_front<KV8>(a, b.ext, b.quant, b.sinks);
    if (st != PFA_OK) return st;
    st = check_cache_args(a, 64);
    if (st != PFA_OK) return st;
    st = check_cache_ext(b.ext, a->causal, a->Smax, &m->window);
    if (st != PFA_OK) return st;
    st = check_tree(b.tree, a, m->window, true);
    if (st != PFA_OK) return st;
    *pl = plan(a, m->window);
    if (pl->items > 0x7fffffffLL || (int64_t)a->B * a->H * a->Sq * (a->D / 4) / 256 + 1 > 0x7fffffffLL) return PFA_ERR_SHAPE;
    if (pl->ws_bytes) {
        if (!a->workspace || a->workspace_bytes < pl->ws_bytes) return PFA_ERR_NULL;
        if (!aligned16(a->workspace)) return PFA_ERR_ALIGN;
    }
    m->tree = b.tree; m->quant = b.quant; m->sinks = b.sinks;
    return PFA_OK;
}

// ... of the workspace queries, which stop in front of the pointer rules -> the bytes, 0 for arguments no plan can be made from
template <bool KV8 = false>
size_t workspace_bytes(const pfa_fa3_decode_args* a, const Blocks& b) {
    if (check_blocks_front<KV8>(a, b.ext, b.quant, b.sinks, false) != PFA_OK) return 0;
    if (!a || a->size != sizeof(pfa_fa3_decode_args) || check_cache_shape(a) != PFA_OK) return 0;
    int window;
    if (check_cache_ext(b.ext, a->causal, a->Smax, &window) != PFA_OK || check_tree(b.tree, a, window, false) != PFA_OK) return 0;
    return plan(a, window).ws_bytes;
}

template <bool KV8 = false>
int check_only(const pfa_fa3_decode_args* a, const Blocks& b) {
    CacheModes m;
    Plan pl;
    return check<KV8>(a, b, &m, &pl);
}

// of arguments that pass: the kernel's name into buf, the split count into *nsplit -> workgroups
template <bool KV8 = false>
int describe(const pfa_fa3_decode_args* a, const Blocks& b, char* buf, size_t n, int32_t* nsplit) {
    CacheModes m;
    Plan pl;
    const int st = check<KV8>(a, b, &m, &pl);
    if (st != PFA_OK) return st;
    if (buf && n)
        snprintf(buf, n, "fa3_decode_%s_d%d_%s%s%s%s%s%s", a->dtype_in == PFA_DTYPE_BF16 ? "bf16" : "fp16", a->D,
                 a->dtype_out == PFA_DTYPE_FP32 ? "o32" : "o16", m.tree ? "_tree" : m.window ? "_win" : "", m.quant ? "_kv8" : "",
                 m.sinks ? "_sink" : "", pl.nsplit > 1 ? "+combine" : "", a->block_table ? "_paged" : "");
    if (nsplit) *nsplit = pl.nsplit;
    return (int)pl.items;
}

// of arguments that pass: the block of the call's mode set, the main kernel on `stream` and, where the plan splits, the combine behind it.
// The run-time modes become the kernel's flags here; a set the unit does not name (ON, MAY) instantiates nothing.
template <unsigned ON, unsigned MAY = 0>
int run(const pfa_fa3_decode_args* a, const Blocks& b, void* stream) {
    CacheModes m;
    Plan pl;
    const int st = check<(ON & MODE_KV8) != 0>(a, b, &m, &pl);
    if (st != PFA_OK) return st;
    return dispatch_bools([&](auto w, auto t, auto k8, auto sk) -> int {
        constexpr bool W = w.value, T = t.value, K8 = k8.value, SK = sk.value;
        if constexpr (!unit_has(ON, MAY, mode_bits(W, T, false, K8, SK)) || !dec::decode_kernel_exists(W, T, K8, SK)) {
            return PFA_ERR_FLAGS;      // not this unit's: its check lets no such call through
        } else {
            Params<W, T, K8, SK> p;
            fill_params(p, a, pl);
            fill_modes<W, T, false, K8, SK>(p, m);
            const bool out32 = a->dtype_out == PFA_DTYPE_FP32;
            const auto fn = kernel<W, T, K8, SK>(a->dtype_in, a->D, out32, a->block_table != nullptr);
            const auto cfn = combine(a->dtype_in, a->D, out32);
            const DeviceScope dev(a->device_id);
            if (hip_failed(dev.error())) return PFA_ERR_DEVICE;
            const int st_main = pfa::launch(fn, dim3((unsigned)pl.items), dec::THREADS, p, 0, stream);
            if (st_main != PFA_OK || pl.nsplit <= 1) return st_main;
            const int64_t threads = (int64_t)a->B * a->H * a->Sq * (a->D / 4);
            return pfa::launch(cfn, dim3((unsigned)((threads + 255) / 256)), 256, p, 0, stream);
        }
    }, m.window != 0, m.tree != nullptr, m.quant != nullptr, m.sinks != nullptr);
}

}  // namespace decode
}  // namespace pfa

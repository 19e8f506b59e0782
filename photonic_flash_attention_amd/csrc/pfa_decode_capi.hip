// pfa_decode_capi.hip -- C ABI of the split-KV decode path (include/pfa_hip.h, ABI v9): validation, the split rule, launches.
// One body per entry point: the *_tree calls; the *_ex calls are those with no tree, the plain calls those with no extension either.
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

// Everything here depends on shapes and the host window only (never on cache_seqlens / key_mask / the block table or the page size), so a
// captured graph stays valid while they change, and a paged call splits exactly as the contiguous call of the same (B, H, Hkv, Sq, Smax,
// D, window).  window (0: none, else 1 .. Smax): the keys a batch's splits divide are at most window + Sq - 1 and the up to 63 below
// them in the first tile, so that span, rounded to tiles, stands where Smax does -- a 4096-key window over a 128K cache is not cut
// into 128 splits of a few tiles.
Plan plan(const pfa_fa3_decode_args* a, int window) {
    Plan pl;
    pl.G = a->H / a->Hkv;
    pl.nrb = (int)(((int64_t)a->Sq * pl.G + pfa::dec::ROWS - 1) / pfa::dec::ROWS);
    const int64_t base = (int64_t)a->B * a->Hkv * pl.nrb;
    int64_t ns = (kTargetWorkgroups + base - 1) / base;
    int64_t keys = a->Smax;
    if (window > 0) {
        const int64_t span = ((int64_t)window + a->Sq - 1 + pfa::dec::SPLIT_ALIGN - 1) / pfa::dec::SPLIT_ALIGN * pfa::dec::SPLIT_ALIGN;
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

// The tree block's field rules (include/pfa_hip.h, pfa_fa3_tree_mask), in the order their errors are reported; NULL is no tree.
// pointers = false leaves out the two rules about `words` (the workspace query takes no pointers).
int check_tree(const pfa_fa3_tree_mask* t, const pfa_fa3_decode_args* a, int window, bool pointers) {
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

// -> PFA_OK and the kernels' window (0: none) in *window
int check(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_tree_mask* tree, int* window) {
    int st = pfa::check_cache_args(a, 64);
    if (st != PFA_OK) return st;
    st = pfa::check_cache_ext(ext, a->causal, a->Smax, window);
    if (st != PFA_OK) return st;
    st = check_tree(tree, a, *window, true);
    if (st != PFA_OK) return st;
    const Plan pl = plan(a, *window);
    if (pl.items > 0x7fffffffLL || (int64_t)a->B * a->H * a->Sq * (a->D / 4) / 256 + 1 > 0x7fffffffLL) return PFA_ERR_SHAPE;
    if (pl.ws_bytes) {
        if (!a->workspace || a->workspace_bytes < pl.ws_bytes) return PFA_ERR_NULL;
        if (!pfa::aligned16(a->workspace)) return PFA_ERR_ALIGN;
    }
    return PFA_OK;
}

template <typename T, int D, bool WINDOW, bool TREE>
const void* main_fn(bool out32, bool paged) {
    if (paged)
        return out32 ? (const void*)&pfa::dec::fa3_decode_kernel<T, D, float, true, WINDOW, TREE>
                     : (const void*)&pfa::dec::fa3_decode_kernel<T, D, T, true, WINDOW, TREE>;
    return out32 ? (const void*)&pfa::dec::fa3_decode_kernel<T, D, float, false, WINDOW, TREE>
                 : (const void*)&pfa::dec::fa3_decode_kernel<T, D, T, false, WINDOW, TREE>;
}
template <bool WINDOW, bool TREE = false>
const void* main_fn(int dtype, int D, bool out32, bool paged) {
    return pfa::dispatch_elem_dim(dtype, D, [&](auto t) { return main_fn<typename decltype(t)::type, decltype(t)::D, WINDOW, TREE>(out32, paged); });
}
template <typename T, int D>
const void* combine_fn(bool out32) {
    return out32 ? (const void*)&pfa::dec::fa3_decode_combine_kernel<D, float> : (const void*)&pfa::dec::fa3_decode_combine_kernel<D, T>;
}

}  // namespace

extern "C" {

size_t pfa_fa3_decode_tree_workspace_bytes(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_tree_mask* tree) {
    if (!a || a->size != sizeof(pfa_fa3_decode_args) || pfa::check_cache_shape(a) != PFA_OK) return 0;
    int window;
    if (pfa::check_cache_ext(ext, a->causal, a->Smax, &window) != PFA_OK || check_tree(tree, a, window, false) != PFA_OK) return 0;
    return plan(a, window).ws_bytes;
}

int pfa_fa3_decode_tree_check(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_tree_mask* tree) {
    int window;
    return check(a, ext, tree, &window);
}

int pfa_fa3_decode_tree_describe(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_tree_mask* tree, char* buf, size_t n,
                                 int32_t* nsplit) {
    int window;
    const int st = check(a, ext, tree, &window);
    if (st != PFA_OK) return st;
    const Plan pl = plan(a, window);
    if (buf && n)
        snprintf(buf, n, "fa3_decode_%s_d%d_%s%s%s%s", a->dtype_in == PFA_DTYPE_BF16 ? "bf16" : "fp16", a->D,
                 a->dtype_out == PFA_DTYPE_FP32 ? "o32" : "o16", tree ? "_tree" : window ? "_win" : "", pl.nsplit > 1 ? "+combine" : "",
                 a->block_table ? "_paged" : "");
    if (nsplit) *nsplit = pl.nsplit;
    return (int)pl.items;
}

// The split count and the workspace are those of the call without a tree (plan() never sees it), so a captured graph replays while
// the words change with lengths, table and cache.
int pfa_fa3_decode_tree(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_tree_mask* tree, void* stream) {
    int window;
    const int st = check(a, ext, tree, &window);
    if (st != PFA_OK) return st;
    const Plan pl = plan(a, window);
    pfa::dec::DecodeWinParams p;    // the window-less kernels take its DecodeParams base, unchanged
    pfa::fill_attention_params(p, a);
    p.key_mask = a->key_mask; p.km_sb = a->key_mask_stride_b;
    p.part_o = pl.nsplit > 1 ? (float*)a->workspace : nullptr;
    p.part_ml = pl.nsplit > 1 ? (float*)((char*)a->workspace + (size_t)pl.nsplit * a->B * a->H * a->Sq * a->D * sizeof(float)) : nullptr;
    p.Hkv = a->Hkv; p.G = pl.G; p.nrb = pl.nrb; p.nsplit = pl.nsplit;
    p.causal = a->causal != 0;
    p.window = window;

    const bool out32 = a->dtype_out == PFA_DTYPE_FP32, paged = a->block_table != nullptr;
    const void* fn = tree     ? main_fn<false, true>(a->dtype_in, a->D, out32, paged)
                     : window ? main_fn<true>(a->dtype_in, a->D, out32, paged)
                              : main_fn<false>(a->dtype_in, a->D, out32, paged);
    const void* cfn = pfa::dispatch_elem_dim(a->dtype_in, a->D, [&](auto t) { return combine_fn<typename decltype(t)::type, decltype(t)::D>(out32); });
    const pfa::DeviceScope dev(a->device_id);
    if (pfa::hip_failed(dev.error())) return PFA_ERR_DEVICE;
    int st_main;
    if (tree) {
        pfa::dec::DecodeTreeParams tp;
        static_cast<pfa::dec::DecodeParams&>(tp) = p;
        tp.tree = tree->words; tp.tree_sb = tree->stride_b;
        st_main = pfa::launch(fn, dim3((unsigned)pl.items), pfa::dec::THREADS, tp, 0, stream);
    } else {
        st_main = pfa::launch(fn, dim3((unsigned)pl.items), pfa::dec::THREADS, p, 0, stream);
    }
    if (st_main != PFA_OK || pl.nsplit <= 1) return st_main;
    const int64_t threads = (int64_t)a->B * a->H * a->Sq * (a->D / 4);
    return pfa::launch(cfn, dim3((unsigned)((threads + 255) / 256)), 256, p, 0, stream);
}

// the calls without a tree
size_t pfa_fa3_decode_workspace_bytes_ex(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext) {
    return pfa_fa3_decode_tree_workspace_bytes(a, ext, nullptr);
}
int pfa_fa3_decode_check_ex(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext) { return pfa_fa3_decode_tree_check(a, ext, nullptr); }
int pfa_fa3_decode_describe_ex(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, char* buf, size_t n, int32_t* nsplit) {
    return pfa_fa3_decode_tree_describe(a, ext, nullptr, buf, n, nsplit);
}
int pfa_fa3_decode_ex(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, void* stream) { return pfa_fa3_decode_tree(a, ext, nullptr, stream); }

// ... and without the extension block
size_t pfa_fa3_decode_workspace_bytes(const pfa_fa3_decode_args* a) { return pfa_fa3_decode_workspace_bytes_ex(a, nullptr); }
int pfa_fa3_decode_check(const pfa_fa3_decode_args* a) { return pfa_fa3_decode_check_ex(a, nullptr); }
int pfa_fa3_decode_describe(const pfa_fa3_decode_args* a, char* buf, size_t n, int32_t* nsplit) {
    return pfa_fa3_decode_describe_ex(a, nullptr, buf, n, nsplit);
}
int pfa_fa3_decode(const pfa_fa3_decode_args* a, void* stream) { return pfa_fa3_decode_ex(a, nullptr, stream); }

}  // extern "C"

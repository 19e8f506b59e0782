// pfa_decode_capi.hip -- C ABI of the split-KV decode path (include/pfa_hip.h, ABI v9): validation and the calls; the split rule, the
// kernel table, the parameter fill and the launches are pfa_decode_host.h's, which the FP8 unit shares.
// One body per entry point: the *_tree calls; the *_ex calls are those with no tree, the plain calls those with no extension either.
// No allocation, no synchronisation, no process-wide state.
#include <stdio.h>

#include "pfa_decode_host.h"

namespace {

using pfa::decode::Plan;
using pfa::decode::plan;

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
    if (tree) {
        pfa::dec::DecodeTreeParams p;
        pfa::decode::fill_params(p, a, pl);
        p.tree = tree->words; p.tree_sb = tree->stride_b;
        return pfa::decode::launch<false, true>(a, pl, p, stream);
    }
    if (window) {
        pfa::dec::DecodeWinParams p;
        pfa::decode::fill_params(p, a, pl);
        p.window = window;
        return pfa::decode::launch<true>(a, pl, p, stream);
    }
    pfa::dec::DecodeParams p;
    pfa::decode::fill_params(p, a, pl);
    return pfa::decode::launch<false>(a, pl, p, stream);
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

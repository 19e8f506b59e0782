// pfa_cache_modes.h -- the modes of one call over a KV cache (internal): what a passed check hands to the describe and to the launch of
// pfa_decode_host.h, pfa_prefill_host.h and pfa_prefill_split_host.h, the bits a unit names its instantiations with, and the field rules
// of pfa_fa3_sinks (those of pfa_fa3_cache_ext are pfa_host.h's, those of pfa_fa3_kv_quant pfa_fp8_host.h's).
#pragma once
#include "pfa_fp8_host.h"
#include "pfa_host.h"

namespace pfa {

// The optional blocks of a call as its check found them: null (0) for a mode that is off.  The kernels' template flags follow from it.
struct CacheModes {
    int window = 0;                            // of pfa_fa3_cache_ext, clamped to Smax (check_cache_ext)
    const pfa_fa3_tree_mask* tree = nullptr;   // decode only
    const pfa_fa3_kv_quant* quant = nullptr;
    const pfa_fa3_sinks* sinks = nullptr;
    int nsplit = 1;                            // pfa_fa3_prefill_split only: the resolved count and, above 1, the two workspace bases
    float* part_o = nullptr;
    float* part_lse = nullptr;
};

// A unit names the mode sets it instantiates by two masks: ON, the modes every kernel of the unit has, and MAY, those a call may add.
// A set outside them is unreachable behind the unit's check, and the dispatchers instantiate nothing for it.
enum : unsigned { MODE_WINDOW = 1, MODE_TREE = 2, MODE_SPLIT = 4, MODE_KV8 = 8, MODE_SINK = 16 };
constexpr unsigned mode_bits(bool window, bool tree, bool split, bool kv8, bool sink) {
    return (window ? MODE_WINDOW : 0u) | (tree ? MODE_TREE : 0u) | (split ? MODE_SPLIT : 0u) | (kv8 ? MODE_KV8 : 0u) | (sink ? MODE_SINK : 0u);
}
constexpr bool unit_has(unsigned ON, unsigned MAY, unsigned set) { return (set & ON) == ON && (set & ~(ON | MAY)) == 0; }

// include/pfa_hip.h, pfa_fa3_sinks, in the order the errors are reported; the caller has seen that the block is there (a NULL block is
// the sibling call).  pointers = false leaves out the two rules about `sinks` (a workspace query takes no pointers).
inline int check_sinks(const pfa_fa3_sinks* s, bool pointers = true) {
    if (s->size != sizeof(pfa_fa3_sinks)) return PFA_ERR_STRUCT_SIZE;
    if (s->flags != 0) return PFA_ERR_FLAGS;
    if (pointers) {
        if (!s->sinks) return PFA_ERR_NULL;
        if (!aligned4(s->sinks)) return PFA_ERR_ALIGN;
    }
    return PFA_OK;
}

// What the calls with more blocks check in front of the plain call's rules (`a` itself is not looked at before FP8 is): the sink block's
// own rules where there is one, then for a unit over an FP8 cache (KV8) the argument block's NULL and size, the rules of
// pfa_fa3_kv_quant and the refusal of a window.  pointers = false: for a workspace query.
template <bool KV8, typename Args>
inline int check_blocks_front(const Args* a, const pfa_fa3_cache_ext* ext, const pfa_fa3_kv_quant* quant, const pfa_fa3_sinks* sinks,
                              bool pointers = true) {
    if (sinks) {
        const int st = check_sinks(sinks, pointers);
        if (st != PFA_OK) return st;
    }
    if constexpr (KV8) {
        if (!a) return PFA_ERR_NULL;
        if (a->size != sizeof(Args)) return PFA_ERR_STRUCT_SIZE;
        const int st = check_kv_quant(quant, a, pointers);
        if (st != PFA_OK) return st;
        if (fp8_refuses_window(ext)) return PFA_ERR_FLAGS;
    }
    return PFA_OK;
}

// The mode members of a kernel's argument block (fa3_decode_kernel.h, fa3_prefill_kernel.h: the parts' members have one name in both)
template <bool WINDOW, bool TREE, bool SPLIT, bool KV8, bool SINK, typename Block>
inline void fill_modes(Block& p, const CacheModes& m) {
    if constexpr (WINDOW) p.window = m.window;
    if constexpr (TREE) {
        p.tree = m.tree->words; p.tree_sb = m.tree->stride_b;
    }
    if constexpr (SPLIT) {
        p.nsplit = m.nsplit; p.part_o = m.part_o; p.part_lse = m.part_lse;
    }
    if constexpr (KV8) {
        p.k_descale = m.quant->k_descale; p.v_descale = m.quant->v_descale; p.ds_sb = m.quant->descale_stride_b;
    }
    if constexpr (SINK) p.sinks = m.sinks->sinks;
}

}  // namespace pfa

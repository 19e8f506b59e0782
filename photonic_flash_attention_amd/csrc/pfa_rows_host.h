// pfa_rows_host.h -- the host rules of a "rows" argument block, once: pfa_rotary_args, pfa_qk_norm_args and pfa_qk_norm_bwd_args describe
// one or two 16-bit tensors (x0 with H0 heads, optionally x1 with H1) over the same rows, dense [B, H, S, D] by strides or packed
// [total, H, D] with cu_seqlens, positions from position_ids or pos_offsets, fp32 tables [max_pos, rot_dim / 2].  The fields have one
// name in all three blocks, so every rule is a template over the block; a call's check() states them in ITS order (which of two
// broken rules wins is part of the ABI) and keeps what is its own: head dims, dtypes, weights, workspace, kernels.
#pragma once
#include <initializer_list>

#include "pfa_host.h"

namespace pfa {
namespace rows {

constexpr int kPiece = 16;     // a work item is 16 elements of a row: a rotation's pairs lie inside it
constexpr int64_t kLim = 0x7fffffffLL;

// ---- pointers ------------------------------------------------------------------------------------------------------------------------
template <typename A>
bool positions_exclusive(const A* a) { return !(a->position_ids && a->pos_offsets); }
// the forward blocks: in place is x_out == x, for both tensors or for neither
template <typename A>
bool in_place(const A* a) { return a->x0_out == a->x0; }
template <typename A>
bool in_place_consistent(const A* a) { return !(a->x1 && a->x1_out && (a->x1_out == a->x1) != in_place(a)); }
// every pointer NULL exactly when `none`: the x1 fields with H1 == 0, the tables with rot_dim == 0
inline bool null_iff(bool none, std::initializer_list<const void*> ptrs) {
    for (const void* p : ptrs)
        if ((p == nullptr) != none) return false;
    return true;
}
inline bool all_aligned16(std::initializer_list<const void*> ptrs) {
    for (const void* p : ptrs)
        if (!aligned16(p)) return false;
    return true;
}
template <typename A>
bool ints_aligned(const A* a) { return aligned4(a->cu_seqlens) && aligned4(a->pos_offsets) && aligned4(a->position_ids); }

// ---- shapes --------------------------------------------------------------------------------------------------------------------------
// rot_optional: rot_dim == 0 is the call without a rotation, which has no tables and asks nothing of max_pos
template <typename A>
bool shape_ok(const A* a, bool rot_optional) {
    if (a->B < 1 || a->S < 1 || a->H0 < 1 || a->H1 < 0) return false;
    if (!(rot_optional && a->rot_dim == 0) && a->max_pos < 1) return false;
    return !a->cu_seqlens || (a->total >= 1 && a->S <= a->total);
}
template <typename A>
bool rot_dim_ok(const A* a, bool rot_optional) {
    if (rot_optional && a->rot_dim == 0) return true;
    return a->rot_dim >= kPiece && a->rot_dim % kPiece == 0 && a->rot_dim <= a->D;
}
template <typename A>
bool tables_ok(const A* a) { return a->rot_dim == 0 || (a->cs_stride % 4 == 0 && a->cs_stride >= a->rot_dim / 2); }

// ---- strides of the forward blocks (x0, x0o, x1, x1o) ----------------------------------------------------------------------------------
template <typename A>
bool fwd_strides_ok(const A* a) {
    if (!multiples_of(8, {a->x0_stride_s, a->x0_stride_h, a->x0o_stride_s, a->x0o_stride_h, a->x1_stride_s, a->x1_stride_h, a->x1o_stride_s,
                          a->x1o_stride_h}))
        return false;
    return a->cu_seqlens || multiples_of(8, {a->x0_stride_b, a->x0o_stride_b, a->x1_stride_b, a->x1o_stride_b});
}
// in place is the same tensor: an item reads what it writes and nothing else
template <typename A>
bool in_place_strides_equal(const A* a) {
    if (a->x0o_stride_s != a->x0_stride_s || a->x0o_stride_h != a->x0_stride_h || a->x1o_stride_s != a->x1_stride_s ||
        a->x1o_stride_h != a->x1_stride_h)
        return false;
    return a->cu_seqlens || (a->x0o_stride_b == a->x0_stride_b && a->x1o_stride_b == a->x1_stride_b);
}

// ---- grids ---------------------------------------------------------------------------------------------------------------------------
template <typename A>
int64_t units(const A* a, int head_elems) { return ((int64_t)a->H0 + a->H1) * (head_elems / kPiece); }     // items of a row
template <typename A>
int64_t nchunk(const A* a, int64_t units, int threads) { return ((int64_t)a->S * units + threads - 1) / threads; }
template <typename A>
int64_t workgroups(const A* a, int64_t units, int threads) {     // saturated so that the product cannot wrap
    const int64_t n = nchunk(a, units, threads);
    return n > kLim ? kLim + 1 : (int64_t)a->B * n;
}
// a sequence's item index inside 32 bits
template <typename A>
bool items_fit(const A* a, int64_t units, int threads) { return (int64_t)a->S * units + threads <= kLim; }

// ---- kernel parameters ---------------------------------------------------------------------------------------------------------------
template <typename Params, typename A>
void fill_common(Params& p, const A* a) {
    p.cos = a->cos; p.sin = a->sin;
    p.cu_seqlens = a->cu_seqlens; p.pos_offsets = a->pos_offsets; p.position_ids = a->position_ids;
    p.pid_sb = a->pid_stride_b; p.pid_ss = a->pid_stride_s; p.cs_stride = a->cs_stride;
    p.S = a->S; p.total = a->total; p.H0 = a->H0;
    p.runits = a->rot_dim / kPiece;
    p.max_pos = a->max_pos;
}
template <typename Params, typename A>
void fill_fwd(Params& p, const A* a, int64_t units, int threads) {     // a forward block: fill_common, the four tensors and the grid
    fill_common(p, a);
    p.x0 = a->x0; p.x0_out = a->x0_out; p.x1 = a->x1; p.x1_out = a->x1_out;
    PFA_FILL_STRIDES(p, a, x0); PFA_FILL_STRIDES(p, a, x0o); PFA_FILL_STRIDES(p, a, x1); PFA_FILL_STRIDES(p, a, x1o);
    p.nchunk = (int32_t)nchunk(a, units, threads);
    p.units = (int32_t)units;
}

}  // namespace rows
}  // namespace pfa

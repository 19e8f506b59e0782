// pfa_prefill_split_host.h -- what pfa_prefill_split_capi.hip and pfa_prefill_split_sink_capi.hip share behind pfa_fa3_prefill_split's
// arguments (internal): the plan of key_splits = 0, the workspace layout, the merge's argument block, validation, and the bodies of the
// entry points: the launch of fa3_prefill_kernel's SPLIT instantiations (with MODE_SINK in the sink unit) and the merge behind it.
#pragma once
#include "pfa_prefill_host.h"

static_assert(PFA_PREFILL_MAX_SPLITS == PFA_MERGE_MAX_PARTS, "one merge joins every split");

namespace pfa {
namespace prefill_split {

// The plan of key_splits = 0, set from profiles/prefill_split.md (H 32 / Hkv 8, D 128, chunks of 256 .. 2048 rows over 8192 .. 131072 keys).
constexpr int kTargetWorkgroups = 256;   // one D = 128 workgroup per CU: every measured row with 512 workgroups lost against 256
constexpr int kMinSplitKeys = 1024;      // a split covers at least sixteen 64-key tiles of capacity: the smallest share measured, and it wins

// From (B, H, Sq, Smax) only -- never pointers, lengths, the block table or the page size -- so a captured graph stays valid while they
// change and a paged call plans like the contiguous one: the largest count that keeps B * H * ceil(Sq / 256) * N within the target (the
// splits then run in one round; a count that spills into a second round was slower than the next smaller one wherever it was measured),
// capped by the keys a split must hold and by the merge's part limit.
inline int plan(const pfa_fa3_decode_args* a) {
    const int64_t base = prefill::workgroups(a);
    int64_t ns = kTargetWorkgroups / base;
    const int64_t max_by_len = a->Smax / kMinSplitKeys;
    if (ns > max_by_len) ns = max_by_len;
    if (ns > PFA_PREFILL_MAX_SPLITS) ns = PFA_PREFILL_MAX_SPLITS;
    return ns < 1 ? 1 : (int)ns;
}

// of shape-checked arguments -> the resolved count 1 .. 8, or PFA_ERR_SHAPE
inline int resolve(const pfa_fa3_decode_args* a, int32_t key_splits) {
    if (key_splits < 0 || key_splits > PFA_PREFILL_MAX_SPLITS) return PFA_ERR_SHAPE;
    return key_splits ? key_splits : plan(a);
}

// the rules a plan can be made from (pfa_fa3_prefill_split_plan and _workspace_bytes stop here: no pointers, no strides)
inline int resolve_from_shapes(const pfa_fa3_decode_args* a, int32_t key_splits) {
    if (!a) return PFA_ERR_NULL;
    if (a->size != sizeof(pfa_fa3_decode_args)) return PFA_ERR_STRUCT_SIZE;
    const int st = check_cache_shape(a);
    return st != PFA_OK ? st : resolve(a, key_splits);
}

inline int64_t part_elems(const pfa_fa3_decode_args* a) { return (int64_t)a->B * a->Sq * a->H * a->D; }   // of one split's partial O
inline int64_t part_rows(const pfa_fa3_decode_args* a) { return (int64_t)a->B * a->H * a->Sq; }           // ... and of its partial LSE
inline size_t workspace_bytes(const pfa_fa3_decode_args* a, int nsplit) {
    return nsplit > 1 ? (size_t)nsplit * (size_t)(part_elems(a) + part_rows(a)) * sizeof(float) : 0;
}

// The merge of the N parts in the workspace, in split order, into a->o / a->lse: the workspace layout as pfa_attn_merge's argument block.
inline pfa_attn_merge_args merge_args(const pfa_fa3_decode_args* a, int nsplit) {
    pfa_attn_merge_args m = {};
    m.size = sizeof(m);
    const float* part_o = (const float*)a->workspace;
    const float* part_lse = part_o + (int64_t)nsplit * part_elems(a);
    for (int n = 0; n < nsplit; ++n) {
        m.o_part[n] = part_o + n * part_elems(a);                       // [B][Sq][H][D]
        m.op_stride_b[n] = (int64_t)a->Sq * a->H * a->D; m.op_stride_s[n] = (int64_t)a->H * a->D; m.op_stride_h[n] = a->D;
        m.lse_part[n] = part_lse + n * part_rows(a);                    // [B][H][Sq]
        m.lp_stride_b[n] = (int64_t)a->H * a->Sq; m.lp_stride_h[n] = a->Sq; m.lp_stride_s[n] = 1;
    }
    m.o = a->o; m.o_stride_b = a->o_stride_b; m.o_stride_h = a->o_stride_h; m.o_stride_s = a->o_stride_s;
    m.lse_out = a->lse; m.lo_stride_b = (int64_t)a->H * a->Sq; m.lo_stride_h = a->Sq; m.lo_stride_s = 1;
    m.n_parts = nsplit; m.B = a->B; m.H = a->H; m.Sq = a->Sq; m.D = a->D;
    m.dtype_part = PFA_DTYPE_FP32; m.dtype_out = a->dtype_out; m.device_id = a->device_id;
    return m;
}

// -> PFA_OK and the modes in *m: the resolved count and, above 1, the workspace bases; the sinks (NULL: none), whose own rules come
// first.  A count of 1 is pfa_fa3_prefill's check and nothing else.
inline int check(const pfa_fa3_decode_args* a, int32_t key_splits, const pfa_fa3_sinks* sinks, CacheModes* m) {
    *m = CacheModes{};
    int st = check_blocks_front<false>(a, nullptr, nullptr, sinks);
    if (st != PFA_OK) return st;
    st = check_cache_args(a, INT_MAX);
    if (st != PFA_OK) return st;
    st = prefill::check_own_rules(a);
    if (st != PFA_OK) return st;
    const int ns = resolve(a, key_splits);
    if (ns < 0) return ns;
    if (prefill::workgroups(a) * ns > 0x7fffffffLL) return PFA_ERR_SHAPE;
    m->sinks = sinks;
    if (ns == 1) return PFA_OK;
    // the merge writes o: a 16-bit o in rows of 8 elements
    if (a->dtype_out != PFA_DTYPE_FP32 && !multiples_of(8, {a->o_stride_b, a->o_stride_h, a->o_stride_s})) return PFA_ERR_STRIDE;
    if (!a->workspace || a->workspace_bytes < workspace_bytes(a, ns)) return PFA_ERR_NULL;
    if (!aligned16(a->workspace)) return PFA_ERR_ALIGN;
    const pfa_attn_merge_args mg = merge_args(a, ns);
    st = pfa_attn_merge_check(&mg);           // what is left of its rules: the merge's own grid
    if (st != PFA_OK) return st;
    m->nsplit = ns;
    m->part_o = (float*)a->workspace;
    m->part_lse = m->part_o + (int64_t)ns * part_elems(a);
    return PFA_OK;
}

// the bodies of the entry points, with and without sinks
inline size_t entry_workspace_bytes(const pfa_fa3_decode_args* a, int32_t key_splits, const pfa_fa3_sinks* sinks) {
    if (sinks && check_sinks(sinks, false) != PFA_OK) return 0;
    const int ns = resolve_from_shapes(a, key_splits);
    return ns < 0 ? 0 : workspace_bytes(a, ns);
}
inline int entry_check(const pfa_fa3_decode_args* a, int32_t key_splits, const pfa_fa3_sinks* sinks) {
    CacheModes m;
    return check(a, key_splits, sinks, &m);
}
inline int entry_describe(const pfa_fa3_decode_args* a, int32_t key_splits, const pfa_fa3_sinks* sinks, char* buf, size_t n, int32_t* nsplit) {
    CacheModes m;
    const int st = check(a, key_splits, sinks, &m);
    if (st != PFA_OK) return st;
    if (nsplit) *nsplit = m.nsplit;
    return prefill::describe(a, m, buf, n);
}
// ON: MODE_SPLIT, with MODE_SINK in the sink unit.  A count of 1 is the unsplit call (its export: the kernel function, grid and bits are
// that unit's); above 1 the SPLIT kernel into the workspace (SINK: with the sinks, which split 0 of every q block carries) and
// pfa_attn_merge, unchanged, behind it.
template <unsigned ON>
int entry_run(const pfa_fa3_decode_args* a, int32_t key_splits, const pfa_fa3_sinks* sinks, void* stream) {
    if constexpr ((ON & MODE_SINK) != 0)
        if (!sinks) return pfa_fa3_prefill_split(a, key_splits, stream);       // a NULL block is the sink-less call itself
    CacheModes m;
    const int st = check(a, key_splits, sinks, &m);
    if (st != PFA_OK) return st;
    if (m.nsplit == 1) {
        if constexpr ((ON & MODE_SINK) != 0) return pfa_fa3_prefill_sink(a, nullptr, sinks, stream);
        else return pfa_fa3_prefill(a, stream);
    }
    const int st_main = prefill::launch<ON>(a, m, stream);      // the caller's device is back before the merge
    if (st_main != PFA_OK) return st_main;
    const pfa_attn_merge_args mg = merge_args(a, m.nsplit);
    return pfa_attn_merge(&mg, stream);
}

}  // namespace prefill_split
}  // namespace pfa

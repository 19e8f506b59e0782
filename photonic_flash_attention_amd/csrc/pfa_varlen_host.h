// pfa_varlen_host.h -- what the two packed ("varlen") training entry points share on the host (include/pfa_hip.h, pfa_fa3_varlen_args /
// pfa_fa3_varlen_bwd_args): the field rules the two argument blocks have in common and the grids.  Internal, like pfa_host.h.
#pragma once
#include "pfa_host.h"

namespace pfa {
namespace varlen {

// workgroups of the forward / dQ launch and of the dK/dV launch, from host shapes only
template <typename Args>
inline int64_t q_workgroups(const Args* a) { return (int64_t)((a->max_seqlen_q + 255) / 256) * a->B * a->H; }
template <typename Args>
inline int64_t k_workgroups(const Args* a) { return (int64_t)((a->max_seqlen_k + 127) / 128) * a->B * a->Hkv; }

// The rules of the fields both blocks name alike, up to and including the dtype-independent shape rules, in the order their errors are
// reported (tests/test_varlen_host.py pins it).  `extra_null`: a required pointer of the caller's own that is missing.
template <typename Args>
inline int check_head(const Args* a, bool extra_null) {
    if (a->flags != 0 || a->reserved0 != 0) return PFA_ERR_FLAGS;
    if (!a->q || !a->k || !a->v || !a->o || !a->cu_seqlens_q || !a->cu_seqlens_k || extra_null) return PFA_ERR_NULL;
    if (a->B <= 0 || a->H <= 0 || a->Hkv <= 0 || a->H % a->Hkv != 0) return PFA_ERR_SHAPE;
    if (a->total_q < 1 || a->total_k < 1 || a->max_seqlen_q < 1 || a->max_seqlen_k < 1) return PFA_ERR_SHAPE;
    if (a->max_seqlen_q > a->total_q || a->max_seqlen_k > a->total_k) return PFA_ERR_SHAPE;
    if (a->D != 64 && a->D != 128) return PFA_ERR_HEAD_DIM;
    return PFA_OK;
}
// ... and behind the caller's dtype, stride and alignment rules: the 32-bit slabs of the operands the kernels read through buffer
// descriptors (one sequence's max_seqlen rows at the row stride), k / v rows forward, and the grids.
template <typename Args>
inline int check_tail(const Args* a) {
    if (!aligned4(a->lse) || !aligned4(a->cu_seqlens_q) || !aligned4(a->cu_seqlens_k)) return PFA_ERR_ALIGN;
    if (!slab_fits32(a->max_seqlen_q, a->q_stride_s, a->D, 2) || !slab_fits32(a->max_seqlen_k, a->k_stride_s, a->D, 2) ||
        !slab_fits32(a->max_seqlen_k, a->v_stride_s, a->D, 2))
        return PFA_ERR_SHAPE;
    if (!kv_rows_forward(a) || a->q_stride_s < 0 || a->k_stride_s * 64 > 0x3fffffffLL || a->v_stride_s * 64 > 0x3fffffffLL) return PFA_ERR_STRIDE;
    if (q_workgroups(a) > 0x7fffffffLL || k_workgroups(a) > 0x7fffffffLL) return PFA_ERR_SHAPE;
    return PFA_OK;
}

// fa3_fwd_kernel's parameter block (FwdParams, or a block derived from it) of a checked packed forward call
template <typename Params>
inline void fill_fwd_params(Params& p, const pfa_fa3_varlen_args* a) {
    p.q = a->q; p.k = a->k; p.v = a->v; p.o = a->o; p.lse = a->lse;
    p.seqlens_k = nullptr; p.mask = nullptr; p.mbits = nullptr; p.dbg = nullptr;
    p.q_sb = p.k_sb = p.v_sb = p.o_sb = 0;
    p.m_sb = p.m_sh = p.m_sq = p.m_sk = 0; p.mb_sb = p.mb_sh = p.mb_sq = 0;
    p.q_sh = a->q_stride_h; p.q_ss = a->q_stride_s; p.k_sh = a->k_stride_h; p.k_ss = a->k_stride_s;
    p.v_sh = a->v_stride_h; p.v_ss = a->v_stride_s; p.o_sh = a->o_stride_h; p.o_ss = a->o_stride_s;
    p.B = a->B; p.H = a->H; p.Sq = a->max_seqlen_q; p.Sk = a->max_seqlen_k;
    p.nqblk = (a->max_seqlen_q + 255) / 256;      // Q blocks of 256 rows, as q_workgroups counts them
    p.kv_group = a->H / a->Hkv;
    p.xcd_group = 0; p.magic_h = p.magic_g = 0;
    p.scale_log2 = a->softmax_scale * LOG2E;
    p.cu_q = a->cu_seqlens_q; p.cu_k = a->cu_seqlens_k; p.total_q = a->total_q; p.total_k = a->total_k;
}

inline const char* elem_name(int dtype) { return dtype == PFA_DTYPE_BF16 ? "bf16" : "fp16"; }

}  // namespace varlen
}  // namespace pfa

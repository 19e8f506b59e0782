// pfa_rope_append_capi.hip -- C ABI of the rotary embedding fused into the KV-cache append (include/pfa_hip.h, pfa_rope_append*):
// validation and the launch of rope_append_kernel.  No allocation, no synchronisation, no process-wide state, no workspace.
// This object alone is compiled with -ffp-contract=off (csrc/Makefile): the kernel's products and sums round separately.
#include <stdio.h>

#include "pfa_append_host.h"

namespace {

constexpr int kPiece = 16;     // a work item is 16 elements of a row: a rotation's pairs lie inside it
int64_t heads(const pfa_rope_append_args* a) { return (int64_t)a->H + 2 * (int64_t)a->Hkv; }      // of a row: q, k_new and v_new
int64_t workgroups(const pfa_rope_append_args* a) { return pfa::append::workgroups(a, heads(a), kPiece); }

int check(const pfa_rope_append_args* a) {
    const int st = pfa::append::check_args(a, false);      // pfa_kv_append's rules, in its order; the flag bits are among the rules below
    if (st != PFA_OK) return st;
    // the rotary rules
    if (a->flags & ~PFA_ROPE_INTERLEAVED) return PFA_ERR_FLAGS;
    if (!a->cos || !a->sin) return PFA_ERR_NULL;
    if ((a->q == nullptr) != (a->q_out == nullptr)) return PFA_ERR_NULL;
    if (a->q && a->H < 1) return PFA_ERR_SHAPE;
    if (!a->q && a->H != 0) return PFA_ERR_FLAGS;
    if (a->max_pos < 1) return PFA_ERR_SHAPE;
    if (a->D % 16 != 0 || a->rot_dim < 16 || a->rot_dim % 16 != 0 || a->rot_dim > a->D) return PFA_ERR_HEAD_DIM;
    if (!pfa::multiples_of(8, {a->q_stride_b, a->q_stride_s, a->q_stride_h, a->qo_stride_b, a->qo_stride_s, a->qo_stride_h}))
        return PFA_ERR_STRIDE;
    if (a->cs_stride % 4 != 0 || a->cs_stride < a->rot_dim / 2) return PFA_ERR_STRIDE;
    if (!pfa::aligned16(a->q) || !pfa::aligned16(a->q_out) || !pfa::aligned16(a->cos) || !pfa::aligned16(a->sin)) return PFA_ERR_ALIGN;
    if (!pfa::aligned4(a->pos_offsets)) return PFA_ERR_ALIGN;
    if (a->cu_seqlens_q && (a->q_stride_b != 0 || a->qo_stride_b != 0)) return PFA_ERR_FLAGS;
    return pfa::append::grid_fits(a, heads(a), kPiece) ? PFA_OK : PFA_ERR_SHAPE;
}

}  // namespace

extern "C" {

int pfa_rope_append_check(const pfa_rope_append_args* a) { return check(a); }

int pfa_rope_append_describe(const pfa_rope_append_args* a, char* buf, size_t n) {
    const int st = check(a);
    if (st != PFA_OK) return st;
    if (buf && n)
        snprintf(buf, n, "rope_append_%s_d%d_r%d%s%s%s", a->dtype == PFA_DTYPE_BF16 ? "bf16" : "fp16", a->D, a->rot_dim,
                 (a->flags & PFA_ROPE_INTERLEAVED) ? "_il" : "", a->cu_seqlens_q ? "_varlen" : "", a->block_table ? "_paged" : "");
    return (int)workgroups(a);
}

int pfa_rope_append(const pfa_rope_append_args* a, void* stream) {
    const int st = check(a);
    if (st != PFA_OK) return st;
    pfa::RopeAppendParams p;
    pfa::append::fill_params(p, a, heads(a), kPiece);
    p.q = a->q; p.q_out = a->q_out; p.cos = a->cos; p.sin = a->sin; p.pos_offsets = a->pos_offsets;
    p.q_sb = a->q_stride_b; p.q_ss = a->q_stride_s; p.q_sh = a->q_stride_h;
    p.qo_sb = a->qo_stride_b; p.qo_ss = a->qo_stride_s; p.qo_sh = a->qo_stride_h;
    p.cs_stride = a->cs_stride;
    p.H = a->H; p.Hkv = a->Hkv;
    p.dunits = a->D / kPiece; p.runits = a->rot_dim / kPiece;
    p.max_pos = a->max_pos;

    const bool varlen = a->cu_seqlens_q != nullptr, paged = a->block_table != nullptr, il = (a->flags & PFA_ROPE_INTERLEAVED) != 0;
    const auto fn = a->dtype == PFA_DTYPE_BF16 ? pfa::append::rope_kernel<__bf16>(varlen, paged, il) : pfa::append::rope_kernel<_Float16>(varlen, paged, il);
    const pfa::DeviceScope dev(a->device_id);
    if (pfa::hip_failed(dev.error())) return PFA_ERR_DEVICE;
    return pfa::launch(fn, dim3((unsigned)workgroups(a)), pfa::ROPE_APPEND_THREADS, p, 0, stream);
}

}  // extern "C"

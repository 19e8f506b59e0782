/*
 * pfa_hip_train_sinks.h -- attention sinks for training: the part of libpfa_hip.so's C ABI (v9, additive) that pfa_hip.h does not
 * declare.  A header of its own beside pfa_hip.h, which it includes and whose conventions (pfa_status, argument blocks with a size
 * field, streams as void*, no allocation, no synchronisation) hold here; the ctypes mirror is photonic_flash_attention_amd/_capi_sinks.py.
 */
#ifndef PFA_HIP_TRAIN_SINKS_H
#define PFA_HIP_TRAIN_SINKS_H

#include "pfa_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Attention sinks for training (ABI v9, additive): pfa_fa3_fwd and pfa_fa3_varlen_fwd with a pfa_fa3_sinks block, and the gradient of
 * the sinks.  The sink's meaning, units and row rules are those of the calls over a cache above: one extra key of score sinks[h] and a
 * zero value row per QUERY head, inside the LSE; a row with no visible key gets O = 0 exactly and LSE = sinks[h]; sinks[h] = -inf gives
 * head h the O and LSE bits of the sink-less 8-wave call (selector 44), -inf in the LSE of a row without keys included.
 *
 * Forward: the 8-wave kernel in its SINK mode, and only that kernel: with a sink block the selectors 43 (4-wave kernel) and 45
 * (persistent assembly kernel) are refused with PFA_ERR_FLAGS, 0 and 44 both mean the 8-wave kernel.  bf16 / fp16 operands (fp32
 * operands -> PFA_ERR_DTYPE; with them a drop_mask -> PFA_ERR_FLAGS as before), D 64 / 128, causal and full, seqlens_k, key and element
 * masks (workspace and pfa_fa3_workspace_bytes as in pfa_fa3_fwd), 16-bit and fp32 output, with and without PFA_FLAG_SPLIT_P, grouped
 * heads (the sink is indexed by the query head), and the packed mode.  Workgroups are the sink-less 8-wave call's, from host shapes
 * alone; the sink pointer is a launch argument and its contents are read on the device, so a captured step replays while the values
 * change.  pfa_fa3_weights takes no sinks.
 *
 * Backward: pfa_fa3_bwd / pfa_fa3_varlen_bwd are called UNCHANGED on the sink-holding o and lse.  They recompute P = exp(x - LSE) from
 * that LSE, which is the softmax over keys plus sink, and delta = rowsum(dO o O) needs no sink term because the sink's value row is
 * zero: dq, dk, dv are the gradients of the forward with sinks.  What is left is the sink's own gradient,
 *     d_sinks[h] = - sum over b, i of exp(sinks[h] - LSE[b,h,i]) * delta[b,h,i],
 * which pfa_fa3_sink_grad computes from the LSE and the delta scratch the backward leaves behind (same stream, after it).
 *
 * Field rules of the two forward calls, in the order their errors are reported: the rules of pfa_fa3_sinks (size, flags, NULL,
 * alignment); then those of pfa_fa3_check / pfa_fa3_varlen_check; then, for pfa_fa3_fwd_sink, fp32 operands -> PFA_ERR_DTYPE and a
 * selector 43 or 45 -> PFA_ERR_FLAGS.  `sinks` NULL: the call IS pfa_fa3_fwd / pfa_fa3_varlen_fwd (_check, _describe) in every respect.
 */
int pfa_fa3_fwd_sink_check(const pfa_fa3_args* a, const pfa_fa3_sinks* sinks);
int pfa_fa3_fwd_sink(const pfa_fa3_args* a, const pfa_fa3_sinks* sinks, void* stream);
/* As pfa_fa3_describe: the 8-wave kernel's name with "_sink" in front of its "_v<tag>" suffix, "fa3_fwd_..._{o16|o32}_sink_v8269". */
int pfa_fa3_fwd_sink_describe(const pfa_fa3_args* a, const pfa_fa3_sinks* sinks, char* buf, size_t n);
int pfa_fa3_varlen_fwd_sink_check(const pfa_fa3_varlen_args* a, const pfa_fa3_sinks* sinks);
int pfa_fa3_varlen_fwd_sink(const pfa_fa3_varlen_args* a, const pfa_fa3_sinks* sinks, void* stream);
/* As pfa_fa3_varlen_describe, "_sink" appended: "fa3_fwd_varlen_..._{o16|o32}_sink". */
int pfa_fa3_varlen_fwd_sink_describe(const pfa_fa3_varlen_args* a, const pfa_fa3_sinks* sinks, char* buf, size_t n);

/*
 * pfa_fa3_sink_grad: d_sinks[h] as above, fp32 [H], OVERWRITTEN (not accumulated).
 *
 *   lse, delta      dense (cu_seqlens_q NULL): fp32 [B, H, Sq], entry b * stride_b + h * stride_h + i (rows contiguous), as pfa_fa3_fwd_sink
 *                   and pfa_fa3_bwd leave them.  Packed (cu_seqlens_q set): fp32 [H, total_q], entry h * total_q + s_b + i, as
 *                   pfa_fa3_varlen_fwd_sink and pfa_fa3_varlen_bwd leave them; Sq is max_seqlen_q, the strides are unused, sequence b owns
 *                   rows s_b .. s_b + min(e_b - s_b, Sq) - 1 with s_b, e_b clamped as the packed kernels clamp them.  Rows no sequence
 *                   covers (the tail behind cu[B], gaps, rows past max_seqlen_q) are never read.
 *   sinks, d_sinks  fp32 [H] on the device.
 *   workspace       pfa_fa3_sink_grad_workspace_bytes() bytes of device scratch, 4-byte aligned: H * B * ceil(Sq / 2048) fp32 partial sums.
 * A row with LSE = -inf is skipped (delta there may hold anything); sinks[h] = -inf gives d_sinks[h] = 0.
 *
 * Two launches, no atomics: H * B * ceil(Sq / 2048) workgroups leave one partial sum each, then one workgroup per head adds its
 * partials.  Every sum runs in an order fixed by the shapes, so the result is bitwise reproducible; the grids come from host shapes only,
 * so a captured step replays while the sinks, the lengths and the data change.
 *
 * Field rules, in the order their errors are reported: size wrong -> PFA_ERR_STRUCT_SIZE; flags / reserved0 non-zero -> PFA_ERR_FLAGS;
 * lse, delta, sinks, d_sinks or workspace NULL -> PFA_ERR_NULL; B, H or Sq < 1, packed: total_q < 1 or Sq > total_q -> PFA_ERR_SHAPE;
 * dense: a negative stride, or stride_h < Sq where H > 1, or stride_b < Sq where B > 1 -> PFA_ERR_STRIDE; a pointer not 4-byte aligned
 * -> PFA_ERR_ALIGN; Sq + 2048 or H * B * ceil(Sq / 2048) past 2^31 - 1 (the row index and the grid) -> PFA_ERR_SHAPE; workspace_bytes
 * below pfa_fa3_sink_grad_workspace_bytes() -> PFA_ERR_NULL.
 */
typedef struct pfa_fa3_sink_grad_args {
    uint32_t size;              /* = sizeof(pfa_fa3_sink_grad_args) */
    uint32_t flags;             /* must be 0 */
    const float* lse;
    const float* delta;
    const float* sinks;         /* [H] */
    float*       d_sinks;       /* [H], overwritten */
    const int32_t* cu_seqlens_q;   /* NULL: dense [B, H, Sq]; else int32 [B + 1] on the device: packed [H, total_q] */
    void*  workspace;
    size_t workspace_bytes;
    int64_t lse_stride_b, lse_stride_h;       /* dense only, in elements */
    int64_t delta_stride_b, delta_stride_h;
    int32_t B, H, Sq;           /* packed: Sq = max_seqlen_q */
    int32_t total_q;            /* packed only */
    int32_t device_id;
    int32_t reserved0;          /* must be 0 */
} pfa_fa3_sink_grad_args;

/* Bytes of `workspace` (0 for a NULL block or shapes the check refuses): from B, H, Sq alone; of the pointers only cu_seqlens_q is looked
 * at, NULL or not, for the packed shape rules. */
size_t pfa_fa3_sink_grad_workspace_bytes(const pfa_fa3_sink_grad_args* a);
int pfa_fa3_sink_grad_check(const pfa_fa3_sink_grad_args* a);
int pfa_fa3_sink_grad(const pfa_fa3_sink_grad_args* a, void* stream);
/* Introspection: "sink_grad_{dense|packed}_c2048+final" into buf; returns the first launch's workgroups, or a pfa_status. */
int pfa_fa3_sink_grad_describe(const pfa_fa3_sink_grad_args* a, char* buf, size_t n);

#ifdef __cplusplus
}
#endif
#endif /* PFA_HIP_TRAIN_SINKS_H */

/*
 * pfa_hip_mla_prefill.h -- multi-head latent attention (MLA) prefill in its non-absorbed form over packed sequences: the part of
 * libpfa_hip.so's C ABI (v9, additive) that neither pfa_hip.h nor pfa_hip_mla.h declares.  A header of its own beside pfa_hip_mla.h;
 * it includes pfa_hip.h, whose conventions (pfa_status, argument blocks with a size field, streams as void*, no allocation, no
 * synchronisation) hold here.  The ctypes mirror is photonic_flash_attention_amd/_capi_mla_prefill.py.
 */
#ifndef PFA_HIP_MLA_PREFILL_H
#define PFA_HIP_MLA_PREFILL_H

#include "pfa_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PFA_MLA_PREFILL_D_NOPE 128      /* per-head key columns without position; q columns 0 .. 127 */
#define PFA_MLA_PREFILL_D_ROPE 64       /* rotary key columns; q columns 128 .. 191 */
#define PFA_MLA_PREFILL_D_V 128         /* value columns */

/*
 * pfa_mla_prefill: the prompt of DeepSeek-V2 / V3 / R1 and Kimi K2.  B sequences packed as in flash_attn_varlen_func; sequence b owns
 * the rows cu_seqlens_q[b] .. cu_seqlens_q[b + 1] - 1 and the keys cu_seqlens_k[b] .. cu_seqlens_k[b + 1] - 1 (Lq_b rows, Lk_b keys):
 *
 *   s[i,h,j] = softmax_scale * (<q[i,h,0:128], k_nope[j,h,:]> + <q[i,h,128:192], k_rope[j,hr,:]>),   hr = 0 if rope_heads == 1, else h
 *   o[i,h,:] = sum_j softmax_j(s) * v[j,h,:]
 *
 *   q               [total_q, H, 192] by element strides (row, head), last dim contiguous
 *   k_nope, v       [total_k, H, 128] likewise -- in practice two column ranges of one [total_k, H, 256] projection output
 *   k_rope          [total_k, rope_heads, 64], rope_heads 1 (one row per token, shared by all heads; kr_stride_h is then not read) or H
 *   o               [total_q, H, 128] by element strides, in dtype_in or fp32
 *   lse             optional fp32 [H, total_q], natural log: the layout pfa_fa3_prefill_varlen writes and pfa_attn_merge reads
 *   cu_seqlens_q/k  int32 [B + 1] on the device, non-decreasing.  Read as s = clamp(cu[b], 0, total), e = clamp(cu[b + 1], s, total),
 *                   L_b = min(e - s, max_seqlen): bad values give wrong numbers, never an access outside the packed tensors
 *   max_seqlen_q/k  host bounds on Lq_b / Lk_b, 1 .. total; the grid comes from max_seqlen_q alone
 *   causal          1: bottom-right per sequence -- row i sees key j iff j <= i + (Lk_b - Lq_b); 0: every key of the sequence
 *   softmax_scale   required (finite, positive): no default is right for these models
 *
 * A row with no visible key (Lk_b = 0; the first Lq_b - Lk_b rows of a causal sequence with Lk_b < Lq_b) gets O = 0 and LSE = -inf.  A
 * sequence with Lq_b = 0 writes nothing, and packed rows no sequence covers are never written.  Keys of another sequence and rows behind
 * cu_seqlens_k[B] are never read.  One kernel of its own (csrc/fa3_mla_prefill_kernel.h), one launch of ceil(max_seqlen_q / 256) * B * H
 * workgroups; no workspace and no atomics: the same bits every run, and a sequence's rows are those of a call that holds it alone.  The
 * grid comes from host shapes only, so a captured call replays while the contents of both cu_seqlens arrays and of the operands change.
 *
 * Field rules, in the order their errors are reported: a NULL block -> PFA_ERR_NULL; size -> PFA_ERR_STRUCT_SIZE; flags or reserved not 0
 * -> PFA_ERR_FLAGS; q, k_nope, k_rope, v, o, cu_seqlens_q or cu_seqlens_k NULL -> PFA_ERR_NULL; B, H, total_q or total_k < 1, rope_heads
 * neither 1 nor H, max_seqlen_q outside 1 .. total_q, max_seqlen_k outside 1 .. total_k, or a softmax_scale that is not finite and
 * positive -> PFA_ERR_SHAPE; dtype_in not bf16 / fp16, dtype_out neither dtype_in nor fp32 -> PFA_ERR_DTYPE; a q / k_nope / k_rope / v
 * stride that is no multiple of 8 elements, an o stride that is no multiple of 4, a row stride below the tensor's width (192, 128, 64,
 * 128, 128) or a key row stride too large for a tile's 32-bit offsets -> PFA_ERR_STRIDE; q, k_nope, k_rope, v, o not 16-byte aligned,
 * lse or a cu_seqlens array not 4-byte aligned -> PFA_ERR_ALIGN; a grid above 2^31 - 1 workgroups -> PFA_ERR_SHAPE.
 */
typedef struct pfa_mla_prefill_args {
    uint32_t size;              /* = sizeof(pfa_mla_prefill_args) */
    uint32_t flags;             /* must be 0 */
    const void* q;
    const void* k_nope;
    const void* k_rope;
    const void* v;
    void*       o;
    float*      lse;
    const int32_t* cu_seqlens_q;
    const int32_t* cu_seqlens_k;
    int64_t q_stride_s, q_stride_h;         /* element strides: s between packed rows, h between heads */
    int64_t kn_stride_s, kn_stride_h;       /* k_nope */
    int64_t kr_stride_s, kr_stride_h;       /* k_rope */
    int64_t v_stride_s, v_stride_h;
    int64_t o_stride_s, o_stride_h;
    int32_t B, H;
    int32_t rope_heads;         /* 1 | H */
    int32_t total_q, total_k;
    int32_t max_seqlen_q, max_seqlen_k;
    int32_t dtype_in;           /* PFA_DTYPE_BF16 | PFA_DTYPE_FP16 */
    int32_t dtype_out;          /* = dtype_in, or PFA_DTYPE_FP32 */
    int32_t causal;             /* bottom-right, see above */
    float   softmax_scale;
    int32_t device_id;
    int32_t reserved;           /* must be 0 */
} pfa_mla_prefill_args;

/* Validate `a` without launching: PFA_OK or the error pfa_mla_prefill would return. */
int pfa_mla_prefill_check(const pfa_mla_prefill_args* a);
/* Enqueue the prefill (one launch) on `stream`. */
int pfa_mla_prefill(const pfa_mla_prefill_args* a, void* stream);
/* "mla_prefill_{bf16|fp16}_{o16|o32}_{causal|full}_{rope1|ropeH}" into buf (NUL terminated, truncated to n; may be NULL): rope1 is the
 * rotary key shared by all heads, ropeH one per head.  Returns the workgroups of the launch, from host shapes only, or a pfa_status. */
int pfa_mla_prefill_describe(const pfa_mla_prefill_args* a, char* buf, size_t n);

#ifdef __cplusplus
}
#endif
#endif /* PFA_HIP_MLA_PREFILL_H */

/*
 * pfa_hip_rotary.h -- rotary embedding for the training calls: the part of libpfa_hip.so's C ABI (v9, additive) that pfa_hip.h does
 * not declare.  A header of its own beside pfa_hip.h, which it includes and whose conventions (pfa_status, argument blocks with a size
 * field, streams as void*, no allocation, no synchronisation) hold here; the ctypes mirror is photonic_flash_attention_amd/_capi_rotary.py.
 */
#ifndef PFA_HIP_ROTARY_H
#define PFA_HIP_ROTARY_H

#include "pfa_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * pfa_rotary: rotates up to two 16-bit tensors that share rows and positions in ONE launch -- x0 with H0 heads (Q, or dQ in the
 * backward) and optionally x1 with H1 heads (K or dK; x1 = x1_out = NULL and H1 = 0 without it).  The arithmetic, the table format and
 * the pairing are pfa_rope_append's, bit for bit: tables fp32 [max_pos, rot_dim / 2] with row stride cs_stride; the pair is
 * (x[j], x[j + rot_dim / 2]), or with PFA_ROTARY_INTERLEAVED (x[2j], x[2j + 1]); y1 = x1 * c - x2 * s, y2 = x2 * c + x1 * s with the
 * operands widened to fp32, each product and the add / subtract rounded to fp32 separately, then one round-to-nearest-even to the dtype.
 * PFA_ROTARY_CONJUGATE rotates by -sin: the backward of the rotation (dx1 = dy1 * c + dy2 * s, dx2 = dy2 * c - dy1 * s).
 *
 *   dense   (cu_seqlens NULL)  x [B, H, S, D] by the element strides (stride_b, stride_s, stride_h), D contiguous: a permuted
 *                              [B, S, H, D] tensor is legal.  Every sequence has S rows.
 *   packed  (cu_seqlens set)   x [total, H, D] by (stride_s, stride_h); the stride_b fields are not looked at.  cu_seqlens is int32
 *                              [B + 1] on the device, S is max_seqlen.  s_b = clamp(cu[b], 0, total), e_b = clamp(cu[b + 1], s_b, total),
 *                              rows_b = min(e_b - s_b, S).  Rows no sequence covers, and rows past max_seqlen of a sequence, are
 *                              neither read nor written.
 *
 * Row i of sequence b is rotated at position clamp(p, 0, max_pos - 1), computed in 64 bits: p = position_ids[...] when that pointer
 * is given (int32 on the device; dense entry b * pid_stride_b + i * pid_stride_s, packed entry s_b + i of [total]), else
 * p = i + pos_offsets[b] (int32 [B] on the device, or NULL for 0).  An out-of-range position gives wrong numbers, never an address
 * outside the tables.
 *
 * Out of place the elements at and past rot_dim are copied.  In place means x0_out == x0 (and x1_out == x1), the same pointer with
 * the same strides; then elements at and past rot_dim are neither read nor written.  Either both tensors are in place or neither is.
 *
 * One launch of 256-thread workgroups, a work item being one 16-element unit of one head of one row (units per head: D / 16, in place
 * rot_dim / 16): B * ceil(S * units / 256) workgroups with units = (H0 + H1) * units per head, from host shapes only, so a captured
 * call replays while cu_seqlens, pos_offsets, position_ids, the tables' contents and the inputs change.  No workspace, no atomics.
 *
 * Field rules, in the order their errors are reported: size wrong -> PFA_ERR_STRUCT_SIZE; a flag bit other than the two below,
 * position_ids together with pos_offsets, or one tensor in place and the other not -> PFA_ERR_FLAGS; x0, x0_out, cos or sin NULL, or
 * x1 / x1_out not both NULL exactly when H1 = 0 -> PFA_ERR_NULL; B, S, H0 or max_pos < 1, H1 < 0, packed: total < 1 or S > total
 * -> PFA_ERR_SHAPE; D not a multiple of 16 in 16 .. 256, rot_dim not a multiple of 16 in 16 .. D -> PFA_ERR_HEAD_DIM; dtype not bf16 /
 * fp16 -> PFA_ERR_DTYPE; a tensor stride that is not a multiple of 8 elements, an in-place tensor whose output strides differ from its
 * input strides, cs_stride not a multiple of 4 or below rot_dim / 2 -> PFA_ERR_STRIDE; a tensor, cos or sin not 16-byte aligned,
 * cu_seqlens, pos_offsets or position_ids not 4-byte aligned -> PFA_ERR_ALIGN; S * units + 256 or the workgroups past 2^31 - 1
 * -> PFA_ERR_SHAPE.
 */
#define PFA_ROTARY_INTERLEAVED 1u
#define PFA_ROTARY_CONJUGATE   2u

typedef struct pfa_rotary_args {
    uint32_t size;              /* = sizeof(pfa_rotary_args) */
    uint32_t flags;             /* PFA_ROTARY_* */
    const void* x0;
    void*       x0_out;
    const void* x1;             /* NULL with H1 = 0 */
    void*       x1_out;
    const float* cos;           /* [max_pos, rot_dim / 2] fp32, row stride cs_stride */
    const float* sin;
    const int32_t* cu_seqlens;  /* NULL: dense; else int32 [B + 1] on the device: packed */
    const int32_t* pos_offsets; /* int32 [B] on the device, or NULL */
    const int32_t* position_ids;/* int32 on the device, dense [B, S] by pid_stride_*, packed [total]; or NULL */
    int64_t x0_stride_b, x0_stride_s, x0_stride_h;       /* in elements */
    int64_t x0o_stride_b, x0o_stride_s, x0o_stride_h;
    int64_t x1_stride_b, x1_stride_s, x1_stride_h;
    int64_t x1o_stride_b, x1o_stride_s, x1o_stride_h;
    int64_t pid_stride_b, pid_stride_s;                  /* dense position_ids only */
    int64_t cs_stride;
    int32_t B, S;               /* packed: S = max_seqlen */
    int32_t total;              /* packed only */
    int32_t H0, H1, D, rot_dim, max_pos;
    int32_t dtype;              /* PFA_DTYPE_BF16 / PFA_DTYPE_FP16 */
    int32_t device_id;
} pfa_rotary_args;

int pfa_rotary_check(const pfa_rotary_args* a);
int pfa_rotary(const pfa_rotary_args* a, void* stream);
/* Introspection: "rotary_{bf16|fp16}[_packed][_interleaved][_conj][_inplace]" into buf; returns the workgroups, or a pfa_status. */
int pfa_rotary_describe(const pfa_rotary_args* a, char* buf, size_t n);

#ifdef __cplusplus
}
#endif
#endif /* PFA_HIP_ROTARY_H */

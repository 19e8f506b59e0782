/*
 * pfa_hip_qk_norm.h -- QK-norm fused with the rotary embedding of the training calls, forward and backward: the part of libpfa_hip.so's
 * C ABI (v9, additive) that pfa_hip.h does not declare.  A header of its own beside pfa_hip.h and pfa_hip_rotary.h; pfa_hip.h's
 * conventions (pfa_status, argument blocks with a size field, streams as void*, no allocation, no synchronisation) hold here; the
 * ctypes mirror is photonic_flash_attention_amd/_capi_qk_norm.py.
 */
#ifndef PFA_HIP_QK_NORM_H
#define PFA_HIP_QK_NORM_H

#include "pfa_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * pfa_qk_norm: an RMSNorm over the head dim of every head, then the rotary embedding, of up to two 16-bit tensors that share rows and
 * positions, in ONE launch -- x0 with H0 heads (Q) and optionally x1 with H1 heads (K; x1 = x1_out = w1 = NULL and H1 = 0 without it).
 * Layouts, clamps, positions, tables and pairing are pfa_rotary's (pfa_hip_rotary.h), word for word:
 *
 *   dense   (cu_seqlens NULL)  x [B, H, S, D] by the element strides (stride_b, stride_s, stride_h), D contiguous.
 *   packed  (cu_seqlens set)   x [total, H, D] by (stride_s, stride_h); the stride_b fields are not looked at.  cu_seqlens is int32
 *                              [B + 1] on the device, S is max_seqlen.  s_b = clamp(cu[b], 0, total), e_b = clamp(cu[b + 1], s_b, total),
 *                              rows_b = min(e_b - s_b, S).  Rows no sequence covers, and rows past max_seqlen of a sequence, are
 *                              neither read nor written.
 *
 * Row i of sequence b is rotated at clamp(p, 0, max_pos - 1) in 64 bits, p = position_ids[...] (int32; dense entry b * pid_stride_b +
 * i * pid_stride_s, packed entry s_b + i of [total]) or i + pos_offsets[b] (int32 [B], or NULL for 0).  Tables are fp32 [max_pos,
 * rot_dim / 2] with row stride cs_stride; the pair is (x[j], x[j + rot_dim / 2]) or with PFA_QKNORM_INTERLEAVED (x[2j], x[2j + 1]).
 * rot_dim is a multiple of 16 in 16 .. D, or 0 with cos = sin = NULL: the norm alone (max_pos and cs_stride are then not looked at).
 * D is 64 or 128.
 *
 * The arithmetic is all fp32 on widened operands, every product and every sum rounded separately: sq_j = x_j * x_j; each aligned
 * 8-element chunk summed left to right; the chunk sums added in pairs as a 16-element unit holds them (the chunks (u, u + rot_dim / 16)
 * in the rotated region of the half pairing, else (2u, 2u + 1)); the D / 16 unit sums by an xor butterfly (masks 1, 2, .. D / 32);
 * ms = sum * (1 / D); r = 1.0f / sqrtf(ms + eps), the IEEE square root and divide; n_j = (x_j * r) * s_j with s_j = w_j widened, or
 * with PFA_QKNORM_UNIT_OFFSET (Gemma) 1.0f + w_j; elements under rot_dim rotated on the fp32 n (y1 = n1 * c - n2 * s, y2 = n2 * c +
 * n1 * s: three roundings), elements at and past rot_dim are n; one round-to-nearest-even to the dtype.  The weights w0[D] / w1[D] are
 * contiguous, shared by the heads of a tensor, and of w_dtype: PFA_DTYPE_FP32 or the tensors' dtype.
 *
 * In place means x0_out == x0 (and x1_out == x1), the same pointer with the same strides.  Either both tensors are in place or neither.
 *
 * One launch of 256-thread workgroups, a work item being one 16-element unit of one head of one row: B * ceil(S * units / 256)
 * workgroups with units = (H0 + H1) * D / 16, from host shapes only, so a captured call replays while cu_seqlens, pos_offsets,
 * position_ids, the tables, the weights and the inputs change.  No LDS, no workspace, no atomics.
 *
 * Field rules, in the order their errors are reported: size wrong -> PFA_ERR_STRUCT_SIZE; a flag bit other than the two below,
 * position_ids together with pos_offsets, or one tensor in place and the other not -> PFA_ERR_FLAGS; x0, x0_out or w0 NULL, x1 / x1_out /
 * w1 not all NULL exactly when H1 = 0, cos / sin not both NULL exactly when rot_dim = 0 -> PFA_ERR_NULL; B, S or H0 < 1, H1 < 0,
 * max_pos < 1 with rot_dim != 0, eps negative or not finite, packed: total < 1 or S > total -> PFA_ERR_SHAPE; D not 64 / 128, rot_dim
 * not 0 or a multiple of 16 in 16 .. D -> PFA_ERR_HEAD_DIM; dtype not bf16 / fp16 (an fp32 x is refused), w_dtype neither dtype nor
 * fp32 -> PFA_ERR_DTYPE; a tensor stride that is not a multiple of 8 elements, an in-place tensor whose output strides differ from
 * its input strides, with rot_dim != 0 cs_stride not a multiple of 4 or below rot_dim / 2 -> PFA_ERR_STRIDE; a tensor, a weight, cos
 * or sin not 16-byte aligned, cu_seqlens, pos_offsets or position_ids not 4-byte aligned -> PFA_ERR_ALIGN; S * units + 256 or the
 * workgroups past 2^31 - 1 -> PFA_ERR_SHAPE.
 */
#define PFA_QKNORM_INTERLEAVED 1u
#define PFA_QKNORM_UNIT_OFFSET 2u

typedef struct pfa_qk_norm_args {
    uint32_t size;              /* = sizeof(pfa_qk_norm_args) */
    uint32_t flags;             /* PFA_QKNORM_* */
    const void* x0;
    void*       x0_out;
    const void* x1;             /* NULL with H1 = 0 */
    void*       x1_out;
    const void* w0;             /* [D] of w_dtype */
    const void* w1;             /* NULL with H1 = 0 */
    const float* cos;           /* [max_pos, rot_dim / 2] fp32, row stride cs_stride; NULL with rot_dim = 0 */
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
    float   eps;
    int32_t B, S;               /* packed: S = max_seqlen */
    int32_t total;              /* packed only */
    int32_t H0, H1, D, rot_dim, max_pos;
    int32_t dtype;              /* PFA_DTYPE_BF16 / PFA_DTYPE_FP16 */
    int32_t w_dtype;            /* = dtype, or PFA_DTYPE_FP32 */
    int32_t device_id;
} pfa_qk_norm_args;

int pfa_qk_norm_check(const pfa_qk_norm_args* a);
int pfa_qk_norm(const pfa_qk_norm_args* a, void* stream);
/* Introspection: "qk_norm_{bf16|fp16}_d{64|128}[_packed][_interleaved][_rot][_unit][_w32][_inplace]" into buf (_rot: rot_dim != 0);
 * returns the workgroups, or a pfa_status. */
int pfa_qk_norm_describe(const pfa_qk_norm_args* a, char* buf, size_t n);

/*
 * pfa_qk_norm_bwd: the backward of pfa_qk_norm, two launches, from x, dy, the weights, the tables and the positions of the forward
 * (same layouts, flags and rules).  Per head: r is recomputed from x by the forward's rule; g = the conjugate rotation of the widened
 * dy in fp32 (g1 = dy1 * c + dy2 * s, g2 = dy2 * c - dy1 * s; g = dy with rot_dim = 0 and at and past rot_dim); xh_j = x_j * r;
 * a_j = g_j * s_j; c = the forward's sum tree over a_j * xh_j, times (1 / D); dx_j = r * (a_j - xh_j * c), one narrowing to the dtype.
 * dw_j = the sum over rows and heads of g_j * xh_j, fp32 [D], OVERWRITTEN, computed without atomics in an order the shapes alone fix
 * (bitwise reproducible): stage 1, one workgroup per (tensor, sequence, chunk of 32 rows), computes dx and leaves one fp32 [D] partial
 * in the workspace; stage 2, D / 16 workgroups per tensor, adds the tensor's partials in 16 interleaved groups, each in index order,
 * and then the 16 sums in order.  Rows no sequence covers contribute nothing and are never read.  Workgroups of stage 1: T * B * ceil(S / 32) with T = 1, or 2 with x1, from host shapes only.
 *
 * workspace: T * B * ceil(S / 32) * D floats on the device, 4-byte aligned; pfa_qk_norm_bwd_workspace_bytes gives the bytes from the
 * shape fields (size, B, S, total with cu_seqlens, H0, H1, D) alone -- 0 for a block those rules refuse.
 *
 * Field rules, in the order their errors are reported: size -> PFA_ERR_STRUCT_SIZE; flags as above, position_ids together with
 * pos_offsets, or dx0 == x0 / dx0 == dy0 / dx1 == x1 / dx1 == dy1 (in place is refused in the backward) -> PFA_ERR_FLAGS; x0, dy0, dx0,
 * w0, dw0 or workspace NULL, x1 / dy1 / dx1 / w1 / dw1 not all NULL exactly when H1 = 0, cos / sin not both NULL exactly when rot_dim
 * = 0 -> PFA_ERR_NULL; then shape, head dim, dtype, stride (x, dy and dx of both tensors) and alignment (dw0 / dw1 / workspace 4-byte)
 * as above; (H0 + H1) * S * D / 16 + 256 or the workgroups past 2^31 - 1 -> PFA_ERR_SHAPE; workspace_bytes below the answer of
 * pfa_qk_norm_bwd_workspace_bytes -> PFA_ERR_NULL.
 */
typedef struct pfa_qk_norm_bwd_args {
    uint32_t size;              /* = sizeof(pfa_qk_norm_bwd_args) */
    uint32_t flags;             /* PFA_QKNORM_* */
    const void* x0;
    const void* dy0;
    void*       dx0;
    const void* w0;
    float*      dw0;            /* fp32 [D] */
    const void* x1;             /* x1, dy1, dx1, w1, dw1: NULL with H1 = 0 */
    const void* dy1;
    void*       dx1;
    const void* w1;
    float*      dw1;
    const float* cos;
    const float* sin;
    const int32_t* cu_seqlens;
    const int32_t* pos_offsets;
    const int32_t* position_ids;
    void*       workspace;
    size_t      workspace_bytes;
    int64_t x0_stride_b, x0_stride_s, x0_stride_h;       /* in elements */
    int64_t dy0_stride_b, dy0_stride_s, dy0_stride_h;
    int64_t dx0_stride_b, dx0_stride_s, dx0_stride_h;
    int64_t x1_stride_b, x1_stride_s, x1_stride_h;
    int64_t dy1_stride_b, dy1_stride_s, dy1_stride_h;
    int64_t dx1_stride_b, dx1_stride_s, dx1_stride_h;
    int64_t pid_stride_b, pid_stride_s;
    int64_t cs_stride;
    float   eps;
    int32_t B, S;
    int32_t total;
    int32_t H0, H1, D, rot_dim, max_pos;
    int32_t dtype;
    int32_t w_dtype;
    int32_t device_id;
} pfa_qk_norm_bwd_args;

size_t pfa_qk_norm_bwd_workspace_bytes(const pfa_qk_norm_bwd_args* a);
int pfa_qk_norm_bwd_check(const pfa_qk_norm_bwd_args* a);
int pfa_qk_norm_bwd(const pfa_qk_norm_bwd_args* a, void* stream);
/* Introspection: "qk_norm_bwd_{bf16|fp16}_d{64|128}[_packed][_interleaved][_rot][_unit][_w32]_r32+dw" into buf (r32: the rows a
 * stage-1 workgroup walks); returns the stage-1 workgroups, or a pfa_status. */
int pfa_qk_norm_bwd_describe(const pfa_qk_norm_bwd_args* a, char* buf, size_t n);

#ifdef __cplusplus
}
#endif
#endif /* PFA_HIP_QK_NORM_H */

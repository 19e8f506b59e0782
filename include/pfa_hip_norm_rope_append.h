/*
 * pfa_hip_norm_rope_append.h -- QK-norm, rotary embedding and the FP8 store fused into the KV-cache append: the part of libpfa_hip.so's
 * C ABI (v9, additive) that pfa_hip.h does not declare.  A header of its own beside pfa_hip.h, pfa_hip_rotary.h and pfa_hip_qk_norm.h;
 * pfa_hip.h's conventions (pfa_status, argument blocks with a size field, streams as void*, no allocation, no synchronisation) hold
 * here; the ctypes mirror is photonic_flash_attention_amd/_capi_norm_rope_append.py.
 */
#ifndef PFA_HIP_NORM_ROPE_APPEND_H
#define PFA_HIP_NORM_ROPE_APPEND_H

#include "pfa_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * pfa_norm_rope_append: the write side of a serving step in ONE launch -- an RMSNorm over the head dim of every head of the step's Q and
 * of its new K (each optional), the rotary embedding of both at positions derived on the device (optional), K and V placed into the KV
 * cache, contiguous or paged, 16-bit or FP8 (e4m3fn), and Q written to q_out.  pfa_rope_append with pfa_qk_norm's norm in front of the
 * rotation and pfa_kv_append_q8's store behind it.
 *
 * Placement -- sequences, lengths, clamps, drops, paging, positions, tables, pairing, q / q_out, max_seqlen_q and the grid -- is
 * pfa_rope_append's (pfa_hip.h), word for word, and the fields it shares with that block mean what they mean there: new row i of
 * sequence b belongs to logical key pos = len_b - Sq_b + i and is rotated at p = clamp(pos + pos_offsets[b], 0, max_pos - 1) in 64
 * bits; K rows with pos < 0 and rows whose page id lies outside the pool are dropped with their V rows; Q is written for every row.
 * rot_dim is a multiple of 16 in 16 .. D, or 0 with cos = sin = NULL: no rotation (max_pos and cs_stride are then not looked at).
 * D is 64 or 128.
 *
 * Arithmetic is pfa_qk_norm's forward rule (pfa_hip_qk_norm.h), word for word: all fp32 on widened operands, every product and every sum
 * rounded separately; sq_j = x_j * x_j; each aligned 8-element chunk summed left to right; the chunk sums added in pairs as a 16-element
 * unit holds them (the chunks (u, u + rot_dim / 16) in the rotated region of the half pairing, else (2u, 2u + 1)); the D / 16 unit sums by
 * an xor butterfly; ms = sum * (1 / D); r = 1.0f / sqrtf(ms + eps), the IEEE square root and divide; n_j = (x_j * r) * s_j with s_j = w_j
 * widened, or with PFA_NRA_UNIT_OFFSET 1.0f + w_j; elements under rot_dim rotated on the fp32 n (three roundings), elements at and past
 * rot_dim are n; one round-to-nearest-even to the dtype.  q_weight[D] / k_weight[D] are contiguous, shared by the heads of a tensor,
 * and of weight_dtype: PFA_DTYPE_FP32 or dtype.  A tensor whose weight is NULL is not normalised -- n = x exactly, no multiply -- so with
 * both weights NULL the call returns pfa_rope_append's bits.  V is never normalised or rotated.
 *
 * FP8 cache: kv_dtype = PFA_DTYPE_FP8_E4M3 with both descales set (fp32 on the device, k_descale[b * ds_sb + hk]; ds_sb = 0: one row for
 * every sequence, else >= Hkv).  The cache strides are then in bytes, multiples of 16.  The 16-bit result of K, and the raw V, are stored
 * as e4m3fn(clamp(float(x16) / descale, -448, 448)) -- an IEEE fp32 division, NaN stays NaN, round to nearest even: pfa_kv_append_q8's
 * rule applied to the value ALREADY narrowed to 16 bits, so the cache bytes equal those of pfa_kv_append_q8 run on what the 16-bit call
 * would have stored.  Q stays 16-bit.  With a 16-bit cache kv_dtype = dtype and both descales are NULL.
 *
 * One launch of 256-thread workgroups, a work item being one 16-element unit of one head of one row: B * ceil(max_seqlen_q * (H + 2 *
 * Hkv) * (D / 16) / 256) workgroups from host shapes only, so a captured call replays while cu_seqlens_q, cache_seqlens, pos_offsets,
 * the block table, the tables, the weights, the descales and the tensors change.  No LDS, no workspace, no atomics.
 *
 * Field rules, in the order their errors are reported (one rung per status: size, flags, NULL, shape, head dim, dtype, stride,
 * alignment, grid):
 *   size wrong -> PFA_ERR_STRUCT_SIZE;
 *   a flag bit other than the two below, reserved0 / reserved1 non-zero, H != 0 without q, q_weight without q, PFA_NRA_UNIT_OFFSET
 *     without a weight, rot_dim = 0 with no weight at all (nothing to do: that call is pfa_kv_append), paging fields set without a block
 *     table, ragged with a non-zero q / qo / kn / vn stride_b -> PFA_ERR_FLAGS;
 *   k_new, v_new, k_cache, v_cache or cache_seqlens NULL, exactly one of q / q_out NULL, one descale without the other, cos / sin not
 *     both NULL exactly when rot_dim = 0 -> PFA_ERR_NULL;
 *   B, Hkv, Smax, total_new or max_seqlen_q < 1, H < 1 with q, max_pos < 1 with rot_dim != 0, eps negative or not finite, the paging
 *     fields as in pfa_fa3_decode_args, ragged with max_seqlen_q > total_new, uniform with B * max_seqlen_q > total_new -> PFA_ERR_SHAPE;
 *   D not 64 / 128, rot_dim not 0 or a multiple of 16 in 16 .. D -> PFA_ERR_HEAD_DIM;
 *   dtype not bf16 / fp16 (fp32 operands are refused), weight_dtype neither dtype nor fp32 (with a weight), kv_dtype neither dtype nor
 *     PFA_DTYPE_FP8_E4M3, a descale with a 16-bit cache, an FP8 cache without descales -> PFA_ERR_DTYPE;
 *   a q / qo / kn / vn stride not a multiple of 8, a cache stride not a multiple of 8 (FP8: of 16), a negative cache token stride, with
 *     rot_dim != 0 cs_stride not a multiple of 4 or below rot_dim / 2, ds_sb neither 0 nor >= Hkv -> PFA_ERR_STRIDE;
 *   a tensor, a weight, cos or sin not 16-byte aligned, cu_seqlens_q, cache_seqlens, pos_offsets, the block table or a descale not
 *     4-byte aligned -> PFA_ERR_ALIGN;
 *   more workgroups than a grid holds, or max_seqlen_q * (H + 2 * Hkv) * (D / 16) + 256 past 2^31 - 1 -> PFA_ERR_SHAPE.
 */
#define PFA_NRA_INTERLEAVED 1u      /* pair (x[2j], x[2j + 1]) instead of (x[j], x[j + rot_dim / 2]) */
#define PFA_NRA_UNIT_OFFSET 2u      /* s = 1.0f + w (Gemma) */

typedef struct pfa_norm_rope_append_args {
    uint32_t size;              /* = sizeof(pfa_norm_rope_append_args) */
    uint32_t flags;             /* PFA_NRA_* */
    const void* q;              /* NULL with q_out NULL and H = 0: K / V only */
    void*       q_out;          /* may be q (in place) */
    const void* k_new;
    const void* v_new;
    void*       k_cache;
    void*       v_cache;
    const float* cos;           /* device fp32 [max_pos, rot_dim / 2] by cs_stride; NULL with rot_dim = 0 */
    const float* sin;
    const int32_t* cu_seqlens_q;   /* device [B + 1], or NULL = uniform */
    const int32_t* cache_seqlens;  /* device [B], required: lengths after the step */
    const int32_t* pos_offsets;    /* device [B], or NULL = 0 */
    const void* q_weight;       /* [D] of weight_dtype, or NULL: Q is not normalised */
    const void* k_weight;       /* [D] of weight_dtype, or NULL: K is not normalised */
    const float* k_descale;     /* FP8 cache: device fp32, entry b * ds_sb + hk; else NULL */
    const float* v_descale;
    int64_t q_stride_b, q_stride_s, q_stride_h;      /* in elements; *_b: uniform only, else 0 */
    int64_t qo_stride_b, qo_stride_s, qo_stride_h;   /* of q_out */
    int64_t kn_stride_b, kn_stride_s, kn_stride_h;
    int64_t vn_stride_b, vn_stride_s, vn_stride_h;
    int64_t k_stride_b, k_stride_h, k_stride_s;      /* in cache elements: bytes with an FP8 cache */
    int64_t v_stride_b, v_stride_h, v_stride_s;
    int64_t cs_stride;          /* row stride of cos and of sin, in elements */
    int64_t ds_sb;              /* batch stride of the descales: 0, or >= Hkv */
    float   eps;
    int32_t B, H, Hkv, total_new, max_seqlen_q, Smax, D, rot_dim, max_pos;
    int32_t dtype;              /* PFA_DTYPE_BF16 | PFA_DTYPE_FP16: q, k_new, v_new */
    int32_t weight_dtype;       /* = dtype, or PFA_DTYPE_FP32 */
    int32_t kv_dtype;           /* = dtype, or PFA_DTYPE_FP8_E4M3: the caches */
    int32_t device_id;
    /* paged cache, as in pfa_fa3_decode_args.  NULL / 0: the contiguous cache. */
    const int32_t* block_table;
    int64_t block_table_stride_b;
    int32_t page_size;          /* keys per page, a multiple of 64 */
    int32_t num_pages;          /* pages in the pools */
    int32_t reserved0, reserved1;   /* must be 0 */
} pfa_norm_rope_append_args;

/* Validate `a` without launching: PFA_OK or the error pfa_norm_rope_append would return. */
int pfa_norm_rope_append_check(const pfa_norm_rope_append_args* a);
/* Enqueue the call (one launch) on `stream`. */
int pfa_norm_rope_append(const pfa_norm_rope_append_args* a, void* stream);
/* Introspection: "norm_rope_append_{bf16|fp16}_d{64|128}[_varlen][_paged][_il][_rot][_qn][_kn][_unit][_w32][_q8]" into buf (NUL
 * terminated, truncated to n; _rot: rot_dim != 0, _qn / _kn: that weight is given); returns the workgroups, or a pfa_status. */
int pfa_norm_rope_append_describe(const pfa_norm_rope_append_args* a, char* buf, size_t n);

#ifdef __cplusplus
}
#endif
#endif /* PFA_HIP_NORM_ROPE_APPEND_H */

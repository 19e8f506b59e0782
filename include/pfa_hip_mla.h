/*
 * pfa_hip_mla.h -- multi-head latent attention (MLA) decode over a latent KV cache: the part of libpfa_hip.so's C ABI (v9, additive) that
 * pfa_hip.h does not declare.  A header of its own beside pfa_hip.h, which it includes and whose conventions (pfa_status, argument blocks
 * with a size field, streams as void*, no allocation, no synchronisation) hold here.  The ctypes mirror is
 * photonic_flash_attention_amd/_capi_mla.py.
 */
#ifndef PFA_HIP_MLA_H
#define PFA_HIP_MLA_H

#include "pfa_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PFA_MLA_D_QK 576        /* score width: 512 compressed + 64 rotary columns of the latent row */
#define PFA_MLA_D_V 512         /* value width: the compressed columns */

/*
 * pfa_mla_decode: the decode step of DeepSeek-V2 / V3 / R1 and Kimi K2 in its absorbed form.  Every token has one 576-wide latent row
 * that all H query heads share; it is the key at width 576 and its first 512 columns are the value:
 *
 *   s[b,h,i,j] = softmax_scale * <q[b,h,i,:576], kv[b,j,:576]>,    o[b,h,i,:] = sum_j softmax_j(s) * kv[b,j,:512]
 *
 *   q               [B, H, Sq, 576] by element strides (last dim contiguous), 1 <= Sq <= 64: columns 0 .. 511 are the query already
 *                   multiplied by W_UK, columns 512 .. 575 the rotated part
 *   kv_cache        contiguous [B, Smax, 576]: kv_stride_b between batches, kv_stride_s between tokens (>= 576); or, with block_table,
 *                   a pool [num_pages, page_size, 576] where kv_stride_b is the PAGE stride -- the paging fields and their rules are
 *                   pfa_fa3_decode_args' (page_size a multiple of 64, Smax = max_pages * page_size, ids clamped into the pool, entries at
 *                   and past ceil(cache_seqlens[b] / page_size) never read)
 *   o               [B, H, Sq, 512] by element strides, in dtype_in or fp32
 *   lse             optional fp32 [B, H, Sq] natural-log LSE.  A row with no visible key gets O = 0 and LSE = -inf.
 *   cache_seqlens   int32 [B] on the device, required: valid keys of each batch (clamped to [0, Smax]; keys at and past it are never read)
 *   causal          1: bottom-right aligned per batch, as in pfa_fa3_decode -- row i sees key j iff j <= cache_seqlens[b] - Sq + i
 *   softmax_scale   required (finite, positive): 576^-0.5 is wrong for every model that uses this
 *
 * One kernel of its own (csrc/fa3_mla_decode_kernel.h): work items (b, 16 rows packed over all heads, key split), the cache read once per
 * item.  Splits and the workspace follow pfa_fa3_decode's plan for (B, H, Hkv = 1, Sq, Smax): nsplit * B * H * Sq * (512 + 2) * 4 bytes when
 * nsplit > 1, else 0; pfa_fa3_decode's combine kernel joins the splits.  Grid and workspace come from host shapes only, so a captured
 * call replays while lengths, block table and cache contents change.  No atomics: the same bits every run, and a paged call returns the
 * bits of the contiguous call on the gathered cache.
 *
 * Field rules, in the order their errors are reported: a NULL block -> PFA_ERR_NULL; size -> PFA_ERR_STRUCT_SIZE; flags or reserved not 0
 * -> PFA_ERR_FLAGS; q, kv_cache, o or cache_seqlens NULL -> PFA_ERR_NULL; B, H, Smax < 1, Sq outside 1 .. 64, or a softmax_scale that is
 * not finite and positive -> PFA_ERR_SHAPE; dtype_in not bf16 / fp16, dtype_out neither dtype_in nor fp32 -> PFA_ERR_DTYPE; a q or cache
 * stride that is no multiple of 8 elements, an o stride that is no multiple of 4, kv_stride_s < 576 or too large for a tile's 32-bit
 * offsets -> PFA_ERR_STRIDE; q, kv_cache, o not 16-byte aligned, lse or cache_seqlens not 4-byte aligned -> PFA_ERR_ALIGN; then the
 * paging rules of pfa_fa3_decode_args; then the grid limit (PFA_ERR_SHAPE) and the workspace (missing or too small: PFA_ERR_NULL;
 * not 16-byte aligned: PFA_ERR_ALIGN).
 */
typedef struct pfa_mla_decode_args {
    uint32_t size;              /* = sizeof(pfa_mla_decode_args) */
    uint32_t flags;             /* must be 0 */
    const void* q;
    const void* kv_cache;
    void*       o;
    float*      lse;
    const int32_t* cache_seqlens;
    int64_t q_stride_b, q_stride_h, q_stride_s;
    int64_t o_stride_b, o_stride_h, o_stride_s;
    int64_t kv_stride_b, kv_stride_s;
    /* paged cache, as in pfa_fa3_decode_args.  NULL / 0: the contiguous cache. */
    const int32_t* block_table;
    int64_t block_table_stride_b;
    int32_t page_size;
    int32_t num_pages;
    int32_t B, H, Sq, Smax;
    int32_t dtype_in;           /* PFA_DTYPE_BF16 | PFA_DTYPE_FP16 */
    int32_t dtype_out;          /* = dtype_in, or PFA_DTYPE_FP32 */
    int32_t causal;             /* bottom-right, see above */
    float   softmax_scale;
    int32_t device_id;
    int32_t reserved;           /* must be 0 */
    void*   workspace;          /* pfa_mla_decode_workspace_bytes() bytes */
    size_t  workspace_bytes;
} pfa_mla_decode_args;

/* Scratch bytes pfa_mla_decode needs for `a` (0: none); from shapes only.  0 also for arguments pfa_mla_decode_check refuses. */
size_t pfa_mla_decode_workspace_bytes(const pfa_mla_decode_args* a);
/* Validate `a` without launching: PFA_OK or the error pfa_mla_decode would return. */
int pfa_mla_decode_check(const pfa_mla_decode_args* a);
/* Enqueue the decode (one launch, plus the combine launch when the keys are split) on `stream`. */
int pfa_mla_decode(const pfa_mla_decode_args* a, void* stream);
/* "mla_decode_{bf16|fp16}_{o16|o32}[+combine][_paged]" into buf (NUL terminated, truncated to n), the number of key splits into *nsplit
 * (either may be NULL); returns the workgroups of the main launch, or a pfa_status. */
int pfa_mla_decode_describe(const pfa_mla_decode_args* a, char* buf, size_t n, int32_t* nsplit);

#ifdef __cplusplus
}
#endif
#endif /* PFA_HIP_MLA_H */

/*
 * pfa_hip_mla_cache.h -- the latent KV cache of multi-head latent attention (MLA) as a serving step needs it: the decode over an FP8
 * (OCP e4m3fn) latent cache and the device-side append at width 576, 16-bit or quantising.  The part of libpfa_hip.so's C ABI (v9,
 * additive) that pfa_hip_mla.h does not declare; a header of its own beside it, which it includes and whose conventions hold here.  The
 * ctypes mirror is photonic_flash_attention_amd/_capi_mla_cache.py.
 */
#ifndef PFA_HIP_MLA_CACHE_H
#define PFA_HIP_MLA_CACHE_H

#include "pfa_hip_mla.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * pfa_mla_kv_quant: a latent cache of one-byte elements.  The cache (contiguous [B, Smax, 576] or a pool [num_pages, page_size, 576])
 * holds OCP e4m3fn bytes, strides are in elements = bytes, and a cache element stands for e4m3(byte) * kv_descale[b * descale_stride_b].
 * The row is key and value at once, so there is one descale, not two; descale_stride_b = 0 is one value for all sequences (what pages
 * that sequences share need).  The block points into the caller's memory: a captured call sees the descales change.
 *
 * Field rules, in the order their errors are reported: NULL -> PFA_ERR_NULL; size wrong -> PFA_ERR_STRUCT_SIZE; flags or reserved
 * non-zero -> PFA_ERR_FLAGS; kv_dtype other than PFA_DTYPE_FP8_E4M3 -> PFA_ERR_DTYPE; kv_descale NULL -> PFA_ERR_NULL; not 4-byte aligned
 * -> PFA_ERR_ALIGN; descale_stride_b < 0 -> PFA_ERR_STRIDE.
 */
typedef struct pfa_mla_kv_quant {
    uint32_t size;              /* = sizeof(pfa_mla_kv_quant) */
    uint32_t flags;             /* must be 0 */
    int32_t kv_dtype;           /* PFA_DTYPE_FP8_E4M3 */
    int32_t reserved;           /* must be 0 */
    const float* kv_descale;    /* fp32, on the device: kv_descale[b * descale_stride_b] */
    int64_t descale_stride_b;   /* 0: one value for every sequence */
} pfa_mla_kv_quant;

/*
 * pfa_mla_decode_q8: pfa_mla_decode over an FP8 latent cache.  `a` is pfa_mla_decode's block with kv_cache the e4m3fn cache and the
 * kv strides in bytes; q and o are as there (Q, P and the matrix products stay 16-bit, the conversion of a cache byte is exact).  The
 * descale is folded into the score multiplier and into the one multiplication of the epilogue, so with descales that are powers of two
 * the result has the bits of pfa_mla_decode on the dequantised cache.  Splits, grid and workspace are pfa_mla_decode's for the same
 * shapes -- the cache's element type plays no part -- and so is everything said there about capture, atomics and paging.
 *
 * Field rules, in the order their errors are reported: `a` NULL -> PFA_ERR_NULL, a->size wrong -> PFA_ERR_STRUCT_SIZE (the rules below
 * read the block); the rules of pfa_mla_kv_quant as listed above; kv_stride_b or kv_stride_s not a multiple of 16 -> PFA_ERR_STRIDE;
 * kv_cache not 16-byte aligned -> PFA_ERR_ALIGN; then the unchanged rules of pfa_mla_decode_check.
 */
size_t pfa_mla_decode_q8_workspace_bytes(const pfa_mla_decode_args* a, const pfa_mla_kv_quant* quant);
int pfa_mla_decode_q8_check(const pfa_mla_decode_args* a, const pfa_mla_kv_quant* quant);
int pfa_mla_decode_q8(const pfa_mla_decode_args* a, const pfa_mla_kv_quant* quant, void* stream);
/* "mla_decode_q8_{bf16|fp16}_{o16|o32}[+combine][_paged]" into buf, the number of key splits into *nsplit (either may be NULL);
 * returns the workgroups of the main launch, or a pfa_status. */
int pfa_mla_decode_q8_describe(const pfa_mla_decode_args* a, const pfa_mla_kv_quant* quant, char* buf, size_t n, int32_t* nsplit);

/*
 * pfa_mla_append: the write side of the latent cache, from device data alone (vLLM's concat_and_cache_mla): a step's new latent rows,
 * given in two parts, into the cache pfa_mla_decode reads.
 *
 *   kv_c            rows of 512 columns, the normalised compressed latent; k_pe rows of 64 columns, already rotated.  16-bit (dtype),
 *                   element strides, last dim contiguous.  Uniform: row i of sequence b at b * stride_b + i * stride_s, max_seqlen_q rows
 *                   each.  Ragged (cu_seqlens_q int32 [B + 1]): packed rows at row * stride_s, the batch strides 0.
 *   kv_cache        contiguous [B, Smax, 576] or, with block_table, a pool [num_pages, page_size, 576]; kv_stride_b is then the page
 *                   stride.  With quant NULL elements of dtype; with quant e4m3fn bytes and strides in bytes.
 *   cache_seqlens   int32 [B], the lengths AFTER the step
 *
 * The placement rule is pfa_kv_append's, word for word: with len_b = clamp(cache_seqlens[b], 0, Smax) and Sq_b the sequence's rows
 * (ragged: clamped as pfa_fa3_prefill_varlen clamps them, and to max_seqlen_q), row i goes to key len_b - Sq_b + i; rows in front of key 0
 * are dropped; a row whose page id lies outside the pool is dropped, never clamped; nothing else is written, lengths and table included.
 * 16-bit cache: a copy in 16-byte pieces, 72 a row.  FP8 cache: every element x is stored as
 * e4m3fn(clamp(float(x) / kv_descale[b * descale_stride_b], -448, 448)): an IEEE fp32 division, round to nearest even, NaN kept.
 * One launch whose grid comes from host shapes only (B, max_seqlen_q): capturable, and valid while cu_seqlens_q, lengths, table and
 * cache change.  No workspace, no atomics.
 *
 * Field rules, in the order their errors are reported: `a` NULL -> PFA_ERR_NULL; size wrong -> PFA_ERR_STRUCT_SIZE; with a quant block its
 * rules as listed above; flags or reserved non-zero -> PFA_ERR_FLAGS; kv_c, k_pe, kv_cache or cache_seqlens NULL -> PFA_ERR_NULL; B, Smax,
 * total_new or max_seqlen_q < 1 -> PFA_ERR_SHAPE; dtype not bf16 / fp16 -> PFA_ERR_DTYPE; a stride not a multiple of 8 (of 16 for the
 * strides of an FP8 cache), or kv_stride_s < 576 -> PFA_ERR_STRIDE; kv_c, k_pe or kv_cache not 16-byte aligned, cache_seqlens or
 * cu_seqlens_q not 4-byte aligned -> PFA_ERR_ALIGN; the paging fields as in pfa_fa3_decode_args; ragged with a non-zero batch stride ->
 * PFA_ERR_FLAGS; ragged with max_seqlen_q > total_new, uniform with B * max_seqlen_q > total_new, or more workgroups than a grid holds
 * -> PFA_ERR_SHAPE.
 */
typedef struct pfa_mla_append_args {
    uint32_t size;              /* = sizeof(pfa_mla_append_args) */
    uint32_t flags;             /* must be 0 */
    const void* kv_c;
    const void* k_pe;
    void*       kv_cache;
    const int32_t* cache_seqlens;
    const int32_t* cu_seqlens_q;    /* NULL: uniform */
    int64_t kvc_stride_b, kvc_stride_s;
    int64_t kpe_stride_b, kpe_stride_s;
    int64_t kv_stride_b, kv_stride_s;
    const int32_t* block_table;
    int64_t block_table_stride_b;
    int32_t page_size;
    int32_t num_pages;
    int32_t B, Smax;
    int32_t total_new;          /* rows kv_c / k_pe hold */
    int32_t max_seqlen_q;       /* host bound on one sequence's rows; uniform: the rows of each */
    int32_t dtype;              /* PFA_DTYPE_BF16 | PFA_DTYPE_FP16: kv_c, k_pe, and a 16-bit cache */
    int32_t device_id;
    int32_t reserved;           /* must be 0 */
    int32_t reserved1;          /* must be 0 */
} pfa_mla_append_args;

int pfa_mla_append_check(const pfa_mla_append_args* a, const pfa_mla_kv_quant* quant /* NULL: 16-bit cache */);
int pfa_mla_append(const pfa_mla_append_args* a, const pfa_mla_kv_quant* quant /* NULL: 16-bit cache */, void* stream);
/* "mla_append[_q8_{bf16|fp16}][_varlen][_paged]" into buf (may be NULL); returns the workgroups of the launch, or a pfa_status. */
int pfa_mla_append_describe(const pfa_mla_append_args* a, const pfa_mla_kv_quant* quant, char* buf, size_t n);

#ifdef __cplusplus
}
#endif
#endif /* PFA_HIP_MLA_CACHE_H */

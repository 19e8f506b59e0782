/*
 * pfa_hip_prefill_d256.h -- the forward over a KV cache at head dim 256, uniform and ragged: the part of libpfa_hip.so's C ABI (v9,
 * additive) that pfa_hip.h does not declare.  A header of its own beside pfa_hip.h, which it includes and whose conventions (pfa_status,
 * argument blocks with a size field, streams as void*, no allocation, no synchronisation) hold here; it declares no struct.  The ctypes
 * mirror is photonic_flash_attention_amd/_capi_prefill_d256.py.
 */
#ifndef PFA_HIP_PREFILL_D256_H
#define PFA_HIP_PREFILL_D256_H

#include "pfa_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * pfa_fa3_prefill_d256: pfa_fa3_prefill_ex for D = 256 (Gemma 2 / 3, Qwen3-Next), on a kernel of its own: 128 query rows per workgroup,
 * 4 waves x 32 rows with one wave per SIMD, 64-key K/V tiles in 128 KiB of LDS (csrc/fa3_prefill_d256_kernel.h).  The argument block is
 * pfa_fa3_decode_args and every field means what it means for pfa_fa3_prefill_ex: q [B, H, Sq, 256] with any Sq >= 1, the caches
 * contiguous or paged (page_size a multiple of 64), cache_seqlens, causal bottom-right aligned, dtype_out = dtype_in or fp32, lse; no
 * key mask, no workspace.  ext is pfa_fa3_cache_ext (NULL: no window); a window needs causal = 1.  Rows with no visible key get O = 0
 * and LSE = -inf; keys at and past a length, table entries at and past ceil(len_b / page_size) and, with a window, keys below
 * floor64(lo_b) are never read.  One launch of B * H * ceil(Sq / 128) workgroups from host shapes only: a captured call replays while
 * lengths, block table and cache contents change.  No atomics: the same bits every run, and a paged call returns the bits of the
 * contiguous call on the gathered cache.  There is no split over keys, no FP8 cache and no sink at this head dim.
 *
 * pfa_fa3_prefill_varlen_d256: pfa_fa3_prefill_varlen_ex for D = 256 likewise: packed q / o [total_q, H, 256], lse [H, total_q], a device
 * cu_seqlens_q [B + 1] and the host bound max_seqlen_q, which sizes the grid, B * H * ceil(max_seqlen_q / 128).  Packed rows no sequence
 * covers are never written, and the result is bit for bit that of pfa_fa3_prefill_d256 called per sequence.
 *
 * Field rules: those of pfa_fa3_prefill_ex / pfa_fa3_prefill_varlen_ex in their order, with D == 256 where those say 64 / 128 -- any
 * other D, 64 and 128 included, is PFA_ERR_HEAD_DIM (those are the other calls', which in turn refuse 256) -- and 128 rows per workgroup
 * in the grid rule.
 *
 * The describe calls write "fa3_prefill_{bf16|fp16}_d256_{o16|o32}[_causal][_win][_varlen][_paged]" into buf (may be NULL) and return
 * the workgroups of the launch, or a pfa_status.
 */
int pfa_fa3_prefill_d256_check(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext);
int pfa_fa3_prefill_d256(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, void* stream);
int pfa_fa3_prefill_d256_describe(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, char* buf, size_t n);

int pfa_fa3_prefill_varlen_d256_check(const pfa_fa3_prefill_varlen_args* a, const pfa_fa3_cache_ext* ext);
int pfa_fa3_prefill_varlen_d256(const pfa_fa3_prefill_varlen_args* a, const pfa_fa3_cache_ext* ext, void* stream);
int pfa_fa3_prefill_varlen_d256_describe(const pfa_fa3_prefill_varlen_args* a, const pfa_fa3_cache_ext* ext, char* buf, size_t n);

#ifdef __cplusplus
}
#endif
#endif /* PFA_HIP_PREFILL_D256_H */

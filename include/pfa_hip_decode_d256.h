/*
 * pfa_hip_decode_d256.h -- decode attention over a KV cache at head dim 256: the part of libpfa_hip.so's C ABI (v9, additive) that
 * pfa_hip.h does not declare.  A header of its own beside pfa_hip.h, which it includes and whose conventions (pfa_status, argument
 * blocks with a size field, streams as void*, no allocation, no synchronisation) hold here; it declares no struct.  The ctypes mirror
 * is photonic_flash_attention_amd/_capi_decode_d256.py.
 */
#ifndef PFA_HIP_DECODE_D256_H
#define PFA_HIP_DECODE_D256_H

#include "pfa_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * pfa_fa3_decode_d256: pfa_fa3_decode_ex for D = 256 (Gemma 2 / 3, Qwen3-Next), on a kernel of its own: the work split, the split
 * rule, the partial layout and the combine kernel of pfa_fa3_decode, a wave tile of 16 keys and the PV product on the 16x16x16 MFMA
 * (csrc/fa3_decode_d256_kernel.h).  The argument block is pfa_fa3_decode_args and every field means what it means there: q
 * [B, H, Sq, 256] with 1 <= Sq <= 64, the caches contiguous or paged (page_size a multiple of 64), cache_seqlens, key_mask, causal
 * bottom-right aligned, dtype_out = dtype_in or fp32, lse, the workspace.  ext is pfa_fa3_cache_ext (NULL: no window); a window needs
 * causal = 1, and only [floor64(lo_b), len_b) is streamed and split, as in pfa_fa3_decode_ex.  There is no tree mask, no FP8 cache and
 * no sink at this head dim.
 *
 * The number of key splits and the workspace are those pfa_fa3_decode_ex picks for the same (B, H, Hkv, Sq, Smax, window): the plan does
 * not look at D.  The workspace is nsplit * B * H * Sq * (256 + 2) * 4 bytes when nsplit > 1, else 0.  Grid and workspace come from host
 * shapes only, so a captured call replays while lengths, key mask, block table and cache contents change.  No atomics: the same bits
 * every run, and a paged call returns the bits of the contiguous call on the gathered cache.
 *
 * Field rules: those of pfa_fa3_decode_ex in their order, with D == 256 where that call says 64 / 128 -- any other D, 64 and 128
 * included, is PFA_ERR_HEAD_DIM (those are pfa_fa3_decode_ex's, which in turn refuses 256).
 *
 * pfa_fa3_decode_d256_describe writes "fa3_decode_{bf16|fp16}_d256_{o16|o32}[_win][+combine][_paged]" into buf, the split count into
 * *nsplit (either may be NULL) and returns the workgroups of the main launch, or a pfa_status.
 */
size_t pfa_fa3_decode_d256_workspace_bytes(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext);
int pfa_fa3_decode_d256_check(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext);
int pfa_fa3_decode_d256(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, void* stream);
int pfa_fa3_decode_d256_describe(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, char* buf, size_t n, int32_t* nsplit);

#ifdef __cplusplus
}
#endif
#endif /* PFA_HIP_DECODE_D256_H */

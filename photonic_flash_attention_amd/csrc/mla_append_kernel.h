// mla_append_kernel.h -- the write side of an MLA serving step for MI355X (gfx950), hand-written HIP: places a step's new latent rows,
// given as their two parts kv_c (512 columns, the normalised compressed latent) and k_pe (64 columns, rotated), into the 576-wide latent
// cache that fa3_mla_decode_kernel reads -- contiguous or paged, 16-bit or e4m3fn -- from device data alone (vLLM's concat_and_cache_mla).
//
// Placement is kv_append_kernel.h's, word for word: lengths AFTER the step; with len_b = clamp(cache_seqlens[b], 0, Smax) and Sq_b the
// sequence's rows, row i goes to key pos = len_b - Sq_b + i.
//   VARLEN  packed rows: s_b = clamp(cu[b], 0, total_new), e_b = clamp(cu[b + 1], s_b, total_new), Sq_b = min(e_b - s_b, max_seqlen_q);
//           row i of sequence b is packed row s_b + i.  Otherwise Sq_b = Sq and the row is at b * sb + i * ss of each source.
//   PAGED   page = block_table[b][pos / page_size], token pos % page_size; a page id outside [0, num_pages - 1] DROPS the write.
// Rows with pos < 0 are dropped.  Bad device data loses rows, it never makes an address outside the cache or the sources: i < Sq_b <=
// e_b - s_b bounds the source, 0 <= pos < len_b <= Smax the destination, pos / page_size < Smax / page_size <= bt_sb the table entry.
// Nothing but the destination rows is written.
//
// Work item = one 16-byte piece of the cache row.  16-bit cache: 8 elements, 72 pieces a row (64 from kv_c, 8 from k_pe), one
// global_load_dwordx4 and one global_store_dwordx4.  QUANT (e4m3fn cache, strides in bytes): 16 elements, 36 pieces a row (32 + 4), two
// 16-byte loads into one 16-byte store, every element x stored as e4m3fn(clamp(float(x) / kv_descale[b * ds_sb], -448, 448)), the rule
// of kv_quant8 in kv_append_kernel.h (mla_quant8 below): an IEEE fp32 division, the clamp (NaN passes it), round to nearest even.  A piece never straddles
// the two sources (512 is a multiple of both piece widths).  A sequence has Sq_b * pieces items laid out [row][piece], so consecutive
// lanes move consecutive pieces of a row; a workgroup takes 256 consecutive items of ONE sequence.  Grid = B * ceil(max_seqlen_q *
// pieces / 256) from host shapes only: capturable.  b is uniform per workgroup, so cu[b], cu[b + 1], cache_seqlens[b] and the descale are
// scalar loads, and the workgroups past a sequence's last item return before any vector memory instruction.  No LDS, no atomics.
#pragma once
#include "kv_append_kernel.h"     // the 16- and 8-byte vector types, KV_APPEND_THREADS

namespace pfa {

constexpr int MLA_APPEND_DC = 512, MLA_APPEND_DR = 64, MLA_APPEND_D = MLA_APPEND_DC + MLA_APPEND_DR;

struct MlaAppendParams {
    const void* kv_c;
    const void* k_pe;
    void* kv_cache;              // [B, Smax, 576] by strides, or (PAGED) the pool [num_pages, page_size, 576]
    const int32_t* cu_seqlens_q; // VARLEN: [B + 1]
    const int32_t* seqlens;      // [B], after the step
    const int32_t* block_table;  // PAGED: [B][max_pages] page ids
    const float* kv_descale;     // QUANT: kv_descale[b * ds_sb]
    int64_t kvc_sb, kvc_ss;      // element strides; *_sb unused under VARLEN
    int64_t kpe_sb, kpe_ss;
    int64_t k_sb, k_ss;          // the cache's, in its elements; PAGED: k_sb is the page stride
    int64_t bt_sb, ds_sb;
    int32_t nchunk;              // workgroups per sequence: ceil(Sq * pieces / 256)
    int32_t Sq;                  // rows per sequence; VARLEN: max_seqlen_q
    int32_t Smax, total_new;
    int32_t page_size, num_pages;
};

// kv_quant8's rule with the byte of a NaN pinned down.  e4m3fn has two NaN codes, 0x7f and 0xff; v_cvt_pk_fp8_f32 was seen to give a
// positive NaN 0xff on gfx950, while the plain-torch model (a CPU's division, which keeps the operand's sign, and torch's conversion,
// which keeps the sign it is given) stores 0x7f | sign of the source element.  A NaN source element gets that byte here, so that the
// cache is byte-equal to the model's, NaN included.
template <typename T>
__device__ __forceinline__ kv_append_b64 mla_quant8(kv_append_b128 x, float d) {
    typedef T t8 __attribute__((ext_vector_type(8)));
    const t8 e = __builtin_bit_cast(t8, x);
    float s[8], f[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        s[j] = (float)e[j];
        const float y = s[j] / d;
        f[j] = y != y ? y : fminf(fmaxf(y, -448.f), 448.f);
    }
    uint32_t w[2] = {0u, 0u};
    w[0] = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], (int)w[0], false);
    w[0] = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], (int)w[0], true);
    w[1] = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], (int)w[1], false);
    w[1] = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], (int)w[1], true);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const uint32_t sh = 8u * (j & 3), nanb = 0x7fu | ((__builtin_bit_cast(uint32_t, s[j]) >> 24) & 0x80u);
        if (s[j] != s[j]) w[j >> 2] = (w[j >> 2] & ~(0xffu << sh)) | (nanb << sh);
    }
    return kv_append_b64{w[0], w[1]};
}

template <bool VARLEN, bool PAGED, bool QUANT = false, typename T = void>
__global__ __launch_bounds__(KV_APPEND_THREADS) void mla_append_kernel(const MlaAppendParams p) {
    constexpr int CH = QUANT ? 16 : 8;                   // elements per work item
    constexpr int UNITS = MLA_APPEND_D / CH, CUNITS = MLA_APPEND_DC / CH;
    const int b = blockIdx.x / p.nchunk;
    const int item0 = (blockIdx.x - b * p.nchunk) * KV_APPEND_THREADS;      // the workgroup's first item of sequence b

    int sq = p.Sq, row0 = 0;
    if constexpr (VARLEN) {
        const int s_b = min(max(p.cu_seqlens_q[b], 0), p.total_new);
        const int e_b = min(max(p.cu_seqlens_q[b + 1], s_b), p.total_new);
        row0 = s_b;
        sq = min(e_b - s_b, p.Sq);
    }
    if (item0 >= sq * UNITS) return;                     // wave-uniform: nothing of this sequence in the workgroup
    const int len = min(max(p.seqlens[b], 0), p.Smax);

    const int item = item0 + (int)threadIdx.x;
    const int i = item / UNITS;                          // new row of the sequence
    const int c = item - i * UNITS;                      // its piece
    const int pos = len - sq + i;                        // its logical key
    if (i >= sq || pos < 0) return;

    // the piece's source: kv_c for columns below 512, k_pe behind them
    const bool pe = c >= CUNITS;
    const int64_t row = VARLEN ? (int64_t)(row0 + i) * (pe ? p.kpe_ss : p.kvc_ss)
                               : (int64_t)b * (pe ? p.kpe_sb : p.kvc_sb) + (int64_t)i * (pe ? p.kpe_ss : p.kvc_ss);
    const uint16_t* src = (const uint16_t*)(pe ? p.k_pe : p.kv_c) + row + (pe ? c - CUNITS : c) * CH;

    int64_t slab = b, tok = pos;                         // contiguous: the sequence's cache; PAGED: the page and the token inside it
    if constexpr (PAGED) {
        const int lp = pos / p.page_size;
        const int pg = p.block_table[(int64_t)b * p.bt_sb + lp];
        if ((unsigned)pg >= (unsigned)p.num_pages) return;                  // dropped, never clamped
        slab = pg;
        tok = pos - lp * p.page_size;
    }
    const int64_t dst = slab * p.k_sb + tok * p.k_ss + c * CH;

    if constexpr (QUANT) {
        const kv_append_b128* s = reinterpret_cast<const kv_append_b128*>(src);
        const kv_append_b128 x0 = s[0], x1 = s[1];
        const float d = p.kv_descale[(int64_t)b * p.ds_sb];
        const kv_append_b64 lo = mla_quant8<T>(x0, d), hi = mla_quant8<T>(x1, d);
        *reinterpret_cast<kv_append_b128*>((uint8_t*)p.kv_cache + dst) = kv_append_b128{lo[0], lo[1], hi[0], hi[1]};
    } else {
        *reinterpret_cast<kv_append_b128*>((uint16_t*)p.kv_cache + dst) = *reinterpret_cast<const kv_append_b128*>(src);
    }
}

}  // namespace pfa

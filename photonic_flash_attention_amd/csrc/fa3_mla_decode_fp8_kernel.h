// fa3_mla_decode_fp8_kernel.h -- the MLA decode of fa3_mla_decode_kernel.h over a latent cache of OCP e4m3fn bytes, for MI355X (gfx950),
// hand-written HIP.  vLLM's kv_cache_dtype=fp8 for MLA models: the whole 576-wide row as one byte per element with ONE fp32 descale per
// sequence (K and V are the same bytes); a cache element stands for e4m3(byte) * kv_descale[b * ds_sb].  At H 16 the 16-bit kernel is
// bound by HBM bytes, and this halves them.
//
// A sibling of fa3_mla_decode_kernel and not a flag on it: that header is untouched, so its eight kernels are built from what they were
// built from.  Everything behind the registers is shared with it: the work items (b, 16-row block packed over all heads, key split), the
// 4 waves on the 16-key tiles w, w + 4, ..., GeoMla's LDS image, decode_tile16.inc (softmax and the PV product of a tile),
// decode_merge.inc (the waves' merge), the partial layout and fa3_decode_combine_kernel<512, OT>, the XCD block order (mla_grid) and the
// paging by tile_offset / page_id.  Q, P and both MFMAs stay 16-bit: gfx950's unscaled FP8 MFMA runs at the bf16 rate.
//
// Its own is how a tile travels from HBM to the two MFMA operands:
//   * Load.  A tile is 16 keys x 576 bytes = 9 KiB.  Lane (c, h) loads the 8 bytes K[key c][32 ks + 8 h .. + 8] of each of the 18 k-steps:
//     18 buffer_load_dwordx2 per lane and tile, the 16-bit kernel's element-to-k-step mapping.  The descriptor's record count ends at the
//     split's last key, in bytes, so rows past it read as +0 (the byte 0x00).
//   * Convert.  Each register pair goes through cvt_e4m3x8 (exact) right before its S^T MFMA, and the same converted register is
//     written, for k-steps 0 .. 15, into the wave's LDS image at the 16-bit kernel's address (vwr + 64 ks): one conversion serves the K
//     operand and the V image.  The image, the 32 ds_read_b64_tr_b16 and the PV product are the 16-bit kernel's.
//   * Tiles in flight.  A K set as loaded is 36 registers, not 72.  The kernel still runs one wave per SIMD (O^T 128 + Q 72), so latency
//     is hidden inside the wave: PFA_MLA_KV8_SETS (2, 3 or 4) byte sets are in flight, the tile loop unrolled over them; a set is
//     refilled once its conversions have consumed it.  Tiles enter the online softmax in the order w, w + 4, ... whatever the count is.
//   * Descale.  One scalar load per item.  It is folded into the score multiplier and once more into the single multiplication of the
//     epilogue (the normalisation when nsplit == 1, the partial's write otherwise); the combine kernel is the 16-bit call's.  With a
//     descale that is a power of two the result has the bits of the 16-bit kernel on the dequantised cache.
// Template flags: T (bf16 / fp16, of q), OT (T / float), PAGED.  No atomics: bitwise reproducible, paged = contiguous bit for bit.
#pragma once
#include "fa3_mla_decode_kernel.h"
#include "fp8_cvt.h"

#ifndef PFA_MLA_KV8_SETS
#define PFA_MLA_KV8_SETS 2      // byte sets in flight per wave (2, 3 or 4: all fit in the 16-bit kernel's two sets; 2 measured fastest, profiles/mla_fp8.md)
#endif

namespace pfa {
namespace dec {

// the 16-bit block and the descales: kv_descale[b * ds_sb] (ds_sb = 0: one value for every sequence)
struct MlaKv8Params : DecodeParams {
    const float* kv_descale;
    int64_t ds_sb;
};

// decode_tile16.inc reads its score multiplier as p.scale_log2: here it is scale_log2 * kv_descale, under that name
struct MlaKv8ScoreMul {
    float scale_log2;
};

template <typename T, typename OT, bool PAGED = false>
__global__ __launch_bounds__(THREADS, 1) void fa3_mla_decode_kv8_kernel(const MlaKv8Params p) {
    using E = DElem<T>;
    using E16 = DElem16<T>;
    using v8 = typename E::v8;
    using v4 = typename E::v4;
    using Gm = GeoMla;
    constexpr int DV = Gm::DV, KT = Gm::KT, KS = Gm::KS, KSV = Gm::KSV, NDB = Gm::NDB, VROW = Gm::VROW, PCOLS = Gm::PCOLS, SETS = PFA_MLA_KV8_SETS;
    static_assert(SETS >= 2 && SETS <= 4, "two to four byte sets");
    constexpr bool SPLIT_P = sizeof(OT) == 4;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // siblings (the row blocks of one (b, split)) are XCDS ids apart
    const int per = Gm::XCDS * p.nrb;
    const int rem = (int)blockIdx.x % per;
    const int rb = rem / Gm::XCDS;
    const int g = (int)blockIdx.x / per * Gm::XCDS + rem % Gm::XCDS;
    if (g >= p.B * p.nsplit) return;                      // the grid's padding: the whole workgroup, in front of every barrier
    const int s = g % p.nsplit, b = g / p.nsplit;
    int len = min(max(p.seqlens[b], 0), p.Smax), lo, hi;
    split_range(p, s, 0, len, lo, hi);
    len = __builtin_amdgcn_readfirstlane(len);
    lo = __builtin_amdgcn_readfirstlane(lo);
    hi = __builtin_amdgcn_readfirstlane(hi);
    // the item's descale (a scalar load): in the score multiplier, and in the epilogue's one multiplication
    const float out_mul = ((const_f32_ptr)(uintptr_t)p.kv_descale)[(int64_t)b * p.ds_sb];
    const float score_mul = p.scale_log2 * out_mul;

    // this lane's query row (the MFMA column) and lane group
    const int c = lane & 15, h = lane >> 4;
    const int r = rb * ROWS + c;
    const bool row_ok = r < p.Sq * p.H;
    const int qi = row_ok ? r / p.H : 0, head = row_ok ? r % p.H : 0;
    const int row_lim = p.causal ? len - p.Sq + qi + 1 : len;     // exclusive key bound of this row (before the split's)
    const int min_lim = p.causal ? len - p.Sq + 1 : len;          // every row sees at least the keys below this
    // decode_tile16.inc's flags: no window, no key mask; decode_merge.inc's: the rows are packed over all H heads of the one K/V head
    constexpr bool WINDOW = false;
    constexpr int row_lo = 0, window = 0;
    const uint8_t* const km = nullptr;
    constexpr int PASSES = Gm::PASSES, OCOLS = DV, kvh = 0;
    const int grp = p.H;

    f32x4 oacc[NDB];
#pragma unroll
    for (int d = 0; d < NDB; ++d) oacc[d] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = -__builtin_inff(), l = 0.f;

    const int ntile = hi > lo ? (hi - lo + KT - 1) / KT : 0;
    if (wave < ntile) {
        // Q^T operand: lane holds Q[row c][32 ks + 8 h .. + 8]
        v8 qf[KS];
        const T* qrow = (const T*)p.q + (int64_t)b * p.q_sb + (int64_t)qi * p.q_ss + (int64_t)head * p.q_sh;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            u32x4 w = row_ok ? *(const u32x4*)(qrow + 32 * ks + 8 * h) : u32x4{0u, 0u, 0u, 0u};
            qf[ks] = __builtin_bit_cast(v8, w);
        }
        // contiguous: this batch's slab; paged: the pool (the page base is added per tile).  Strides are in elements = bytes
        const char* slab = (const char*)p.k + (PAGED ? 0 : (int64_t)b * p.k_sb);
        const uint32_t ss = (uint32_t)p.k_ss;                     // token stride in bytes
        // per-lane byte offsets inside a tile: of the load (key c, the 8 bytes of columns 32 ks + 8 h ..), and of the image write (the
        // 16 bytes of the same columns as 16-bit elements)
        const uint32_t koff0 = (uint32_t)c * ss + (uint32_t)h * 8u;
        lds_char* vimg = (lds_char*)(smem + wave * Gm::VIMG);
        const uint32_t vwr = (uint32_t)c * VROW + (uint32_t)h * 16u;
        // transposed read: lane 4q + p of its 16-lane group addresses key row 4h + q, columns 4p .. 4p + 3 of the block
        const uint32_t vtr = (uint32_t)(4 * h + ((lane & 15) >> 2)) * VROW + (uint32_t)(lane & 3) * 8u;

        u32x2 kr[SETS][KS];                      // the tiles in flight, as loaded: set u holds tiles wave + (SETS j + u) NW
        // paged: the (unclamped) page id of tile t, called only for t < ntile
        const const_i32_ptr table = PAGED ? (const_i32_ptr)(uintptr_t)(p.block_table + (int64_t)b * p.bt_sb) : nullptr;
        auto page_of = [&](int t) { return page_id(table, lo + t * KT, p.page_size); };
        int pg_next = 0;
        if constexpr (PAGED) pg_next = page_of(wave);
        // issue(t, ks): tile t's loads into the set ks.  Tiles are issued in the order t, t + NW, ..., so pg_next is tile t's entry
        auto issue = [&](int t, u32x2(&kset)[KS]) __attribute__((always_inline)) {
            const int t0 = lo + t * KT;
            const int nk = min(KT, hi - t0);     // rows past the split's end read as zeros
            const int64_t koff = tile_offset<PAGED>(p, t0, pg_next, p.k_sb, p.k_ss);     // from slab, in bytes
            const srd_t srd = uniform_srd(slab + koff, (uint32_t)(nk - 1) * ss + Gm::DQK);
#pragma unroll
            for (int q = 0; q < KS; ++q) kset[q] = __builtin_amdgcn_raw_buffer_load_b64(srd, (int)(koff0 + q * 32), 0, 0);
            if constexpr (PAGED)
                if (t + NW < ntile) pg_next = page_of(t + NW);   // behind this tile's loads, for the next issue()
        };

        // tile(t, kset): the math of tile t, whose bytes are in kset; refills kset with tile t + SETS NW once it is consumed
        auto tile = [&](int t, u32x2(&kset)[KS]) __attribute__((always_inline)) {
            const int t0 = lo + t * KT;
            // S^T = K Q^T: one 16 x 16 block, 18 k-steps, each on the register converted for it; columns 0 .. 511 also go, converted,
            // into this wave's LDS image (row-major, padded rows)
            f32x4 sacc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int q = 0; q < KS; ++q) {
                const v8 kf = cvt_e4m3x8<T, v8>(kset[q][0], kset[q][1]);
                if (q < KSV) *(__attribute__((address_space(3))) u32x4*)(vimg + vwr + q * 64) = __builtin_bit_cast(u32x4, kf);
                sacc = E::mfma(kf, qf[q], sacc);
            }
            if (t + SETS * NW < ntile) issue(t + SETS * NW, kset);

            // scores in log2 units; masks only where the tile reaches past the split or the causal cut
            const bool edge = t0 + KT > hi || t0 + KT > min_lim;
            {
                const MlaKv8ScoreMul p = {score_mul};     // what the tile's math reads of p (see MlaKv8ScoreMul)
#include "decode_tile16.inc"
            }
        };

#pragma unroll
        for (int u = 0; u < SETS; ++u)
            if (wave + u * NW < ntile) issue(wave + u * NW, kr[u]);
        for (int t = wave; t < ntile; t += SETS * NW) {
#pragma unroll
            for (int u = 0; u < SETS; ++u)
                if (t + u * NW < ntile) tile(t + u * NW, kr[u]);
        }
    }
#include "decode_merge.inc"     // ... which leaves its pass loop open, at a live row's thread with the pass's first column `col`
        const float inv = (L > 0.f ? 1.f / L : 0.f) * out_mul;
        const int64_t prow = (((int64_t)s * p.B + b) * p.H + oh) * p.Sq + oi;
#pragma unroll
        for (int d = 0; d < DPT; d += 4) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int w = 0; w < NW; ++w) acc += sc[w] * *(const f32x4*)(mo + (w * ROWS + orow) * PCOLS + d0 + d);
            if (p.nsplit == 1) store4<OT>((OT*)p.o + (int64_t)b * p.o_sb + (int64_t)oi * p.o_ss + (int64_t)oh * p.o_sh + col + d, acc * inv);
            else *(f32x4*)(p.part_o + prow * OCOLS + col + d) = acc * out_mul;
        }
        if (col != 0) continue;
        if (p.nsplit == 1) {
            if (p.lse) p.lse[((int64_t)b * p.H + oh) * p.Sq + oi] = L > 0.f ? (M + __log2f(L)) * 0.6931471805599453f : -__builtin_inff();
        } else {
            p.part_ml[prow * 2] = M;
            p.part_ml[prow * 2 + 1] = L;
        }
    }
}

}  // namespace dec
}  // namespace pfa

// fa3_mla_decode_kernel.h -- multi-head latent attention (MLA) decode in its absorbed form over a latent KV cache for MI355X (gfx950),
// hand-written HIP.  DeepSeek-V2 / V3 / R1, Kimi K2: every token has ONE 576-wide latent row (512 compressed + 64 rotary columns) that all
// query heads share; the row is the key at width 576 and its first 512 columns are the value.
//
// fa3_decode_d256_kernel.h's design at these widths: DecodeParams (k is the latent cache, v is unused, Hkv = 1 and G = H), 4 waves with
// wave w on the 16-key tiles w, w + 4, ..., and the fp32 partial layout [nsplit][B][H][Sq][512] + (m, l), so that
// fa3_decode_combine_kernel<512, OT> and the host's plan serve this kernel as they are.  What the two kernels share is written once, in
// decode_parts.h (split_range, uniform_srd, the paged lookup and the clamped per-tile offset, DElem16, the image's row padding),
// decode_tile16.inc (the score step and the PV product of a 16-key tile) and decode_merge.inc (the waves' merge).
//
//   * Work item (b, 16-row block, key split).  There is one "K/V head", so the rows of a block are packed r = i * H + h over all H heads;
//     the last block is zero-padded and the key limit is per row (a block can span two values of i).
//   * ONE load serves K and V.  A tile is 16 keys x 1152 bytes: 18 buffer_load_dwordx4 per lane, lane (c, h) holding
//     K[key c][32 ks + 8 h .. + 8] for the 18 k-steps of the 16x16x32 MFMA -- the A operand of S^T = K Q^T against Q resident in 72 VGPRs.
//     The first 16 k-steps' registers (columns 0 .. 511) are also written, as loaded, into the wave's row-major LDS image (16 rows of
//     1024 + 32 bytes: the padding and the transposed addressing of the head dim 256 kernel), from which one ds_read_b64_tr_b16 per
//     16-column block feeds O^T += V^T P^T on the 16x16x16 MFMA (32 a tile; 64 with the hi + lo P of an fp32 output).  The cache is read
//     from HBM once per work item.
//   * O^T is 16 x 512 fp32 = 128 registers, Q 72, a K set 72: past 256, so the kernel runs one wave per SIMD on the 512-register file.
//     With no partner wave to hide latency a wave keeps PFA_MLA_SETS (2) tiles in flight: two K register sets, the tile loop unrolled
//     over them; a set is refilled as soon as its S^T MFMAs and its image write have consumed it.
//   * LDS: four images = 66 KiB, dynamic (the host opts in above 64 KiB).  The waves' merge runs in four passes of 128 columns through a
//     [NW][16][128] fp32 buffer laid under the images.
//   * Block order: with H Sq > 16 several row blocks stream the same keys.  Workgroup n runs on XCD n % 8, so the row blocks of one
//     (b, split) are 8 workgroup ids apart and share one XCD's L2: id = (g / 8) * 8 nrb + rb * 8 + g % 8 with g = b * nsplit + s; the
//     grid is padded to whole groups of 8 (mla_grid), and a workgroup past the last g leaves at once.
// Template flags: T (bf16 / fp16), OT (T / float), PAGED.  cache_seqlens and bottom-right causal (Sq <= 64) are run-time.  No key mask,
// window, sinks, tree or FP8 cache.  No atomics: bitwise reproducible, and a paged call returns the bits of the contiguous call on the
// gathered cache.
#pragma once
#include "fa3_decode_kernel.h"     // decode_parts.h, and fa3_decode_combine_kernel for the unit

#ifndef PFA_MLA_SETS
#define PFA_MLA_SETS 2      // tiles in flight per wave (-DPFA_MLA_SETS=1: one K register set, for measurement)
#endif

namespace pfa {
namespace dec {

struct GeoMla {
    static constexpr int DQK = 576;                       // score width: the whole latent row
    static constexpr int DV = 512;                        // value width: its compressed part
    static constexpr int KT = KT16;                       // keys per wave tile: 18 KiB
    static constexpr int KS = DQK / 32;                   // QK^T k-steps = 16-byte loads per lane per tile
    static constexpr int KSV = DV / 32;                   // ... of which the first go into the image
    static constexpr int NDB = DV / 16;                   // 16-column blocks of O^T
    static constexpr int VROW = image_row(DV);            // LDS bytes per key row of the image
    static constexpr int VIMG = KT * VROW;                // per wave
    static constexpr int PASSES = 4;                      // merge passes
    static constexpr int PCOLS = DV / PASSES;             // columns per merge pass
    static constexpr int MERGE = NW * ROWS * PCOLS * 4 + NW * ROWS * 8;
    static constexpr int LDS = VIMG * NW;                 // 66 KiB
    static constexpr int XCDS = 8;                        // workgroup n runs on XCD n % 8
};
static_assert(GeoMla::MERGE <= GeoMla::LDS, "the merge buffer lies under the images");

// workgroups of the main launch: (b, split) pairs padded to whole groups of XCDS, times the row blocks
constexpr int64_t mla_grid(int64_t B, int64_t nsplit, int64_t nrb) {
    return (B * nsplit + GeoMla::XCDS - 1) / GeoMla::XCDS * GeoMla::XCDS * nrb;
}

template <typename T, typename OT, bool PAGED = false>
__global__ __launch_bounds__(THREADS, 1) void fa3_mla_decode_kernel(const DecodeParams p) {
    using E = DElem<T>;
    using E16 = DElem16<T>;
    using v8 = typename E::v8;
    using v4 = typename E::v4;
    using Gm = GeoMla;
    constexpr int DV = Gm::DV, KT = Gm::KT, KS = Gm::KS, KSV = Gm::KSV, NDB = Gm::NDB, VROW = Gm::VROW, PCOLS = Gm::PCOLS, SETS = PFA_MLA_SETS;
    static_assert(SETS == 1 || SETS == 2, "one or two K register sets");
    // fp32 output: P carried as a 16-bit hi + lo pair (two PV MFMAs), as in fa3_decode_kernel
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
        // contiguous: this batch's slab; paged: the pool (the page base is added per tile)
        const char* slab = (const char*)p.k + (PAGED ? 0 : (int64_t)b * p.k_sb) * 2;
        const uint32_t ss2 = (uint32_t)p.k_ss * 2u;               // token stride in bytes
        // per-lane byte offsets inside a tile, in the A-operand layout (key c, columns 32 ks + 8 h ..): of the load, and of the image write
        const uint32_t koff0 = (uint32_t)c * ss2 + (uint32_t)h * 16u;
        lds_char* vimg = (lds_char*)(smem + wave * Gm::VIMG);
        const uint32_t vwr = (uint32_t)c * VROW + (uint32_t)h * 16u;
        // transposed read: lane 4q + p of its 16-lane group addresses key row 4h + q, columns 4p .. 4p + 3 of the block
        const uint32_t vtr = (uint32_t)(4 * h + ((lane & 15) >> 2)) * VROW + (uint32_t)(lane & 3) * 8u;

        u32x4 ka[KS], kb[SETS > 1 ? KS : 1];     // the tiles in flight, as loaded: set u holds tiles wave + (2 j + u) NW
        // paged: the (unclamped) page id of tile t, called only for t < ntile
        const const_i32_ptr table = PAGED ? (const_i32_ptr)(uintptr_t)(p.block_table + (int64_t)b * p.bt_sb) : nullptr;
        auto page_of = [&](int t) { return page_id(table, lo + t * KT, p.page_size); };
        int pg_next = 0;
        if constexpr (PAGED) pg_next = page_of(wave);
        // issue(t, kr): tile t's loads into the set kr.  Tiles are issued in the order t, t + NW, ..., so pg_next is tile t's entry
        auto issue = [&](int t, u32x4(&kr)[KS]) __attribute__((always_inline)) {
            const int t0 = lo + t * KT;
            const int nk = min(KT, hi - t0);     // rows past the split's end read as zeros
            const int64_t koff = tile_offset<PAGED>(p, t0, pg_next, p.k_sb, p.k_ss);     // from slab, in elements
            const srd_t ks = uniform_srd(slab + koff * 2, (uint32_t)(nk - 1) * ss2 + Gm::DQK * 2);
#pragma unroll
            for (int q = 0; q < KS; ++q) kr[q] = __builtin_amdgcn_raw_buffer_load_b128(ks, (int)(koff0 + q * 64), 0, 0);
            if constexpr (PAGED)
                if (t + NW < ntile) pg_next = page_of(t + NW);   // behind this tile's loads, for the next issue()
        };

        // tile(t, kr): the math of tile t, whose loads are in kr; refills kr with tile t + SETS NW once it is consumed
        auto tile = [&](int t, u32x4(&kr)[KS]) __attribute__((always_inline)) {
            const int t0 = lo + t * KT;
            // columns 0 .. 511 -> this wave's LDS image (row-major, padded rows)
#pragma unroll
            for (int q = 0; q < KSV; ++q) *(__attribute__((address_space(3))) u32x4*)(vimg + vwr + q * 64) = kr[q];
            // S^T = K Q^T: one 16 x 16 block, 18 k-steps
            f32x4 sacc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int q = 0; q < KS; ++q) sacc = E::mfma(__builtin_bit_cast(v8, kr[q]), qf[q], sacc);
            if (t + SETS * NW < ntile) issue(t + SETS * NW, kr);

            // scores in log2 units; masks only where the tile reaches past the split or the causal cut
            const bool edge = t0 + KT > hi || t0 + KT > min_lim;
#include "decode_tile16.inc"
        };

        issue(wave, ka);
        if constexpr (SETS > 1) {
            if (wave + NW < ntile) issue(wave + NW, kb);
            for (int t = wave; t < ntile; t += 2 * NW) {
                tile(t, ka);
                if (t + NW < ntile) tile(t + NW, kb);
            }
        } else {
            for (int t = wave; t < ntile; t += NW) tile(t, ka);
        }
    }
#include "decode_merge.inc"     // ... which leaves its pass loop open, at a live row's thread with the pass's first column `col`
        const float inv = L > 0.f ? 1.f / L : 0.f;
        const int64_t prow = (((int64_t)s * p.B + b) * p.H + oh) * p.Sq + oi;
#pragma unroll
        for (int d = 0; d < DPT; d += 4) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int w = 0; w < NW; ++w) acc += sc[w] * *(const f32x4*)(mo + (w * ROWS + orow) * PCOLS + d0 + d);
            if (p.nsplit == 1) store4<OT>((OT*)p.o + (int64_t)b * p.o_sb + (int64_t)oi * p.o_ss + (int64_t)oh * p.o_sh + col + d, acc * inv);
            else *(f32x4*)(p.part_o + prow * OCOLS + col + d) = acc;
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

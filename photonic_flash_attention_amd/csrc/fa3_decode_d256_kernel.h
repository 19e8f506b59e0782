// fa3_decode_d256_kernel.h -- split-KV decode attention over a KV cache at head dim 256 for MI355X (gfx950), hand-written HIP.
//
// fa3_decode_kernel.h's work split with a tile of its own.  Kept from there: the work item (batch, K/V head, 16-row block, key split) with
// rows packed r = i * G + g, 4 waves with wave w on tiles w, w + 4, ..., the window part, and the fp32 partial layout
// [nsplit][B][H][Sq][D] + (m, l), so that fa3_decode_combine_kernel<256, OT> and the host's plan serve this kernel as they are.  Shared with
// it and with fa3_mla_decode_kernel.h, each written once: decode_parts.h (DecodeParams, split_range, uniform_srd, the paged lookup and
// the clamped per-tile offset, DElem16, the image's row padding), decode_tile16.inc (the score step and the PV product of a 16-key tile)
// and decode_merge.inc (the waves' merge).
//
// The tile.  Geo<256> in that kernel would be a 32-key tile feeding the 16x16x32 MFMA's 32-key k-step in PV: 64 (O^T) + 32 (Q) + 64 (K) +
// 64 (V) = 224 VGPRs before an address or a score.  Here a wave tile is 16 keys -- 8 KiB of K + 8 KiB of V, the 16 KiB per wave in
// flight of the other head dims; 16 divides 64, so a tile lies inside one split and one page:
//   * S^T = K Q^T is ONE 16x16 block, eight k-steps of the 16x16x32 MFMA: lane (c, h) holds K[key c][32 ks + 8 h .. + 8] (8 x b128,
//     32 VGPRs) against the resident Q[row c][32 ks + 8 h .. + 8] (32 VGPRs).
//   * O^T += V^T P^T on the 16x16x16 MFMA, whose k dimension is the tile's 16 keys: one per 16-column block of O^T (16 a tile; twice
//     that with the hi + lo P of an fp32 output).  Element e of the S^T accumulator in lane (c, h) is key 4 h + e of row c -- the x16
//     instruction's B-operand order -- so P goes in as converted, with no key permutation.  The A operand is one ds_read_b64_tr_b16 per
//     block from the wave's row-major LDS image of the V tile (16 rows of 512 + 32 bytes: the padding and the addressing of the other
//     kernel's image): lane 4 q + p of lane group h addresses row 4 h + q, columns 4 p .. 4 p + 3 of the block, and receives
//     V[keys 4 h .. 4 h + 3][column lane & 15].
//   * V goes HBM -> registers -> image: 8 x b128 per lane, two keys an instruction (32 VGPRs).  64 + 32 + 32 + 32 = 160 VGPRs of tile
//     state.
//   * The waves' merge runs in two halves of 128 columns through a [NW][16][128] fp32 buffer, which fits under the four images: the
//     workgroup's LDS stays at the images' 34 KiB (static, below 64 KiB), so LDS never bounds the occupancy.
// Template flags: T (bf16 / fp16), OT (T / float), PAGED, WINDOW.  Key mask, cache_seqlens, bottom-right causal (Sq <= 64) and grouped
// heads are run-time.  No tree, no FP8 cache, no sinks.  No atomics: bitwise reproducible, and a paged call returns the bits of the
// contiguous call on the gathered cache.
#pragma once
#include "fa3_decode_kernel.h"     // ... which includes decode_parts.h

namespace pfa {
namespace dec {

struct Geo256 {
    static constexpr int D = 256;
    static constexpr int KT = KT16;                       // keys per wave tile: 8 KiB of K + 8 KiB of V
    static constexpr int KS = D / 32;                     // QK^T k-steps
    static constexpr int NDB = D / 16;                    // 16-column blocks of O^T
    static constexpr int KPI = 2;                         // keys per 1-KiB V load instruction
    static constexpr int VLD = KT / KPI;                  // 16-byte V loads per lane per tile
    static constexpr int VROW = image_row(D);             // LDS bytes per key row of the V image
    static constexpr int VIMG = KT * VROW;                // per wave
    static constexpr int PASSES = 2;                      // merge passes
    static constexpr int PCOLS = D / PASSES;              // columns per merge pass
    static constexpr int MERGE = NW * ROWS * PCOLS * 4 + NW * ROWS * 8;
    static constexpr int LDS = VIMG * NW > MERGE ? VIMG * NW : MERGE;
};

template <typename T, typename OT, bool PAGED = false, bool WINDOW = false>
__global__ __launch_bounds__(THREADS, 2) void fa3_decode_d256_kernel(const typename DecodeParamsOf<WINDOW>::type p) {
    using E = DElem<T>;
    using E16 = DElem16<T>;
    using v8 = typename E::v8;
    using v4 = typename E::v4;
    using Gm = Geo256;
    constexpr int D = Gm::D, KT = Gm::KT, KS = Gm::KS, NDB = Gm::NDB, VLD = Gm::VLD, VROW = Gm::VROW, PASSES = Gm::PASSES, PCOLS = Gm::PCOLS, OCOLS = D;
    // fp32 output: P carried as a 16-bit hi + lo pair (two PV MFMAs), as in fa3_decode_kernel
    constexpr bool SPLIT_P = sizeof(OT) == 4;
    __shared__ __attribute__((aligned(16))) char smem[Gm::LDS];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int x = blockIdx.x;
    const int s = x % p.nsplit;
    x /= p.nsplit;
    const int rb = x % p.nrb;
    x /= p.nrb;
    const int kvh = x % p.Hkv, b = x / p.Hkv;
    const int grp = p.G;                                          // the item's rows are packed r = i * grp + g
    int len = p.seqlens ? min(max(p.seqlens[b], 0), p.Smax) : p.Smax, lo, hi;
    int base = 0;
    if constexpr (WINDOW) base = max(0, len - p.Sq - p.window + 1) & ~(SPLIT_ALIGN - 1);
    split_range(p, s, base, len, lo, hi);
    len = __builtin_amdgcn_readfirstlane(len);
    lo = __builtin_amdgcn_readfirstlane(lo);
    hi = __builtin_amdgcn_readfirstlane(hi);

    // this lane's query row (the MFMA column) and lane group
    const int c = lane & 15, h = lane >> 4;
    const int r = rb * ROWS + c;
    const bool row_ok = r < p.Sq * p.G;
    const int qi = row_ok ? r / p.G : 0, qg = row_ok ? r % p.G : 0;
    const int head = kvh * p.G + qg;
    const int row_lim = p.causal ? len - p.Sq + qi + 1 : len;     // exclusive key bound of this row (before the split's)
    const int min_lim = p.causal ? len - p.Sq + 1 : len;          // every row sees at least the keys below this
    // WINDOW (causal): the row's lowest visible key, and the largest of them among the item's rows (its last row's)
    int row_lo = 0, max_lo = 0, window = 0;
    if constexpr (WINDOW) {
        window = p.window;
        row_lo = row_lim - p.window;
        const int last = min(rb * ROWS + ROWS - 1, p.Sq * p.G - 1);
        max_lo = __builtin_amdgcn_readfirstlane(len - p.Sq + last / p.G + 1 - p.window);
    }

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
        // contiguous: this batch's and head's slab; paged: the head's offset inside every page (the page base is added per tile)
        const char* kslab = (const char*)p.k + ((PAGED ? 0 : (int64_t)b * p.k_sb) + (int64_t)kvh * p.k_sh) * 2;
        const char* vslab = (const char*)p.v + ((PAGED ? 0 : (int64_t)b * p.v_sb) + (int64_t)kvh * p.v_sh) * 2;
        const uint32_t kss2 = (uint32_t)p.k_ss * 2u, vss2 = (uint32_t)p.v_ss * 2u;     // token strides in bytes
        // per-lane byte offsets inside a tile: K in the A-operand layout (key c, head dims 32 ks + 8 h ..), V one 1-KiB piece per
        // instruction (key 2 i + lane / 32, 16-byte chunk lane % 32)
        const uint32_t koff0 = (uint32_t)c * kss2 + (uint32_t)h * 16u;
        const uint32_t vkey = (uint32_t)lane >> 5, vch = (uint32_t)lane & 31u;
        const uint32_t voff0 = vkey * vss2 + vch * 16u;
        lds_char* vimg = (lds_char*)(smem + wave * Gm::VIMG);
        const uint32_t vwr = vkey * VROW + vch * 16u;
        // transposed read: lane 4q + p of its 16-lane group addresses key row 4h + q, columns 4p .. 4p + 3 of the block
        const uint32_t vtr = (uint32_t)(4 * h + ((lane & 15) >> 2)) * VROW + (uint32_t)(lane & 3) * 8u;

        u32x4 kr[KS], vr[VLD];     // the tile in flight, as loaded
        // paged: the (unclamped) page id of tile t, called only for t < ntile
        const const_i32_ptr table = PAGED ? (const_i32_ptr)(uintptr_t)(p.block_table + (int64_t)b * p.bt_sb) : nullptr;
        auto page_of = [&](int t) { return page_id(table, lo + t * KT, p.page_size); };
        int pg_next = 0;
        if constexpr (PAGED) pg_next = page_of(wave);
        auto issue = [&](int t) {
            const int t0 = lo + t * KT;
            const int nk = min(KT, hi - t0);     // rows past the split's end read as zeros
            const int64_t koff = tile_offset<PAGED>(p, t0, pg_next, p.k_sb, p.k_ss), voff = tile_offset<PAGED>(p, t0, pg_next, p.v_sb, p.v_ss);
            const srd_t vs = uniform_srd(vslab + voff * 2, (uint32_t)(nk - 1) * vss2 + D * 2);
            const srd_t ks = uniform_srd(kslab + koff * 2, (uint32_t)(nk - 1) * kss2 + D * 2);
#pragma unroll
            for (int i = 0; i < VLD; ++i)
                vr[i] = __builtin_amdgcn_raw_buffer_load_b128(vs, (int)(voff0 + (uint32_t)(i * Gm::KPI) * vss2), 0, 0);
#pragma unroll
            for (int q = 0; q < KS; ++q) kr[q] = __builtin_amdgcn_raw_buffer_load_b128(ks, (int)(koff0 + q * 64), 0, 0);
            if constexpr (PAGED)
                if (t + NW < ntile) pg_next = page_of(t + NW);   // behind this tile's loads, for the next issue()
        };
        issue(wave);
        const uint8_t* km = p.key_mask ? p.key_mask + (int64_t)b * p.km_sb : nullptr;

        for (int t = wave; t < ntile; t += NW) {
            const int t0 = lo + t * KT;
            // V tile -> this wave's LDS image (row-major, padded rows)
#pragma unroll
            for (int i = 0; i < VLD; ++i) *(__attribute__((address_space(3))) u32x4*)(vimg + vwr + i * Gm::KPI * VROW) = vr[i];
            // S^T = K Q^T: one 16 x 16 block
            f32x4 sacc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int q = 0; q < KS; ++q) sacc = E::mfma(__builtin_bit_cast(v8, kr[q]), qf[q], sacc);
            if (t + NW < ntile) issue(t + NW);

            // scores in log2 units; masks only where the tile reaches past the split, the causal cut, below a row's window, or a key mask exists
            const bool edge = km != nullptr || t0 + KT > hi || t0 + KT > min_lim || (WINDOW && t0 < max_lo);
#include "decode_tile16.inc"
        }
    }
#include "decode_merge.inc"     // ... which leaves its pass loop open, at a live row's thread with the pass's first column `col`
        if (p.nsplit == 1) {
            const float inv = L > 0.f ? 1.f / L : 0.f;
            OT* orow_p = (OT*)p.o + (int64_t)b * p.o_sb + (int64_t)oi * p.o_ss + (int64_t)oh * p.o_sh;
#pragma unroll
            for (int d = 0; d < DPT; d += 4) {
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int w = 0; w < NW; ++w) acc += sc[w] * *(const f32x4*)(mo + (w * ROWS + orow) * PCOLS + d0 + d);
                store4<OT>(orow_p + col + d, acc * inv);
            }
            if (p.lse && col == 0)
                p.lse[((int64_t)b * p.H + oh) * p.Sq + oi] = L > 0.f ? (M + __log2f(L)) * 0.6931471805599453f : -__builtin_inff();
        } else {
            const int64_t prow = (((int64_t)s * p.B + b) * p.H + oh) * p.Sq + oi;
            float* po = p.part_o + prow * OCOLS;
#pragma unroll
            for (int d = 0; d < DPT; d += 4) {
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int w = 0; w < NW; ++w) acc += sc[w] * *(const f32x4*)(mo + (w * ROWS + orow) * PCOLS + d0 + d);
                *(f32x4*)(po + col + d) = acc;
            }
            if (col == 0) {
                p.part_ml[prow * 2] = M;
                p.part_ml[prow * 2 + 1] = L;
            }
        }
    }
}

}  // namespace dec
}  // namespace pfa

// norm_rope_append_kernel.h -- QK-norm, rotary embedding and (optionally) the FP8 store fused into the write side of a serving step for
// MI355X (gfx950), hand-written HIP: ONE launch normalises every head of the step's Q and new K (an RMSNorm over the head dim, optional per
// tensor), rotates both at positions derived on the device, places K and V into the KV cache (contiguous or paged, 16-bit or e4m3fn) and
// writes Q.  What a Qwen3 / Gemma-3 server otherwise runs as qk_norm + rope_append (two launches, Q and K twice through HBM), and what a
// rotary model over an FP8 cache otherwise has no fused form of at all.
//
// Placement is rope_append_kernel.h's, to the letter, through rope_parts.h: len_b = clamp(cache_seqlens[b], 0, Smax); VARLEN: s_b =
// clamp(cu[b], 0, total_new), e_b = clamp(cu[b + 1], s_b, total_new), Sq_b = min(e_b - s_b, max_seqlen_q), else Sq_b = Sq; new row i is
// logical key pos = len_b - Sq_b + i and is rotated at p = clamp(pos + pos_offsets[b], 0, max_pos - 1) in 64 bits.  K rows with pos < 0
// and (PAGED) rows whose page id lies outside the pool are dropped with their V rows; Q is written for every one of the Sq_b rows.  Never
// read: packed rows no sequence covers, table rows other than the p of a processed row.  Never written: anything but the destination
// rows of cache or pool and the covered rows of q_out.
//
// Arithmetic is qk_norm_kernel.h's forward rule, to the letter, through its forced-inline parts (qkn_widen8, qkn_scale8, qkn_head_sum,
// qkn_rotate, qkn_narrow8): all fp32 on widened operands, every product and sum rounded SEPARATELY (the unit is built with
// -ffp-contract=off); sq_j = x_j * x_j, each 8-element chunk left to right, the lane's chunk pair, an xor butterfly over the head's G lanes,
// ms = sum * (1 / D), r = 1.0f / sqrtf(ms + eps) with the IEEE root and divide, n_j = (x_j * r) * s_j with s = w or 1.0f + w, the elements
// under R rotated on the fp32 n with rope_pair_f32's three roundings, ONE round-to-nearest-even to the 16-bit type.  A tensor whose weight
// pointer is NULL is not normalised: n = x exactly, no multiply, so with both weights NULL the rotation is rope_pair's, bit for bit; a
// unit that is neither normalised nor rotated (all of V, K / Q at and past R without a weight) moves its 32 bytes untouched.
//
// QUANT (both descale pointers set): the cache holds OCP e4m3fn bytes and its strides are in bytes.  The 16-bit result of K, and the raw
// V, go through kv_append_kernel.h's kv_quant8 -- e4m3fn(clamp(float(x16) / descale[b * ds_sb + hk], -448, 448)), NaN stays NaN, round to
// nearest even -- so the call is byte-equal, by construction, to pfa_kv_append_q8 applied to what the 16-bit call would have stored.  A
// unit stores its 16 bytes in one store, or in two 8-byte stores for the split chunks (u, u + R / 16) of the half style.  Q stays 16-bit.
//
// Work split.  A work item is one 16-element unit of one head of one new row, laid out [row][head][unit]: the Q heads, then the K heads,
// then the V heads, (H + 2 * Hkv) * G items a row with G = D / 16 (D 64 / 128: G 4 / 8, a template parameter).  A head is G consecutive
// lanes; G divides 64 and 256 and a row's items are a multiple of G, so a head never straddles a wave or a workgroup, and every condition
// under which an item has nothing to do -- i >= Sq_b, pos < 0, a dropped page -- is a property of its ROW and therefore uniform over a
// head's lanes.  THE LANE RULE IS qk_norm_kernel's: past the one workgroup-uniform return there is no return at all.  An item with nothing
// to do stays: it loads nothing, computes on zeros, takes part in the butterfly and stores nothing.  No exchange stands under a
// lane-dependent branch.  The lanes of V heads (and of tensors without a weight) run the butterfly on their own values and drop the sum.
//
// 256 threads; a workgroup takes 256 consecutive items of ONE sequence.  Grid = B * ceil(max_seqlen_q * items_per_row / 256) from host
// shapes only: capturable, and valid while cu_seqlens_q, lengths, offsets, block table, tables, weights, descales and inputs change
// between replays.  b is uniform per workgroup, so cu[b], cu[b + 1], cache_seqlens[b] and pos_offsets[b] are scalar loads; the block-table
// lookup and the descale are per-lane loads (a workgroup's items span rows and heads).  An item reads all it needs before it writes and
// every source chunk is read by exactly one item: q_out may be q.  No LDS, no atomics, no workspace.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kv_append_kernel.h"
#include "qk_norm_kernel.h"
#include "rope_append_kernel.h"

namespace pfa {

constexpr int NORM_ROPE_APPEND_THREADS = 256;

// RopeAppendParams (dunits is G here; with QUANT the cache strides are in bytes) and what the norm and the quantising store add
struct NormRopeAppendParams : RopeAppendParams {
    const void* q_weight;        // [D], fp32 (w_fp32) or the tensors' dtype; NULL: Q is not normalised
    const void* k_weight;        // NULL: K is not normalised
    const float* k_descale;      // QUANT: fp32 descales, k_descale[b * ds_sb + hk] (ds_sb = 0: one row for every sequence)
    const float* v_descale;
    int64_t ds_sb;
    float eps;
    float inv_d;                 // 1 / D: a power of two
    int32_t w_fp32;              // non-zero: the weights are fp32
    int32_t unit_offset;         // non-zero: s = 1.0f + w
};

template <typename T, int G, bool VARLEN, bool PAGED, bool INTERLEAVED, bool QUANT>
__global__ __launch_bounds__(NORM_ROPE_APPEND_THREADS) void norm_rope_append_kernel(const NormRopeAppendParams p) {
    constexpr int CB = QUANT ? 1 : 2;                    // bytes of a cache element
    const int b = blockIdx.x / p.nchunk;
    const int item0 = (blockIdx.x - b * p.nchunk) * NORM_ROPE_APPEND_THREADS;          // the workgroup's first item of sequence b

    int sq, row0;
    rope_seq_rows<VARLEN>(p.cu_seqlens_q, b, p.total_new, p.Sq, row0, sq);
    if (item0 >= sq * p.units) return;                   // workgroup-uniform: the only return (see the header of this file)
    const int len = min(max(p.seqlens[b], 0), p.Smax);
    const int64_t off = p.pos_offsets ? (int64_t)p.pos_offsets[b] : 0;

    const int item = item0 + (int)threadIdx.x;
    const int i = item / p.units;                        // new row of the sequence
    const int rem = item - i * p.units;
    const int h = rem / G;                               // Q heads, then K heads, then V heads
    const int u = rem - h * G;
    const int pos = len - sq + i;                        // its logical key
    const bool is_q = h < p.H, is_v = h >= p.H + p.Hkv;
    const int64_t row = VARLEN ? (int64_t)(row0 + i) : (int64_t)i;
    const int64_t bb = VARLEN ? 0 : (int64_t)b;          // packed rows have no batch stride

    bool act = i < sq;                                   // has this item anything to do?  Uniform over the G lanes of a head.
    const uint16_t* src;
    uint8_t* dst;
    const void* w = nullptr;
    float dsc = 1.0f;
    if (is_q) {
        src = (const uint16_t*)p.q + bb * p.q_sb + row * p.q_ss + (int64_t)h * p.q_sh;
        dst = (uint8_t*)p.q_out + 2 * (bb * p.qo_sb + row * p.qo_ss + (int64_t)h * p.qo_sh);
        w = p.q_weight;
    } else {
        act = act && pos >= 0;
        int64_t slab = b, tok = pos;                     // contiguous: the sequence's cache; PAGED: the page and the token inside it
        if constexpr (PAGED) {
            if (act) {
                const int lp = pos / p.page_size;
                const int pg = p.block_table[(int64_t)b * p.bt_sb + lp];
                act = (unsigned)pg < (unsigned)p.num_pages;                 // dropped, never clamped (kv_append_kernel.h)
                slab = pg;
                tok = pos - lp * p.page_size;
            }
        }
        const int64_t hk = is_v ? h - p.H - p.Hkv : h - p.H;
        if (is_v) {
            src = (const uint16_t*)p.v_new + bb * p.vn_sb + row * p.vn_ss + hk * p.vn_sh;
            dst = (uint8_t*)p.v_cache + CB * (slab * p.v_sb + tok * p.v_ss + hk * p.v_sh);
        } else {
            src = (const uint16_t*)p.k_new + bb * p.kn_sb + row * p.kn_ss + hk * p.kn_sh;
            dst = (uint8_t*)p.k_cache + CB * (slab * p.k_sb + tok * p.k_ss + hk * p.k_sh);
            w = p.k_weight;
        }
        if constexpr (QUANT) {
            if (act) dsc = (is_v ? p.v_descale : p.k_descale)[(int64_t)b * p.ds_sb + hk];
        }
    }
    const bool normed = w != nullptr;

    const bool rot = !is_v && u < p.runits;
    int c0 = u * 16, c1 = u * 16 + 8;                    // element offsets of the unit's two chunks
    if (!INTERLEAVED && rot) {
        c0 = u * 8;
        c1 = (u + p.runits) * 8;
    }
    rope_b128 y0 = {0u, 0u, 0u, 0u}, y1 = {0u, 0u, 0u, 0u};
    float xa[8], xb[8], wa[8], wb[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) xa[k] = xb[k] = wa[k] = wb[k] = 0.f;
    if (act) {
        y0 = *reinterpret_cast<const rope_b128*>(src + c0);
        y1 = *reinterpret_cast<const rope_b128*>(src + c1);
        qkn_widen8<T>(y0, xa);
        qkn_widen8<T>(y1, xb);
        if (normed) {
            qkn_scale8<T>(w, c0, p.w_fp32 != 0, p.unit_offset != 0, wa);
            qkn_scale8<T>(w, c1, p.w_fp32 != 0, p.unit_offset != 0, wb);
        }
    }

    const float ms = qkn_head_sum<G>(xa, xa, xb, xb) * p.inv_d;             // every lane of the wave is here
    const float r = 1.0f / sqrtf(ms + p.eps);

    if (normed) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            xa[k] = (xa[k] * r) * wa[k];
            xb[k] = (xb[k] * r) * wb[k];
        }
    }
    if (act && rot) {
        float cs[8], sn[8];
        rope_tables(p.cos, p.sin, (int64_t)pos + off, p.max_pos, p.cs_stride, u, cs, sn);
        qkn_rotate<INTERLEAVED>(xa, xb, cs, sn);
    }
    if (normed || rot) {                                 // else the unit's 32 bytes as they were loaded
        y0 = qkn_narrow8<T>(xa);
        y1 = qkn_narrow8<T>(xb);
    }
    if (!act) {
        // nothing to store
    } else if (QUANT && !is_q) {
        const kv_append_b64 a8 = kv_quant8<T>(kv_append_b128{y0[0], y0[1], y0[2], y0[3]}, dsc);
        const kv_append_b64 b8 = kv_quant8<T>(kv_append_b128{y1[0], y1[1], y1[2], y1[3]}, dsc);
        if (c1 == c0 + 8) {
            *reinterpret_cast<kv_append_b128*>(dst + c0) = kv_append_b128{a8[0], a8[1], b8[0], b8[1]};
        } else {                                         // the half style's split chunks
            *reinterpret_cast<kv_append_b64*>(dst + c0) = a8;
            *reinterpret_cast<kv_append_b64*>(dst + c1) = b8;
        }
    } else {
        *reinterpret_cast<rope_b128*>(dst + 2 * c0) = y0;
        *reinterpret_cast<rope_b128*>(dst + 2 * c1) = y1;
    }
}

}  // namespace pfa

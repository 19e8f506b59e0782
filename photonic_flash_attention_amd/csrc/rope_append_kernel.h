// rope_append_kernel.h -- rotary embedding fused into the write side of a serving step for MI355X (gfx950), hand-written HIP: rotates
// a step's Q and new K rows by each row's position, places K and the unrotated V into a KV cache (contiguous or paged) and writes the
// rotated Q, all from device data alone.  Sequences, lengths, clamps, drops and paging are kv_append_kernel.h's, to the letter:
//   len_b = clamp(cache_seqlens[b], 0, Smax); VARLEN: s_b = clamp(cu[b], 0, total_new), e_b = clamp(cu[b + 1], s_b, total_new),
//   Sq_b = min(e_b - s_b, max_seqlen_q), else Sq_b = Sq; new row i belongs to logical key pos = len_b - Sq_b + i.
// The rotary position of row i is p = clamp(pos + pos_offsets[b], 0, max_pos - 1), computed in 64 bits (pos_offsets NULL: 0): an
// out-of-range position gives wrong numbers, never an address outside the tables -- the rule for page ids.
//
// With R = rot_dim, half = R / 2, c = cos[p][j], s = sin[p][j] (fp32 tables [max_pos, half], row stride cs_stride), the pair
// (x1, x2) = (x[j], x[j + half]) -- or, INTERLEAVED, (x[2j], x[2j + 1]) -- becomes
//   y1 = x1 * c - x2 * s,   y2 = x2 * c + x1 * s
// with the operands widened to fp32, each product and the one add / subtract rounded to fp32 SEPARATELY and the result converted
// round-to-nearest-even.  The translation unit that includes this header is compiled with -ffp-contract=off (csrc/Makefile): under
// the library's -ffp-contract=fast the compiler fuses a product into the add, and a plain-torch model could not be bit-equal.
// Elements at and past R of every head, and all of V, are copied.
//
// K rows with pos < 0 and (PAGED) rows whose page id lies outside the pool are dropped with their V rows, as the append drops them.
// Q is written for every one of the sequence's Sq_b rows, those with pos < 0 included (the attention call gives them O = 0 whatever
// Q holds).  Never read: packed rows no sequence covers, table rows other than the p of a processed row.  Never written: anything
// but the destination rows of cache or pool and the covered rows of q_out.
//
// Work item = one 16-element unit of one head of one new row: two 16-byte loads, two 16-byte stores.  A row has
// (H + 2 * Hkv) * D / 16 items -- the Q heads, then the K heads, then the V heads, D / 16 units each -- laid out [row][head][unit],
// so consecutive lanes move consecutive pieces.  Unit u of a head takes the 8-element chunks
//   (u, u + R / 16)    in the rotated region of the half style (u < R / 16): x1 and x2 of eight pairs;
//   (2u, 2u + 1)       everywhere else: eight interleaved pairs (one pair per 32-bit word), or 16 elements to copy.
// Either way the unit's cos / sin are the eight floats at [p][8u]: two 16-byte loads each.  Every source chunk is read by exactly one
// item, every destination chunk written by exactly one, and an item reads all it needs before it writes: q_out may be q itself.
//
// 256 threads; a workgroup takes 256 consecutive items of ONE sequence.  Grid = B * ceil(max_seqlen_q * items_per_row / 256) from
// host shapes only: capturable, and valid while cu_seqlens_q, lengths, offsets, block table, the tables' contents and the inputs
// change between replays.  b is uniform per workgroup, so cu[b], cu[b + 1], cache_seqlens[b] and pos_offsets[b] are scalar loads and
// the workgroups past a sequence's last item return before any vector memory instruction.  The block-table lookup is per lane.  No
// LDS, no atomics, no workspace.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rope_parts.h"

namespace pfa {

constexpr int ROPE_APPEND_THREADS = 256;

struct RopeAppendParams {
    const void* q;               // [total_new, H, D] packed, or [B, Sq, H, D] by strides; NULL (with H = 0): K / V only
    void* q_out;
    const void* k_new;
    const void* v_new;
    void* k_cache;               // cache [B, Smax, Hkv, D] by strides, or (PAGED) pool [num_pages, page_size, Hkv, D]
    void* v_cache;
    const float* cos;            // [max_pos, R / 2], row stride cs_stride
    const float* sin;
    const int32_t* cu_seqlens_q; // VARLEN: [B + 1]
    const int32_t* seqlens;      // [B], after the step
    const int32_t* pos_offsets;  // [B] or NULL
    const int32_t* block_table;  // PAGED: [B][max_pages] page ids
    int64_t q_sb, q_ss, q_sh;    // element strides; *_sb unused under VARLEN
    int64_t qo_sb, qo_ss, qo_sh;
    int64_t kn_sb, kn_ss, kn_sh;
    int64_t vn_sb, vn_ss, vn_sh;
    int64_t k_sb, k_sh, k_ss;    // PAGED: k_sb / v_sb are the page strides
    int64_t v_sb, v_sh, v_ss;
    int64_t bt_sb, cs_stride;
    int32_t nchunk;              // workgroups per sequence: ceil(Sq * units / 256)
    int32_t Sq;                  // rows per sequence; VARLEN: max_seqlen_q
    int32_t Smax, total_new;
    int32_t H, Hkv;              // H = 0 without q
    int32_t dunits;              // D / 16
    int32_t runits;              // R / 16
    int32_t units;               // (H + 2 * Hkv) * D / 16; Sq * units + 256 fits 32 bits (checked by the host)
    int32_t max_pos;
    int32_t page_size, num_pages;
};

template <typename T, bool VARLEN, bool PAGED, bool INTERLEAVED>
__global__ __launch_bounds__(ROPE_APPEND_THREADS) void rope_append_kernel(const RopeAppendParams p) {
    const int b = blockIdx.x / p.nchunk;
    const int item0 = (blockIdx.x - b * p.nchunk) * ROPE_APPEND_THREADS;    // the workgroup's first item of sequence b

    int sq, row0;
    rope_seq_rows<VARLEN>(p.cu_seqlens_q, b, p.total_new, p.Sq, row0, sq);
    if (item0 >= sq * p.units) return;                   // wave-uniform: nothing of this sequence in the workgroup
    const int len = min(max(p.seqlens[b], 0), p.Smax);
    const int64_t off = p.pos_offsets ? (int64_t)p.pos_offsets[b] : 0;

    const int item = item0 + (int)threadIdx.x;
    const int i = item / p.units;                        // new row of the sequence
    const int rem = item - i * p.units;
    const int h = rem / p.dunits;                        // Q heads, then K heads, then V heads
    const int u = rem - h * p.dunits;
    if (i >= sq) return;
    const int pos = len - sq + i;                        // its logical key
    const bool is_q = h < p.H, is_v = h >= p.H + p.Hkv;
    const int64_t row = VARLEN ? (int64_t)(row0 + i) : (int64_t)i;
    const int64_t bb = VARLEN ? 0 : (int64_t)b;          // packed rows have no batch stride

    const uint16_t* src;
    uint16_t* dst;
    if (is_q) {
        src = (const uint16_t*)p.q + bb * p.q_sb + row * p.q_ss + (int64_t)h * p.q_sh;
        dst = (uint16_t*)p.q_out + bb * p.qo_sb + row * p.qo_ss + (int64_t)h * p.qo_sh;
    } else {
        if (pos < 0) return;
        int64_t slab = b, tok = pos;                     // contiguous: the sequence's cache; PAGED: the page and the token inside it
        if constexpr (PAGED) {
            const int lp = pos / p.page_size;
            const int pg = p.block_table[(int64_t)b * p.bt_sb + lp];
            if ((unsigned)pg >= (unsigned)p.num_pages) return;              // dropped, never clamped (kv_append_kernel.h)
            slab = pg;
            tok = pos - lp * p.page_size;
        }
        if (is_v) {
            const int64_t hk = h - p.H - p.Hkv;
            src = (const uint16_t*)p.v_new + bb * p.vn_sb + row * p.vn_ss + hk * p.vn_sh;
            dst = (uint16_t*)p.v_cache + slab * p.v_sb + tok * p.v_ss + hk * p.v_sh;
        } else {
            const int64_t hk = h - p.H;
            src = (const uint16_t*)p.k_new + bb * p.kn_sb + row * p.kn_ss + hk * p.kn_sh;
            dst = (uint16_t*)p.k_cache + slab * p.k_sb + tok * p.k_ss + hk * p.k_sh;
        }
    }

    const bool rot = !is_v && u < p.runits;
    int c0 = u * 16, c1 = u * 16 + 8;                    // element offsets of the unit's two chunks
    if (!INTERLEAVED && rot) {
        c0 = u * 8;
        c1 = (u + p.runits) * 8;
    }
    rope_b128 x0 = *reinterpret_cast<const rope_b128*>(src + c0);
    rope_b128 x1 = *reinterpret_cast<const rope_b128*>(src + c1);

    if (rot) {
        float cs[8], sn[8];
        rope_tables(p.cos, p.sin, (int64_t)pos + off, p.max_pos, p.cs_stride, u, cs, sn);
        if constexpr (INTERLEAVED) {
#pragma unroll
            for (int w = 0; w < 4; ++w) {                // a 32-bit word is one pair: pairs 0..3 in x0, 4..7 in x1
                uint32_t lo, hi;
                rope_pair<T>(x0[w] & 0xffffu, x0[w] >> 16, cs[w], sn[w], lo, hi);
                x0[w] = lo | (hi << 16);
                rope_pair<T>(x1[w] & 0xffffu, x1[w] >> 16, cs[4 + w], sn[4 + w], lo, hi);
                x1[w] = lo | (hi << 16);
            }
        } else {
#pragma unroll
            for (int w = 0; w < 4; ++w) {                // x0 holds x[8u ..], x1 holds x[half + 8u ..]: word w is pairs 2w and 2w + 1
                uint32_t a_lo, b_lo, a_hi, b_hi;
                rope_pair<T>(x0[w] & 0xffffu, x1[w] & 0xffffu, cs[2 * w], sn[2 * w], a_lo, b_lo);
                rope_pair<T>(x0[w] >> 16, x1[w] >> 16, cs[2 * w + 1], sn[2 * w + 1], a_hi, b_hi);
                x0[w] = a_lo | (a_hi << 16);
                x1[w] = b_lo | (b_hi << 16);
            }
        }
    }
    *reinterpret_cast<rope_b128*>(dst + c0) = x0;
    *reinterpret_cast<rope_b128*>(dst + c1) = x1;
}

}  // namespace pfa

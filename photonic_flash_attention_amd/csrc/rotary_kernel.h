// rotary_kernel.h -- rotary embedding for the training calls on MI355X (gfx950), hand-written HIP: rotates up to two tensors that share
// rows and positions -- x0 with H0 heads (Q, or dQ in the backward) and optionally x1 with H1 heads (K or dK) -- in one launch, from
// device data alone.  Dense: a [B, H, S, D] shape by element strides (sb, ss, sh), D contiguous, so a permuted [B, S, H, D] tensor is
// legal.  PACKED: [total, H, D] rows by (ss, sh), with the clamps of the other packed kernels:
//   s_b = clamp(cu[b], 0, total), e_b = clamp(cu[b + 1], s_b, total), rows_b = min(e_b - s_b, S)   (S: max_seqlen).
// The rotary position of row i of sequence b is clamp(p, 0, max_pos - 1), computed in 64 bits, where p = position_ids[...] when that
// pointer is given (int32; dense by (pid_sb, pid_ss), packed [total]) and else i + pos_offsets[b] (pos_offsets NULL: 0): an
// out-of-range position gives wrong numbers, never an address outside the tables.
//
// The arithmetic is rope_append_kernel.h's, to the letter (rope_pair, rope_widen and rope_narrow are rope_parts.h's): with R = rot_dim,
// half = R / 2, c = cos[p][j], s = sin[p][j] (fp32 tables [max_pos, half], row stride cs_stride) the pair (x1, x2) = (x[j], x[j + half])
// -- or, INTERLEAVED, (x[2j], x[2j + 1]) -- becomes y1 = x1 * c - x2 * s, y2 = x2 * c + x1 * s, operands widened to fp32, each product
// and the one add / subtract rounded to fp32 SEPARATELY (the unit is built with -ffp-contract=off), one round-to-nearest-even to the
// dtype.  The conjugate rotation (the backward: dx1 = dy1 * c + dy2 * s, dx2 = dy2 * c - dy1 * s) is the same rule with the sign of
// sin flipped, which is exact: a run-time value here, as the in-place mode is, so that both directions are the same eight kernels.
//
// Work item = one 16-element unit of one head of one row: two 16-byte loads, two 16-byte stores, laid out [row][head][unit] with the
// H0 heads of x0 in front of the H1 heads of x1.  Unit u of a head takes the 8-element chunks
//   (u, u + R / 16)    in the rotated region of the half style (u < R / 16): x1 and x2 of eight pairs;
//   (2u, 2u + 1)       everywhere else: eight interleaved pairs (one pair per 32-bit word), or 16 elements to copy.
// Out of place a head has D / 16 units and the elements at and past R are copied.  In place (the output IS the input: same pointer,
// same strides) a head has R / 16 units: elements at and past R are neither read nor written, so a partial rotation moves only the
// bytes it changes.  Every source chunk is read by exactly one item, every destination chunk written by exactly one, and an item
// reads all it needs before it writes.
//
// 256 threads; a workgroup takes 256 consecutive items of ONE sequence.  Grid = B * ceil(S * units / 256) from host shapes only:
// capturable, and valid while cu_seqlens, offsets, position_ids, the tables' contents and the inputs change between replays.  b is
// uniform per workgroup, so cu[b], cu[b + 1] and pos_offsets[b] are scalar loads and a workgroup past its sequence's last item returns
// before any vector memory instruction.  Never read or written: packed rows no sequence covers, rows past max_seqlen of a sequence.
// No LDS, no atomics, no workspace.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rope_parts.h"

namespace pfa {

constexpr int ROTARY_THREADS = 256;

struct RotaryParams {
    const void* x0;              // [B, H0, S, D] by strides, or PACKED [total, H0, D]
    void* x0_out;
    const void* x1;              // H1 heads over the same rows; NULL with H1 = 0
    void* x1_out;
    const float* cos;            // [max_pos, R / 2], row stride cs_stride
    const float* sin;
    const int32_t* cu_seqlens;   // PACKED: [B + 1]
    const int32_t* pos_offsets;  // [B] or NULL
    const int32_t* position_ids; // dense [B, S] by (pid_sb, pid_ss), PACKED [total]; or NULL
    int64_t x0_sb, x0_ss, x0_sh; // element strides; *_sb unused under PACKED
    int64_t x0o_sb, x0o_ss, x0o_sh;
    int64_t x1_sb, x1_ss, x1_sh;
    int64_t x1o_sb, x1o_ss, x1o_sh;
    int64_t pid_sb, pid_ss, cs_stride;
    int32_t nchunk;              // workgroups per sequence: ceil(S * units / 256)
    int32_t S;                   // rows per sequence; PACKED: max_seqlen
    int32_t total;
    int32_t H0;
    int32_t hunits;              // units of one head: D / 16, in place R / 16
    int32_t runits;              // R / 16
    int32_t units;               // (H0 + H1) * hunits; S * units + 256 fits 32 bits (checked by the host)
    int32_t max_pos;
    int32_t conjugate;           // non-zero: the sign of sin flipped
};

template <typename T, bool PACKED, bool INTERLEAVED>
__global__ __launch_bounds__(ROTARY_THREADS) void rotary_kernel(const RotaryParams p) {
    const int b = blockIdx.x / p.nchunk;
    const int item0 = (blockIdx.x - b * p.nchunk) * ROTARY_THREADS;         // the workgroup's first item of sequence b

    int rows, row0;
    rope_seq_rows<PACKED>(p.cu_seqlens, b, p.total, p.S, row0, rows);
    if (item0 >= rows * p.units) return;                 // wave-uniform: nothing of this sequence in the workgroup
    const int64_t off = p.pos_offsets ? (int64_t)p.pos_offsets[b] : 0;

    const int item = item0 + (int)threadIdx.x;
    const int i = item / p.units;                        // row of the sequence
    const int rem = item - i * p.units;
    const int h = rem / p.hunits;                        // the heads of x0, then those of x1
    const int u = rem - h * p.hunits;
    if (i >= rows) return;
    const int64_t row = PACKED ? (int64_t)(row0 + i) : (int64_t)i;
    const int64_t bb = PACKED ? 0 : (int64_t)b;          // packed rows have no batch stride

    const uint16_t* src;
    uint16_t* dst;
    if (h < p.H0) {
        src = (const uint16_t*)p.x0 + bb * p.x0_sb + row * p.x0_ss + (int64_t)h * p.x0_sh;
        dst = (uint16_t*)p.x0_out + bb * p.x0o_sb + row * p.x0o_ss + (int64_t)h * p.x0o_sh;
    } else {
        const int64_t h1 = h - p.H0;
        src = (const uint16_t*)p.x1 + bb * p.x1_sb + row * p.x1_ss + h1 * p.x1_sh;
        dst = (uint16_t*)p.x1_out + bb * p.x1o_sb + row * p.x1o_ss + h1 * p.x1o_sh;
    }

    const bool rot = u < p.runits;                       // in place: every unit
    int c0 = u * 16, c1 = u * 16 + 8;                    // element offsets of the unit's two chunks
    if (!INTERLEAVED && rot) {
        c0 = u * 8;
        c1 = (u + p.runits) * 8;
    }
    rope_b128 a0 = *reinterpret_cast<const rope_b128*>(src + c0);
    rope_b128 a1 = *reinterpret_cast<const rope_b128*>(src + c1);

    if (rot) {
        float cs[8], sn[8];
        rope_tables(p.cos, p.sin, rope_row_pos<PACKED>(p.position_ids, bb, row, p.pid_sb, p.pid_ss, i, off), p.max_pos, p.cs_stride, u, cs, sn);
        if (p.conjugate) {
#pragma unroll
            for (int w = 0; w < 8; ++w) sn[w] = -sn[w];  // exact: the conjugate is the same three roundings
        }
        if constexpr (INTERLEAVED) {
#pragma unroll
            for (int w = 0; w < 4; ++w) {                // a 32-bit word is one pair: pairs 0..3 in a0, 4..7 in a1
                uint32_t lo, hi;
                rope_pair<T>(a0[w] & 0xffffu, a0[w] >> 16, cs[w], sn[w], lo, hi);
                a0[w] = lo | (hi << 16);
                rope_pair<T>(a1[w] & 0xffffu, a1[w] >> 16, cs[4 + w], sn[4 + w], lo, hi);
                a1[w] = lo | (hi << 16);
            }
        } else {
#pragma unroll
            for (int w = 0; w < 4; ++w) {                // a0 holds x[8u ..], a1 holds x[half + 8u ..]: word w is pairs 2w and 2w + 1
                uint32_t a_lo, b_lo, a_hi, b_hi;
                rope_pair<T>(a0[w] & 0xffffu, a1[w] & 0xffffu, cs[2 * w], sn[2 * w], a_lo, b_lo);
                rope_pair<T>(a0[w] >> 16, a1[w] >> 16, cs[2 * w + 1], sn[2 * w + 1], a_hi, b_hi);
                a0[w] = a_lo | (a_hi << 16);
                a1[w] = b_lo | (b_hi << 16);
            }
        }
    }
    *reinterpret_cast<rope_b128*>(dst + c0) = a0;
    *reinterpret_cast<rope_b128*>(dst + c1) = a1;
}

}  // namespace pfa

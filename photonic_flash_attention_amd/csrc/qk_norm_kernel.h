// qk_norm_kernel.h -- QK-norm (an RMSNorm over the head dim of every head of Q and K) fused with the rotary embedding of the training
// calls, forward and backward, hand-written HIP for MI355X (gfx950).  One launch handles x0 with H0 heads (Q) and optionally x1 with H1
// heads (K) over the same rows and positions.  Layouts, clamps, positions, tables and the grid rule are rotary_kernel.h's, to the letter
// (the clamp, the position and the table load are rope_parts.h's functions, shared with it):
// dense [B, H, S, D] by element strides (sb, ss, sh), D contiguous; PACKED [total, H, D] with
//   s_b = clamp(cu[b], 0, total), e_b = clamp(cu[b + 1], s_b, total), rows_b = min(e_b - s_b, S)   (S: max_seqlen);
// the position of row i of sequence b is clamp(p, 0, max_pos - 1) in 64 bits, p = position_ids[...] or i + pos_offsets[b]; tables fp32
// [max_pos, R / 2] with row stride cs_stride; the pairing half or INTERLEAVED.  R = rot_dim is a multiple of 16 with R <= D, or R = 0 with
// cos = sin = NULL: the norm alone.
//
// Work item = one 16-element unit of one head of one row, with rotary_kernel.h's chunk pairing: unit u takes the 8-element chunks
// (u, u + R / 16) in the rotated region of the half style (u < R / 16) and (2u, 2u + 1) everywhere else.  A head is G = D / 16
// consecutive lanes (D 64 / 128: G 4 / 8, a template parameter).  G divides 64 and the items are laid out [row][head][unit], a multiple
// of G a row, so a head never straddles a wave and is either wholly inside its sequence or wholly outside it.
// NO LANE OF A LIVE GROUP MAY RETURN BEFORE THE GROUP'S CROSS-LANE EXCHANGE: past the workgroup-uniform early return the kernels have
// no return at all -- a lane past its sequence's last item loads nothing, computes on zeros, takes part in every exchange and stores
// nothing -- and no exchange stands under a lane-dependent branch.
//
// The arithmetic is all fp32 on widened operands, every product and every sum rounded SEPARATELY (the unit is built with
// -ffp-contract=off, csrc/Makefile):
//   sq_j = x_j * x_j; each 8-element chunk summed left to right; a lane adds its two chunk sums in the order of its chunk pair; the G
//   lanes of a head summed by an xor butterfly (masks 1, 2, .. G / 2: every lane ends with the same bits); ms = sum * (1 / D);
//   r = 1.0f / sqrtf(ms + eps)  (IEEE square root and divide, correctly rounded; no v_rsq_f32);
//   n_j = (x_j * r) * s_j, s_j = w_j widened, or with UNIT_OFFSET (Gemma) 1.0f + w_j;
//   elements under R rotated on the fp32 n with the three roundings of rope_pair (y1 = n1 * c - n2 * s, y2 = n2 * c + n1 * s), elements
//   at and past R are n; one round-to-nearest-even to the dtype.
// Weights w0[D], w1[D] are shared by the heads of a tensor, contiguous, fp32 or of the tensors' dtype (a run-time field, wave-uniform).
// In place (x_out == x, same strides) is legal in the forward: an item reads everything it needs before it writes, and every element
// is read by exactly one item.  No LDS, no atomics, no workspace in the forward; grid = B * ceil(S * units / 256), host shapes only.
//
// Backward, two launches.  Per head: r recomputed from x by the forward's rule (nothing but x is saved); g = the conjugate rotation of
// the widened dy in fp32 (g1 = dy1 * c + dy2 * s, g2 = dy2 * c - dy1 * s: rope_pair at -sin, which is exact), g = dy with R = 0 and at
// and past R; xh_j = x_j * r; a_j = g_j * s_j; c = the forward's sum tree over a_j * xh_j, times (1 / D); dx_j = r * (a_j - xh_j * c),
// one narrowing.  The weight gradient dw_j = sum over rows and heads of g_j * xh_j, with no atomics:
//   1. qk_norm_bwd_kernel: workgroup (tensor t, sequence b, chunk c) walks rows [c * QKNORM_BWD_ROWS, (c + 1) * QKNORM_BWD_ROWS) of
//      sequence b of tensor t, 256 items (256 / G heads) a step in item order.  256 and a row's items are multiples of G, so a lane keeps
//      its unit u -- its 16 element indices, its weights -- for the whole walk and keeps 16 fp32 sums in registers, each += g * xh in
//      step order.  The 256 / G head slots are folded through LDS in slot order and ONE fp32 [D] partial goes to the workspace,
//      partial[(t * B + b) * nrc + c][D].  A chunk past its sequence's rows leaves zeros and reads nothing.
//   2. qk_norm_dw_kernel: D / 16 workgroups per tensor, 16 elements of the head dim each; thread (k, j) of 16 x 16 adds the partials
//      k, k + 16, ... of its element in index order, the 16 sums are folded through LDS in order, and dw[j] is OVERWRITTEN.
// Rows no sequence covers contribute nothing and are never read.  Every sum's order is fixed by the shapes alone: bitwise reproducible.
// Both grids come from host shapes only, so a captured step replays while lengths, positions and data change.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rope_parts.h"

namespace pfa {

constexpr int QKNORM_THREADS = 256;
constexpr int QKNORM_BWD_ROWS = 32;        // rows of one sequence a stage-1 workgroup of the backward walks
constexpr int QKNORM_DW_GROUPS = 16;       // interleaved groups of partials a stage-2 workgroup adds side by side

struct QkNormParams {
    const void* x0;              // [B, H0, S, D] by strides, or PACKED [total, H0, D]
    void* x0_out;
    const void* x1;              // H1 heads over the same rows; NULL with H1 = 0
    void* x1_out;
    const void* w0;              // [D], fp32 (w_fp32) or the tensors' dtype
    const void* w1;
    const float* cos;            // [max_pos, R / 2], row stride cs_stride; NULL with R = 0
    const float* sin;
    const int32_t* cu_seqlens;   // PACKED: [B + 1]
    const int32_t* pos_offsets;  // [B] or NULL
    const int32_t* position_ids; // dense [B, S] by (pid_sb, pid_ss), PACKED [total]; or NULL
    int64_t x0_sb, x0_ss, x0_sh; // element strides; *_sb unused under PACKED
    int64_t x0o_sb, x0o_ss, x0o_sh;
    int64_t x1_sb, x1_ss, x1_sh;
    int64_t x1o_sb, x1o_ss, x1o_sh;
    int64_t pid_sb, pid_ss, cs_stride;
    float eps;
    float inv_d;                 // 1 / D: a power of two
    int32_t nchunk;              // workgroups per sequence: ceil(S * units / 256)
    int32_t S;                   // rows per sequence; PACKED: max_seqlen
    int32_t total;
    int32_t H0;
    int32_t runits;              // R / 16
    int32_t units;               // (H0 + H1) * D / 16; S * units + 256 fits 32 bits (checked by the host)
    int32_t max_pos;
    int32_t w_fp32;              // non-zero: the weights are fp32
    int32_t unit_offset;         // non-zero: s = 1.0f + w
};

struct QkNormBwdParams {
    const void* x0;              // as the forward's
    const void* dy0;
    void* dx0;
    const void* x1;
    const void* dy1;
    void* dx1;
    const void* w0;
    const void* w1;
    float* dw0;                  // fp32 [D], overwritten
    float* dw1;
    float* partial;              // [(t * B + b) * nrc + c][D]
    const float* cos;
    const float* sin;
    const int32_t* cu_seqlens;
    const int32_t* pos_offsets;
    const int32_t* position_ids;
    int64_t x0_sb, x0_ss, x0_sh;
    int64_t dy0_sb, dy0_ss, dy0_sh;
    int64_t dx0_sb, dx0_ss, dx0_sh;
    int64_t x1_sb, x1_ss, x1_sh;
    int64_t dy1_sb, dy1_ss, dy1_sh;
    int64_t dx1_sb, dx1_ss, dx1_sh;
    int64_t pid_sb, pid_ss, cs_stride;
    float eps;
    float inv_d;
    int32_t nrc;                 // row chunks per sequence: ceil(S / QKNORM_BWD_ROWS)
    int32_t B;
    int32_t S;
    int32_t total;
    int32_t H0, H1;
    int32_t runits;
    int32_t max_pos;
    int32_t w_fp32;
    int32_t unit_offset;
};

template <typename T>
__device__ __forceinline__ void qkn_widen8(const rope_b128 v, float* f) {
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        f[2 * w] = rope_widen<T>(v[w] & 0xffffu);
        f[2 * w + 1] = rope_widen<T>(v[w] >> 16);
    }
}
template <typename T>
__device__ __forceinline__ rope_b128 qkn_narrow8(const float* f) {
    rope_b128 v;
#pragma unroll
    for (int w = 0; w < 4; ++w) v[w] = rope_narrow<T>(f[2 * w]) | (rope_narrow<T>(f[2 * w + 1]) << 16);
    return v;
}

// the scale s of the eight elements at `at`: w widened, or 1.0f + w
template <typename T>
__device__ __forceinline__ void qkn_scale8(const void* w, int at, bool w_fp32, bool unit_offset, float* s) {
    if (w_fp32) {                                        // wave-uniform
        const rope_f4 a = *reinterpret_cast<const rope_f4*>((const float*)w + at), b = *reinterpret_cast<const rope_f4*>((const float*)w + at + 4);
        s[0] = a.x; s[1] = a.y; s[2] = a.z; s[3] = a.w; s[4] = b.x; s[5] = b.y; s[6] = b.z; s[7] = b.w;
    } else {
        qkn_widen8<T>(*reinterpret_cast<const rope_b128*>((const uint16_t*)w + at), s);
    }
    if (unit_offset) {
#pragma unroll
        for (int k = 0; k < 8; ++k) s[k] = 1.0f + s[k];
    }
}

// sum over a head of the lane's 16 products a[k] * b[k] (chunk A, then chunk B): each chunk left to right, the two chunk sums, then the
// xor butterfly over the head's G lanes.  Every lane of the wave must call it.
template <int G>
__device__ __forceinline__ float qkn_head_sum(const float* a0, const float* b0, const float* a1, const float* b1) {
    float sa = a0[0] * b0[0], sb = a1[0] * b1[0];
#pragma unroll
    for (int k = 1; k < 8; ++k) {
        sa = sa + a0[k] * b0[k];
        sb = sb + a1[k] * b1[k];
    }
    float v = sa + sb;
#pragma unroll
    for (int m = 1; m < G; m <<= 1) v = v + __shfl_xor(v, m);
    return v;
}

// the unit's eight pairs rotated in fp32, in registers: half style (na[k], nb[k]), INTERLEAVED (n[2w], n[2w + 1]) with pairs 0..3 in na
template <bool INTERLEAVED>
__device__ __forceinline__ void qkn_rotate(float* na, float* nb, const float* cs, const float* sn) {
    if constexpr (INTERLEAVED) {
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            float y1, y2;
            rope_pair_f32(na[2 * w], na[2 * w + 1], cs[w], sn[w], y1, y2);
            na[2 * w] = y1; na[2 * w + 1] = y2;
            rope_pair_f32(nb[2 * w], nb[2 * w + 1], cs[4 + w], sn[4 + w], y1, y2);
            nb[2 * w] = y1; nb[2 * w + 1] = y2;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            float y1, y2;
            rope_pair_f32(na[k], nb[k], cs[k], sn[k], y1, y2);
            na[k] = y1; nb[k] = y2;
        }
    }
}

template <typename T, int G, bool PACKED, bool INTERLEAVED>
__global__ __launch_bounds__(QKNORM_THREADS) void qk_norm_kernel(const QkNormParams p) {
    const int b = blockIdx.x / p.nchunk;
    const int item0 = (blockIdx.x - b * p.nchunk) * QKNORM_THREADS;         // the workgroup's first item of sequence b

    int rows, row0;
    rope_seq_rows<PACKED>(p.cu_seqlens, b, p.total, p.S, row0, rows);
    if (item0 >= rows * p.units) return;                 // workgroup-uniform: the only return (see the header of this file)
    const int64_t off = p.pos_offsets ? (int64_t)p.pos_offsets[b] : 0;

    const int item = item0 + (int)threadIdx.x;
    const int i = item / p.units;                        // row of the sequence
    const int rem = item - i * p.units;
    const int h = rem / G;                               // the heads of x0, then those of x1
    const int u = rem - h * G;
    const bool live = i < rows;                          // uniform over the G lanes of a head
    const int64_t row = PACKED ? (int64_t)(row0 + i) : (int64_t)i;
    const int64_t bb = PACKED ? 0 : (int64_t)b;          // packed rows have no batch stride

    const uint16_t* src;
    uint16_t* dst;
    const void* w;
    if (h < p.H0) {
        src = (const uint16_t*)p.x0 + bb * p.x0_sb + row * p.x0_ss + (int64_t)h * p.x0_sh;
        dst = (uint16_t*)p.x0_out + bb * p.x0o_sb + row * p.x0o_ss + (int64_t)h * p.x0o_sh;
        w = p.w0;
    } else {
        const int64_t h1 = h - p.H0;
        src = (const uint16_t*)p.x1 + bb * p.x1_sb + row * p.x1_ss + h1 * p.x1_sh;
        dst = (uint16_t*)p.x1_out + bb * p.x1o_sb + row * p.x1o_ss + h1 * p.x1o_sh;
        w = p.w1;
    }

    const bool rot = u < p.runits;
    int c0 = u * 16, c1 = u * 16 + 8;                    // element offsets of the unit's two chunks
    if (!INTERLEAVED && rot) {
        c0 = u * 8;
        c1 = (u + p.runits) * 8;
    }
    float xa[8], xb[8], wa[8], wb[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) xa[k] = xb[k] = wa[k] = wb[k] = 0.f;
    if (live) {
        qkn_widen8<T>(*reinterpret_cast<const rope_b128*>(src + c0), xa);
        qkn_widen8<T>(*reinterpret_cast<const rope_b128*>(src + c1), xb);
        qkn_scale8<T>(w, c0, p.w_fp32 != 0, p.unit_offset != 0, wa);
        qkn_scale8<T>(w, c1, p.w_fp32 != 0, p.unit_offset != 0, wb);
    }

    const float ms = qkn_head_sum<G>(xa, xa, xb, xb) * p.inv_d;             // every lane of the wave is here
    const float r = 1.0f / sqrtf(ms + p.eps);

    float na[8], nb[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        na[k] = (xa[k] * r) * wa[k];
        nb[k] = (xb[k] * r) * wb[k];
    }
    if (live && rot) {
        float cs[8], sn[8];
        rope_tables(p.cos, p.sin, rope_row_pos<PACKED>(p.position_ids, bb, row, p.pid_sb, p.pid_ss, i, off), p.max_pos, p.cs_stride, u, cs, sn);
        qkn_rotate<INTERLEAVED>(na, nb, cs, sn);
    }
    if (live) {
        *reinterpret_cast<rope_b128*>(dst + c0) = qkn_narrow8<T>(na);
        *reinterpret_cast<rope_b128*>(dst + c1) = qkn_narrow8<T>(nb);
    }
}

template <typename T, int G, bool PACKED, bool INTERLEAVED>
__global__ __launch_bounds__(QKNORM_THREADS) void qk_norm_bwd_kernel(const QkNormBwdParams p) {
    constexpr int D = 16 * G, SLOTS = QKNORM_THREADS / G;
    __shared__ float fold[SLOTS][D];                     // 16 KiB

    const int c = blockIdx.x % p.nrc;                    // ((t * B) + b) * nrc + c
    const int tb = blockIdx.x / p.nrc, b = tb % p.B, t = tb / p.B;
    const int tid = (int)threadIdx.x;
    float* part = p.partial + (int64_t)blockIdx.x * D;

    int rows, row0;
    rope_seq_rows<PACKED>(p.cu_seqlens, b, p.total, p.S, row0, rows);
    const int r0 = c * QKNORM_BWD_ROWS;
    if (r0 >= rows) {                                    // workgroup-uniform: a chunk past its sequence leaves zeros and reads nothing
        if (tid < D) part[tid] = 0.f;
        return;
    }
    const int64_t off = p.pos_offsets ? (int64_t)p.pos_offsets[b] : 0;
    const int hg = (t ? p.H1 : p.H0) * G;                // items of a row of this tensor
    const int nitems = min(QKNORM_BWD_ROWS, rows - r0) * hg;
    const uint16_t* xt = (const uint16_t*)(t ? p.x1 : p.x0);
    const uint16_t* dyt = (const uint16_t*)(t ? p.dy1 : p.dy0);
    uint16_t* dxt = (uint16_t*)(t ? p.dx1 : p.dx0);
    const int64_t x_sb = t ? p.x1_sb : p.x0_sb, x_ss = t ? p.x1_ss : p.x0_ss, x_sh = t ? p.x1_sh : p.x0_sh;
    const int64_t dy_sb = t ? p.dy1_sb : p.dy0_sb, dy_ss = t ? p.dy1_ss : p.dy0_ss, dy_sh = t ? p.dy1_sh : p.dy0_sh;
    const int64_t dx_sb = t ? p.dx1_sb : p.dx0_sb, dx_ss = t ? p.dx1_ss : p.dx0_ss, dx_sh = t ? p.dx1_sh : p.dx0_sh;
    const int64_t bb = PACKED ? 0 : (int64_t)b;

    const int u = tid % G, slot = tid / G;               // the lane's unit for the whole walk: 256 and hg are multiples of G
    const bool rot = u < p.runits;
    int c0 = u * 16, c1 = u * 16 + 8;
    if (!INTERLEAVED && rot) {
        c0 = u * 8;
        c1 = (u + p.runits) * 8;
    }
    float wa[8], wb[8], acc_a[8], acc_b[8];
    qkn_scale8<T>(t ? p.w1 : p.w0, c0, p.w_fp32 != 0, p.unit_offset != 0, wa);
    qkn_scale8<T>(t ? p.w1 : p.w0, c1, p.w_fp32 != 0, p.unit_offset != 0, wb);
#pragma unroll
    for (int k = 0; k < 8; ++k) acc_a[k] = acc_b[k] = 0.f;

    for (int it0 = 0; it0 < nitems; it0 += QKNORM_THREADS) {                // workgroup-uniform trip count
        const int item = it0 + tid;
        const bool live = item < nitems;                 // uniform over the G lanes of a head; no lane leaves the loop early
        const int il = item / hg;
        const int h = (item - il * hg) / G;
        const int i = r0 + il;
        const int64_t row = PACKED ? (int64_t)(row0 + i) : (int64_t)i;
        const uint16_t* xs = xt + bb * x_sb + row * x_ss + (int64_t)h * x_sh;
        const uint16_t* dys = dyt + bb * dy_sb + row * dy_ss + (int64_t)h * dy_sh;
        uint16_t* dxs = dxt + bb * dx_sb + row * dx_ss + (int64_t)h * dx_sh;

        float xa[8], xb[8], ga[8], gb[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) xa[k] = xb[k] = ga[k] = gb[k] = 0.f;
        if (live) {
            qkn_widen8<T>(*reinterpret_cast<const rope_b128*>(xs + c0), xa);
            qkn_widen8<T>(*reinterpret_cast<const rope_b128*>(xs + c1), xb);
            qkn_widen8<T>(*reinterpret_cast<const rope_b128*>(dys + c0), ga);
            qkn_widen8<T>(*reinterpret_cast<const rope_b128*>(dys + c1), gb);
        }
        if (live && rot) {
            float cs[8], sn[8];
            rope_tables(p.cos, p.sin, rope_row_pos<PACKED>(p.position_ids, bb, row, p.pid_sb, p.pid_ss, i, off), p.max_pos, p.cs_stride, u, cs, sn);
#pragma unroll
            for (int k = 0; k < 8; ++k) sn[k] = -sn[k];  // exact: the conjugate is the same three roundings
            qkn_rotate<INTERLEAVED>(ga, gb, cs, sn);
        }

        const float ms = qkn_head_sum<G>(xa, xa, xb, xb) * p.inv_d;         // every lane of the wave is here
        const float r = 1.0f / sqrtf(ms + p.eps);
        float ha[8], hb[8], aa[8], ab[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            ha[k] = xa[k] * r;
            hb[k] = xb[k] * r;
            aa[k] = ga[k] * wa[k];
            ab[k] = gb[k] * wb[k];
        }
        const float cc = qkn_head_sum<G>(aa, ha, ab, hb) * p.inv_d;
        if (live) {
            float da[8], db[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                da[k] = r * (aa[k] - ha[k] * cc);
                db[k] = r * (ab[k] - hb[k] * cc);
                acc_a[k] = acc_a[k] + ga[k] * ha[k];
                acc_b[k] = acc_b[k] + gb[k] * hb[k];
            }
            *reinterpret_cast<rope_b128*>(dxs + c0) = qkn_narrow8<T>(da);
            *reinterpret_cast<rope_b128*>(dxs + c1) = qkn_narrow8<T>(db);
        }
    }

#pragma unroll
    for (int k = 0; k < 8; ++k) {
        fold[slot][c0 + k] = acc_a[k];
        fold[slot][c1 + k] = acc_b[k];
    }
    __syncthreads();
    if (tid < D) {
        float s = fold[0][tid];
        for (int q = 1; q < SLOTS; ++q) s = s + fold[q][tid];               // slot order
        part[tid] = s;
    }
}

template <int D>
__global__ __launch_bounds__(QKNORM_THREADS) void qk_norm_dw_kernel(const QkNormBwdParams p) {
    constexpr int NG = QKNORM_DW_GROUPS, PER = D / 16;   // 16 groups of 16 lanes; PER workgroups a tensor, 16 elements of the head dim each
    __shared__ float fold[QKNORM_THREADS];
    const int t = blockIdx.x / PER, col0 = (blockIdx.x - t * PER) * 16, tid = (int)threadIdx.x;
    const int P = p.B * p.nrc;                           // the tensor's partials
    const float* part = p.partial + (int64_t)t * P * D;
    const int k = tid / 16, j = col0 + (tid & 15);
    float s = 0.f;
#pragma unroll 4
    for (int q = k; q < P; q += NG) s = s + part[(int64_t)q * D + j];      // index order
    fold[tid] = s;
    __syncthreads();
    if (tid < 16) {
        float v = fold[tid];
#pragma unroll
        for (int q = 1; q < NG; ++q) v = v + fold[q * 16 + tid];
        (t ? p.dw1 : p.dw0)[col0 + tid] = v;
    }
}

}  // namespace pfa

// rope_parts.h -- what the kernels that handle 16-bit rows by position share (rope_append_kernel.h, rotary_kernel.h, qk_norm_kernel.h):
// the 16-byte vector types, the widening and narrowing of an element, one rotated pair, the rows of a packed sequence, a row's position
// and the load of a unit's cos / sin.  Every function is forced inline and leaves each kernel the instructions it had with the text
// spelled out (tools/isa_same.py).  The 16-element chunk pairing (c0, c1) and the unrolled rotation of a 16-bit unit are NOT here: as
// functions they changed register allocation and scheduling of the kernels, so those stay inline in each kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pfa {

typedef uint32_t rope_b128 __attribute__((ext_vector_type(4)));
typedef float rope_f4 __attribute__((ext_vector_type(4)));

template <typename T>
__device__ __forceinline__ float rope_widen(uint32_t h) {
    return static_cast<float>(__builtin_bit_cast(T, (uint16_t)h));
}
template <typename T>
__device__ __forceinline__ uint32_t rope_narrow(float f) {       // round to nearest even
    return __builtin_bit_cast(uint16_t, static_cast<T>(f));
}
// one pair: the three roundings are separate fp32 operations (the objects that use it are built with -ffp-contract=off)
template <typename T>
__device__ __forceinline__ void rope_pair(uint32_t x1, uint32_t x2, float c, float s, uint32_t& y1, uint32_t& y2) {
    const float a = rope_widen<T>(x1), b = rope_widen<T>(x2);
    y1 = rope_narrow<T>(a * c - b * s);
    y2 = rope_narrow<T>(b * c + a * s);
}
// rope_pair on fp32 operands: the same three roundings, no narrowing
__device__ __forceinline__ void rope_pair_f32(float a, float b, float c, float s, float& y1, float& y2) {
    y1 = a * c - b * s;
    y2 = b * c + a * s;
}

// the rows of sequence b: dense, rows [0, S) of batch b; PACKED, with cu = cu_seqlens and S = max_seqlen,
//   s_b = clamp(cu[b], 0, total), e_b = clamp(cu[b + 1], s_b, total): rows [s_b, s_b + min(e_b - s_b, S)) of the packed tensor.
// b is workgroup-uniform in every caller, so the two loads are scalar.
template <bool PACKED>
__device__ __forceinline__ void rope_seq_rows(const int32_t* cu, int b, int total, int S, int& row0, int& rows) {
    row0 = 0;
    rows = S;
    if constexpr (PACKED) {
        const int s_b = min(max(cu[b], 0), total);
        const int e_b = min(max(cu[b + 1], s_b), total);
        row0 = s_b;
        rows = min(e_b - s_b, S);
    }
}

// the position of row i of its sequence, before the clamp: position_ids[...] when given (dense by (pid_sb, pid_ss) from batch bb, PACKED
// [total] by the packed row), else i + off (off: the sequence's pos_offsets entry, 0 without)
template <bool PACKED>
__device__ __forceinline__ int64_t rope_row_pos(const int32_t* position_ids, int64_t bb, int64_t row, int64_t pid_sb, int64_t pid_ss, int i,
                                                int64_t off) {
    int64_t pos = (int64_t)i + off;
    if (position_ids) pos = PACKED ? (int64_t)position_ids[row] : (int64_t)position_ids[bb * pid_sb + row * pid_ss];
    return pos;
}

// unit u's eight cos and eight sin at clamp(pos, 0, max_pos - 1), in 64 bits: an out-of-range position gives wrong numbers, never an
// address outside the tables.  Two 16-byte loads each.
__device__ __forceinline__ void rope_tables(const float* cos, const float* sin, int64_t pos, int max_pos, int64_t cs_stride, int u, float* cs, float* sn) {
    const int64_t rp = min(max(pos, (int64_t)0), (int64_t)max_pos - 1);
    const int64_t at = rp * cs_stride + u * 8;
    const rope_f4 ca = *reinterpret_cast<const rope_f4*>(cos + at), cb = *reinterpret_cast<const rope_f4*>(cos + at + 4);
    const rope_f4 sa = *reinterpret_cast<const rope_f4*>(sin + at), sb = *reinterpret_cast<const rope_f4*>(sin + at + 4);
    cs[0] = ca.x; cs[1] = ca.y; cs[2] = ca.z; cs[3] = ca.w; cs[4] = cb.x; cs[5] = cb.y; cs[6] = cb.z; cs[7] = cb.w;
    sn[0] = sa.x; sn[1] = sa.y; sn[2] = sa.z; sn[3] = sa.w; sn[4] = sb.x; sn[5] = sb.y; sn[6] = sb.z; sn[7] = sb.w;
}

}  // namespace pfa

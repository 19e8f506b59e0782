// attn_merge_kernel.h -- merge of partial attention results for MI355X (gfx950), hand-written HIP: N results (O_n, LSE_n) over disjoint
// key sets become the result over their union.  What a cut of the keys needs behind it: a shared prefix computed once for the whole
// batch, a split over keys, keys spread over several GPUs.
//
// For every row (b, i, h), in fp32 and in part order n = 0 .. N - 1:
//       m    = max_n lse_n                    over the parts with lse_n > -inf
//       w_n  = exp(lse_n - m),  s = sum_n w_n
//       O[d] = (sum_n w_n * O_n[d]) / s,      LSE = m + log(s)
// A part with lse_n = -inf (no visible key) is SKIPPED, not multiplied by zero: its O may hold anything, NaN included.  All parts -inf:
// O = 0, LSE = -inf, the library's row with no visible key.  A NaN LSE gives a NaN row.  Rows are independent.
// exp is v_exp_f32 of (lse_n - m) * log2(e) and log is v_log_f32 * ln(2): exp2(0) = 1 and log2(1) = 0 are exact there, and the
// division is a correctly rounded one by s itself, so one finite part among -inf parts comes out bit for bit (w = 1, s = 1: fma(1, o,
// 0) / 1 = o and m + 0 = m).  No epsilon, no reciprocal.  Fixed order, no atomics: two runs give the same bits.
//
// Work item = 8 consecutive elements of one (row, head): per part one 16-byte load (16-bit parts) or two (fp32 parts) and the row's
// LSE, one or two 16-byte stores.  Items are laid out [b][i][h][chunk], so consecutive lanes move consecutive pieces of the
// [B, Sq, H, D] buffers the cache calls write.  Grid = ceil(B * Sq * H * (D / 8) / 256) from host shapes only.  N is a template
// parameter: the loop over the parts is unrolled, every part's pointer and strides are scalar kernel arguments at constant offsets
// and all N loads are in flight before the first is used.  The O of a skipped part is loaded and not used (its address is valid;
// the select keeps its bits out).  No LDS, no workspace.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pfa {

constexpr int ATTN_MERGE_THREADS = 256;
constexpr int ATTN_MERGE_MAX_PARTS = 8;      // PFA_MERGE_MAX_PARTS

struct AttnMergePart {                                // 64 bytes: one scalar load brings a part's whole description
    const void* o;
    const float* lse;
    int64_t o_sb, o_sh, o_ss;                         // element strides
    int64_t l_sb, l_sh, l_ss;
};

struct AttnMergeParams {
    AttnMergePart part[ATTN_MERGE_MAX_PARTS];
    void* o;
    float* lse_out;                                   // or null
    int64_t o_sb, o_sh, o_ss;
    int64_t lo_sb, lo_sh, lo_ss;
    int32_t items;                                    // B * Sq * H * dchunks; items + 256 fits 32 bits (checked by the host)
    int32_t H, Sq;
    int32_t dchunks;                                  // D / 8
};

typedef uint32_t attn_merge_b128 __attribute__((ext_vector_type(4)));
typedef float attn_merge_f4 __attribute__((ext_vector_type(4)));

// 8 consecutive elements at p (16-byte aligned) widened to fp32
template <typename T>
__device__ inline void attn_merge_load8(const T* p, float (&x)[8]) {
    if constexpr (sizeof(T) == 4) {
        const attn_merge_f4 a = *reinterpret_cast<const attn_merge_f4*>(p);
        const attn_merge_f4 b = *reinterpret_cast<const attn_merge_f4*>(p + 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) { x[j] = a[j]; x[4 + j] = b[j]; }
    } else {
        const attn_merge_b128 a = *reinterpret_cast<const attn_merge_b128*>(p);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            x[2 * j] = static_cast<float>(__builtin_bit_cast(T, (uint16_t)(a[j] & 0xffffu)));
            x[2 * j + 1] = static_cast<float>(__builtin_bit_cast(T, (uint16_t)(a[j] >> 16)));
        }
    }
}

// ... and back: fp32 as it is, 16-bit round-to-nearest-even
template <typename T>
__device__ inline void attn_merge_store8(T* p, const float (&x)[8]) {
    if constexpr (sizeof(T) == 4) {
        attn_merge_f4 a, b;
#pragma unroll
        for (int j = 0; j < 4; ++j) { a[j] = x[j]; b[j] = x[4 + j]; }
        *reinterpret_cast<attn_merge_f4*>(p) = a;
        *reinterpret_cast<attn_merge_f4*>(p + 4) = b;
    } else {
        attn_merge_b128 a;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            a[j] = (uint32_t)__builtin_bit_cast(uint16_t, static_cast<T>(x[2 * j])) |
                   ((uint32_t)__builtin_bit_cast(uint16_t, static_cast<T>(x[2 * j + 1])) << 16);
        *reinterpret_cast<attn_merge_b128*>(p) = a;
    }
}

template <typename TP, typename TO, int N>
__global__ __launch_bounds__(ATTN_MERGE_THREADS) void attn_merge_kernel(const AttnMergeParams p) {
    const int item = (int)blockIdx.x * ATTN_MERGE_THREADS + (int)threadIdx.x;
    if (item >= p.items) return;
    const int t = item / p.dchunks;
    const int c = item - t * p.dchunks;
    const int r = t / p.H;                               // row b * Sq + i
    const int h = t - r * p.H;
    const int b = r / p.Sq;
    const int i = r - b * p.Sq;

    float l[N], x[N][8];
#pragma unroll
    for (int n = 0; n < N; ++n) {
        const AttnMergePart& q = p.part[n];
        l[n] = q.lse[(int64_t)b * q.l_sb + (int64_t)h * q.l_sh + (int64_t)i * q.l_ss];
        attn_merge_load8((const TP*)q.o + ((int64_t)b * q.o_sb + (int64_t)h * q.o_sh + (int64_t)i * q.o_ss + c * 8), x[n]);
    }

    constexpr float NEG_INF = -__builtin_huge_valf();
    constexpr float LOG2E = 1.4426950408889634f, LN2 = 0.6931471805599453f;
    float m = NEG_INF;
    bool nan = false;
#pragma unroll
    for (int n = 0; n < N; ++n) {
        nan |= l[n] != l[n];
        m = l[n] > m ? l[n] : m;                         // a NaN never wins: it is reported through `nan`
    }
    float s = 0.f, acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int n = 0; n < N; ++n) {
        const bool live = l[n] > NEG_INF;                // false for -inf and for NaN
        const float w = __builtin_amdgcn_exp2f((l[n] - m) * LOG2E);
        s = live ? s + w : s;
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = live ? __builtin_fmaf(w, x[n][j], acc[j]) : acc[j];
    }
    float lse = m + __builtin_amdgcn_logf(s) * LN2;
    const bool none = !(m > NEG_INF);                    // no part with a visible key
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = none ? 0.f : acc[j] / s;
    if (none) lse = NEG_INF;
    if (nan) {
        lse = __builtin_nanf("");
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = lse;
    }
    attn_merge_store8((TO*)p.o + ((int64_t)b * p.o_sb + (int64_t)h * p.o_sh + (int64_t)i * p.o_ss + c * 8), acc);
    if (p.lse_out && c == 0) p.lse_out[(int64_t)b * p.lo_sb + (int64_t)h * p.lo_sh + (int64_t)i * p.lo_ss] = lse;
}

}  // namespace pfa

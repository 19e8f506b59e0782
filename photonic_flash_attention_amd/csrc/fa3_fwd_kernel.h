// fa3_fwd_kernel.h -- Flash-Attention forward for MI355X (gfx950 / CDNA4), hand-written HIP.
//
// Replaces the reference's eager two-level tile loop (core/flash_attention_3.py:182-262 and the
// dense branch :152-180) with ONE kernel: per 256-row Q block a workgroup of 8 waves walks the
// K/V sequence in 64-key tiles, S^T = K Q^T and O^T += V^T P^T on the bf16/f16 32x32x16 MFMA,
// online softmax in registers (flash_attention_3.py:239-250, but un-normalised until the end).
//
// Geometry (one workgroup = 512 threads = 8 waves, one per 32 Q rows; 1 workgroup per CU):
//   * "Swapped" products: the MFMA computes S^T (keys on the accumulator rows, the Q row on the lane),
//     so one lane holds 32 scores of ONE query row: row max / row sum are in-lane reductions plus one
//     v_permlane32_swap with the lane that holds the row's other 32 keys.
//   * The S^T accumulator registers, converted pairwise to bf16, ARE the B operand of the PV product
//     (k order permuted: element j of lane half h of k-step s is key 16s + 8(j>>2) + 4h + (j&3)); the
//     V^T A operand is fetched in that same key order with ds_read_b64_tr_b16 (hardware transpose
//     read), so P never touches LDS and V is staged row-major exactly as it lies in HBM.
//   * K/V tiles: HBM -> LDS by LDS-DMA (buffer_load ... lds, issued BEFORE the tile's math, into the other of two LDS
//     buffers) -> one barrier per tile.
//   * LDS image: 256-byte rows, 16-byte chunk index XOR-swizzled with ((R&3)<<2 | (R>>2)&3), which is
//     conflict-free for the ds_read_b128 row reads of K and for the transposed reads of V alike.
//
// HBM traffic per workgroup: Q block once, K/V of its (b,h) once (L2/MALL absorb re-reads by the
// other Q blocks of the head), O once.  Algorithmic bytes per forward: 2(Sq+Sk)*D*2 B per (b,h)*... see
// DESIGN.md.  The kernel is MFMA-bound at D=128 (1024 flop/B causal) -- roofline = bf16 dense MFMA peak.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "param_parts.h"

namespace pfa {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(4))) _Float16 f16x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;
typedef __attribute__((address_space(3))) char lds_char;

constexpr int WAVE_M = 32;    // Q rows per wave
constexpr int BLOCK_N = 64;   // keys per K/V tile

struct FwdParams {
    const void* q;
    const void* k;
    const void* v;
    void* o;
    float* lse;
    const int32_t* seqlens_k;
    const uint8_t* mask;       // optional u8 mask, 0 = masked, addressed [b][h][q][k] by the four byte strides below
    int64_t q_sb, q_sh, q_ss;
    int64_t k_sb, k_sh, k_ss;
    int64_t v_sb, v_sh, v_ss;
    int64_t o_sb, o_sh, o_ss;
    int64_t m_sb, m_sh, m_sq, m_sk;   // a 2-D [B,Sk] key mask is (stride, 0, 0, 1)
    int32_t B, H, Sq, Sk;
    int32_t nqblk;        // ceil(Sq / BLOCK_M)
    int32_t kv_group;     // query heads per K/V head (>= 1): query head h reads K/V head h / kv_group
    int32_t xcd_group;    // 4-wave kernel: walk the heads of an XCD in groups of this many (0 = all of them side by side)
    uint32_t magic_h, magic_g;   // 4-wave kernel: floor(2^32 / H) + 1 and floor(2^32 / kv_group) + 1 -- n / d == mulhi(n, magic) while n * d < 2^32
    float scale_log2;     // softmax_scale * log2(e)
    unsigned long long* dbg;   // diagnostic builds of the 4-wave kernel only (PFA_W4_STAMP): per-wave cycle sums; no shipped kernel touches it
    // mask condensed to 64-bit words by fa3_maskbits_kernel: bit i of word (b, h, q, j) = key 64 j + i is visible to row q of head h
    // of batch b; word address mbits + b*mb_sb + h*mb_sh + q*mb_sq + j (strides in words, 0 = broadcast: a [B,Sk] key mask has
    // mb_sh = mb_sq = 0).  null: the mask is read a byte per score.
    const unsigned long long* mbits;
    int64_t mb_sb, mb_sh, mb_sq;
    // ... and, per 256 mask rows, the first and last tile holding ANY visible key (fa3_maskrange_kernel): pairs (lo, hi) at
    // mrange + 2 * (b*mr_sb + h*mr_sh + (mr_q ? q / 256 : 0)).  A Q block runs only tiles lo .. hi: a structured mask (a band, a
    // triangle, padding) skips what it hides -- no fetch, no barrier -- instead of masking it.  null: every tile runs.
    const int* mrange = nullptr;
    int64_t mr_sb = 0, mr_sh = 0;
    int32_t mr_q = 0;
    // The packed ("varlen") mode of fa3_fwd_kernel (include/pfa_hip.h, pfa_fa3_varlen_args; no other kernel reads these): q / k / v / o
    // are [total, heads, D] with no batch stride (the *_sb members are unused), Sq / Sk hold max_seqlen_q / max_seqlen_k (they size the
    // grid), lse is [H, total_q], and a workgroup reads its sequence's rows and keys from the two cu_seqlens arrays.
    const int32_t* cu_q = nullptr;       // int32 [B + 1] on the device
    const int32_t* cu_k = nullptr;
    int32_t total_q = 0, total_k = 0;
};

// The packed mode of a kernel is selected by handing Packed<store type> where the dense instantiations hand the store type: a mode of
// the same kernel template that leaves the dense instantiations, their symbols included, as they are.
template <typename OT> struct Packed {};
template <typename OT> struct StoreMode {
    using type = OT;
    static constexpr bool packed = false;
};
template <typename OT> struct StoreMode<Packed<OT>> {
    using type = OT;
    static constexpr bool packed = true;
};

// One sequence of a packed tensor, read by a workgroup from cu[b], cu[b + 1] (b wave-uniform: scalar loads, SALU clamps):
// s = clamp(cu[b], 0, total), e = clamp(cu[b + 1], s, total), len = min(e - s, max_len) -- bad values give wrong numbers, never a row
// outside the packed tensor.
struct PackedSeq {
    int32_t start, len;
};
__device__ __forceinline__ PackedSeq packed_seq(const int32_t* __restrict__ cu, int b, int32_t total, int32_t max_len) {
    const int32_t s = min(max(cu[b], 0), total), e = min(max(cu[b + 1], s), total);
    return {s, min(e - s, max_len)};
}
// base + rows * stride elements, as 64-bit arithmetic on the pointer (never folded into a 32-bit buffer offset)
template <typename T>
__device__ __forceinline__ const void* rebase_rows(const void* base, int32_t rows, int64_t stride) {
    return (const void*)((const T*)base + (int64_t)rows * stride);
}

template <typename T> struct Elem;
template <> struct Elem<__bf16> {
    using v8 = bf16x8;
    using v4 = bf16x4;
    static __device__ __forceinline__ f32x16 mfma(v8 a, v8 b, f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ v4 tr_read(const lds_char* p) {
        return __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) v4*)p);
    }
};
template <> struct Elem<_Float16> {
    using v8 = f16x8;
    using v4 = f16x4;
    static __device__ __forceinline__ f32x16 mfma(v8 a, v8 b, f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ v4 tr_read(const lds_char* p) {
        typedef __attribute__((__vector_size__(4 * sizeof(__fp16)))) __fp16 h4;
        return __builtin_bit_cast(v4, __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) h4*)p));
    }
};

// Byte offset of 16-byte chunk `ch` of key row `key` inside one K or V tile image.
// D=128: one key per 256-B LDS row.  D=64: two keys per LDS row (odd key in the upper 128 B).
template <int D>
__device__ __forceinline__ uint32_t tile_off(uint32_t key, uint32_t ch) {
    uint32_t R, c;
    if constexpr (D == 128) {
        R = key;
        c = ch;
    } else {
        R = key >> 1;
        c = ((key & 1) << 3) | ch;
    }
    const uint32_t sw = ((R & 3) << 2) | ((R >> 2) & 3);
    return R * 256u + ((c ^ sw) << 4);
}

// Row maximum over one 16-register S block as ONE asm statement: hipcc puts an s_nop between consecutive
// single-instruction asm statements that depend on each other (15 per tile), and the VALU issue port -- not the
// MFMA pipe -- is what this kernel runs out of (MI355X_MICROARCH.md, 'vector-instruction ISSUE cost').
__device__ __forceinline__ float max16_first(const f32x16& a) {
    float r;
    asm("v_max3_f32 %0, %1, %2, %3\n\t"
        "v_max3_f32 %0, %0, %4, %5\n\t"
        "v_max3_f32 %0, %0, %6, %7\n\t"
        "v_max3_f32 %0, %0, %8, %9\n\t"
        "v_max3_f32 %0, %0, %10, %11\n\t"
        "v_max3_f32 %0, %0, %12, %13\n\t"
        "v_max3_f32 %0, %0, %14, %15\n\t"
        "v_max_f32 %0, %0, %16"
        : "=&v"(r)
        : "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "v"(a[4]), "v"(a[5]), "v"(a[6]), "v"(a[7]), "v"(a[8]), "v"(a[9]),
          "v"(a[10]), "v"(a[11]), "v"(a[12]), "v"(a[13]), "v"(a[14]), "v"(a[15]));
    return r;
}
__device__ __forceinline__ float max16_next(float r, const f32x16& a) {
    asm("v_max3_f32 %0, %0, %1, %2\n\t"
        "v_max3_f32 %0, %0, %3, %4\n\t"
        "v_max3_f32 %0, %0, %5, %6\n\t"
        "v_max3_f32 %0, %0, %7, %8\n\t"
        "v_max3_f32 %0, %0, %9, %10\n\t"
        "v_max3_f32 %0, %0, %11, %12\n\t"
        "v_max3_f32 %0, %0, %13, %14\n\t"
        "v_max3_f32 %0, %0, %15, %16"
        : "+&v"(r)
        : "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "v"(a[4]), "v"(a[5]), "v"(a[6]), "v"(a[7]), "v"(a[8]), "v"(a[9]),
          "v"(a[10]), "v"(a[11]), "v"(a[12]), "v"(a[13]), "v"(a[14]), "v"(a[15]));
    return r;
}

__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

// max(x[lane], x[lane ^ 32]) in every lane: the two lanes that share a query row.  Raw instructions: fmaxf() on a
// permlane result makes hipcc add a canonicalising v_max_f32 x,x (the scores are never sNaN).  s_nop 1: VALU write -> permlane read.
__device__ __forceinline__ float row_pair_max_asm(float x) {
    float t;
    asm("v_mov_b32 %1, %0\n\ts_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\tv_max_f32 %0, %0, %1" : "+v"(x), "=&v"(t));
    return x;
}
__device__ __forceinline__ float row_pair_sum(float x) {
    auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

template <int N> struct IC { static constexpr int value = N; };

// s_memtime stamp as ONE statement with its own lgkmcnt(0) (cdna guide section 7, in-kernel stamps)
__device__ __forceinline__ unsigned long long stamp() {
    unsigned long long t;
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    __builtin_amdgcn_sched_barrier(0);
    return t;
}
typedef __amdgpu_buffer_rsrc_t srd_t;

// Second half of the LDS-staged row store (every epilogue: forward O, backward dQ / dK / dV): read a [32 rows][RB bytes] image
// (16-byte chunk index XOR row) back so that one store instruction covers 64 / CPRW WHOLE rows.  All reads are issued before the
// first store: written as one loop, hipcc sinks each ds_read_b128 into its store's predicated block and the epilogue pays 8
// serial LDS round trips (ds_read, s_waitcnt lgkmcnt(0), store, next ...).  rows_valid is wave-uniform.
template <int RB>
__device__ __forceinline__ void store_rows_from_lds(uint32_t lbase, int lane, char* grow0, int64_t row_stride_bytes, int rows_valid) {
    typedef __attribute__((address_space(3))) u32x4 lds_u32x4_t;
    constexpr int CPRW = RB / 16, RPI = 64 / CPRW, NI = 32 / RPI;      // chunks per row, rows per store instruction, instructions
    const int cc = lane & (CPRW - 1), lr = lane / CPRW;
    u32x4 x[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int row = RPI * i + lr;
        x[i] = *(const lds_u32x4_t*)(uintptr_t)(lbase + row * RB + ((cc ^ (row & (CPRW - 1))) << 4));
    }
#pragma unroll
    for (int i = 0; i < NI; ++i) asm volatile("" : "+v"(x[i]));
    char* g = grow0 + 16 * cc + (int64_t)lr * row_stride_bytes;
    if (rows_valid >= 32) {
#pragma unroll
        for (int i = 0; i < NI; ++i) *(u32x4*)(g + (int64_t)(RPI * i) * row_stride_bytes) = x[i];
    } else {
#pragma unroll
        for (int i = 0; i < NI; ++i)
            if (RPI * i + lr < rows_valid) *(u32x4*)(g + (int64_t)(RPI * i) * row_stride_bytes) = x[i];
    }
}

// LDS-DMA piece through a buffer descriptor: lane address = SRD base + voff, out-of-range lanes (rows past the
// end of the K/V slab) deliver zeros, so ragged tails need no clamp.  s_nop 4: SGPR-written-by-SALU -> VMEM.
// Inline asm and not the builtin: hipcc treats the builtin DMA as a possibly-aliasing LDS store and puts
// s_waitcnt vmcnt(0) in front of the next ds_read of the OTHER buffer, exposing the whole HBM latency every
// tile.  Hidden in asm the DMA is invisible to the waitcnt pass; the kernels retire it themselves with an
// s_waitcnt vmcnt(N) in front of the barrier that publishes the tile (cdna guide section 5.7 item 1).
// M0 (LDS base of the DMA) is saved/restored inside the statement.
__device__ __forceinline__ void lds_dma16_buf(srd_t srd, uint32_t voff, uint32_t lds_dst) {
    uint32_t keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 4\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds\n\ts_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(voff), "s"(srd), "s"(lds_dst)
        : "memory");
}

// u8 mask (0 = masked; byte strides, 0 = broadcast) -> one 64-bit word per mask row and 64-key tile.  The forward then reads
// ONE word per row and tile: all ones = no masking work, all zero = the tile is skipped, anything else = bit tests -- where
// reading the mask itself cost 32 scattered byte loads per lane and tile (2-6 x the run time of the unmasked problem).
// One wave per word: grid (ceil(nt / 4), rows = Qm, Bm * Hm) with Bm / Hm / Qm = the mask's own (un-broadcast) extents.
template <int UNUSED = 0>   // (a template only so that the three translation units including this header do not each define it)
__global__ __launch_bounds__(256) void fa3_maskbits_kernel(const uint8_t* m, int64_t sb, int64_t sh, int64_t sq, int64_t sk, int Hm, int Sk,
                                                          int nt, unsigned long long* out, int64_t ob, int64_t oh, int64_t oq) {
    const int lane = threadIdx.x & 63, tile = blockIdx.x * 4 + (threadIdx.x >> 6), q = blockIdx.y;
    const int b = blockIdx.z / Hm, hh = blockIdx.z - b * Hm;
    if (tile >= nt) return;
    const int key = tile * 64 + lane;
    const bool on = key < Sk && m[(int64_t)b * sb + (int64_t)hh * sh + (int64_t)q * sq + (int64_t)key * sk] != 0;
    const unsigned long long bits = __builtin_amdgcn_ballot_w64(on);
    if (lane == 0) out[(int64_t)b * ob + (int64_t)hh * oh + (int64_t)q * oq + tile] = bits;
}

// The same for keys contiguous in memory (m_sk = 1, rows / bases / Sk multiples of 16 bytes): a lane reads 16 mask bytes at once, four
// lanes make a word, a wave 16 words of one row -- the byte-per-lane form above runs at 0.4 TB/s of mask, a 16 MB [S,S] mask cost
// 43 us in front of a 280 us forward.
template <int UNUSED = 0>
__global__ __launch_bounds__(256) void fa3_maskbits16_kernel(const uint8_t* m, int64_t sb, int64_t sh, int64_t sq, int Hm, int Sk, int nt,
                                                            unsigned long long* out, int64_t ob, int64_t oh, int64_t oq) {
    const int lane = threadIdx.x & 63, grp = blockIdx.x * 4 + (threadIdx.x >> 6), q = blockIdx.y;     // grp: 16 tiles = 1024 keys
    const int b = blockIdx.z / Hm, hh = blockIdx.z - b * Hm;
    if (grp * 16 >= nt) return;
    const int key0 = grp * 1024 + 16 * lane;
    uint32_t bits = 0;
    if (key0 < Sk) {
        const u32x4 x = *(const u32x4*)(m + (int64_t)b * sb + (int64_t)hh * sh + (int64_t)q * sq + key0);
#pragma unroll
        for (int w = 0; w < 4; ++w)
#pragma unroll
            for (int i = 0; i < 4; ++i) bits |= (((x[w] >> (8 * i)) & 0xFFu) != 0 ? 1u : 0u) << (4 * w + i);
    }
    unsigned long long word = (unsigned long long)bits << (16 * (lane & 3));
    word |= __shfl_xor(word, 1);
    word |= __shfl_xor(word, 2);
    const int tile = grp * 16 + (lane >> 2);
    if ((lane & 3) == 0 && tile < nt) out[(int64_t)b * ob + (int64_t)hh * oh + (int64_t)q * oq + tile] = word;
}

// Enqueue the kernel that condenses a u8 mask (Bm x Hm x Qm rows of Sk keys; byte strides sb / sh / sq / sk) into nt 64-bit words
// per row at `out` (word strides ob / oh / oq): 16 mask bytes per lane where keys are contiguous and every row is 16-byte aligned,
// else a byte per lane.  Host side, for the forward, the weights pass and the backward; a launch error is left for the caller's
// hipGetLastError().
template <int UNUSED = 0>   // (as for the kernels: one definition however many translation units include this)
void launch_mask_words(const uint8_t* m, int64_t sb, int64_t sh, int64_t sq, int64_t sk, int Bm, int Hm, int Qm, int Sk, int nt,
                       unsigned long long* out, int64_t ob, int64_t oh, int64_t oq, hipStream_t stream) {
    const bool wide = sk == 1 && Sk % 16 == 0 && sb % 16 == 0 && sh % 16 == 0 && sq % 16 == 0 && ((uintptr_t)m & 15) == 0;
    if (wide)
        hipLaunchKernelGGL(fa3_maskbits16_kernel<UNUSED>, dim3((unsigned)(((nt + 15) / 16 + 3) / 4), (unsigned)Qm, (unsigned)(Bm * Hm)), dim3(256), 0,
                           stream, m, sb, sh, sq, Hm, Sk, nt, out, ob, oh, oq);
    else
        hipLaunchKernelGGL(fa3_maskbits_kernel<UNUSED>, dim3((unsigned)((nt + 3) / 4), (unsigned)Qm, (unsigned)(Bm * Hm)), dim3(256), 0, stream,
                           m, sb, sh, sq, sk, Hm, Sk, nt, out, ob, oh, oq);
}

// first / last tile with a visible key per 256 mask rows (see FwdParams::mrange): RANGE_PARTS workgroups per granule and mask (batch, head),
// each leaves the pair of its share of the rows; the forward kernel takes the minimum / maximum of the parts
constexpr int RANGE_PARTS = 16;
template <int GRAN = 256>      // rows per granule: 256 (a Q block of the forward / dQ kernels) or 128 (a key block of the dK/dV kernel, on transposed words)
__global__ __launch_bounds__(256) void fa3_maskrange_kernel(const unsigned long long* words, int64_t ob, int64_t oh, int64_t oq, int Hm, int Qm,
                                                           int nt, int* out, int ngran) {
    const int g = blockIdx.x / RANGE_PARTS, part = blockIdx.x - g * RANGE_PARTS, b = blockIdx.y / Hm, hh = blockIdx.y - b * Hm;
    const int r0 = min(Qm, g * GRAN + part * (GRAN / RANGE_PARTS)), r1 = min(Qm, r0 + GRAN / RANGE_PARTS);
    const unsigned long long* w = words + (int64_t)b * ob + (int64_t)hh * oh;
    int lo = nt, hi = -1;
    for (int idx = threadIdx.x; idx < (r1 - r0) * nt; idx += 256) {
        const int row = r0 + idx / nt, t = idx - (idx / nt) * nt;
        if (w[(int64_t)row * oq + t] != 0ull) {
            lo = min(lo, t);
            hi = max(hi, t);
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        lo = min(lo, __shfl_xor(lo, off));
        hi = max(hi, __shfl_xor(hi, off));
    }
    __shared__ int slo[4], shi[4];
    if ((threadIdx.x & 63) == 0) {
        slo[threadIdx.x >> 6] = lo;
        shi[threadIdx.x >> 6] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int* o = out + 2 * ((((int64_t)b * Hm + hh) * ngran + g) * RANGE_PARTS + part);
        o[0] = min(min(slo[0], slo[1]), min(slo[2], slo[3]));
        o[1] = max(max(shi[0], shi[1]), max(shi[2], shi[3]));
    }
}

// The words transposed, for the key-stationary dK/dV kernel: bit i of word (b, h, key, tq) = row 64 tq + i sees `key`.  One wave per
// (64 rows, 64 keys): a lane holds its row's word of the key tile, 64 ballots turn the bit matrix over.  rows = the mask's own row
// extent (1: every row alike), Sq = the problem's.
template <int UNUSED = 0>
__global__ __launch_bounds__(256) void fa3_maskbitsT_kernel(const unsigned long long* roww, int64_t ob, int64_t oh, int64_t oq, int Hm, int rows,
                                                           int Sq, int Sk, int nt, int ntq, unsigned long long* colw) {
    const int lane = threadIdx.x & 63, kt = blockIdx.x * 4 + (threadIdx.x >> 6), tq = blockIdx.y;
    const int b = blockIdx.z / Hm, hh = blockIdx.z - b * Hm;
    if (kt >= nt) return;
    const int row = 64 * tq + lane;
    const unsigned long long w = row < Sq ? roww[(int64_t)b * ob + (int64_t)hh * oh + (int64_t)(rows > 1 ? row : 0) * oq + kt] : 0ull;
    unsigned long long kept = 0ull;
    for (int c = 0; c < 64; ++c) {
        const unsigned long long bal = __builtin_amdgcn_ballot_w64(((w >> c) & 1ull) != 0ull);
        if (lane == c) kept = bal;
    }
    const int key = 64 * kt + lane;
    if (key < Sk) colw[(((int64_t)b * Hm + hh) * Sk + key) * ntq + tq] = kept;
}

constexpr int FWD_WAVES = 8;                      // one wave per 32 Q rows
constexpr int FWD_THREADS = FWD_WAVES * 64;
constexpr int FWD_BLOCK_M = FWD_WAVES * WAVE_M;   // 256 Q rows per workgroup

// OTM: the store type (bf16 / fp16 / float): the dense kernel, `pin` used as it is.  Packed<store type>: the packed variable-length mode
// (pfa_fa3_varlen_fwd) -- grid B * H * ceil(max_seqlen_q / 256) from host shapes, lengths and offsets from pin.cu_q / cu_k on the device,
// workgroups past their sequence's rows return at once; the kernel then works on a copy of the block rebased to its sequence (pointers
// moved to the sequence's first row, Sq / Sk its own lengths), so every bound below, K/V descriptors and row guards alike, is the
// sequence's, and a workgroup computes what the dense kernel computes for that sequence alone, bit for bit.  Causal is the dense rule
// in both modes (row i sees key j iff j <= i, top-left aligned), not the caches' bottom-right rule; for packed self-attention (cu_k is
// cu_q) the two coincide.
//
// SINK (fa3_fwd_kernel's overload on FwdBlock<true>, below: pfa_fa3_fwd_sink / pfa_fa3_varlen_fwd_sink; FwdSinkPart carries the pointer): an
// attention sink, one fp32 value per QUERY head in the units of the scaled scores, is one more key with that score and a zero value row
// (fa3_prefill_kernel.h has the same mode and the same arithmetic).  The tile loop and everything in front of it are untouched; a workgroup
// serves one head, so the sink is one scalar load in the prologue.  The epilogue, with mc = m_run * c the deferred-max reference in log2
// units and s2 = sinks[hh] * log2(e):  M' = max(mc, s2),  l' = l_tot * exp2(mc - M') + exp2(s2 - M'),  inv = exp2(mc - M') / l'.
//   - a row with no visible key has l_tot = 0 and mc = -1e30 c: M' = s2, the first factor is 0, l' = 1 -- O = 0 exactly and LSE = sink;
//   - s2 = -inf: M' = mc, the factors are exactly 1 and 0, l' = l_tot and inv = (1 / l_tot) * 1 -- O and LSE keep the bits of the sink-less
//     kernel, -inf in the LSE of a row without keys included.  The LSE is m_run * c + log2 l' where the keys hold the maximum and
//     s2 + log2 l' where the sink does (the two-way select of fa3_prefill_kernel).
// SINK = false compiles to the code the kernel had.

// the sink's part of the argument block (param_parts.h): the dense and packed instantiations without the mode take FwdParams as they did
struct FwdSinkPart {
    const float* sinks;    // SINK: one fp32 sink per query head, sinks[h], in the units of the scaled scores (natural log)
};
template <bool SINK>
struct FwdBlock : FwdParams, PartIf<SINK, FwdSinkPart> {};

template <typename T, int D, bool CAUSAL, bool SPLITP, bool KMASK, typename OTM>
__global__ __launch_bounds__(FWD_THREADS, 2) void fa3_fwd_kernel(const FwdParams pin) {
    constexpr bool SINK = false;
    const float* const sinks = nullptr;
#include "fa3_fwd_body.inc"
}
// ... and with the sink: the same name and the same body on the block that carries the pointer, so that the instantiations above keep their
// symbols and their code
template <typename T, int D, bool CAUSAL, bool SPLITP, bool KMASK, typename OTM>
__global__ __launch_bounds__(FWD_THREADS, 2) void fa3_fwd_kernel(const FwdBlock<true> pin) {
    constexpr bool SINK = true;
    const float* const sinks = pin.sinks;
#include "fa3_fwd_body.inc"
}

}  // namespace pfa

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
template <typename T, int D, bool CAUSAL, bool SPLITP, bool KMASK, typename OTM>
__global__ __launch_bounds__(FWD_THREADS, 2) void fa3_fwd_kernel(const FwdParams pin) {
    constexpr bool VARLEN = StoreMode<OTM>::packed;
    using OT = typename StoreMode<OTM>::type;
    static_assert(!VARLEN || !KMASK, "the packed forward takes no masks");
    constexpr int NW = FWD_WAVES, BLOCK_M = FWD_BLOCK_M;
    using E = Elem<T>;
    using v8 = typename E::v8;
    using v4 = typename E::v4;
    typedef __attribute__((address_space(3))) v8 lds_v8;
    constexpr int KS = D / 16;                // k-steps of the QK^T product
    constexpr int DB = D / 32;                // 32-wide d blocks of the PV product
    constexpr int TILE_BYTES = BLOCK_N * D * 2;
    constexpr int BUF_BYTES = 2 * TILE_BYTES; // K image + V image
    constexpr int HALF_TILE = TILE_BYTES / 2; // 32 keys

    extern __shared__ __attribute__((aligned(16))) char smem[];
    lds_char* const smem_l = (lds_char*)smem;   // [buf][K|V][TILE_BYTES]
    const uint32_t smem_base = (uint32_t)(uintptr_t)smem_l;   // LDS byte address (wave-uniform)

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31;
    const int h = lane >> 5;

    // ---- block -> (q block, batch*head): heaviest (longest causal row) blocks first ----------------
    const int BH = pin.B * pin.H;
    const int n = blockIdx.x;
    const int qrank = n / BH;
    const int bh = n - qrank * BH;
    const int qblk = CAUSAL ? (pin.nqblk - 1 - qrank) : qrank;
    const int b = bh / pin.H;
    const int hh = bh - b * pin.H;

    const int q0 = qblk * BLOCK_M;
    FwdParams pv;                            // VARLEN: the block of this workgroup's sequence
    int64_t lse_row0 = 0;                    // VARLEN: LSE entry of the sequence's row 0 in head hh of the [H, total_q] array
    if constexpr (VARLEN) {
        const PackedSeq sq = packed_seq(pin.cu_q, b, pin.total_q, pin.Sq), sk = packed_seq(pin.cu_k, b, pin.total_k, pin.Sk);
        if (q0 >= sq.len) return;            // no rows of the sequence in this block (wave-uniform, ahead of every barrier)
        pv = pin;
        pv.Sq = sq.len; pv.Sk = sk.len;
        pv.q = rebase_rows<T>(pin.q, sq.start, pin.q_ss); pv.o = (void*)rebase_rows<OT>(pin.o, sq.start, pin.o_ss);
        pv.k = rebase_rows<T>(pin.k, sk.start, pin.k_ss); pv.v = rebase_rows<T>(pin.v, sk.start, pin.v_ss);
        pv.q_sb = pv.k_sb = pv.v_sb = pv.o_sb = 0;
        lse_row0 = (int64_t)hh * pin.total_q + sq.start;
    }
    const FwdParams& p = VARLEN ? (const FwdParams&)pv : (const FwdParams&)pin;
    const int wave_q0 = q0 + wave * WAVE_M;
    const int my_q = wave_q0 + r;

    int kv_len = p.Sk;
    if (p.seqlens_k) kv_len = min(kv_len, max(p.seqlens_k[b], 0));
    const int kv_end = CAUSAL ? min(kv_len, q0 + BLOCK_M) : kv_len;          // keys the block needs
    const int wave_kv_end = CAUSAL ? min(kv_len, wave_q0 + WAVE_M) : kv_len; // keys this wave needs
    int nt = (kv_end + BLOCK_N - 1) / BLOCK_N;
    int j0 = 0;                              // first tile of the block (0 unless the mask's tile range says otherwise)
    if constexpr (KMASK) {
        if (p.mrange) {
            const int* rg = p.mrange + 2 * RANGE_PARTS * ((int64_t)b * p.mr_sb + (int64_t)hh * p.mr_sh + (p.mr_q ? (q0 >> 8) : 0));
            int lo = rg[2 * (lane & (RANGE_PARTS - 1))], hi = rg[2 * (lane & (RANGE_PARTS - 1)) + 1];
#pragma unroll
            for (int off = RANGE_PARTS / 2; off >= 1; off >>= 1) {
                lo = min(lo, __shfl_xor(lo, off));
                hi = max(hi, __shfl_xor(hi, off));
            }
            lo = __builtin_amdgcn_readfirstlane(lo);
            hi = __builtin_amdgcn_readfirstlane(hi);
            nt = min(nt, hi + 1);                                    // nothing visible past tile hi (hi = -1: nothing at all -> zeros, LSE -inf)
            j0 = min(lo, max(nt, 0)) & ~1;                           // (even: the two LDS buffers keep their parity)
            nt = max(nt, 0);
        }
    }

    const T* __restrict__ qp = (const T*)p.q + (int64_t)b * p.q_sb + (int64_t)hh * p.q_sh;
    const T* __restrict__ kp = (const T*)p.k + (int64_t)b * p.k_sb + (int64_t)(hh / p.kv_group) * p.k_sh;
    const T* __restrict__ vp = (const T*)p.v + (int64_t)b * p.v_sb + (int64_t)(hh / p.kv_group) * p.v_sh;
    const uint8_t* __restrict__ kmp =
        KMASK ? p.mask + (int64_t)b * p.m_sb + (int64_t)hh * p.m_sh + (int64_t)min(my_q, p.Sq - 1) * p.m_sq : nullptr;

    // ---- Q fragments: B operand of S^T = K Q^T, lane (r,h) holds Q[my_q][16 ks + 8 h .. +7] -----------
    v8 qf[KS];
    {
        const int qrow = min(my_q, p.Sq - 1);
        const T* src = qp + (int64_t)qrow * p.q_ss + 8 * h;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) qf[ks] = *(const v8*)(src + 16 * ks);
    }

    // ---- K/V staging by LDS-DMA: one wave-instruction moves 64 x 16 B = 1 KiB into LINEAR LDS, so the
    // XOR swizzle is applied to the per-lane SOURCE chunk (guide rule 21).  Wave w issues pieces w, w+8, ...
    // piece i covers LDS rows 4i..4i+3 (256 B each); lane l -> row 4i + (l>>4), stored chunk l&15.
    constexpr int PIECES = TILE_BYTES / 1024;            // 16 (D=128) or 8 (D=64)
    constexpr int PPW = PIECES / NW;                     // pieces per wave
    int dma_key[PPW];
    int dma_col;                                         // element offset of the source chunk in its key row
    {
        const int R0 = 4 * (wave % NW) + (lane >> 4);    // LDS row of piece `wave` (% NW: a no-op the shipped code carries)
        const int sw = ((R0 & 3) << 2) | ((R0 >> 2) & 3);   // rows 4*NW apart share the swizzle term
        const int cc = (lane & 15) ^ sw;                 // logical chunk stored at this lane's position
        if constexpr (D == 128) {
            dma_col = cc * 8;
#pragma unroll
            for (int t = 0; t < PPW; ++t) dma_key[t] = R0 + 4 * NW * t;
        } else {
            dma_col = (cc & 7) * 8;
#pragma unroll
            for (int t = 0; t < PPW; ++t) dma_key[t] = 2 * (R0 + 4 * NW * t) + (cc >> 3);
        }
    }
    // through a buffer descriptor: per-lane byte offsets are loop invariant, the tile steps the SRD base (SALU only, no per-tile VALU)
    uint32_t kvoff[PPW], vvoff[PPW];
#pragma unroll
    for (int t = 0; t < PPW; ++t) {
        kvoff[t] = (uint32_t)(dma_key[t] * (int)p.k_ss + dma_col) * 2u;
        vvoff[t] = (uint32_t)(dma_key[t] * (int)p.v_ss + dma_col) * 2u;
    }
    const int64_t k_slab = ((int64_t)(p.Sk - 1) * p.k_ss + D) * 2;   // bytes of this (b,h) K slab
    const int64_t v_slab = ((int64_t)(p.Sk - 1) * p.v_ss + D) * 2;
    auto dma_tile = [&](auto bufc, int j) {
        constexpr int BUF = decltype(bufc)::value;
        const int64_t kstep = (int64_t)j * BLOCK_N * p.k_ss * 2, vstep = (int64_t)j * BLOCK_N * p.v_ss * 2;
        const srd_t ksrd = __builtin_amdgcn_make_buffer_rsrc(
            (void*)((const char*)kp + kstep), 0, (int)max((int64_t)0, k_slab - kstep), 0x00020000);
        const srd_t vsrd = __builtin_amdgcn_make_buffer_rsrc(
            (void*)((const char*)vp + vstep), 0, (int)max((int64_t)0, v_slab - vstep), 0x00020000);
#pragma unroll
        for (int t = 0; t < PPW; ++t) {
            const uint32_t kd = smem_base + BUF * BUF_BYTES + (wave % NW + NW * t) * 1024;
            lds_dma16_buf(ksrd, kvoff[t], kd);
            lds_dma16_buf(vsrd, vvoff[t], kd + TILE_BYTES);
        }
    };

    // ---- per-lane LDS read offsets, loop invariant; (buffer, key block, k-step) become immediates ----------
    // K row read (kb, ks): key = 32 kb + r, chunk 2 ks + h.   +32 keys leaves the swizzle term unchanged.
    // The addresses are made opaque to the optimiser (empty asm): otherwise it keeps row and chunk parts apart and
    // re-adds them every tile (25 v_add_u32) -- the VALU issue port, not the MFMA pipe, is what this kernel runs out of.
    uint32_t koff[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) koff[ks] = smem_base + tile_off<D>(r, 2 * ks + h);   // absolute LDS address
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) asm volatile("" : "+v"(koff[ks]));
    // V transposed read (kb, s2, db, hi8): lane 4q+p of a 16-lane group supplies row q, columns 4p..4p+3 of the
    // 4-key x 16-d block at key0 = 32 kb + 16 s2 + 4 h (+8), d0 = 32 db + 16 ((lane>>4)&1)
    const int g1 = (lane >> 4) & 1;
    const int tq = (lane & 15) >> 2;
    const int tp = lane & 3;
    constexpr int NS2 = (D == 128) ? 1 : 2;   // D=64: two keys per LDS row, the swizzle term depends on s2
    uint32_t voff[NS2][DB][2];
#pragma unroll
    for (int s2 = 0; s2 < NS2; ++s2)
#pragma unroll
        for (int db = 0; db < DB; ++db)
#pragma unroll
            for (int hi = 0; hi < 2; ++hi)
            {
                voff[s2][db][hi] = smem_base + tile_off<D>(16 * s2 + 4 * h + tq + 8 * hi, db * 4 + 2 * g1 + (tp >> 1)) + 8 * (tp & 1);
                asm volatile("" : "+v"(voff[s2][db][hi]));
            }

    f32x16 o[DB];
#pragma unroll
    for (int i = 0; i < DB; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) o[i][e] = 0.f;
    float m_run = -1e30f;   // reference max of the exponentials, raw score units
    float l_run = 0.f;      // this lane's share of the row sum
    const float c = p.scale_log2;
    const float thr = 8.0f / c;                 // deferred max: raw-score headroom (2^8 in the exponent) before O is rescaled
    float m_thr = -1e30f, mc = -1e30f * c;      // m_run + thr and m_run * c, updated with m_run

    // ---- one K/V tile: S^T = K Q^T, online softmax, O^T += V^T P^T -------------------------------------------
    // KMASK + mbits: the row's mask word of the current tile, fetched one tile ahead (consumed after the previous step's
    // s_waitcnt vmcnt(0), so the wait hipcc puts in front of its use never holds up the K/V prefetch issued behind it)
    unsigned long long tile_bits = ~0ull, next_bits = ~0ull;
    bool tile_all_ones = true;
    const unsigned long long* mrow = nullptr;
    if constexpr (KMASK) {
        if (p.mbits) mrow = p.mbits + (int64_t)b * p.mb_sb + (int64_t)hh * p.mb_sh + (int64_t)min(my_q, p.Sq - 1) * p.mb_sq;
    }
    auto fetch_bits = [&](int j) {
        if constexpr (KMASK) {
            if (mrow) next_bits = mrow[min(j, (p.Sk + BLOCK_N - 1) / BLOCK_N - 1)];
        }
    };
    auto tile_live = [&](int j) {              // does this wave compute tile j?  (wave-uniform)
        if (!(j * BLOCK_N < wave_kv_end)) return false;
        if constexpr (KMASK) {
            if (mrow) {
                tile_bits = next_bits;
                fetch_bits(j + 1);
                tile_all_ones = __builtin_amdgcn_ballot_w64(tile_bits != ~0ull) == 0;
                return __builtin_amdgcn_ballot_w64(tile_bits != 0ull) != 0;   // no key of the tile is visible to any row: skip it
            }
        }
        return true;
    };
    auto compute_tile = [&](auto bufc, int key_base) {
        constexpr int BUF = decltype(bufc)::value;
        const lds_char* kimg = (const lds_char*)(uintptr_t)(BUF * BUF_BYTES);   // koff[]/voff[] carry the LDS base
        const lds_char* vimg = kimg + TILE_BYTES;

        // S^T = K Q^T: 16 MFMAs (2 key blocks x KS k-steps), A fragments prefetched PF deep from LDS so the
        // ds_read latency hides behind the MFMAs already issued (hipcc otherwise emits read -> wait -> mfma)
        f32x16 s[2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int e = 0; e < 16; ++e) s[kb][e] = 0.f;
        constexpr int NQK = 2 * KS, PF = 4;
        v8 afr[PF];
        // step i -> key block i / KS, k-step i % KS
#pragma unroll
        for (int i = 0; i < PF; ++i) afr[i] = *(const lds_v8*)(kimg + koff[i % KS] + (i / KS) * HALF_TILE);
#pragma unroll
        for (int i = 0; i < NQK; ++i) {
            s[i / KS] = E::mfma(afr[i % PF], qf[i % KS], s[i / KS]);
            if (i + PF < NQK) afr[i % PF] = *(const lds_v8*)(kimg + koff[(i + PF) % KS] + ((i + PF) / KS) * HALF_TILE);
        }
        // pin the read / MFMA interleave: PF reads, then one MFMA per read, then the last PF MFMAs
        __builtin_amdgcn_sched_group_barrier(0x100, PF, 0);
#pragma unroll
        for (int i = 0; i < NQK - PF; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        }
        __builtin_amdgcn_sched_group_barrier(0x008, PF, 0);

        // mask: wave-uniform test, only diagonal / tail / key-mask tiles pay
        const bool bits_mode = KMASK && mrow != nullptr;                         // mask as one word per row and tile (tile_bits)
        const bool need_mask = (key_base + BLOCK_N > kv_len) || (CAUSAL && key_base + BLOCK_N - 1 > wave_q0) ||
                               (KMASK && (!bits_mode || !tile_all_ones));
        if (need_mask) {
            asm volatile("" ::: "memory");   // keep this a real (wave-uniform) branch: hipcc otherwise if-converts
                                             // it into 32 v_cmp + 32 v_cndmask on EVERY tile
            // the lane's 32 mask bits of each key block: keys 32 kb + 4 h + {0..3, 8..11, 16..19, 24..27}
            const uint32_t mw[2] = {(uint32_t)(tile_bits >> (4 * h)), (uint32_t)(tile_bits >> (32 + 4 * h))};
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int key = key_base + 32 * kb + (e & 3) + 8 * (e >> 2) + 4 * h;
                    bool ok = key < kv_len;
                    if (CAUSAL) ok = ok && (key <= my_q);
                    if (KMASK) {
                        if (bits_mode) ok = ok && (((mw[kb] >> ((e & 3) + 8 * (e >> 2))) & 1u) != 0);
                        else ok = ok && (kmp[(int64_t)min(key, p.Sk - 1) * p.m_sk] != 0);
                    }
                    s[kb][e] = ok ? s[kb][e] : -INFINITY;
                }
        }

        // online softmax (flash_attention_3.py:239-246); a row lives in lanes (l, l^32)
        float mx = max16_first(s[0]);
        mx = max16_next(mx, s[1]);
        mx = row_pair_max_asm(mx);
        // rescale O only when some row's max outgrew the headroom: until then the exponentials may reach 2^8,
        // harmless in fp32/bf16 and cancelled by l
        if (__builtin_amdgcn_ballot_w64(mx > m_thr) != 0) {
            const float m_new = fmaxf(m_run, mx);
            const float alpha = fast_exp2((m_run - m_new) * c);
            m_run = m_new;
            m_thr = m_new + thr;
            mc = m_new * c;
            l_run *= alpha;
#pragma unroll
            for (int i = 0; i < DB; ++i)
#pragma unroll
                for (int e = 0; e < 16; ++e) o[i][e] *= alpha;
        }
        float psum0 = 0.f, psum1 = 0.f;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            s[0][e] = fast_exp2(__builtin_fmaf(s[0][e], c, -mc));
            s[1][e] = fast_exp2(__builtin_fmaf(s[1][e], c, -mc));
            psum0 += s[0][e];
            asm volatile("" : "+v"(psum0));   // keeps SLP from pairing the sums into v_pk_add_f32
            psum1 += s[1][e];
        }
        l_run += psum0 + psum1;

        // O^T += V^T P^T
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                v8 ph, pl;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float pv = s[kb][8 * s2 + e];
                    const T hi = (T)pv;
                    ph[e] = hi;
                    if (SPLITP) pl[e] = (T)(pv - (float)hi);
                }
                constexpr int S2I = (D == 128) ? 0 : 1;
                const int koffs = kb * HALF_TILE + ((D == 128) ? s2 * 16 * 256 : 0);
#pragma unroll
                for (int db = 0; db < DB; ++db) {
                    const v4 lo = E::tr_read(vimg + voff[s2 * S2I][db][0] + koffs);
                    const v4 hi4 = E::tr_read(vimg + voff[s2 * S2I][db][1] + koffs);
                    v8 a;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        a[e] = lo[e];
                        a[4 + e] = hi4[e];
                    }
                    o[db] = E::mfma(a, ph, o[db]);
                    if (SPLITP) o[db] = E::mfma(a, pl, o[db]);
                }
            }
    };

    auto step = [&](auto bufc, int j) {
        constexpr int BUF = decltype(bufc)::value;
        const bool live = tile_live(j);
        if (j + 1 < nt) dma_tile(IC<BUF ^ 1>{}, j + 1);   // lands in the other buffer under this tile's math
        if (live) compute_tile(bufc, j * BLOCK_N);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's DMA pieces have landed ...
        __builtin_amdgcn_s_waitcnt(0xC07F);               // (lgkmcnt(0): this wave's LDS reads are done)
        __builtin_amdgcn_s_barrier();                     // ... and so have everybody else's
    };

    fetch_bits(j0);
    if (nt > j0) dma_tile(IC<0>{}, j0);
    // Q must have LANDED before the loop: hipcc's waitcnt pass otherwise keeps vmcnt(7..0) waits for the Q
    // loads inside the loop body, where they drain the K/V prefetch of the next tile on every iteration.
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) asm volatile("" : "+v"(qf[ks]));
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int j = j0; j < nt; j += 2) {
        step(IC<0>{}, j);
        if (j + 1 < nt) step(IC<1>{}, j + 1);
    }

    // ---- epilogue: normalise (flash_attention_3.py:250 does it per tile; once is equivalent) ------------
    const float l_tot = row_pair_sum(l_run);
    const float inv = l_tot > 0.f ? 1.0f / l_tot : 0.f;   // fully masked row -> zeros (documented divergence)
    if constexpr (sizeof(OT) == 2) {
        // 16-bit store: lanes l and l+32 hold the two 8-byte halves of every 16-byte column group of one row.  One
        // v_permlane32_swap per dword pairs group k (even) with k+1 so that each lane owns 16 contiguous bytes:
        // 8 dwordx4 stores per lane instead of 16 dwordx2 -- the tail is store-issue bound (cdna guide T21).
        // The 16-byte chunks then go through LDS (free after the loop's last barrier; 32 rows x D*2 bytes per wave, chunk
        // index XOR-swizzled by the row) and come back so that one store instruction covers WHOLE rows: per-lane stores
        // at the row stride touch 64 cache lines per instruction, these 8 (D = 128) or 16 (D = 64).
        typedef __attribute__((address_space(3))) u32x4 lds_u32x4_t;
        constexpr int RB = D * 2, CPRW = RB / 16;      // row bytes, 16-byte chunks per row
        const uint32_t lbase = smem_base + wave * (32 * RB);
#pragma unroll
        for (int db = 0; db < DB; ++db)
#pragma unroll
            for (int g = 0; g < 4; g += 2) {
                v4 wa, wb;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    wa[e] = (T)(o[db][4 * g + e] * inv);
                    wb[e] = (T)(o[db][4 * g + 4 + e] * inv);
                }
                u32x2 a = __builtin_bit_cast(u32x2, wa), bq = __builtin_bit_cast(u32x2, wb);
                auto r0 = __builtin_amdgcn_permlane32_swap(a[0], bq[0], false, false);
                auto r1 = __builtin_amdgcn_permlane32_swap(a[1], bq[1], false, false);
                u32x4 w = {r0[0], r1[0], r0[1], r1[1]};
                const uint32_t ch = 4 * db + g + h;
                *(lds_u32x4_t*)(uintptr_t)(lbase + r * RB + ((ch ^ (r & (CPRW - 1))) << 4)) = w;
            }
        store_rows_from_lds<RB>(lbase, lane, (char*)((OT*)p.o + (int64_t)b * p.o_sb + (int64_t)hh * p.o_sh + (int64_t)wave_q0 * p.o_ss),
                                p.o_ss * 2, p.Sq - wave_q0);
    } else if (my_q < p.Sq) {      // fp32 rows straight from the accumulators
        OT* orow = (OT*)p.o + (int64_t)b * p.o_sb + (int64_t)hh * p.o_sh + (int64_t)my_q * p.o_ss;
#pragma unroll
        for (int db = 0; db < DB; ++db)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int d = db * 32 + 8 * g + 4 * h;
                f32x4 w;
#pragma unroll
                for (int e = 0; e < 4; ++e) w[e] = o[db][4 * g + e] * inv;
                *(f32x4*)(orow + d) = w;
            }
    }
    if (my_q < p.Sq) {
        if (p.lse && h == 0) {
            const float lse = l_tot > 0.f ? (m_run * c + __builtin_amdgcn_logf(l_tot)) * 0.6931471805599453f : -INFINITY;
            if constexpr (VARLEN) p.lse[lse_row0 + my_q] = lse;
            else p.lse[((int64_t)b * p.H + hh) * p.Sq + my_q] = lse;
        }
    }
}

}  // namespace pfa

// decode_parts.h -- what the split-KV decode kernels share on the device (internal): the vector types, the argument block, the split rule,
// the descriptor helper and the page lookup of all three (fa3_decode_kernel.h, fa3_decode_d256_kernel.h, fa3_mla_decode_kernel.h), and of
// the two kernels of the 16-key wave tile the x16 MFMA, the image's row padding and the per-tile offset.  The tile's math and the waves'
// merge are textual bodies beside this file, decode_tile16.inc and decode_merge.inc: written as functions they change the kernels'
// register assignment (tools/isa_same.py: renamed), as files every kernel keeps its machine code.  What differs between the kernels (row
// packing over G or H, window, key mask, the loads and the register sets, the block order, the form of the merge's stores) stays in the
// kernel files.
//
// The 16-key tile.  S^T = K Q^T is one 16x16 block: lane (c, h) = (lane & 15, lane >> 4) holds query row c, and element e of its S^T
// accumulator is key 4 h + e of the tile -- the x16 MFMA's B-operand order, so P goes into O^T += V^T P^T as converted, with no key
// permutation.  The A operand of that product is one ds_read_b64_tr_b16 per 16-column block from the wave's row-major LDS image of the
// tile's value rows; a row of the image is the row's bytes + 32 (image_row: the padding keeps the transposed reads conflict-free).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pfa {
namespace dec {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(4))) _Float16 f16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(4))) short i16x4;
typedef __amdgpu_buffer_rsrc_t srd_t;
typedef __attribute__((address_space(3))) char lds_char;
typedef const __attribute__((address_space(4))) int32_t* const_i32_ptr;   // read-only for the kernel's lifetime: scalar loads
typedef const __attribute__((address_space(4))) float* const_f32_ptr;

constexpr int NW = 4;            // waves per workgroup
constexpr int ROWS = 16;         // query rows per row block (the MFMA's 16-wide dimension)
constexpr int SPLIT_ALIGN = 64;  // split boundaries are multiples of this many keys
constexpr int THREADS = NW * 64;

struct DecodeParams {
    const void* q;
    const void* k;
    const void* v;
    void* o;
    float* lse;                  // optional [B, H, Sq]
    const int32_t* seqlens;      // optional [B]
    const uint8_t* key_mask;     // optional [B, Smax] bytes, 0 = masked
    int64_t q_sb, q_sh, q_ss;    // element strides
    int64_t k_sb, k_sh, k_ss;
    int64_t v_sb, v_sh, v_ss;
    int64_t o_sb, o_sh, o_ss;
    int64_t km_sb;
    float* part_o;               // nsplit > 1: [nsplit][B][H][Sq][D] fp32, un-normalised
    float* part_ml;              // nsplit > 1: [nsplit][B][H][Sq][2] fp32 (running max in log2 units, row sum)
    int32_t B, H, Hkv, G, Sq, Smax, nrb, nsplit;
    int32_t causal;              // bottom-right: row i sees key j iff j <= len_b - Sq + i
    float scale_log2;            // softmax_scale * log2(e)
    // PAGED only: k / v are the pools, k_sb / v_sb the page strides, Smax = max_pages * page_size the logical capacity
    const int32_t* block_table;  // [B][max_pages] page ids
    int64_t bt_sb;               // entries between batches
    int32_t page_size, num_pages;
};

template <typename T> struct DElem;
template <> struct DElem<__bf16> {
    using v8 = bf16x8;
    using v4 = bf16x4;
    static __device__ __forceinline__ f32x4 mfma(v8 a, v8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ v4 tr_read(const lds_char* p) {
        return __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) v4*)p);
    }
};
template <> struct DElem<_Float16> {
    using v8 = f16x8;
    using v4 = f16x4;
    static __device__ __forceinline__ f32x4 mfma(v8 a, v8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ v4 tr_read(const lds_char* p) {
        typedef __attribute__((__vector_size__(4 * sizeof(__fp16)))) __fp16 h4;
        return __builtin_bit_cast(v4, __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) h4*)p));
    }
};

// the x16 MFMA of the 16-key tile's PV product: A = V^T (4 keys of one column per lane), B = P^T (4 keys of one row per lane)
template <typename T> struct DElem16;
template <> struct DElem16<__bf16> {
    static __device__ __forceinline__ f32x4 mfma(bf16x4 a, bf16x4 b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(i16x4, a), __builtin_bit_cast(i16x4, b), c, 0, 0, 0);
    }
};
template <> struct DElem16<_Float16> {
    static __device__ __forceinline__ f32x4 mfma(f16x4 a, f16x4 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x16f16(a, b, c, 0, 0, 0); }
};

// raw-buffer descriptor whose inputs are provably wave-uniform.  A tile's descriptor is given the record count that ends at the split's
// last key, so rows past it read as zeros
__device__ __forceinline__ srd_t uniform_srd(const char* base, uint32_t bytes) {
    const uint64_t a = (uint64_t)(uintptr_t)base;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a), hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
    return __builtin_amdgcn_make_buffer_rsrc((void*)(uintptr_t)(((uint64_t)hi << 32) | lo), 0, (int)__builtin_amdgcn_readfirstlane(bytes),
                                             0x00020000);
}

template <typename OT> __device__ __forceinline__ void store4(OT* p, f32x4 x);
template <> __device__ __forceinline__ void store4<float>(float* p, f32x4 x) { *(f32x4*)p = x; }
template <> __device__ __forceinline__ void store4<__bf16>(__bf16* p, f32x4 x) { *(bf16x4*)p = bf16x4{(__bf16)x[0], (__bf16)x[1], (__bf16)x[2], (__bf16)x[3]}; }
template <> __device__ __forceinline__ void store4<_Float16>(_Float16* p, f32x4 x) {
    *(f16x4*)p = f16x4{(_Float16)x[0], (_Float16)x[1], (_Float16)x[2], (_Float16)x[3]};
}

// The split of batch b this item covers: [lo, hi) (empty when lo >= hi).  len is the batch's valid key count.  The splits divide
// [base, len): base = 0, or under a window the 64-key boundary at or below the lowest key row 0 of the batch sees.
__device__ __forceinline__ void split_range(const DecodeParams& p, int s, int base, int len, int& lo, int& hi) {
    const int per = (len - base + p.nsplit - 1) / p.nsplit;
    const int c = (per + SPLIT_ALIGN - 1) / SPLIT_ALIGN * SPLIT_ALIGN;
    lo = min(base + s * c, len);
    hi = min(lo + c, len);
}

// ---- the parts of the 16-key tile ----------------------------------------------------------------------------------------------------

constexpr int KT16 = 16;                                          // keys per wave tile
static_assert(SPLIT_ALIGN % KT16 == 0, "a tile must not straddle a split boundary or a page");
constexpr int image_row(int cols) { return cols * 2 + 32; }       // LDS bytes per key row of the image
// paged: the (unclamped) page id of the tile at key t0, a wave-uniform scalar load.  Called only for tiles below hi <= len_b, so table
// entries at and past ceil(len_b / page_size) are never read.  The kernels fetch it one issue ahead, right behind the loads of the tile
// before, so that no dependent load stands in front of a tile's loads.
__device__ __forceinline__ int page_id(const_i32_ptr table, int t0, int page_size) { return table[(uint32_t)t0 / (uint32_t)page_size]; }

// element offset of the tile's first key row from the slab (sb: batch or page stride, ss: token stride).  Paged: the tile lies inside one
// page (page_size % 64 == 0, lo % 64 == 0, 64 % KT16 == 0); pg is device data and is clamped: never an address outside the pool
template <bool PAGED>
__device__ __forceinline__ int64_t tile_offset(const DecodeParams& p, int t0, int pg, int64_t sb, int64_t ss) {
    if constexpr (PAGED) {
        pg = min(max(pg, 0), p.num_pages - 1);
        const int tok = (int)((uint32_t)t0 % (uint32_t)p.page_size);
        return (int64_t)pg * sb + (int64_t)tok * ss;
    } else {
        return (int64_t)t0 * ss;
    }
}

}  // namespace dec
}  // namespace pfa

// fa3_decode_kernel.h -- split-KV decode attention over a KV cache for MI355X (gfx950), hand-written HIP.
//
// A decode step reads the whole cache once and does little arithmetic per byte, so the kernel is built around the HBM stream:
//   * One work item = (batch, K/V head, row block, key split).  Its rows are the Sq x (H / Hkv) query rows that share the K/V
//     head, packed 16 to a row block (row r = i * G + g: query position i, head g of the group), so each K/V byte is fetched
//     once per group instead of once per query head.
//   * Split over keys: the host picks nsplit from shapes alone; split s of batch b covers [s c_b, min((s+1) c_b, len_b)) with
//     c_b = roundup(ceil(len_b / nsplit), 64), so ragged batches spread over all their splits and a split past a batch's
//     length writes an empty partial without loading anything.
//   * A workgroup is 4 waves; wave w takes the split's key tiles w, w + 4, ...  K and V go HBM -> registers by buffer_load_dwordx4
//     (per-tile descriptor whose record count ends at the split's last key: rows past it read as zeros), one tile ahead of the
//     math (16 KiB per wave in flight).  S^T = K Q^T and O^T += V^T P^T on the 16x16x32 MFMA: the S^T accumulator holds one
//     query row per lane, so it is, converted to 16 bits, the P^T operand of the PV product as it stands (key order permuted:
//     element j of lane group h of PV k-step u is key 32u + 16(j>>2) + 4h + (j&3)); V^T is read in that order from a per-wave
//     row-major LDS image with ds_read_b64_tr_b16 (rows padded by 32 bytes: conflict-free transposed reads).
//   * Online softmax in fp32 (log2 domain; with an fp32 output P is carried as 16-bit hi + lo), masks (key mask, split end, bottom-right causal cut) only on tiles they touch.
//   * The 4 waves' (m, l, O) merge through LDS; the workgroup writes O and LSE (nsplit == 1) or fp32 partials (O, m, l) that
//     fa3_decode_combine_kernel reduces.  No atomics: bitwise reproducible.
//   * PAGED = true: the cache is a pool of fixed-size pages [num_pages, page_size, Hkv, D] (page / head / token strides) and a device
//     block table int32 [B][max_pages]; logical key j of batch b lives in page block_table[b][j / page_size] at token j % page_size.
//     page_size is a multiple of 64 (= SPLIT_ALIGN and the largest wave tile), so a tile never straddles a page: issue(t) takes one
//     wave-uniform table entry and builds the same per-tile descriptors from the page's base.  The entry is a scalar load, fetched
//     one issue ahead (right behind the previous tile's K / V loads) and carried in a scalar register, so that no dependent load
//     stands in front of a tile's K / V loads (-DPFA_DECODE_PAGE_LOOKAHEAD=0 fetches it in place, for measurement).  The page id is clamped to
//     [0, num_pages - 1] (a bad table gives wrong numbers, never an out-of-range address), and an entry at or past
//     ceil(len_b / page_size) is never read, because a tile exists only below the split's hi <= len_b.  Everything else (split rule,
//     masks by logical key, softmax, merge, combine) is the one code path, so a paged call returns the bits of the contiguous call
//     on the gathered cache.  Pages of 16 or 32 keys would put several pages under one tile and are out of scope.
//   * WINDOW = true (pfa_fa3_decode_ex with a window W, causal only; DecodeWindowPart carries W): row i sees key j iff j < len_b,
//     j <= i + off_b and j > i + off_b - W, off_b = len_b - Sq.  The splits divide [base_b, len_b) instead of [0, len_b), with
//     base_b = floor64(lo_b) and lo_b = max(0, off_b - W + 1) the lowest key row 0 sees: c_b = roundup(ceil((len_b - base_b) / nsplit), 64),
//     split s covers [base_b + s c_b, min(base_b + (s+1) c_b, len_b)).  Boundaries stay multiples of 64, so a tile still lies inside
//     one page.  No tile exists below base_b: keys below it, and table entries below lo_b / page_size, are never read (a server may
//     have given those pages away).  Each row's lower bound row_lo = len_b - Sq + i + 1 - W joins the visibility test on the tiles that
//     reach below the item's largest row_lo; keys in [base_b, row_lo) are read and masked.  The other instantiations are untouched:
//     WINDOW = false compiles to the code and the kernel arguments it had.
//   * TREE = true (pfa_fa3_decode_tree, causal only, no window; DecodeTreePart carries the words): a 64-bit word per query row
//     replaces the causal triangle over the step's own Sq keys.  Row i sees key j iff j < len_b and (j < off_b or bit (j - off_b) of
//     tree[b][i] is set), off_b = len_b - Sq.  Each lane loads its row's word once, by a vector load, in front of the tile loop.  Key off_b
//     itself can be hidden, so the masked path starts one key earlier than under causal (a tile is unmasked only when it ends at or
//     below off_b) and a row's upper bound is len_b.  Keys in [off_b, len_b) that a word hides are read and masked.  Split rule, paging,
//     merge, partials and combine are the one code path: the chain words give the bits of the causal call, all-ones those of
//     causal = 0.  TREE = false compiles to the code and the kernel arguments it had.
//   * KV8 = true (pfa_fa3_decode_q8; no window, no tree; DecodeKv8Part carries the descales): the cache holds OCP e4m3fn bytes, one per
//     element, strides in elements = bytes, and one fp32 descale per (batch, K/V head) each for K and V, read by scalar loads once per
//     item.  Tiles, splits, masks and descriptors are those of the 16-bit kernel (the record count ends at the split's last key in
//     bytes, so rows past it read as zero bytes = +0).  K: an 8-byte load per lane per k-step, the 16-bit kernel's element-to-k-step
//     mapping, converted to T in registers (v_cvt_pk_f32_fp8, then the pack to T: every e4m3 value is a bf16 and an fp16 value, so
//     both steps are exact) in front of the same MFMA against the same Q operand.  V: a 16-byte load per lane (16 elements of one
//     key), converted to T and written as two 16-byte pieces into the same row-major LDS image, so the transposed reads and the PV
//     product stand as they are.  A tile is half the bytes, so two tiles are in flight per wave (two register sets, the tile loop
//     unrolled by two): 16 KiB, as in the 16-bit kernel.  k_descale is folded into the score multiplier, v_descale into the one
//     multiplication of the epilogue (the normalisation, or the partial's write), so the combine kernel is reused unchanged.  With both
//     descales 1 the result has the bits of the 16-bit kernel on the converted cache.  KV8 = false compiles to the code and the kernel
//     arguments it had.
//   * SINK = true (pfa_fa3_decode_sink; plain and WINDOW, no tree, no FP8 cache; DecodeSinkPart carries the pointer): an attention sink,
//     one fp32 value per QUERY head in the units of the scaled scores, is one more key with that score and a zero value row.  Nothing
//     in front of the waves' merge changes.  In the merge, the workgroup of the item's split 0 takes the row's sink (a vector load: the
//     rows of a packed head group belong to different query heads) times log2(e) as a fifth partial (m, l, O) = (sink, 1, 0): the
//     maximum runs over it and the row sum gains exp2(sink - M).  nsplit == 1: that normalises the output and enters the LSE.
//     nsplit > 1: it is part of split 0's (M, L) pair and of the scale of its partial O, and fa3_decode_combine_kernel, unchanged, does
//     the rest; the other splits' workgroups take -inf for the sink, which adds exp2(-inf) = 0.  An empty split passes the tile loop
//     (no wave has a tile) and runs the merge like any other, so split 0 writes the sink's partial -- O = 0, (M, L) = (sink, 1) -- also
//     when its own key range is empty, and a row with no visible key anywhere gets O = 0 and LSE = sink.  A sink of -inf leaves every
//     value as it was (M unchanged, L + 0): the bits of the sink-less kernel; the Mu guard covers -inf - (-inf).  SINK = false compiles
//     to the code and the kernel arguments it had.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "fp8_cvt.h"               // cvt_e4m3x8: the KV8 conversion, shared with fa3_prefill_kernel.h
#include "param_parts.h"

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
typedef __amdgpu_buffer_rsrc_t srd_t;
typedef __attribute__((address_space(3))) char lds_char;
typedef const __attribute__((address_space(4))) int32_t* const_i32_ptr;   // read-only for the kernel's lifetime: scalar loads
typedef const __attribute__((address_space(4))) float* const_f32_ptr;

#ifndef PFA_DECODE_PAGE_LOOKAHEAD
#define PFA_DECODE_PAGE_LOOKAHEAD 1
#endif
#ifndef PFA_DECODE_KV8_SETS
#define PFA_DECODE_KV8_SETS 2      // KV8: tiles in flight per wave (-DPFA_DECODE_KV8_SETS=1: one, 8 KiB, for measurement)
#endif

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

// The mode flags' parts, behind the base in this order.  WINDOW: the sliding window, 1 <= window <= Smax (the host clamps it)
struct DecodeWindowPart {
    int32_t window;
};
// TREE: one 64-bit visibility word per query row, words[b * tree_sb + i]
struct DecodeTreePart {
    const uint64_t* tree;
    int64_t tree_sb;
};
// KV8: fp32 descales, k_descale[b * ds_sb + kvh] (ds_sb = 0: one row for every batch)
struct DecodeKv8Part {
    const float* k_descale;
    const float* v_descale;
    int64_t ds_sb;
};
// SINK: one fp32 sink per query head, sinks[h], in the units of the scaled scores (natural log)
struct DecodeSinkPart {
    const float* sinks;
};
template <bool WINDOW, bool TREE, bool KV8, bool SINK>
struct DecodeBlock : DecodeParams, PartIf<WINDOW, DecodeWindowPart>, PartIf<TREE, DecodeTreePart>, PartIf<KV8, DecodeKv8Part>,
                     PartIf<SINK, DecodeSinkPart> {};
template <bool WINDOW, bool TREE = false, bool KV8 = false, bool SINK = false>
struct DecodeParamsOf { typedef DecodeBlock<WINDOW, TREE, KV8, SINK> type; };

// Which instantiations of fa3_decode_kernel exist: the one statement of it, for the kernel and the host's dispatch.
constexpr bool decode_kernel_exists(bool WINDOW, bool TREE, bool KV8, bool SINK) {
    return !(WINDOW && TREE)                // a tree does not combine with a window
           && !(SINK && (TREE || KV8))      // the sink is built for the plain and the windowed 16-bit cache
           && !(KV8 && (WINDOW || TREE));   // the FP8 cache takes neither a window nor a tree
}

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

// Per head dim: keys per wave tile, loads per lane, LDS image geometry.
template <int D> struct Geo {
    static constexpr int KT = D == 128 ? 32 : 64;        // keys per wave tile: 16 KiB of K + V either way
    static constexpr int NKB = KT / 16;                   // 16-key blocks of S^T
    static constexpr int KS = D / 32;                     // QK^T k-steps (32 head-dim elements each)
    static constexpr int NDB = D / 16;                    // 16-column blocks of O^T
    static constexpr int KLD = NKB * KS;                  // 16-byte K loads per lane per tile
    static constexpr int KPI = 512 / D;                   // keys per 1-KiB V load instruction
    static constexpr int VLD = KT / KPI;                  // 16-byte V loads per lane per tile
    static constexpr int KPI8 = 1024 / D;                 // KV8: keys per 1-KiB V load instruction (16 one-byte elements per lane)
    static constexpr int VLD8 = KT / KPI8;                // KV8: 16-byte V loads per lane per tile
    static constexpr int VROW = D * 2 + 32;               // LDS bytes per key row of the V image
    static constexpr int VIMG = KT * VROW;                // per wave
    static constexpr int MERGE = NW * ROWS * D * 4 + NW * ROWS * 8;
    static constexpr int LDS = VIMG * NW > MERGE ? VIMG * NW : MERGE;
};

// raw-buffer descriptor whose inputs are provably wave-uniform
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

template <typename T, int D, typename OT, bool PAGED = false, bool WINDOW = false, bool TREE = false, bool KV8 = false, bool SINK = false>
__global__ __launch_bounds__(THREADS, 2) void fa3_decode_kernel(const typename DecodeParamsOf<WINDOW, TREE, KV8, SINK>::type p) {
    static_assert(decode_kernel_exists(WINDOW, TREE, KV8, SINK), "no such mode set: see decode_kernel_exists");
    using E = DElem<T>;
    using v8 = typename E::v8;
    using v4 = typename E::v4;
    using Gm = Geo<D>;
    constexpr int KT = Gm::KT, NKB = Gm::NKB, KS = Gm::KS, NDB = Gm::NDB, VLD = Gm::VLD, VROW = Gm::VROW;
    // fp32 output: P carried as a 16-bit hi + lo pair (two PV MFMAs) so that the result is within 1e-3 of the exact one; the
    // matrix pipe has time to spare here, the kernel waits on HBM
    constexpr bool SPLIT_P = sizeof(OT) == 4;
    constexpr uint32_t EB = KV8 ? 1 : 2;       // bytes per cache element
    __shared__ __attribute__((aligned(16))) char smem[Gm::LDS];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int x = blockIdx.x;
    const int s = x % p.nsplit;
    x /= p.nsplit;
    const int rb = x % p.nrb;
    x /= p.nrb;
    const int kvh = x % p.Hkv, b = x / p.Hkv;
    // KV8: the item's two descales (scalar loads); k_descale rides in the score multiplier, v_descale in the epilogue.  Both are
    // used under if constexpr (KV8) only, so that the other kernels keep their expressions
    float score_mul = p.scale_log2, out_mul = 1.f;
    if constexpr (KV8) {
        score_mul *= ((const_f32_ptr)(uintptr_t)p.k_descale)[(int64_t)b * p.ds_sb + kvh];
        out_mul = ((const_f32_ptr)(uintptr_t)p.v_descale)[(int64_t)b * p.ds_sb + kvh];
    }
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
    // every row sees at least the keys below this (TREE: a word may hide key off_b = len - Sq itself)
    const int min_lim = TREE ? len - p.Sq : p.causal ? len - p.Sq + 1 : len;
    // WINDOW (causal): the row's lowest visible key, and the largest of them among the item's rows (its last row's)
    int row_lo = 0, max_lo = 0;
    if constexpr (WINDOW) {
        row_lo = row_lim - p.window;
        const int last = min(rb * ROWS + ROWS - 1, p.Sq * p.G - 1);
        max_lo = __builtin_amdgcn_readfirstlane(len - p.Sq + last / p.G + 1 - p.window);
    }
    // TREE: the row's visibility word over keys off .. off + Sq - 1 (a per-lane vector load; a row past the item's last sees nothing)
    uint64_t tw = 0;
    const int off = len - p.Sq;
    if constexpr (TREE) tw = row_ok ? p.tree[(int64_t)b * p.tree_sb + qi] : 0;

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
        const char* kslab = (const char*)p.k + ((PAGED ? 0 : (int64_t)b * p.k_sb) + (int64_t)kvh * p.k_sh) * EB;
        const char* vslab = (const char*)p.v + ((PAGED ? 0 : (int64_t)b * p.v_sb) + (int64_t)kvh * p.v_sh) * EB;
        const uint32_t kss2 = (uint32_t)p.k_ss * EB, vss2 = (uint32_t)p.v_ss * EB;     // token strides in bytes
        // per-lane byte offsets inside a tile: K in the A-operand layout (key kb*16 + c, head dims 32 ks + 8 h ..),
        // V one 1-KiB piece per instruction (key vi*KPI + lane / (D/8), chunk lane % (D/8); KV8: 16 elements per lane, D/16 chunks a key)
        constexpr int VCH = KV8 ? D / 16 : D / 8, VKPI = KV8 ? Gm::KPI8 : Gm::KPI, NVLD = KV8 ? Gm::VLD8 : VLD;
        const uint32_t koff0 = (uint32_t)c * kss2 + (uint32_t)h * (8u * EB);
        const uint32_t vkey = (uint32_t)lane / VCH, vch = (uint32_t)lane % VCH;
        const uint32_t voff0 = vkey * vss2 + vch * 16u;
        lds_char* vimg = (lds_char*)(smem + wave * Gm::VIMG);
        const uint32_t vwr = vkey * VROW + vch * (KV8 ? 32u : 16u);
        // transposed read: lane 4q + p of its 16-lane group addresses key row (block base + 4h + q), columns 4p .. 4p + 3
        const uint32_t vtr = (uint32_t)(4 * h + ((lane & 15) >> 2)) * VROW + (uint32_t)(lane & 3) * 8u;

        // the tile(s) in flight, one register set each: K as loaded (KV8: 8 bytes per k-step), V as loaded.  The one-set kernels name
        // their set as they always did (kr, vr): arrays of sets, or pointers handed to issue(), change their register allocation
        constexpr int SETS = KV8 ? PFA_DECODE_KV8_SETS : 1;
        using kreg_t = typename std::conditional<KV8, u32x2, u32x4>::type;
        kreg_t kr[NKB * KS], kr2[SETS > 1 ? NKB * KS : 1];
        u32x4 vr[NVLD], vr2[SETS > 1 ? NVLD : 1];
        // paged: the (unclamped) page id of tile t, a wave-uniform scalar load.  Called only for t < ntile, i.e. for keys below
        // hi <= len_b, so table entries at and past ceil(len_b / page_size) are never read.
        const const_i32_ptr table = PAGED ? (const_i32_ptr)(uintptr_t)(p.block_table + (int64_t)b * p.bt_sb) : nullptr;
        auto page_of = [&](int t) { return table[(uint32_t)(lo + t * KT) / (uint32_t)p.page_size]; };
        int pg_next = 0;
        if constexpr (PAGED && PFA_DECODE_PAGE_LOOKAHEAD) pg_next = page_of(wave);
        // issue(t): tile t's loads into kr / vr; issue(t, true) (KV8): into the second set
        auto issue = [&](int t, auto... second) {
            constexpr bool SECOND = sizeof...(second) > 0;
            const int t0 = lo + t * KT;
            const int nk = min(KT, hi - t0);     // rows past the split's end read as zeros
            int64_t koff, voff;                  // element offsets of the tile's first key row from kslab / vslab
            if constexpr (PAGED) {
                // the tile lies inside one page (page_size % 64 == 0, t0 % KT == 0, KT <= 64)
                int pg = PFA_DECODE_PAGE_LOOKAHEAD ? pg_next : page_of(t);
                pg = min(max(pg, 0), p.num_pages - 1);           // device data: never an address outside the pool
                const int tok = (int)((uint32_t)t0 % (uint32_t)p.page_size);
                koff = (int64_t)pg * p.k_sb + (int64_t)tok * p.k_ss;
                voff = (int64_t)pg * p.v_sb + (int64_t)tok * p.v_ss;
            } else {
                koff = (int64_t)t0 * p.k_ss;
                voff = (int64_t)t0 * p.v_ss;
            }
            const srd_t vs = uniform_srd(vslab + voff * EB, (uint32_t)(nk - 1) * vss2 + D * EB);
            const srd_t ks = uniform_srd(kslab + koff * EB, (uint32_t)(nk - 1) * kss2 + D * EB);
#pragma unroll
            for (int i = 0; i < NVLD; ++i)
                (SECOND ? vr2 : vr)[i] = __builtin_amdgcn_raw_buffer_load_b128(vs, (int)(voff0 + (uint32_t)(i * VKPI) * vss2), 0, 0);
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
                for (int q = 0; q < KS; ++q) {
                    const int at = (int)(koff0 + (uint32_t)(kb * 16) * kss2 + q * (32 * EB));
                    if constexpr (KV8) (SECOND ? kr2 : kr)[kb * KS + q] = __builtin_amdgcn_raw_buffer_load_b64(ks, at, 0, 0);
                    else kr[kb * KS + q] = __builtin_amdgcn_raw_buffer_load_b128(ks, at, 0, 0);
                }
            if constexpr (PAGED && PFA_DECODE_PAGE_LOOKAHEAD)
                if (t + NW < ntile) pg_next = page_of(t + NW);   // behind this tile's loads, for the next issue()
        };
        issue(wave);
        if constexpr (SETS > 1)
            if (wave + NW < ntile) issue(wave + NW, true);
        const uint8_t* km = p.key_mask ? p.key_mask + (int64_t)b * p.km_sb : nullptr;

        // One set: the tile loop as it always was (the do-while and u fold away).  Two sets: set u holds tile tb + u NW, the inner loop
        // is unrolled over the sets, and a set is refilled with tile t + SETS NW once the math has consumed it.  (Written so, and not as
        // a lambda or a loop over sets around the body, because those change the one-set kernels' code: tools/isa_same.py.)
        int tb = wave;
        do {
#pragma unroll
        for (int t = tb, u = 0; t < ntile && (SETS == 1 || u < SETS); t += NW, ++u) {
            const bool second = SETS > 1 && u > 0;
            const kreg_t* const krt = second ? kr2 : kr;
            const u32x4* const vrt = second ? vr2 : vr;
            const int t0 = lo + t * KT;
            // V tile -> this wave's LDS image (row-major, padded rows)
#pragma unroll
            for (int i = 0; i < NVLD; ++i) {
                if constexpr (KV8) {
                    typedef __attribute__((address_space(3))) v8 lds_v8;
                    *(lds_v8*)(vimg + vwr + i * VKPI * VROW) = cvt_e4m3x8<T, v8>(vrt[i][0], vrt[i][1]);
                    *(lds_v8*)(vimg + vwr + i * VKPI * VROW + 16) = cvt_e4m3x8<T, v8>(vrt[i][2], vrt[i][3]);
                } else {
                    *(__attribute__((address_space(3))) u32x4*)(vimg + vwr + i * VKPI * VROW) = vr[i];
                }
            }
            // S^T = K Q^T
            f32x4 sacc[NKB];
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb) {
                sacc[kb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int q = 0; q < KS; ++q) {
                    v8 kf;
                    if constexpr (KV8) kf = cvt_e4m3x8<T, v8>(krt[kb * KS + q][0], krt[kb * KS + q][1]);
                    else kf = __builtin_bit_cast(v8, kr[kb * KS + q]);
                    sacc[kb] = E::mfma(kf, qf[q], sacc[kb]);
                }
            }
            if (t + SETS * NW < ntile) {
                if (second) issue(t + SETS * NW, true);
                else issue(t + SETS * NW);
            }

            // scores in log2 units; masks only where the tile reaches past the split, the causal cut (TREE: the step's own keys), below a row's window, or a key mask exists
            const bool edge = km != nullptr || t0 + KT > hi || t0 + KT > min_lim || (WINDOW && t0 < max_lo);
            float mx = -__builtin_inff();
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float sc;
                    if constexpr (KV8) sc = sacc[kb][e] * score_mul;
                    else sc = sacc[kb][e] * p.scale_log2;
                    if (edge) {
                        const int key = t0 + kb * 16 + 4 * h + e;
                        bool vis;
                        if constexpr (WINDOW) vis = key < hi && (uint32_t)(key - row_lo) < (uint32_t)p.window;   // row_lo <= key < row_lim
                        else if constexpr (TREE) vis = key < hi && (key < off || ((tw >> ((key - off) & 63)) & 1));   // hi <= len: the bit is below Sq
                        else vis = key < hi && key < row_lim;
                        if (vis && km) vis = km[key] != 0;
                        sc = vis ? sc : -__builtin_inff();
                    }
                    sacc[kb][e] = sc;
                    mx = fmaxf(mx, sc);
                }
            mx = fmaxf(mx, __shfl_xor(mx, 16));
            mx = fmaxf(mx, __shfl_xor(mx, 32));
            const float m_new = fmaxf(m, mx);
            const float m_use = m_new == -__builtin_inff() ? 0.f : m_new;
            const float alpha = __builtin_amdgcn_exp2f(m - m_use);
            m = m_new;
            float ps = 0.f;
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float pe = __builtin_amdgcn_exp2f(sacc[kb][e] - m_use);
                    sacc[kb][e] = pe;
                    ps += pe;
                }
            l = l * alpha + ps;
#pragma unroll
            for (int d = 0; d < NDB; ++d) oacc[d] *= alpha;

            asm volatile("" ::: "memory");     // the image writes above stay ahead of the transposed reads below (in-order LDS)
            // O^T += V^T P^T, one 32-key k-step per pair of S^T blocks
#pragma unroll
            for (int u = 0; u < NKB / 2; ++u) {
                v8 pf, plo;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    pf[e] = (T)sacc[2 * u][e];
                    pf[4 + e] = (T)sacc[2 * u + 1][e];
                    if constexpr (SPLIT_P) {
                        plo[e] = (T)(sacc[2 * u][e] - (float)pf[e]);
                        plo[4 + e] = (T)(sacc[2 * u + 1][e] - (float)pf[4 + e]);
                    }
                }
#pragma unroll
                for (int d = 0; d < NDB; ++d) {
                    const v4 a0 = E::tr_read(vimg + vtr + (uint32_t)(32 * u) * VROW + d * 32);
                    const v4 a1 = E::tr_read(vimg + vtr + (uint32_t)(32 * u + 16) * VROW + d * 32);
                    const v8 va = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
                    oacc[d] = E::mfma(va, pf, oacc[d]);
                    if constexpr (SPLIT_P) oacc[d] = E::mfma(va, plo, oacc[d]);
                }
            }
            asm volatile("" ::: "memory");     // ... and the next tile's image writes behind them
        }
        tb += SETS * NW;
        } while (SETS > 1 && tb < ntile);
    }
    // row sum over the row's four lane groups
    l += __shfl_xor(l, 16);
    l += __shfl_xor(l, 32);

    // merge the waves' partials through LDS (the V images are dead after this barrier)
    __syncthreads();
    float* mo = (float*)smem;                                   // [NW][ROWS][D]
    float* mml = (float*)(smem + NW * ROWS * D * 4);            // [NW][ROWS][2]
#pragma unroll
    for (int d = 0; d < NDB; ++d) *(f32x4*)(mo + (wave * ROWS + c) * D + 16 * d + 4 * h) = oacc[d];
    if (h == 0) {
        mml[(wave * ROWS + c) * 2] = m;
        mml[(wave * ROWS + c) * 2 + 1] = l;
    }
    __syncthreads();
    constexpr int TPR = THREADS / ROWS, DPT = D / TPR;          // threads per row, head-dim elements per thread
    const int orow = tid / TPR, d0 = (tid % TPR) * DPT;
    const int rr = rb * ROWS + orow;
    if (rr >= p.Sq * p.G) return;
    float mw[NW], M = -__builtin_inff();
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        mw[w] = mml[(w * ROWS + orow) * 2];
        M = fmaxf(M, mw[w]);
    }
    // SINK: the row's sink in log2 units as one more partial (m, l, O) = (sink, 1, 0), in the item's split 0 only (-inf elsewhere: + 0)
    float sink = -__builtin_inff();
    if constexpr (SINK) {
        if (s == 0) sink = p.sinks[kvh * p.G + rr % p.G] * 1.4426950408889634f;
        M = fmaxf(M, sink);
    }
    const float Mu = M == -__builtin_inff() ? 0.f : M;
    float L = 0.f, sc[NW];
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        sc[w] = __builtin_amdgcn_exp2f(mw[w] - Mu);
        L += sc[w] * mml[(w * ROWS + orow) * 2 + 1];
    }
    if constexpr (SINK) L += __builtin_amdgcn_exp2f(sink - Mu);     // a sink of -inf with M = -inf: exp2(-inf - 0) = 0
    const int oi = rr / p.G, oh = kvh * p.G + rr % p.G;
    if (p.nsplit == 1) {
        const float inv = L > 0.f ? 1.f / L : 0.f;
        OT* orow_p = (OT*)p.o + (int64_t)b * p.o_sb + (int64_t)oi * p.o_ss + (int64_t)oh * p.o_sh;
#pragma unroll
        for (int d = 0; d < DPT; d += 4) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int w = 0; w < NW; ++w) acc += sc[w] * *(const f32x4*)(mo + (w * ROWS + orow) * D + d0 + d);
            if constexpr (KV8) store4<OT>(orow_p + d0 + d, acc * (inv * out_mul));
            else store4<OT>(orow_p + d0 + d, acc * inv);
        }
        if (p.lse && d0 == 0)
            p.lse[((int64_t)b * p.H + oh) * p.Sq + oi] = L > 0.f ? (M + __log2f(L)) * 0.6931471805599453f : -__builtin_inff();
    } else {
        const int64_t prow = (((int64_t)s * p.B + b) * p.H + oh) * p.Sq + oi;
        float* po = p.part_o + prow * D;
#pragma unroll
        for (int d = 0; d < DPT; d += 4) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int w = 0; w < NW; ++w) acc += sc[w] * *(const f32x4*)(mo + (w * ROWS + orow) * D + d0 + d);
            if constexpr (KV8) acc *= out_mul;
            *(f32x4*)(po + d0 + d) = acc;
        }
        if (d0 == 0) {
            p.part_ml[prow * 2] = M;
            p.part_ml[prow * 2 + 1] = L;
        }
    }
}

// Reduce the splits of every (b, h, i) row: one thread per 4 head-dim elements of a row.
template <int D, typename OT>
__global__ __launch_bounds__(256) void fa3_decode_combine_kernel(const DecodeParams p) {
    constexpr int TPR = D / 4;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t rows = (int64_t)p.B * p.H * p.Sq;
    const int64_t row = t / TPR;
    if (row >= rows) return;
    const int d0 = (int)(t % TPR) * 4;
    const int64_t pstride = rows;
    float M = -__builtin_inff();
#pragma unroll 8
    for (int s = 0; s < p.nsplit; ++s) M = fmaxf(M, p.part_ml[(s * pstride + row) * 2]);
    const float Mu = M == -__builtin_inff() ? 0.f : M;
    float L = 0.f;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8   // (eight splits' loads in flight: the launch is a few microseconds of latency, not bandwidth)
    for (int s = 0; s < p.nsplit; ++s) {
        const int64_t pr = s * pstride + row;
        const float w = __builtin_amdgcn_exp2f(p.part_ml[pr * 2] - Mu);
        L += w * p.part_ml[pr * 2 + 1];
        acc += w * *(const f32x4*)(p.part_o + pr * D + d0);
    }
    const int i = (int)(row % p.Sq);
    const int64_t bh = row / p.Sq;
    const int hh = (int)(bh % p.H), b = (int)(bh / p.H);
    const float inv = L > 0.f ? 1.f / L : 0.f;
    store4<OT>((OT*)p.o + (int64_t)b * p.o_sb + (int64_t)i * p.o_ss + (int64_t)hh * p.o_sh + d0, acc * inv);
    if (p.lse && d0 == 0) p.lse[row] = L > 0.f ? (M + __log2f(L)) * 0.6931471805599453f : -__builtin_inff();
}

}  // namespace dec
}  // namespace pfa

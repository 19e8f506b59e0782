// kv_append_kernel.h -- the write side of a serving step for MI355X (gfx950), hand-written HIP: places a step's new K / V rows into a
// KV cache (contiguous or paged) from device data alone, so that append + attention is two launches with no host round trip.
//
// Lengths are those AFTER the step (the convention of the three calls over a KV cache): with len_b = clamp(cache_seqlens[b], 0, Smax)
// and Sq_b the sequence's new rows, row i goes to logical key pos = len_b - Sq_b + i.  The kernel never writes lengths, so a replay
// is idempotent.
//   VARLEN  packed rows [total_new, Hkv, D]: s_b = clamp(cu[b], 0, total_new), e_b = clamp(cu[b + 1], s_b, total_new),
//           Sq_b = min(e_b - s_b, max_seqlen_q) -- fa3_prefill_kernel's clamps; row i of sequence b is packed row s_b + i.
//           Otherwise Sq_b = Sq and row i of sequence b is at b * kn_sb + i * kn_ss.
//   PAGED   page = block_table[b][pos / page_size], token pos % page_size.  A page id outside [0, num_pages - 1] DROPS the write: the
//           readers clamp a bad id (wrong numbers), but a clamped write would land in a live page of another sequence.
// Rows with pos < 0 (len_b < Sq_b: the rows the attention call gives O = 0) are dropped.  Bad device data loses rows, it never makes
// an address outside the cache or the packed tensors: i < Sq_b <= e_b - s_b bounds the source, 0 <= pos < len_b <= Smax the
// destination, pos / page_size < Smax / page_size <= bt_sb the table entry.  Packed rows no sequence covers are never read, and
// nothing but the destination rows is written.
//
// Work item = 8 elements (16 bytes) of one head of one new row, K and V both: one global_load_dwordx4 and one global_store_dwordx4
// each.  A sequence has Sq_b * units items, units = Hkv * D / 8, laid out [row][head][chunk] so that consecutive lanes move
// consecutive 16-byte pieces of a row; a workgroup takes 256 consecutive items of ONE sequence.  Grid = B * ceil(max_seqlen_q * units
// / 256) from host shapes only: capturable, and valid while cu_seqlens_q, lengths, table and cache change between replays.  b is
// uniform per workgroup, so cu[b], cu[b + 1] and cache_seqlens[b] are scalar loads and the workgroups past a sequence's last item
// (all of them for an empty sequence) return before any vector memory instruction.  The table lookup is per lane: a workgroup's rows
// may straddle pages.  No LDS, no atomics, no workspace; the element type does not matter (any 2-byte type moves the same way).
//
// QUANT (pfa_kv_append_q8; T is the source's 16-bit type, KvAppendQ8Params carries the descales): the cache holds OCP e4m3fn bytes, cache
// strides are in bytes, and every source element x is stored as e4m3fn(clamp(float(x) / descale[b * ds_sb + hk], -448, 448)): an IEEE
// fp32 division, the clamp (a NaN passes it and stays NaN), and v_cvt_pk_fp8_f32's round to nearest even.  A work item is 16 elements:
// two 16-byte loads and one 16-byte store each for K and V; dchunks = D / 16, units = Hkv * D / 16.  Placement, drops and the grid rule
// are the code above.  The descale is a per-lane load (a workgroup's items span heads).  QUANT = false compiles to the code it had.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pfa {

constexpr int KV_APPEND_THREADS = 256;

struct KvAppendParams {
    const void* k_new;
    const void* v_new;
    void* k_cache;               // cache [B, Smax, Hkv, D] by strides, or (PAGED) pool [num_pages, page_size, Hkv, D]
    void* v_cache;
    const int32_t* cu_seqlens_q; // VARLEN: [B + 1]
    const int32_t* seqlens;      // [B], after the step
    const int32_t* block_table;  // PAGED: [B][max_pages] page ids
    int64_t kn_sb, kn_ss, kn_sh; // element strides; *_sb unused under VARLEN
    int64_t vn_sb, vn_ss, vn_sh;
    int64_t k_sb, k_sh, k_ss;    // PAGED: k_sb / v_sb are the page strides
    int64_t v_sb, v_sh, v_ss;
    int64_t bt_sb;
    int32_t nchunk;              // workgroups per sequence: ceil(Sq * units / 256)
    int32_t Sq;                  // rows per sequence; VARLEN: max_seqlen_q
    int32_t Smax, total_new;
    int32_t dchunks;             // D / 8
    int32_t units;               // Hkv * D / 8; Sq * units + 256 fits 32 bits (checked by the host)
    int32_t page_size, num_pages;
};

// QUANT only: fp32 descales, k_descale[b * ds_sb + hk] (ds_sb = 0: one row for every sequence)
struct KvAppendQ8Params : KvAppendParams {
    const float* k_descale;
    const float* v_descale;
    int64_t ds_sb;
};
template <bool QUANT> struct KvAppendParamsOf { typedef KvAppendParams type; };
template <> struct KvAppendParamsOf<true> { typedef KvAppendQ8Params type; };

typedef uint32_t kv_append_b128 __attribute__((ext_vector_type(4)));
typedef uint32_t kv_append_b64 __attribute__((ext_vector_type(2)));

// 8 elements of T (16 bytes) -> 8 e4m3fn bytes: x / d in fp32, clamped to the format's finite range (NaN stays NaN), rounded to nearest even
template <typename T>
__device__ __forceinline__ kv_append_b64 kv_quant8(kv_append_b128 x, float d) {
    typedef T t8 __attribute__((ext_vector_type(8)));
    const t8 e = __builtin_bit_cast(t8, x);
    float f[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float y = (float)e[j] / d;
        f[j] = y != y ? y : fminf(fmaxf(y, -448.f), 448.f);
    }
    int a = 0, b = 0;
    a = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], a, false);
    a = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], a, true);
    b = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], b, false);
    b = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], b, true);
    return kv_append_b64{(uint32_t)a, (uint32_t)b};
}

template <bool VARLEN, bool PAGED, bool QUANT = false, typename T = void>
__global__ __launch_bounds__(KV_APPEND_THREADS) void kv_append_kernel(const typename KvAppendParamsOf<QUANT>::type p) {
    constexpr int CH = QUANT ? 16 : 8;                   // elements per work item
    const int b = blockIdx.x / p.nchunk;
    const int item0 = (blockIdx.x - b * p.nchunk) * KV_APPEND_THREADS;      // the workgroup's first item of sequence b

    int sq = p.Sq, row0 = 0;
    if constexpr (VARLEN) {
        const int s_b = min(max(p.cu_seqlens_q[b], 0), p.total_new);
        const int e_b = min(max(p.cu_seqlens_q[b + 1], s_b), p.total_new);
        row0 = s_b;
        sq = min(e_b - s_b, p.Sq);
    }
    if (item0 >= sq * p.units) return;                   // wave-uniform: nothing of this sequence in the workgroup
    const int len = min(max(p.seqlens[b], 0), p.Smax);

    const int item = item0 + (int)threadIdx.x;
    const int i = item / p.units;                        // new row of the sequence
    const int rem = item - i * p.units;
    const int hk = rem / p.dchunks;
    const int c = rem - hk * p.dchunks;
    const int pos = len - sq + i;                        // its logical key
    if (i >= sq || pos < 0) return;

    int64_t ksrc, vsrc;
    if constexpr (VARLEN) {
        ksrc = (int64_t)(row0 + i) * p.kn_ss;
        vsrc = (int64_t)(row0 + i) * p.vn_ss;
    } else {
        ksrc = (int64_t)b * p.kn_sb + (int64_t)i * p.kn_ss;
        vsrc = (int64_t)b * p.vn_sb + (int64_t)i * p.vn_ss;
    }
    ksrc += (int64_t)hk * p.kn_sh + c * CH;
    vsrc += (int64_t)hk * p.vn_sh + c * CH;

    int64_t slab = b, tok = pos;                         // contiguous: the sequence's cache; PAGED: the page and the token inside it
    if constexpr (PAGED) {
        const int lp = pos / p.page_size;
        const int pg = p.block_table[(int64_t)b * p.bt_sb + lp];
        if ((unsigned)pg >= (unsigned)p.num_pages) return;                  // dropped, never clamped (see above)
        slab = pg;
        tok = pos - lp * p.page_size;
    }
    const int64_t kdst = slab * p.k_sb + tok * p.k_ss + (int64_t)hk * p.k_sh + c * CH;
    const int64_t vdst = slab * p.v_sb + tok * p.v_ss + (int64_t)hk * p.v_sh + c * CH;

    if constexpr (QUANT) {
        const kv_append_b128* ks = reinterpret_cast<const kv_append_b128*>((const uint16_t*)p.k_new + ksrc);
        const kv_append_b128* vs = reinterpret_cast<const kv_append_b128*>((const uint16_t*)p.v_new + vsrc);
        const kv_append_b128 k0 = ks[0], k1 = ks[1], v0 = vs[0], v1 = vs[1];
        const float kd = p.k_descale[(int64_t)b * p.ds_sb + hk], vd = p.v_descale[(int64_t)b * p.ds_sb + hk];
        const kv_append_b64 ka = kv_quant8<T>(k0, kd), kb = kv_quant8<T>(k1, kd), va = kv_quant8<T>(v0, vd), vb = kv_quant8<T>(v1, vd);
        *reinterpret_cast<kv_append_b128*>((uint8_t*)p.k_cache + kdst) = kv_append_b128{ka[0], ka[1], kb[0], kb[1]};
        *reinterpret_cast<kv_append_b128*>((uint8_t*)p.v_cache + vdst) = kv_append_b128{va[0], va[1], vb[0], vb[1]};
    } else {
        const kv_append_b128 kx = *reinterpret_cast<const kv_append_b128*>((const uint16_t*)p.k_new + ksrc);
        const kv_append_b128 vx = *reinterpret_cast<const kv_append_b128*>((const uint16_t*)p.v_new + vsrc);
        *reinterpret_cast<kv_append_b128*>((uint16_t*)p.k_cache + kdst) = kx;
        *reinterpret_cast<kv_append_b128*>((uint16_t*)p.v_cache + vdst) = vx;
    }
}

}  // namespace pfa

// fa3_prefill_d256_kernel.h -- compute-bound forward over a KV cache (contiguous or paged) at head dim 256 for MI355X (gfx950),
// hand-written HIP.  The semantics are fa3_prefill_kernel's, rule for rule (read that header first: lengths and the bottom-right causal
// offset from the device, rows without a visible key, descriptors that end at a tile's last valid key, PAGED, VARLEN, WINDOW), with
// BLOCK_M = 128; PrefillParams, its VARLEN / WINDOW parts, Elem, the LDS-DMA helper, the row store through LDS and the softmax helpers
// are that header's and fa3_fwd_kernel.h's, by inclusion.  There is no SPLIT, no KV8 and no SINK at this head dim.  What is its own:
//
// WORK SPLIT.  128 query rows per workgroup: 4 waves x 32 rows, ONE wave per SIMD on the 512-register budget (__launch_bounds__(256, 1)),
// as fa3_fwd_w4_kernel.  O^T (8 blocks of 32x32, 128 registers) and the resident Q operand (64) live in the accumulator half: O through
// the compiler's MFMAs, Q pinned there by W4Asm's "a" constraint; S (two tiles, 64), P (16; 32 with the hi + lo pair of an fp32 output)
// and the K / V^T fragments live in the arch VGPRs.  fa3_prefill_kernel's 8 waves x 32 rows at two waves per SIMD would have 256
// registers for all of that.  Written with the compiler's MFMA for S too, every instantiation spilled 156 - 208 bytes per lane: it kept
// S in the accumulator half and copied it out for the softmax.  The resource gate (0 spills, 0 scratch, VGPR + AGPR <= 512) is checked
// per instantiation with tools/kres.py; the arch half is full (256), and the compiler parks loop-invariant LDS addresses in spare
// accumulator registers.
//
// LDS: 128 KiB dynamic.  K ring [2][64 keys][512 B] at 0, V ring [2][64 keys][512 B] at 64 KiB, both fed by LDS-DMA.  K runs ONE TILE
// AHEAD of V: with no partner wave on the SIMD the softmax of tile j has to overlap matrix work of the wave's own stream, so step j
// issues S^T(j + 1) = K(j + 1) Q^T (32 MFMAs, K fragments by ds_read_b128 through a ring of four) ONE MFMA IN FRONT OF EACH of the 32
// exponentials of tile j (multiply-add, exp2, sum, conversion to P), pinned there by scheduling barriers, then O^T += V(j)^T P(j)^T (32
// MFMAs, 64 with SPLITP; V^T by ds_read_b64_tr_b16).  S lives in two register tiles that swap roles every step.  Step j issues, before
// its math, V(j + 1) into the V slot that V(j - 1) left and K(j + 2) into the slot K(j) left, and ends with vmcnt(0), lgkmcnt(0) and ONE
// barrier.  The masks, the row max, the deferred-max decision and the (rare) rescale of O are not overlapped.
//
// LDS IMAGE.  One key per 512-byte row, 32 chunks of 16 bytes; chunk c of row R is stored at position c ^ sw(R), sw(R) =
// ((R & 3) << 2) | ((R >> 2) & 3) -- fa3_fwd_kernel's term, on the low four bits of the chunk index only.  A bank group is a 16-byte
// column of the 256-byte bank line, i.e. position & 15; rows are a multiple of the bank line apart, so the column is all that matters:
//   - K fragments (ds_read_b128): the 16 lanes served together hold rows r0 .. r0 + 15 at one logical chunk; sw is a bijection of R & 15
//     onto 0 .. 15, so they hit 16 different columns: conflict-free;
//   - V^T (ds_read_b64_tr_b16): a 16-lane group reads rows 4h + tq (+ 8 hi), tq = 0 .. 3, at chunks c0, c0 + 1 (c0 even) in 8-byte halves;
//     the four rows differ in R & 3, which sw moves to bits 2-3 of the position: four different column quads, and inside a quad the two
//     chunks and two halves are distinct 8-byte slots: conflict-free, as at D = 128 (the fifth chunk bit and the doubled row stride do
//     not enter the column);
//   - the DMA writes whole 1-KiB pieces (two rows) linearly; the swizzle is applied to each lane's SOURCE chunk.
// The epilogue's 16-bit rows go through the same LDS (128 rows x 512 B, a wave's 32 rows in its own 16 KiB, store_rows_from_lds<512>).
// Q is read straight into registers (16 loads of 16 bytes per lane, once per workgroup).
//
// PER TILE AND WAVE: 64 MFMAs (96 with SPLITP) of v_mfma_f32_32x32x16, 32 ds_read_b128, 64 ds_read_b64_tr_b16, 16 LDS-DMA pieces
// (8 of K, 8 of V: a tile image is 32 pieces over 4 waves), one barrier.
//
// PAGED: the K stream walks the table (one wave-uniform entry per tile, a scalar load issued when the previous K tile's DMA went out,
// clamped into [0, num_pages - 1]); V(j) is always issued after K(j) and before K(j + 1), and takes the page and token K(j) took.
// Entries at and past ceil(len_b / page_size), and with a WINDOW those below 64 j_lo / page_size, are never read.
// Grid = B * H * ceil(Sq / 128) from host shapes, heaviest blocks first under the causal flag; no workspace, no atomics.
#pragma once
#include "fa3_fwd_w4_kernel.h"
#include "fa3_prefill_kernel.h"

namespace pfa {

constexpr int P256_D = 256;
constexpr int P256_WAVES = 4;
constexpr int P256_THREADS = P256_WAVES * 64;
constexpr int P256_BLOCK_M = P256_WAVES * WAVE_M;             // 128 query rows per workgroup
constexpr int P256_TILE_BYTES = BLOCK_N * P256_D * 2;         // 32 KiB: one K or V image
constexpr int P256_LDS_BYTES = 4 * P256_TILE_BYTES;           // K ring + V ring

// Byte offset of 16-byte chunk `ch` (0 .. 31) of key row `key` inside one image (see LDS IMAGE)
__device__ __forceinline__ uint32_t tile_off_d256(uint32_t key, uint32_t ch) {
    const uint32_t sw = ((key & 3) << 2) | ((key >> 2) & 3);
    return key * 512u + ((ch ^ sw) << 4);
}

template <typename T, bool CAUSAL, bool SPLITP, bool PAGED, typename OT, bool VARLEN = false, bool WINDOW = false>
__global__ __launch_bounds__(P256_THREADS, 1) void fa3_prefill_d256_kernel(const typename PrefillParamsOf<VARLEN, WINDOW>::type p) {
    static_assert(CAUSAL || !WINDOW, "the window is cut from the causal diagonal");
    constexpr int D = P256_D, NW = P256_WAVES, BLOCK_M = P256_BLOCK_M;
    using E = Elem<T>;
    using M = W4Asm<T>;
    using v8 = typename E::v8;
    using v4 = typename E::v4;
    typedef __attribute__((address_space(3))) v8 lds_v8;
    constexpr int KS = D / 16;                // 16 k-steps of the QK^T product
    constexpr int DB = D / 32;                // 8 d blocks of the PV product
    constexpr int TILE_BYTES = P256_TILE_BYTES;
    constexpr int HALF_TILE = TILE_BYTES / 2; // 32 keys
    constexpr int K_BASE = 0, V_BASE = 2 * TILE_BYTES;

    extern __shared__ __attribute__((aligned(16))) char smem[];
    const uint32_t smem_base = (uint32_t)(uintptr_t)(lds_char*)smem;   // LDS byte address (wave-uniform)

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31;
    const int h = lane >> 5;

    // ---- block -> (q block, batch*head): heaviest (longest causal row) blocks first ----------------
    const int BH = p.B * p.H;
    const int n = blockIdx.x;
    const int qrank = n / BH;
    const int bh = n - qrank * BH;
    const int qblk = CAUSAL ? (p.nqblk - 1 - qrank) : qrank;
    const int b = bh / p.H;
    const int hh = bh - b * p.H;

    const int q0 = qblk * BLOCK_M;
    const int wave_q0 = q0 + wave * WAVE_M;
    const int my_q = wave_q0 + r;

    // ---- VARLEN: the batch's rows in the packed tensors, from the device (clamped: never a row outside them) ----
    int sq = p.Sq;
    int row0 = 0;
    if constexpr (VARLEN) {
        const int s_b = min(max(p.cu_seqlens_q[b], 0), p.total_q);
        const int e_b = min(max(p.cu_seqlens_q[b + 1], s_b), p.total_q);
        row0 = __builtin_amdgcn_readfirstlane(s_b);
        sq = __builtin_amdgcn_readfirstlane(min(e_b - s_b, p.Sq));
        if (q0 >= sq) return;                            // nothing of this batch in the block: no load, no store
    }
    const bool wave_has_rows = !VARLEN || wave_q0 < sq;

    // ---- the batch's length and causal offset, from the device ----------------------------------
    int kv_len = p.Smax;
    if (p.seqlens) kv_len = min(kv_len, max(p.seqlens[b], 0));
    kv_len = __builtin_amdgcn_readfirstlane(kv_len);
    const int off = kv_len - sq;                         // row i sees key j iff j <= i + off (may be negative)
    const int kv_end = CAUSAL ? max(0, min(kv_len, q0 + BLOCK_M + off)) : kv_len;       // keys the block needs
    const int wave_kv_end = !wave_has_rows ? 0 : CAUSAL ? min(kv_len, wave_q0 + WAVE_M + off) : kv_len;   // keys this wave needs (<= 0: none)
    const int my_lim = my_q + off;                       // last key this row sees under the causal cut
    const int nt = (kv_end + BLOCK_N - 1) / BLOCK_N;
    // WINDOW: the block's first tile (j_lo < nt whenever nt > 0), the lowest key the wave's first row sees and the lowest its last row sees
    int j_lo = 0, wave_lo = 0, wave_lo_last = 0;
    if constexpr (WINDOW) {
        j_lo = max(0, q0 + off - p.window + 1) / BLOCK_N;
        wave_lo = wave_q0 + off - p.window + 1;
        wave_lo_last = wave_lo + WAVE_M - 1;
    }
    // the tiles this wave computes: none above its rows' causal bound, none wholly below its first row's window
    auto computes = [&](int j) { return j * BLOCK_N < wave_kv_end && (!WINDOW || j * BLOCK_N + BLOCK_N > wave_lo); };

    const int kvh = hh / p.kv_group;
    const T* __restrict__ qp = (const T*)p.q + (VARLEN ? (int64_t)row0 * p.q_ss : (int64_t)b * p.q_sb) + (int64_t)hh * p.q_sh;
    // contiguous: this batch's and head's slab; paged: the head's offset inside every page (the page base is added per tile)
    const char* kp = (const char*)p.k + ((PAGED ? 0 : (int64_t)b * p.k_sb) + (int64_t)kvh * p.k_sh) * 2;
    const char* vp = (const char*)p.v + ((PAGED ? 0 : (int64_t)b * p.v_sb) + (int64_t)kvh * p.v_sh) * 2;

    // ---- Q fragments: B operand of S^T = K Q^T, lane (r,h) holds Q[my_q][16 ks + 8 h .. +7] -----------
    v8 qf[KS];
    {
        const int qrow = min(my_q, sq - 1);
        const T* src = qp + (int64_t)qrow * p.q_ss + 8 * h;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) qf[ks] = *(const v8*)(src + 16 * ks);
    }

    // ---- K/V staging by LDS-DMA: a piece is 1 KiB = LDS rows 2i, 2i + 1; wave w issues pieces w, w + 4, ... of an image.  The lane at
    // position pos of row R fetches the logical chunk pos ^ sw(R): the swizzle is applied to the SOURCE
    constexpr int PPW = (TILE_BYTES / 1024) / NW;        // 8 pieces per wave and image
    // loop-invariant per-lane byte offsets from the tile's first key row, of pieces t = 0 and 1; piece t + 2 lies 16 rows further, where
    // the swizzle term repeats: a wave-uniform addend
    uint32_t kvoff[2], vvoff[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int R = 2 * (wave + NW * t) + (lane >> 5);
        const int sw = ((R & 3) << 2) | ((R >> 2) & 3);
        const int col = ((lane & 31) ^ sw) * 8;
        kvoff[t] = (uint32_t)(R * (int)p.k_ss + col) * 2u;
        vvoff[t] = (uint32_t)(R * (int)p.v_ss + col) * 2u;
    }
    const uint32_t k_rows16 = 32u * (uint32_t)p.k_ss, v_rows16 = 32u * (uint32_t)p.v_ss;     // bytes of 16 key rows
    // PAGED: the K stream's walk -- the raw entry of the NEXT K tile, its index in the table row, the token inside the page -- and
    // the (clamped) page and token the LAST K tile took, which the V tile of the same index takes behind it.
    const prefill_table_ptr table = PAGED ? (prefill_table_ptr)(uintptr_t)(p.block_table + (int64_t)b * p.bt_sb) : nullptr;
    int pg_next = 0, pg_idx = 0, pg_tok = 0, pg_last = 0, tok_last = 0;
    if constexpr (PAGED) {
        if constexpr (WINDOW) {
            pg_idx = (int)((uint32_t)(j_lo * BLOCK_N) / (uint32_t)p.page_size);
            pg_tok = j_lo * BLOCK_N - pg_idx * p.page_size;
        }
        if (j_lo < nt) pg_next = table[pg_idx];
    }
    // K(j) into K slot SLOT.  Called for j = j_lo, j_lo + 1, ... < nt in order; the descriptor ends at the tile's last valid key
    auto dma_k = [&](auto slotc, int j) {
        constexpr int SLOT = decltype(slotc)::value;
        const int nk = min(BLOCK_N, kv_len - j * BLOCK_N);
        int64_t koff;
        if constexpr (PAGED) {
            pg_last = min(max(pg_next, 0), p.num_pages - 1);          // device data: never an address outside the pool
            tok_last = pg_tok;
            koff = (int64_t)pg_last * p.k_sb + (int64_t)pg_tok * p.k_ss;
        } else {
            koff = (int64_t)j * BLOCK_N * p.k_ss;
        }
        const srd_t ksrd = __builtin_amdgcn_make_buffer_rsrc((void*)(kp + koff * 2), 0, (int)((int64_t)(nk - 1) * p.k_ss * 2 + D * 2), 0x00020000);
#pragma unroll
        for (int t = 0; t < PPW; ++t)
            lds_dma16_buf(ksrd, kvoff[t & 1] + (uint32_t)(t >> 1) * k_rows16, smem_base + K_BASE + SLOT * TILE_BYTES + (wave + NW * t) * 1024);
        if constexpr (PAGED) {
            pg_tok += BLOCK_N;
            if (pg_tok == p.page_size) {
                pg_tok = 0;
                ++pg_idx;
                if (j + 1 < nt) pg_next = table[pg_idx];
            }
        }
    };
    // V(j) into V slot SLOT: behind dma_k(j) and in front of dma_k(j + 1)
    auto dma_v = [&](auto slotc, int j) {
        constexpr int SLOT = decltype(slotc)::value;
        const int nk = min(BLOCK_N, kv_len - j * BLOCK_N);
        int64_t voff;
        if constexpr (PAGED) voff = (int64_t)pg_last * p.v_sb + (int64_t)tok_last * p.v_ss;
        else voff = (int64_t)j * BLOCK_N * p.v_ss;
        const srd_t vsrd = __builtin_amdgcn_make_buffer_rsrc((void*)(vp + voff * 2), 0, (int)((int64_t)(nk - 1) * p.v_ss * 2 + D * 2), 0x00020000);
#pragma unroll
        for (int t = 0; t < PPW; ++t)
            lds_dma16_buf(vsrd, vvoff[t & 1] + (uint32_t)(t >> 1) * v_rows16, smem_base + V_BASE + SLOT * TILE_BYTES + (wave + NW * t) * 1024);
    };

    // ---- per-lane LDS read addresses, loop invariant and opaque (the compiler otherwise rebuilds row and chunk parts every tile) ----
    // Chunks 16 .. 31 of a row lie 256 bytes behind chunks 0 .. 15 (the swizzle stays inside the low four bits): k-steps 8 .. 15 and d
    // blocks 4 .. 7 are an immediate offset on the addresses of 0 .. 7 and 0 .. 3
    uint32_t koff[KS / 2];
#pragma unroll
    for (int ks = 0; ks < KS / 2; ++ks) {
        koff[ks] = smem_base + K_BASE + tile_off_d256(r, 2 * ks + h);
        asm volatile("" : "+v"(koff[ks]));
    }
    const int g1 = (lane >> 4) & 1;
    const int tq = (lane & 15) >> 2;
    const int tp = lane & 3;
    uint32_t voff[DB / 2][2];
#pragma unroll
    for (int db = 0; db < DB / 2; ++db)
#pragma unroll
        for (int hi = 0; hi < 2; ++hi) {
            voff[db][hi] = smem_base + V_BASE + tile_off_d256(4 * h + tq + 8 * hi, db * 4 + 2 * g1 + (tp >> 1)) + 8 * (tp & 1);
            asm volatile("" : "+v"(voff[db][hi]));
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

    // ---- S^T = K Q^T of the tile in K slot SLOT: 32 MFMAs behind a ring of PF fragment reads.  The MFMAs are W4Asm's statements: Q is
    // pinned in the accumulator half ("a") and S in the arch VGPRs, where the masks and the softmax work on it, so nothing is copied
    // between the halves.  The compiler does not know them as MFMAs: qk_wait stands between the last one and a vector read of S.
    constexpr int NQK = 2 * KS, PF = 4;
    v8 afr[PF];
    auto k_read = [&](int slot, int i) {
        return *(const lds_v8*)(uintptr_t)(koff[i % (KS / 2)] + ((i % KS) / (KS / 2)) * 256 + slot * TILE_BYTES + (i / KS) * HALF_TILE);
    };
    auto qk_begin = [&](int slot) {
#pragma unroll
        for (int i = 0; i < PF; ++i) afr[i] = k_read(slot, i);
    };
    auto qk_one = [&](auto ic, int slot, f32x16 (&s)[2]) {
        constexpr int i = decltype(ic)::value, kb = i / KS, ks = i % KS;
        if constexpr (ks == 0) M::s0(s[kb], afr[i % PF], qf[ks]);
        else M::s(s[kb], afr[i % PF], qf[ks]);
        if constexpr (i + PF < NQK) afr[i % PF] = k_read(slot, i + PF);
    };
    auto qk_wait = [&]() { asm volatile("s_nop 15\n\ts_nop 15" ::: "memory"); };
    auto qk_tile = [&](int slot, f32x16 (&s)[2]) {          // on its own: the prologue, and a wave's first tile behind the block's first
        qk_begin(slot);
        w4_for<NQK>([&](auto ic) { qk_one(ic, slot, s); });
        qk_wait();
    };
    // ---- the masks of one tile, the row max and the deferred-max decision: everything in front of the exponentials ----
    auto softmax_front = [&](f32x16 (&s)[2], int key_base) {
        // wave-uniform test: only the tiles on the wave's causal diagonal, the batch's last tile and the window's lower edge pay
        const bool need_mask = (key_base + BLOCK_N > kv_len) || (CAUSAL && key_base + BLOCK_N - 1 > wave_q0 + off) ||
                               (WINDOW && key_base < wave_lo_last);
        if (need_mask) {
            asm volatile("" ::: "memory");   // keep this a real (wave-uniform) branch
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int key = key_base + 32 * kb + (e & 3) + 8 * (e >> 2) + 4 * h;
                    bool ok = key < kv_len;
                    if (CAUSAL) ok = ok && (key <= my_lim);
                    if constexpr (WINDOW) ok = ok && (key > my_lim - p.window);
                    s[kb][e] = ok ? s[kb][e] : -INFINITY;
                }
        }
        float mx = max16_first(s[0]);
        mx = max16_next(mx, s[1]);
        mx = row_pair_max_asm(mx);
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
    };
    // ---- the exponentials, the row sum's share and P as the B operand (hi, and lo with SPLITP): fragment f = 2 kb + s2.  One element per
    // step, 32 steps; beside(step) is what the caller issues in front of each: nothing, or one QK^T MFMA of the next tile, in whose
    // shadow the step's vector work then runs (the scheduling barriers keep it there).  The arithmetic is the same either way.
    auto softmax_exp = [&](f32x16 (&s)[2], v8 (&ph)[4], v8 (&pl)[4], auto&& beside) {
        float psum0 = 0.f, psum1 = 0.f;
        w4_for<32>([&](auto ic) {
            constexpr int i = decltype(ic)::value, kb = i / 16, e = i % 16, f = 2 * kb + e / 8;
            beside(ic);
            const float pv = fast_exp2(__builtin_fmaf(s[kb][e], c, -mc));
            if constexpr (kb == 0) psum0 += pv;
            else psum1 += pv;
            const T hi = (T)pv;
            ph[f][e % 8] = hi;
            if (SPLITP) pl[f][e % 8] = (T)(pv - (float)hi);
        });
        l_run += psum0 + psum1;
    };
    // ---- O^T += V^T P^T from V slot SLOT ----
    auto pv_tile = [&](auto slotc, const v8 (&ph)[4], const v8 (&pl)[4]) {
        constexpr int SLOT = decltype(slotc)::value;
        const lds_char* vimg = (const lds_char*)(uintptr_t)(SLOT * TILE_BYTES);     // voff[] carries the LDS base
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            const int koffs = (f >> 1) * HALF_TILE + (f & 1) * 16 * 512;            // 16 rows further: the same swizzle term
#pragma unroll
            for (int db = 0; db < DB; ++db) {
                const v4 lo = E::tr_read(vimg + voff[db % (DB / 2)][0] + (db / (DB / 2)) * 256 + koffs);
                const v4 hi4 = E::tr_read(vimg + voff[db % (DB / 2)][1] + (db / (DB / 2)) * 256 + koffs);
                v8 a;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    a[e] = lo[e];
                    a[4 + e] = hi4[e];
                }
                o[db] = E::mfma(a, ph[f], o[db]);
                if (SPLITP) o[db] = E::mfma(a, pl[f], o[db]);
            }
        }
    };
    // this wave's DMA pieces have landed and its LDS reads are done; then everybody's
    auto publish = [&]() {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_waitcnt(0xC07F);
        __builtin_amdgcn_s_barrier();
    };

    // ---- step j, PAR = (j - j_lo) & 1: K(j + 1) has landed in K slot PAR ^ 1, V(j) in V slot PAR, and sc holds S^T(j) if the wave
    // computes tile j.  sn receives S^T(j + 1).
    auto step = [&](auto parc, int j, f32x16 (&sc)[2], f32x16 (&sn)[2]) {
        constexpr int PAR = decltype(parc)::value;
        if (j + 1 < nt) dma_v(IC<PAR ^ 1>{}, j + 1);          // V(j - 1)'s slot: its readers finished before the last barrier
        if (j + 2 < nt) dma_k(IC<PAR>{}, j + 2);              // K(j)'s slot likewise
        const bool cur = computes(j), nxt = j + 1 < nt && computes(j + 1);
        if (cur) {
            v8 ph[4], pl[4];
            softmax_front(sc, j * BLOCK_N);
            if (nxt) {
                // S^T(j + 1) on the matrix pipe, one MFMA per step, beside the exponentials of tile j on the vector pipe.  S^T(j + 1)
                // is next read by a vector instruction in step j + 1, the PV MFMAs of this step and a barrier later
                qk_begin(PAR ^ 1);
                softmax_exp(sc, ph, pl, [&](auto ic) {
                    __builtin_amdgcn_sched_barrier(0);
                    qk_one(ic, PAR ^ 1, sn);
                    __builtin_amdgcn_sched_barrier(0);
                });
            } else {
                softmax_exp(sc, ph, pl, [](auto) {});
            }
            pv_tile(parc, ph, pl);
        } else if (nxt) {
            qk_tile(PAR ^ 1, sn);                             // the wave's first tile under a window lies behind the block's first
        }
        publish();
    };

    // ---- prologue: K(j_lo); then V(j_lo) and K(j_lo + 1) under S^T(j_lo) ----
    f32x16 S0[2], S1[2];
    if (j_lo < nt) dma_k(IC<0>{}, j_lo);
    // Q must have LANDED before the loop (else its vmcnt waits drain the K/V prefetch every iteration): into the accumulator half, once
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) asm volatile("" : "+a"(qf[ks]));
    publish();
    if (j_lo < nt) dma_v(IC<0>{}, j_lo);
    if (j_lo + 1 < nt) dma_k(IC<1>{}, j_lo + 1);
    if (j_lo < nt && computes(j_lo)) qk_tile(0, S0);
    publish();
    for (int j = j_lo; j < nt; j += 2) {
        step(IC<0>{}, j, S0, S1);
        if (j + 1 < nt) step(IC<1>{}, j + 1, S1, S0);
    }

    // ---- epilogue: normalise once; a row with no visible key -> zeros, LSE = -inf ------------
    const float l_tot = row_pair_sum(l_run);
    const float inv = l_tot > 0.f ? 1.0f / l_tot : 0.f;
    // VARLEN: the batch's rows start at packed row row0, and the row bound of every store is the batch's own count
    const int64_t o_batch = VARLEN ? (int64_t)row0 * p.o_ss : (int64_t)b * p.o_sb;
    if constexpr (sizeof(OT) == 2) {
        // 16-bit store through LDS (free after the last barrier; a wave uses its own 16 KiB) so that one store instruction covers whole rows
        typedef __attribute__((address_space(3))) u32x4 lds_u32x4_t;
        constexpr int RB = D * 2, CPRW = RB / 16;      // 512 row bytes, 32 chunks per row
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
        store_rows_from_lds<RB>(lbase, lane, (char*)((OT*)p.o + o_batch + (int64_t)hh * p.o_sh + (int64_t)wave_q0 * p.o_ss),
                                p.o_ss * 2, sq - wave_q0);
    } else if (my_q < sq) {        // fp32 rows straight from the accumulators
        OT* orow = (OT*)p.o + o_batch + (int64_t)hh * p.o_sh + (int64_t)my_q * p.o_ss;
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
    if (my_q < sq && p.lse && h == 0) {
        const float lse = l_tot > 0.f ? (m_run * c + __builtin_amdgcn_logf(l_tot)) * 0.6931471805599453f : -INFINITY;
        if constexpr (VARLEN) p.lse[(int64_t)hh * p.total_q + row0 + my_q] = lse;
        else p.lse[((int64_t)b * p.H + hh) * p.Sq + my_q] = lse;
    }
}

}  // namespace pfa

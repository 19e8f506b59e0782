// fa3_mla_prefill_kernel.h -- multi-head latent attention (MLA) prefill in its NON-ABSORBED form for MI355X (gfx950), hand-written HIP:
// packed sequences, a 192-wide q.k made of a 128-wide per-head "nope" key and a 64-wide rotary key that all heads may share, 128-wide
// values (DeepSeek-V2 / V3 / R1, Kimi K2; include/pfa_hip_mla_prefill.h).  No head dim of the other forward kernels says 192 != 128 or a
// key in two tensors, so this is a kernel of its own; Elem, tile_off, lds_dma16_buf, packed_seq, store_rows_from_lds and the softmax
// helpers are fa3_fwd_kernel.h's.
//
//   s[i,h,j] = scale * (<q[i,h,0:128], k_nope[j,h,:]> + <q[i,h,128:192], k_rope[j,hr,:]>),  o[i,h,:] = sum_j softmax_j(s) v[j,h,:]
//
// SEQUENCES.  Sequence b owns the packed rows cu_q[b] .. cu_q[b + 1] - 1 and keys cu_k[b] .. cu_k[b + 1] - 1, both read by the workgroup
// with scalar loads and clamped by packed_seq (bad device data gives wrong numbers, never a row outside the packed tensors); its start
// goes into the 64-bit base pointers.  causal is bottom-right per sequence: with off_b = Lk_b - Lq_b, row i sees key j iff j < Lk_b and
// j <= i + off_b.  off_b < 0: the first -off_b rows see nothing, O = 0 and LSE = -inf, as do all rows at Lk_b = 0.  A block with
// q0 >= Lq_b returns before any load or store.  Every K / V descriptor ends at its tile's last valid key of the SEQUENCE, so a
// neighbour's keys and whatever lies behind cu_k[B] land in LDS as zeros (0 * NaN in the PV product would be NaN), and every store is
// bounded by Lq_b.
//
// WORK SPLIT.  256 query rows per workgroup: 8 waves x 32 rows, two waves per SIMD on the 256-register budget -- the split of
// fa3_prefill_kernel, which the narrower value makes possible where head dim 256 and the MLA decode had to run one wave per SIMD:
// O^T is 4 blocks of 32x32 (64 registers), the resident Q operand 12 k-steps x 4 (48), S of one 64-key tile 32, P 4 (8 with the hi + lo
// pair of an fp32 output) per 16 keys.  The partner wave on the SIMD covers a wave's softmax with its own MFMAs.  Per tile and wave:
// S^T = K Q^T is 2 key blocks x (8 nope + 4 rope) k-steps = 24 MFMAs of v_mfma_f32_32x32x16 behind a ring of four ds_read_b128;
// O^T += V^T P^T is 16 (32 with SPLITP), V^T by ds_read_b64_tr_b16; five LDS-DMA pieces; one barrier.
//
// LDS: 80 KiB dynamic, two buffers of three images fed by LDS-DMA one tile ahead of the math:
//   K_nope  64 keys x 256 B at 0       tile_off<128>: one key per 256-byte row, chunk c at position c ^ sw(R)
//   K_rope  64 keys x 128 B at 16 KiB  tile_off<64>:  two keys per 256-byte row (the odd key in the upper half), chunk 8 (key & 1) + c
//   V       64 keys x 256 B at 24 KiB  tile_off<128>
// with sw(R) = ((R & 3) << 2) | ((R >> 2) & 3).  K arrives in two tensors and stays two images: every image then has rows of exactly one
// 256-byte bank line, and the conflict-freedom arguments of the head dim 128 and 64 images (fa3_fwd_kernel.h) hold unchanged -- the 16
// lanes a ds_read_b128 serves together hold 16 rows at one logical chunk, which sw spreads over the 16 columns of the bank line; the
// four rows of a transposed V read differ in R & 3, which sw moves to bits 2-3 of the position.  One 384-byte row of nope + rope would
// be 1.5 bank lines: rows R and R + 2 then start in the same column and the bijection argument is lost.
// The rope tile is the same bytes for every head of a sequence when k_rope has one head (its head stride is then 0 here): the grid puts
// the heads of one (q block, sequence) side by side, so heads h, h + 8, h + 16 ... run on one XCD at about the same time and read the
// tile from that XCD's L2.
//
// Grid = ceil(max_seqlen_q / 256) * B * H from host shapes, the heaviest (last) q blocks first under the causal flag, key tiles past a
// block's diagonal never fetched and those past a wave's never computed.  No workspace, no atomics: the same bits every run, and a
// sequence's rows are those of a call that holds it alone.
#pragma once
#include "fa3_fwd_kernel.h"

namespace pfa {
namespace mlap {

constexpr int DN = 128;                        // per-head key columns without position ("nope") = q columns 0 .. 127
constexpr int DR = 64;                         // rotary key columns = q columns 128 .. 191
constexpr int DV = 128;                        // value columns
constexpr int WAVES = 8;
constexpr int THREADS = WAVES * 64;
constexpr int BLOCK_M = WAVES * WAVE_M;        // 256 query rows per workgroup
constexpr int KN_BYTES = BLOCK_N * DN * 2;     // 16 KiB
constexpr int KR_BYTES = BLOCK_N * DR * 2;     // 8 KiB
constexpr int V_BYTES = BLOCK_N * DV * 2;      // 16 KiB
constexpr int BUF_BYTES = KN_BYTES + KR_BYTES + V_BYTES;
constexpr int LDS_BYTES = 2 * BUF_BYTES;       // 80 KiB

struct Params {
    const void* q;               // [total_q, H, 192] by (row, head) element strides
    const void* kn;              // [total_k, H, 128]
    const void* kr;              // [total_k, 1 or H, 64]; kr_sh = 0 when one head serves all
    const void* v;               // [total_k, H, 128]
    void* o;                     // [total_q, H, 128]
    float* lse;                  // optional [H, total_q]
    const int32_t* cu_q;         // [B + 1] on the device
    const int32_t* cu_k;
    int64_t q_ss, q_sh, kn_ss, kn_sh, kr_ss, kr_sh, v_ss, v_sh, o_ss, o_sh;
    int32_t B, H, total_q, total_k, max_q, max_k;
    int32_t nqblk;               // ceil(max_q / 256)
    float scale_log2;            // softmax_scale * log2(e)
};

template <typename T, bool CAUSAL, bool SPLITP, typename OT>
__global__ __launch_bounds__(THREADS, 2) void fa3_mla_prefill_kernel(const Params p) {
    using E = Elem<T>;
    using v8 = typename E::v8;
    using v4 = typename E::v4;
    typedef __attribute__((address_space(3))) v8 lds_v8;
    constexpr int NW = WAVES;
    constexpr int KSN = DN / 16, KSR = DR / 16, KS = KSN + KSR;   // 8 + 4 k-steps of the QK^T product
    constexpr int DB = DV / 32;                                   // 4 d blocks of the PV product
    constexpr int KR_BASE = KN_BYTES, V_BASE = KN_BYTES + KR_BYTES;

    extern __shared__ __attribute__((aligned(16))) char smem[];
    const uint32_t smem_base = (uint32_t)(uintptr_t)(lds_char*)smem;   // LDS byte address (wave-uniform)

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31;
    const int h = lane >> 5;

    // ---- block -> (q block, sequence, head): heads fastest, heaviest (longest causal row) q blocks first ----
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

    // ---- the sequence's rows and keys, from the device (clamped) ----
    const PackedSeq rows = packed_seq(p.cu_q, b, p.total_q, p.max_q);
    const int row0 = __builtin_amdgcn_readfirstlane(rows.start);
    const int sq = __builtin_amdgcn_readfirstlane(rows.len);
    if (q0 >= sq) return;                                // nothing of this sequence in the block: no load, no store
    const PackedSeq keys = packed_seq(p.cu_k, b, p.total_k, p.max_k);
    const int key0 = __builtin_amdgcn_readfirstlane(keys.start);
    const int kv_len = __builtin_amdgcn_readfirstlane(keys.len);
    const bool wave_has_rows = wave_q0 < sq;

    const int off = kv_len - sq;                         // row i sees key j iff j <= i + off (may be negative)
    const int kv_end = CAUSAL ? max(0, min(kv_len, q0 + BLOCK_M + off)) : kv_len;       // keys the block needs
    const int wave_kv_end = !wave_has_rows ? 0 : CAUSAL ? min(kv_len, wave_q0 + WAVE_M + off) : kv_len;   // keys this wave needs (<= 0: none)
    const int my_lim = my_q + off;                       // last key this row sees under the causal cut
    const int nt = (kv_end + BLOCK_N - 1) / BLOCK_N;

    // the sequence's first row and key in the 64-bit bases: every 32-bit offset below is relative to a tile of this sequence
    const T* __restrict__ qp = (const T*)p.q + (int64_t)row0 * p.q_ss + (int64_t)hh * p.q_sh;
    const char* knp = (const char*)p.kn + ((int64_t)key0 * p.kn_ss + (int64_t)hh * p.kn_sh) * 2;
    const char* krp = (const char*)p.kr + ((int64_t)key0 * p.kr_ss + (int64_t)hh * p.kr_sh) * 2;
    const char* vp = (const char*)p.v + ((int64_t)key0 * p.v_ss + (int64_t)hh * p.v_sh) * 2;

    // ---- Q fragments: B operand of S^T = K Q^T, lane (r,h) holds Q[my_q][16 ks + 8 h .. +7]; k-steps 8 .. 11 are the rotary columns ----
    v8 qf[KS];
    {
        const int qrow = min(my_q, sq - 1);
        const T* src = qp + (int64_t)qrow * p.q_ss + 8 * h;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) qf[ks] = *(const v8*)(src + 16 * ks);
    }

    // ---- K / V staging by LDS-DMA: a piece is 1 KiB = four 256-byte LDS rows, the swizzle applied to each lane's SOURCE chunk.  Wave w
    // issues pieces w and w + 8 of the nope and the V image (LDS rows 4 w .. and 32 + 4 w ..: one key each) and piece w of the rope image
    // (LDS rows 4 w ..: two keys each).  Rows 32 apart share the swizzle term.
    uint32_t knoff[2], vvoff[2], kroff;                  // per-lane byte offsets from the tile's first key row, loop invariant
    {
        const int R0 = 4 * wave + (lane >> 4);
        const int sw = ((R0 & 3) << 2) | ((R0 >> 2) & 3);
        const int cc = (lane & 15) ^ sw;                 // logical chunk stored at this lane's position
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            knoff[t] = (uint32_t)((R0 + 4 * NW * t) * (int)p.kn_ss + cc * 8) * 2u;
            vvoff[t] = (uint32_t)((R0 + 4 * NW * t) * (int)p.v_ss + cc * 8) * 2u;
        }
        kroff = (uint32_t)((2 * R0 + (cc >> 3)) * (int)p.kr_ss + (cc & 7) * 8) * 2u;
    }
    // tile j into buffer BUF; the three descriptors end at the tile's last valid key of this sequence: rows behind it read as zeros
    auto dma_tile = [&](auto bufc, int j) {
        constexpr int BUF = decltype(bufc)::value;
        const int nk = min(BLOCK_N, kv_len - j * BLOCK_N);
        const int64_t first = (int64_t)j * BLOCK_N;
        const srd_t nsrd = __builtin_amdgcn_make_buffer_rsrc((void*)(knp + first * p.kn_ss * 2), 0, (int)((int64_t)(nk - 1) * p.kn_ss * 2 + DN * 2), 0x00020000);
        const srd_t rsrd = __builtin_amdgcn_make_buffer_rsrc((void*)(krp + first * p.kr_ss * 2), 0, (int)((int64_t)(nk - 1) * p.kr_ss * 2 + DR * 2), 0x00020000);
        const srd_t vsrd = __builtin_amdgcn_make_buffer_rsrc((void*)(vp + first * p.v_ss * 2), 0, (int)((int64_t)(nk - 1) * p.v_ss * 2 + DV * 2), 0x00020000);
        const uint32_t dst = smem_base + BUF * BUF_BYTES + wave * 1024;
#pragma unroll
        for (int t = 0; t < 2; ++t) lds_dma16_buf(nsrd, knoff[t], dst + NW * t * 1024);
        lds_dma16_buf(rsrd, kroff, dst + KR_BASE);
#pragma unroll
        for (int t = 0; t < 2; ++t) lds_dma16_buf(vsrd, vvoff[t], dst + V_BASE + NW * t * 1024);
    };

    // ---- per-lane LDS read addresses, loop invariant and opaque (the compiler otherwise rebuilds row and chunk parts every tile).  Key
    // block 1 (keys 32 ..) lies 32 nope / V rows or 16 rope rows further, where the swizzle term repeats: an immediate offset
    uint32_t koffn[KSN], koffr[KSR];
#pragma unroll
    for (int ks = 0; ks < KSN; ++ks) {
        koffn[ks] = smem_base + tile_off<DN>(r, 2 * ks + h);
        asm volatile("" : "+v"(koffn[ks]));
    }
#pragma unroll
    for (int ks = 0; ks < KSR; ++ks) {
        koffr[ks] = smem_base + KR_BASE + tile_off<DR>(r, 2 * ks + h);
        asm volatile("" : "+v"(koffr[ks]));
    }
    const int g1 = (lane >> 4) & 1;
    const int tq = (lane & 15) >> 2;
    const int tp = lane & 3;
    uint32_t voff[DB][2];
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
        for (int hi = 0; hi < 2; ++hi) {
            voff[db][hi] = smem_base + V_BASE + tile_off<DV>(4 * h + tq + 8 * hi, db * 4 + 2 * g1 + (tp >> 1)) + 8 * (tp & 1);
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

    // ---- one tile: S^T = K_nope Q_nope^T + K_rope Q_rope^T, online softmax, O^T += V^T P^T ----
    auto compute_tile = [&](auto bufc, int key_base) {
        constexpr int BUF = decltype(bufc)::value;
        const lds_char* img = (const lds_char*)(uintptr_t)(BUF * BUF_BYTES);    // koffn[] / koffr[] / voff[] carry the LDS base

        // fragment i of the 24: key block i / 12, k-step i % 12 -- the nope image for k-steps 0 .. 7, the rope image behind them
        auto k_frag = [&](int i) {
            const int kb = i / KS, ks = i % KS;
            return ks < KSN ? *(const lds_v8*)(img + koffn[ks] + kb * (KN_BYTES / 2)) : *(const lds_v8*)(img + koffr[ks - KSN] + kb * (KR_BYTES / 2));
        };
        f32x16 s[2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int e = 0; e < 16; ++e) s[kb][e] = 0.f;
        constexpr int NQK = 2 * KS, PF = 4;
        v8 afr[PF];
#pragma unroll
        for (int i = 0; i < PF; ++i) afr[i] = k_frag(i);
#pragma unroll
        for (int i = 0; i < NQK; ++i) {
            s[i / KS] = E::mfma(afr[i % PF], qf[i % KS], s[i / KS]);
            if (i + PF < NQK) afr[i % PF] = k_frag(i + PF);
        }
        // pin the read / MFMA interleave: PF reads, then one MFMA per read, then the last PF MFMAs
        __builtin_amdgcn_sched_group_barrier(0x100, PF, 0);
#pragma unroll
        for (int i = 0; i < NQK - PF; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        }
        __builtin_amdgcn_sched_group_barrier(0x008, PF, 0);

        // mask: wave-uniform test, only the tiles on the wave's causal diagonal and the sequence's last tile pay
        const bool need_mask = (key_base + BLOCK_N > kv_len) || (CAUSAL && key_base + BLOCK_N - 1 > wave_q0 + off);
        if (need_mask) {
            asm volatile("" ::: "memory");   // keep this a real (wave-uniform) branch, not 32 v_cmp + 32 v_cndmask on every tile
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int key = key_base + 32 * kb + (e & 3) + 8 * (e >> 2) + 4 * h;
                    bool ok = key < kv_len;
                    if (CAUSAL) ok = ok && (key <= my_lim);
                    s[kb][e] = ok ? s[kb][e] : -INFINITY;
                }
        }

        // online softmax in the log2 domain; a row lives in lanes (l, l ^ 32)
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

        // O^T += V^T P^T: 16 keys per step, P as the B operand (hi, and lo with SPLITP)
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
                const int koffs = kb * (V_BYTES / 2) + s2 * 16 * 256;
#pragma unroll
                for (int db = 0; db < DB; ++db) {
                    const v4 lo = E::tr_read(img + voff[db][0] + koffs);
                    const v4 hi4 = E::tr_read(img + voff[db][1] + koffs);
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
        if (j + 1 < nt) dma_tile(IC<BUF ^ 1>{}, j + 1);   // lands in the other buffer under this tile's math
        if (j * BLOCK_N < wave_kv_end) compute_tile(bufc, j * BLOCK_N);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's DMA pieces have landed ...
        __builtin_amdgcn_s_waitcnt(0xC07F);               // (lgkmcnt(0): this wave's LDS reads are done)
        __builtin_amdgcn_s_barrier();                     // ... and so have everybody else's
    };

    if (nt > 0) dma_tile(IC<0>{}, 0);
    // Q must have LANDED before the loop (else its vmcnt waits drain the K/V prefetch every iteration)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) asm volatile("" : "+v"(qf[ks]));
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int j = 0; j < nt; j += 2) {
        step(IC<0>{}, j);
        if (j + 1 < nt) step(IC<1>{}, j + 1);
    }

    // ---- epilogue: normalise once; a row with no visible key -> zeros, LSE = -inf.  Every store is bounded by the sequence's own rows ----
    const float l_tot = row_pair_sum(l_run);
    const float inv = l_tot > 0.f ? 1.0f / l_tot : 0.f;
    OT* const obase = (OT*)p.o + (int64_t)row0 * p.o_ss + (int64_t)hh * p.o_sh;
    if constexpr (sizeof(OT) == 2) {
        // 16-bit store through LDS (free after the loop's last barrier; a wave uses its own 8 KiB) so that one store covers whole rows
        typedef __attribute__((address_space(3))) u32x4 lds_u32x4_t;
        constexpr int RB = DV * 2, CPRW = RB / 16;      // 256 row bytes, 16 chunks per row
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
        store_rows_from_lds<RB>(lbase, lane, (char*)(obase + (int64_t)wave_q0 * p.o_ss), p.o_ss * 2, sq - wave_q0);
    } else if (my_q < sq) {        // fp32 rows straight from the accumulators
        OT* orow = obase + (int64_t)my_q * p.o_ss;
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
    if (my_q < sq && p.lse && h == 0)
        p.lse[(int64_t)hh * p.total_q + row0 + my_q] = l_tot > 0.f ? (m_run * c + __builtin_amdgcn_logf(l_tot)) * 0.6931471805599453f : -INFINITY;
}

}  // namespace mlap
}  // namespace pfa

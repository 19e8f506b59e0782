// fa3_prefill_kernel.h -- compute-bound forward over a KV cache (contiguous or paged) for MI355X (gfx950), hand-written HIP.
//
// Chunked prefill, the suffix of a prefix-cached prompt, speculative verification: Sq new query rows per batch (any number) against
// the len_b keys a cache holds, bottom-right causal.  The schedule is the 8-wave forward's (fa3_fwd_kernel.h: 256 Q rows per
// workgroup, one wave per 32 rows, 64-key K/V tiles in two LDS buffers fed by LDS-DMA, swapped products on the 32x32x16 MFMA, V^T by
// ds_read_b64_tr_b16, deferred-max online softmax, SPLITP for the fp32 output); that header supplies Elem, tile_off, lds_dma16_buf,
// store_rows_from_lds and the softmax helpers.  The kernel differs from fa3_fwd_kernel in three places:
//   1. Length and causal offset come from the device: len_b = clamp(cache_seqlens[b], 0, Smax) (Smax without lengths), off_b =
//      len_b - Sq; row i sees key j iff j < len_b and (causal) j <= i + off_b -- the convention of pfa_fa3_decode_args.causal.  A
//      block runs tiles up to min(len_b, q0 + 256 + off_b), a wave computes those below min(len_b, wave_q0 + 32 + off_b).  off_b < 0
//      (len_b < Sq): the first -off_b rows see nothing, O = 0 and LSE = -inf; a block with no visible key runs no tile and writes
//      its zeros.
//   2. PAGED: the cache is a pool of pages and a device block table (DecodeParams' convention: k_sb / v_sb are the page strides).
//      page_size is a multiple of 64, so a tile lies inside one page: dma_tile takes one wave-uniform table entry, fetched by a scalar
//      load when the PREVIOUS tile's DMA was issued (no dependent load in front of a tile's DMA), clamps it to [0, num_pages - 1] and
//      builds both descriptors from the page's base.  Tiles are visited in order, so page index and token offset advance by
//      addition.  Nothing else in the kernel knows about pages: a paged call returns the bits of the contiguous call on the
//      gathered cache.
//   3. Each tile's K and V descriptor ends at the tile's last valid key (< len_b), not at Smax: rows at and past len_b land in LDS
//      as zeros.  The score mask alone is not enough over a cache, whose unfilled tail or half-used last page may hold NaN, and
//      0 * NaN in the PV MFMA is NaN.  Table entries at and past ceil(len_b / page_size) are never read (a tile exists only below
//      len_b).
// Grid = B * H * ceil(Sq / 256) from shapes alone, no workspace, no atomics: capturable, and valid while lengths, table and cache
// change between replays.  These instantiations do not split the keys: a short chunk with few B * H leaves CUs idle;
// SPLIT below is the mode that does.
//
// VARLEN (pfa_fa3_prefill_varlen): every batch brings its own number of query rows.  Q, O are packed [total_q, H, D] (no batch
// stride), LSE is [H, total_q], and a device int32 cu_seqlens_q[B + 1] says where each batch's rows start.  The schedule, the tile
// loop and the grid (B * H * ceil(max_seqlen_q / 256), p.Sq holding max_seqlen_q) are the uniform kernel's; the prologue and the
// stores differ:
//   - s_b = clamp(cu[b], 0, total_q), e_b = clamp(cu[b + 1], s_b, total_q), Sq_b = min(e_b - s_b, max_seqlen_q), off_b = len_b - Sq_b,
//     all wave-uniform.  Bad device data gives wrong numbers, never a row outside the packed tensors.
//   - a block with q0 >= Sq_b returns before any load or store (every block of an empty batch does);
//   - row i of batch b is packed row s_b + i, and every store is bounded by Sq_b: the packed row behind a batch's last row is the
//     next batch's first.  Rows no batch covers (gaps, the tail behind cu[B], rows past max_seqlen_q) are never written;
//   - a wave with wave_q0 >= Sq_b has no rows: it issues its DMA pieces and meets the barriers but computes no tile (the uniform
//     kernel runs such a wave on copies of the last row).  Nothing it holds is stored.
// The Q clamp (row min(my_q, Sq_b - 1)) and therefore the rescale points of the wave-wide deferred max are those of the uniform kernel
// at Sq = Sq_b, so a ragged call returns the bits of per-batch uniform calls.
//
// WINDOW (pfa_fa3_prefill_ex / pfa_fa3_prefill_varlen_ex with a window W; CAUSAL only, PrefillWindowPart carries W, clamped to Smax by the
// host): row i sees key j iff j < len_b, j <= i + off_b and j > i + off_b - W.  What changes:
//   - a block's first tile is j_lo = max(0, q0 + off_b - W + 1) / 64 and its loop runs j_lo .. nt - 1.  Tiles below it are never
//     fetched, so keys below floor64(max(0, off_b - W + 1)) -- block 0's first tile -- are never read by anybody;
//   - a wave computes no tile that lies wholly below its first row's bound wave_q0 + off_b - W + 1, as it computes none above
//     wave_kv_end: it issues its DMA pieces and meets the barriers.  Its first computed tile need not be the block's first, and a
//     row's first visible key may lie in a later tile than the wave's first: such a row carries m_run = -1e30, l = 0, O = 0 through
//     tiles whose scores are all -inf (exp2(-inf) = 0, and the wave-wide rescale another row asks for multiplies its zeros by
//     exp2(0) = 1), and its first finite score rescales them by exp2(-huge) = 0.  The same holds for the rows of len_b < Sq_b;
//   - the lower bound is applied to the scores only on tiles that reach below the wave's LAST row's bound (need_mask grows by one
//     wave-uniform term); a tile inside every row's window takes the unmasked path;
//   - PAGED: dma_tile starts at table entry 64 j_lo / page_size, token 64 j_lo % page_size (one division in the prologue) and
//     advances by addition as before; the first scalar table load is that entry, and entries below it are never read.
// WINDOW = false compiles to the code and the kernel arguments the instantiation had.
//
// SPLIT (pfa_fa3_prefill_split with N = nsplit > 1 key splits; uniform only -- no VARLEN, no WINDOW; PrefillSplitPart carries nsplit and the
// two workspace bases): the keys of a q block are cut over N workgroups, each writes an fp32 partial result, and pfa_attn_merge joins
// the N parts in split order.  What changes:
//   - grid B * H * nqblk * N from host shapes; blockIdx = ((qrank * B * H) + bh) * N + s.  The q-block rank stays the slowest index,
//     so the heaviest causal blocks still start first; the split s is the FASTEST, so the blocks that stream the same K/V tiles -- the
//     H / Hkv query heads of one K/V head at one split -- are N apart in blockIdx and, blocks being dealt round-robin over the 8 XCDs,
//     share an XCD's L2 at N = 8 (every second one at N = 4, every fourth at N = 2); the splits of one q block share no key;
//   - THE SPLIT RULE: with n the 64-key tiles the block would run unsplit (nt, from kv_end: per q block under the causal flag) and
//     per = ceil(n / N), split s runs tiles [s * per, min(n, (s + 1) * per)).  An empty range runs no tile and fetches nothing.  Inside
//     its range the block is the unsplit kernel: wave_kv_end skips a wave's tiles above its rows, descriptors end at the last valid key,
//     need_mask is computed on global key indices -- the partial result of split s is, bit for bit, the fp32 result of the unsplit
//     kernel on the key slice [64 s per, 64 min(n, (s + 1) per)) with the length clamp(len_b - 64 s per, 0, slice);
//   - PAGED: dma_tile starts at table entry 64 s per / page_size, token 64 s per % page_size (one division in the prologue, as WINDOW
//     does for j_lo) and advances by addition: a split may begin in the middle of a page.  Entries outside the split's tiles, and those
//     at or past ceil(len_b / page_size), are never read;
//   - the output is always fp32 from the accumulators (SPLITP, OT = float), into the workspace: partial O [N][B][Sq][H][D], partial
//     LSE [N][B][H][Sq].  p.o, p.lse and the o strides are not used.  Every split writes O and LSE of every row below Sq; a row with
//     no visible key in the split's range (an empty range, rows above the range under the causal cut, len_b < Sq) gets O = 0 and
//     LSE = -inf from the epilogue below, and the merge skips such a part.
// SPLIT = false compiles to the code and the kernel arguments the instantiation had.
//
// KV8 (pfa_fa3_prefill_q8 / pfa_fa3_prefill_varlen_q8; no WINDOW, no SPLIT; PrefillKv8Part carries the descales): the cache holds OCP
// e4m3fn bytes, one per element -- strides in elements = bytes, every stride a multiple of 16, 16-byte bases -- and an element stands for
// e4m3(byte) * descale[b * ds_sb + kvh].  LDS-DMA cannot widen a byte, so the tiles are staged through registers, one tile ahead of the
// LDS image and two ahead of the math.  What changes:
//   - THE CONTRACT: the K and V images in LDS are, byte for byte, the images the 16-bit kernel builds from cache.to(T) (cvt_e4m3x8 is
//     exact).  Everything behind the images -- fragments, V^T reads, MFMAs, masks, softmax, epilogue -- is the one code path;
//   - a tile of K (and of V) is 64 * D bytes: at D = 128 every lane loads 16 bytes of K and 16 of V (key tid / 8, bytes 16 (tid % 8) ..),
//     at D = 64 one load, waves 0-3 of K and waves 4-7 of V (key (tid % 256) / 4).  A load is two 8-element chunks 2c, 2c + 1 of one key,
//     which tile_off puts 16 bytes apart in one LDS row: two ds_write_b128 after the conversion.  8 (4) staging VGPRs;
//   - the loads go through descriptors that end at the tile's last valid key, difference (3) above with byte counts: a row at or past
//     len_b reads as 0x00 = +0.0 and a NaN byte behind a length never reaches LDS;
//   - step j: convert the held tile j + 1 into buffer BUF ^ 1 (its last readers finished in front of the barrier that ended step j - 1),
//     issue the loads of tile j + 2 into the freed registers, compute tile j from BUF, lgkmcnt(0), barrier -- so the reads of a tile
//     come after a barrier that follows its writers' lgkmcnt(0).  There is no vmcnt wait at the barrier: the compiler places the one
//     the conversion needs, a whole tile's math behind the loads.  A wave that computes no tile (VARLEN idle, above the causal cut)
//     still stages its share and meets every barrier;
//   - PAGED: load8 is dma_tile's walk (one scalar entry per tile, fetched when the previous tile's loads were issued, clamped), called
//     for j = 0, 1, ... < nt in order; that it runs two tiles ahead of the math changes no guard: the entry of tile j + 1 is fetched only
//     if j + 1 < nt;
//   - the descales are two scalar loads in the prologue: k_descale multiplies scale_log2 before thr, mc and the LSE are derived from it,
//     v_descale multiplies inv once in the epilogue.  Both are exact at 1: the call then returns the bits of the 16-bit call on the
//     converted cache.
// KV8 = false compiles to the code and the kernel arguments the instantiation had.
//
// SINK (pfa_fa3_prefill_sink / _varlen_sink / _split_sink; uniform, VARLEN and SPLIT, with and without WINDOW; no KV8; PrefillSinkPart
// carries the pointer): an attention sink, one fp32 value per QUERY head in the units of the scaled scores, is one more key with that
// score and a zero value row.  The tile loop and everything in front of it are untouched; a workgroup serves one head, so the sink is one
// scalar load in the prologue.  The epilogue, with mc = m_run * c the deferred-max reference in log2 units and s2 = sinks[hh] * log2(e):
//     M' = max(mc, s2),  l' = l_tot * exp2(mc - M') + exp2(s2 - M'),  inv = exp2(mc - M') / l',  LSE = (M' + log2 l') ln 2.
//   - a row with no visible key has l_tot = 0 and mc = -1e30 c: M' = s2, the first factor is 0, l' = 1 -- O = 0 exactly and LSE = sink;
//   - s2 = -inf: M' = mc, the factors are exactly 1 and 0, l' = l_tot and inv = (1 / l_tot) * 1 -- O keeps the bits of the sink-less
//     kernel, and a row without keys keeps l' = 0, O = 0, LSE = -inf.  The LSE is written as fma(m_run, c, log2 l') ln 2 where the
//     keys hold the maximum (M' = mc) and as (s2 + log2 l') ln 2 where the sink does: the first is the sink-less kernel's value on l',
//     so at s2 = -inf the LSE -- and through a split's partial LSE the merged O -- keeps its bits as well;
//   - SPLIT: only the workgroup of split 0 takes the sink (the others take s2 = -inf), so exactly one part carries it into the merge,
//     and split 0's partial LSE is finite even when it runs no tile;
//   - VARLEN idle waves and rows past sq store nothing, as before.
// SINK = false compiles to the code and the kernel arguments the instantiation had.
#pragma once
#include "fa3_fwd_kernel.h"
#include "fp8_cvt.h"
#include "param_parts.h"

namespace pfa {

struct PrefillParams {
    const void* q;
    const void* k;               // cache [B, Smax, Hkv, D] by strides, or (PAGED) pool [num_pages, page_size, Hkv, D]
    const void* v;
    void* o;
    float* lse;                  // optional [B, H, Sq]
    const int32_t* seqlens;      // optional [B]
    int64_t q_sb, q_sh, q_ss;    // element strides
    int64_t k_sb, k_sh, k_ss;    // PAGED: k_sb / v_sb are the page strides
    int64_t v_sb, v_sh, v_ss;
    int64_t o_sb, o_sh, o_ss;
    int32_t B, H, Sq, Smax;
    int32_t nqblk;               // ceil(Sq / 256)
    int32_t kv_group;            // H / Hkv
    float scale_log2;            // softmax_scale * log2(e)
    const int32_t* block_table;  // PAGED: [B][max_pages] page ids
    int64_t bt_sb;
    int32_t page_size, num_pages;
};

// The mode flags' parts, behind the base in this order.  VARLEN: q_sb / o_sb are unused, Sq is max_seqlen_q, lse is [H, total_q]
struct PrefillVarlenPart : TailPaddingReused {   // (window stands in its padding)
    const int32_t* cu_seqlens_q; // [B + 1] packed row of each batch's first query row
    int32_t total_q;             // rows of the packed q / o
};
// WINDOW: the sliding window, 1 <= window <= Smax
struct PrefillWindowPart {
    int32_t window;
};
// SPLIT: the key splits (2 .. 8) and the workspace, partial O [nsplit][B][Sq][H][D] and partial LSE [nsplit][B][H][Sq], both fp32
struct PrefillSplitPart {
    int32_t nsplit;
    float* part_o;
    float* part_lse;
};
// KV8: fp32 descales, k_descale[b * ds_sb + kvh] (ds_sb = 0: one row for every batch)
struct PrefillKv8Part {
    const float* k_descale;
    const float* v_descale;
    int64_t ds_sb;
};
// SINK: one fp32 sink per query head, sinks[h], in the units of the scaled scores (natural log)
struct PrefillSinkPart {
    const float* sinks;
};
template <bool VARLEN, bool WINDOW, bool SPLIT, bool KV8, bool SINK>
struct PrefillBlock : PrefillParams, PartIf<VARLEN, PrefillVarlenPart>, PartIf<WINDOW, PrefillWindowPart>, PartIf<SPLIT, PrefillSplitPart>,
                      PartIf<KV8, PrefillKv8Part>, PartIf<SINK, PrefillSinkPart> {};
template <bool VARLEN, bool WINDOW = false, bool SPLIT = false, bool KV8 = false, bool SINK = false>
struct PrefillParamsOf { typedef PrefillBlock<VARLEN, WINDOW, SPLIT, KV8, SINK> type; };

// Which instantiations of fa3_prefill_kernel exist: the one statement of it, for the kernel, its table and the host's dispatch.
constexpr bool prefill_kernel_exists(bool CAUSAL, bool SPLITP, int out_bytes, bool VARLEN, bool WINDOW, bool SPLIT, bool KV8, bool SINK) {
    return !(SINK && KV8)                               // the sink is built for the 16-bit cache
           && !(KV8 && (WINDOW || SPLIT))               // the FP8 cache takes neither a window nor a split over keys
           && (CAUSAL || !WINDOW)                       // the window is cut from the causal diagonal
           && !(SPLIT && (VARLEN || WINDOW))            // the split over keys is for the uniform, window-less call
           && (!SPLIT || (SPLITP && out_bytes == 4));   // the partial results are fp32, P carried as hi + lo
}

typedef const __attribute__((address_space(4))) int32_t* prefill_table_ptr;   // read-only for the kernel's lifetime: scalar loads
typedef const __attribute__((address_space(4))) float* prefill_f32_ptr;

template <typename T, int D, bool CAUSAL, bool SPLITP, bool PAGED, typename OT, bool VARLEN = false, bool WINDOW = false, bool SPLIT = false,
          bool KV8 = false, bool SINK = false>
__global__ __launch_bounds__(FWD_THREADS, 2) void fa3_prefill_kernel(const typename PrefillParamsOf<VARLEN, WINDOW, SPLIT, KV8, SINK>::type p) {
    static_assert(prefill_kernel_exists(CAUSAL, SPLITP, sizeof(OT), VARLEN, WINDOW, SPLIT, KV8, SINK), "no such mode set: see prefill_kernel_exists");
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
    constexpr int EB = KV8 ? 1 : 2;           // bytes per cache element

    extern __shared__ __attribute__((aligned(16))) char smem[];
    lds_char* const smem_l = (lds_char*)smem;   // [buf][K|V][TILE_BYTES]
    const uint32_t smem_base = (uint32_t)(uintptr_t)smem_l;   // LDS byte address (wave-uniform)

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31;
    const int h = lane >> 5;

    // ---- block -> (q block, batch*head): heaviest (longest causal row) blocks first ----------------
    // SPLIT: the key split is the fastest index (see the header)
    const int BH = p.B * p.H;
    int n = blockIdx.x;
    int split = 0;
    if constexpr (SPLIT) {
        const int item = n;
        n = item / p.nsplit;
        split = item - n * p.nsplit;
    }
    const int qrank = n / BH;
    const int bh = n - qrank * BH;
    const int qblk = CAUSAL ? (p.nqblk - 1 - qrank) : qrank;
    const int b = bh / p.H;
    const int hh = bh - b * p.H;

    const int q0 = qblk * BLOCK_M;
    const int wave_q0 = q0 + wave * WAVE_M;
    const int my_q = wave_q0 + r;

    // ---- VARLEN: the batch's rows in the packed tensors, from the device (clamped: never a row outside them) ----
    int sq = p.Sq;                                       // query rows of this batch
    int row0 = 0;                                        // packed row of its first
    if constexpr (VARLEN) {
        const int s_b = min(max(p.cu_seqlens_q[b], 0), p.total_q);
        const int e_b = min(max(p.cu_seqlens_q[b + 1], s_b), p.total_q);
        row0 = __builtin_amdgcn_readfirstlane(s_b);
        sq = __builtin_amdgcn_readfirstlane(min(e_b - s_b, p.Sq));
        if (q0 >= sq) return;                            // nothing of this batch in the block: no load, no store
    }
    const bool wave_has_rows = !VARLEN || wave_q0 < sq;

    // ---- (1) the batch's length and causal offset, from the device ----------------------------------
    int kv_len = p.Smax;
    if (p.seqlens) kv_len = min(kv_len, max(p.seqlens[b], 0));
    kv_len = __builtin_amdgcn_readfirstlane(kv_len);
    const int off = kv_len - sq;                         // row i sees key j iff j <= i + off (may be negative)
    const int kv_end = CAUSAL ? max(0, min(kv_len, q0 + BLOCK_M + off)) : kv_len;       // keys the block needs
    const int wave_kv_end = !wave_has_rows ? 0 : CAUSAL ? min(kv_len, wave_q0 + WAVE_M + off) : kv_len;   // keys this wave needs (<= 0: none)
    const int my_lim = my_q + off;                       // last key this row sees under the causal cut
    int nt = (kv_end + BLOCK_N - 1) / BLOCK_N;
    // WINDOW: the block's first tile (j_lo < nt whenever nt > 0: q0 < sq puts the block's lowest bound below kv_end), the lowest
    // key the wave's first row sees, and the lowest its last row sees (both may be negative)
    int j_lo = 0, wave_lo = 0, wave_lo_last = 0;
    if constexpr (WINDOW) {
        j_lo = max(0, q0 + off - p.window + 1) / BLOCK_N;
        wave_lo = wave_q0 + off - p.window + 1;
        wave_lo_last = wave_lo + WAVE_M - 1;
    }
    // SPLIT: this block's share of the nt tiles, [j_lo, nt) from here on (empty: j_lo >= nt)
    if constexpr (SPLIT) {
        const int per = (nt + p.nsplit - 1) / p.nsplit;
        j_lo = split * per;
        nt = min(nt, j_lo + per);
    }

    const int kvh = hh / p.kv_group;
    const T* __restrict__ qp = (const T*)p.q + (VARLEN ? (int64_t)row0 * p.q_ss : (int64_t)b * p.q_sb) + (int64_t)hh * p.q_sh;
    // contiguous: this batch's and head's slab; paged: the head's offset inside every page (the page base is added per tile)
    const char* kp = (const char*)p.k + ((PAGED ? 0 : (int64_t)b * p.k_sb) + (int64_t)kvh * p.k_sh) * EB;
    const char* vp = (const char*)p.v + ((PAGED ? 0 : (int64_t)b * p.v_sb) + (int64_t)kvh * p.v_sh) * EB;
    // KV8: the block's two descales (scalar loads), used under if constexpr (KV8) only so that the other kernels keep their expressions
    float k_mul = 1.f, v_mul = 1.f;
    if constexpr (KV8) {
        k_mul = ((prefill_f32_ptr)(uintptr_t)p.k_descale)[(int64_t)b * p.ds_sb + kvh];
        v_mul = ((prefill_f32_ptr)(uintptr_t)p.v_descale)[(int64_t)b * p.ds_sb + kvh];
    }
    // SINK: the head's sink in log2 units (a scalar load); SPLIT: split 0 alone carries it.  Used under if constexpr (SINK) only
    float s2 = -INFINITY;
    if constexpr (SINK) {
        if (!SPLIT || split == 0) s2 = ((prefill_f32_ptr)(uintptr_t)p.sinks)[hh] * 1.4426950408889634f;
    }

    // ---- Q fragments: B operand of S^T = K Q^T, lane (r,h) holds Q[my_q][16 ks + 8 h .. +7] -----------
    v8 qf[KS];
    {
        const int qrow = min(my_q, sq - 1);
        const T* src = qp + (int64_t)qrow * p.q_ss + 8 * h;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) qf[ks] = *(const v8*)(src + 16 * ks);
    }

    // ---- K/V staging by LDS-DMA, as in fa3_fwd_kernel: wave w issues pieces w, w+8, ...; piece i covers LDS rows 4i..4i+3, the
    // XOR swizzle is applied to the per-lane SOURCE chunk
    constexpr int PIECES = TILE_BYTES / 1024;            // 16 (D=128) or 8 (D=64)
    constexpr int PPW = PIECES / NW;                     // pieces per wave
    int dma_key[PPW];
    int dma_col;                                         // element offset of the source chunk in its key row
    {
        const int R0 = 4 * wave + (lane >> 4);           // LDS row of piece `wave`
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
    // per-lane byte offsets are loop invariant; the tile steps the descriptor base (SALU only, no per-tile VALU)
    uint32_t kvoff[PPW], vvoff[PPW];
#pragma unroll
    for (int t = 0; t < PPW; ++t) {
        kvoff[t] = (uint32_t)(dma_key[t] * (int)p.k_ss + dma_col) * 2u;
        vvoff[t] = (uint32_t)(dma_key[t] * (int)p.v_ss + dma_col) * 2u;
    }
    // (2) paged: page id of the NEXT tile to fetch (a scalar load issued behind the previous tile's DMA), its index in the table
    // row and the token offset inside the page.  dma_tile is called for j = j_lo, j_lo + 1, ... in order (j_lo = 0 without a window),
    // and only for j < nt, i.e. for keys below kv_end <= len_b: entries at and past ceil(len_b / page_size), and those below
    // 64 j_lo / page_size, are never read.  SPLIT: j_lo and nt bound the split's own tiles, so the same holds for the entries outside them.
    const prefill_table_ptr table = PAGED ? (prefill_table_ptr)(uintptr_t)(p.block_table + (int64_t)b * p.bt_sb) : nullptr;
    int pg_next = 0, pg_idx = 0, pg_tok = 0;
    if constexpr (PAGED) {
        if constexpr (WINDOW || SPLIT) {
            pg_idx = (int)((uint32_t)(j_lo * BLOCK_N) / (uint32_t)p.page_size);
            pg_tok = j_lo * BLOCK_N - pg_idx * p.page_size;
        }
        if (j_lo < nt) pg_next = table[pg_idx];
    }
    auto dma_tile = [&](auto bufc, int j) {
        constexpr int BUF = decltype(bufc)::value;
        // (3) the descriptors end at the tile's last valid key: rows at and past len_b read as zeros
        const int nk = min(BLOCK_N, kv_len - j * BLOCK_N);
        int64_t koff, voff;                  // element offsets of the tile's first key row from kp / vp
        if constexpr (PAGED) {
            const int pg = min(max(pg_next, 0), p.num_pages - 1);     // device data: never an address outside the pool
            koff = (int64_t)pg * p.k_sb + (int64_t)pg_tok * p.k_ss;
            voff = (int64_t)pg * p.v_sb + (int64_t)pg_tok * p.v_ss;
        } else {
            koff = (int64_t)j * BLOCK_N * p.k_ss;
            voff = (int64_t)j * BLOCK_N * p.v_ss;
        }
        const srd_t ksrd = __builtin_amdgcn_make_buffer_rsrc((void*)(kp + koff * 2), 0, (int)((int64_t)(nk - 1) * p.k_ss * 2 + D * 2), 0x00020000);
        const srd_t vsrd = __builtin_amdgcn_make_buffer_rsrc((void*)(vp + voff * 2), 0, (int)((int64_t)(nk - 1) * p.v_ss * 2 + D * 2), 0x00020000);
#pragma unroll
        for (int t = 0; t < PPW; ++t) {
            const uint32_t kd = smem_base + BUF * BUF_BYTES + (wave + NW * t) * 1024;
            lds_dma16_buf(ksrd, kvoff[t], kd);
            lds_dma16_buf(vsrd, vvoff[t], kd + TILE_BYTES);
        }
        if constexpr (PAGED) {
            pg_tok += BLOCK_N;
            if (pg_tok == p.page_size) {
                pg_tok = 0;
                ++pg_idx;
                if (j + 1 < nt) pg_next = table[pg_idx];
            }
        }
    };

    // ---- KV8: K/V staging through registers (see the header).  st8 holds the tile that is converted next ----
    constexpr int NLD8 = D == 128 ? 2 : 1;               // 16-byte loads per lane and tile: K and V, or (D = 64) one of the two
    u32x4 st8[NLD8];
    uint32_t src8[NLD8] = {};                            // byte offset of this lane's 16 bytes from the tile's first key row
    uint32_t dst8 = 0;                                   // byte offset of chunk 2c in buffer 0 (chunk 2c + 1: dst8 ^ 16), V image included
    const bool stage_v = D == 64 && wave >= NW / 2;      // D = 64: this wave stages V (wave-uniform)
    if constexpr (KV8) {
        constexpr int LPK = D / 16;                      // lanes (16-byte loads) per key row
        const int t8 = D == 128 ? tid : (tid & 255);
        const int key8 = t8 / LPK, c8 = t8 % LPK;
        if constexpr (D == 128) {
            src8[0] = (uint32_t)(key8 * (int)p.k_ss + 16 * c8);
            src8[NLD8 - 1] = (uint32_t)(key8 * (int)p.v_ss + 16 * c8);
        } else {
            src8[0] = (uint32_t)(key8 * (int)(stage_v ? p.v_ss : p.k_ss) + 16 * c8);
        }
        dst8 = tile_off<D>(key8, 2 * c8) + (stage_v ? TILE_BYTES : 0);
    }
    auto load8 = [&](int j) {
        const int nk = min(BLOCK_N, kv_len - j * BLOCK_N);
        int64_t koff, voff;                  // byte offsets of the tile's first key row from kp / vp
        if constexpr (PAGED) {
            const int pg = min(max(pg_next, 0), p.num_pages - 1);     // device data: never an address outside the pool
            koff = (int64_t)pg * p.k_sb + (int64_t)pg_tok * p.k_ss;
            voff = (int64_t)pg * p.v_sb + (int64_t)pg_tok * p.v_ss;
        } else {
            koff = (int64_t)j * BLOCK_N * p.k_ss;
            voff = (int64_t)j * BLOCK_N * p.v_ss;
        }
        // (3) as dma_tile: the descriptors end at the tile's last valid key, rows at and past len_b read as zero bytes
        if constexpr (D == 128) {
            const srd_t ksrd = __builtin_amdgcn_make_buffer_rsrc((void*)(kp + koff), 0, (int)((int64_t)(nk - 1) * p.k_ss + D), 0x00020000);
            const srd_t vsrd = __builtin_amdgcn_make_buffer_rsrc((void*)(vp + voff), 0, (int)((int64_t)(nk - 1) * p.v_ss + D), 0x00020000);
            st8[0] = __builtin_amdgcn_raw_buffer_load_b128(ksrd, (int)src8[0], 0, 0);
            st8[NLD8 - 1] = __builtin_amdgcn_raw_buffer_load_b128(vsrd, (int)src8[NLD8 - 1], 0, 0);
        } else {
            const char* base = stage_v ? vp + voff : kp + koff;
            const int64_t ss = stage_v ? p.v_ss : p.k_ss;
            const srd_t srd = __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, (int)((int64_t)(nk - 1) * ss + D), 0x00020000);
            st8[0] = __builtin_amdgcn_raw_buffer_load_b128(srd, (int)src8[0], 0, 0);
        }
        if constexpr (PAGED) {
            pg_tok += BLOCK_N;
            if (pg_tok == p.page_size) {
                pg_tok = 0;
                ++pg_idx;
                if (j + 1 < nt) pg_next = table[pg_idx];
            }
        }
    };
    // the held tile into buffer BUF as the 16-bit images: two chunks per load
    auto write8 = [&](auto bufc) {
        constexpr int BUF = decltype(bufc)::value;
        lds_char* const img = smem_l + BUF * BUF_BYTES;
#pragma unroll
        for (int i = 0; i < NLD8; ++i) {
            *(lds_v8*)(img + i * TILE_BYTES + dst8) = cvt_e4m3x8<T, v8>(st8[i][0], st8[i][1]);
            *(lds_v8*)(img + i * TILE_BYTES + (dst8 ^ 16u)) = cvt_e4m3x8<T, v8>(st8[i][2], st8[i][3]);
        }
    };
    // this wave's image writes are done, then everybody's; the two empty statements keep LDS accesses on their side of the barrier
    auto barrier8 = [&]() {
        asm volatile("" ::: "memory");
        __builtin_amdgcn_s_waitcnt(0xC07F);
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    };

    // ---- per-lane LDS read offsets, loop invariant (see fa3_fwd_kernel) ----------
    uint32_t koff[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) koff[ks] = smem_base + tile_off<D>(r, 2 * ks + h);   // absolute LDS address
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) asm volatile("" : "+v"(koff[ks]));
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
    const float c = KV8 ? p.scale_log2 * k_mul : p.scale_log2;   // KV8: raw scores are over the undescaled bytes
    const float thr = 8.0f / c;                 // deferred max: raw-score headroom (2^8 in the exponent) before O is rescaled
    float m_thr = -1e30f, mc = -1e30f * c;      // m_run + thr and m_run * c, updated with m_run

    // ---- one K/V tile: S^T = K Q^T, online softmax, O^T += V^T P^T -------------------------------------------
    auto compute_tile = [&](auto bufc, int key_base) {
        constexpr int BUF = decltype(bufc)::value;
        const lds_char* kimg = (const lds_char*)(uintptr_t)(BUF * BUF_BYTES);   // koff[]/voff[] carry the LDS base
        const lds_char* vimg = kimg + TILE_BYTES;

        f32x16 s[2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int e = 0; e < 16; ++e) s[kb][e] = 0.f;
        constexpr int NQK = 2 * KS, PF = 4;
        v8 afr[PF];
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

        // mask: wave-uniform test, only the tiles on the wave's causal diagonal and the batch's last tile pay
        const bool need_mask = (key_base + BLOCK_N > kv_len) || (CAUSAL && key_base + BLOCK_N - 1 > wave_q0 + off) ||
                               (WINDOW && key_base < wave_lo_last);
        if (need_mask) {
            asm volatile("" ::: "memory");   // keep this a real (wave-uniform) branch, not 32 v_cmp + 32 v_cndmask on every tile
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

        // online softmax; a row lives in lanes (l, l^32)
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
        if constexpr (KV8) {
            if (j + 1 < nt) write8(IC<BUF ^ 1>{});        // the held tile j + 1: its buffer's readers finished before the last barrier
            if (j + 2 < nt) load8(j + 2);                 // into the freed registers, under this tile's math and the next conversion
            if (j * BLOCK_N < wave_kv_end) compute_tile(bufc, j * BLOCK_N);
            barrier8();
        } else {
            if (j + 1 < nt) dma_tile(IC<BUF ^ 1>{}, j + 1);   // lands in the other buffer under this tile's math
            if (j * BLOCK_N < wave_kv_end && (!WINDOW || j * BLOCK_N + BLOCK_N > wave_lo)) compute_tile(bufc, j * BLOCK_N);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's DMA pieces have landed ...
            __builtin_amdgcn_s_waitcnt(0xC07F);               // (lgkmcnt(0): this wave's LDS reads are done)
            __builtin_amdgcn_s_barrier();                     // ... and so have everybody else's
        }
    };

    if constexpr (KV8) {
        if (j_lo < nt) load8(j_lo);
    } else {
        if (j_lo < nt) dma_tile(IC<0>{}, j_lo);
    }
    // Q must have LANDED before the loop (see fa3_fwd_kernel: else its vmcnt waits drain the K/V prefetch every iteration)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) asm volatile("" : "+v"(qf[ks]));
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if constexpr (KV8) {
        if (j_lo < nt) write8(IC<0>{});
        if (j_lo + 1 < nt) load8(j_lo + 1);
        barrier8();
    } else {
        __syncthreads();
    }
    for (int j = j_lo; j < nt; j += 2) {
        step(IC<0>{}, j);
        if (j + 1 < nt) step(IC<1>{}, j + 1);
    }

    // ---- epilogue: normalise once; a row with no visible key -> zeros, LSE = -inf ------------
    const float l_tot = row_pair_sum(l_run);
    float inv = l_tot > 0.f ? 1.0f / l_tot : 0.f;
    if constexpr (KV8) inv *= v_mul;
    // SINK: one more key of score s2 and a zero value row.  e is exactly 1 and l_sink exactly l_tot when s2 = -inf; mc is finite
    // (m_run starts at -1e30), the guard is for a scale so large that mc overflows
    float m_sink = 0.f, l_sink = 0.f;
    if constexpr (SINK) {
        m_sink = fmaxf(mc, s2);
        const float m_use = m_sink == -INFINITY ? 0.f : m_sink;
        const float e = __builtin_amdgcn_exp2f(mc - m_use);
        l_sink = l_tot * e + __builtin_amdgcn_exp2f(s2 - m_use);
        inv = l_sink > 0.f ? (1.0f / l_sink) * e : 0.f;
    }
    // VARLEN: the batch's rows start at packed row row0, and the row bound of every store is the batch's own count -- the next
    // packed row is another batch's
    const int64_t o_batch = VARLEN ? (int64_t)row0 * p.o_ss : (int64_t)b * p.o_sb;
    if constexpr (sizeof(OT) == 2) {
        // 16-bit store through LDS (free after the loop's last barrier) so that one store instruction covers whole rows: see fa3_fwd_kernel
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
        store_rows_from_lds<RB>(lbase, lane, (char*)((OT*)p.o + o_batch + (int64_t)hh * p.o_sh + (int64_t)wave_q0 * p.o_ss),
                                p.o_ss * 2, sq - wave_q0);
    } else if (my_q < sq) {        // fp32 rows straight from the accumulators
        OT* orow;
        if constexpr (SPLIT) orow = p.part_o + ((((int64_t)split * p.B + b) * p.Sq + my_q) * p.H + hh) * D;
        else orow = (OT*)p.o + o_batch + (int64_t)hh * p.o_sh + (int64_t)my_q * p.o_ss;
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
    if (my_q < sq && (SPLIT || p.lse) && h == 0) {
        float lse;
        if constexpr (SINK) {
            // where the keys hold the maximum, the sink-less kernel's value on l_sink -- its m_run * c + log2 l is contracted into one
            // fused multiply-add, spelled out here because the select would keep the compiler from it: at s2 = -inf the partial LSE of a
            // split then has that kernel's bits, and so has the merged O
            const float lg = __builtin_amdgcn_logf(l_sink);
            const float lse_keys = __builtin_fmaf(m_run, c, lg) * 0.6931471805599453f, lse_sink = (s2 + lg) * 0.6931471805599453f;
            lse = l_sink > 0.f ? (mc >= s2 ? lse_keys : lse_sink) : -INFINITY;
        } else lse = l_tot > 0.f ? (m_run * c + __builtin_amdgcn_logf(l_tot)) * 0.6931471805599453f : -INFINITY;
        if constexpr (SPLIT) p.part_lse[(((int64_t)split * p.B + b) * p.H + hh) * p.Sq + my_q] = lse;
        else if constexpr (VARLEN) p.lse[(int64_t)hh * p.total_q + row0 + my_q] = lse;
        else p.lse[((int64_t)b * p.H + hh) * p.Sq + my_q] = lse;
    }
}

}  // namespace pfa

// fa3_fwd_body.inc -- the body of fa3_fwd_kernel (fa3_fwd_kernel.h, which describes it and includes this file once per kernel definition:
// without the sink and with it).  In scope where it is included: the template parameters T, D, CAUSAL, SPLITP, KMASK, OTM; `pin`, the kernel's
// argument block (FwdParams or a block derived from it); `constexpr bool SINK`; and `sinks` (const float*, read under SINK only).
// A file and not a function: called through a function, even one that is always inlined, the sink-less kernels compile to other
// instruction streams than the ones they had.
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

    // SINK: the head's sink in log2 units (a scalar load).  Used under if constexpr (SINK) only
    float s2 = -INFINITY;
    if constexpr (SINK) s2 = ((const __attribute__((address_space(4))) float*)(uintptr_t)sinks)[hh] * 1.4426950408889634f;

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
    float inv = l_tot > 0.f ? 1.0f / l_tot : 0.f;         // fully masked row -> zeros (documented divergence)
    // SINK: one more key of score s2 and a zero value row.  e is exactly 1 and l_sink exactly l_tot when s2 = -inf; mc is finite
    // (m_run starts at -1e30), the guard is for a scale so large that mc overflows
    float l_sink = 0.f;
    if constexpr (SINK) {
        const float m_sink = fmaxf(mc, s2);
        const float m_use = m_sink == -INFINITY ? 0.f : m_sink;
        const float e = __builtin_amdgcn_exp2f(mc - m_use);
        l_sink = l_tot * e + __builtin_amdgcn_exp2f(s2 - m_use);
        inv = l_sink > 0.f ? (1.0f / l_sink) * e : 0.f;
    }
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
            float lse;
            if constexpr (SINK) {
                // where the keys hold the maximum, the sink-less value on l_sink -- its m_run * c + log2 l is contracted into one fused
                // multiply-add, spelled out here because the select would keep the compiler from it: at s2 = -inf the LSE has its bits
                const float lg = __builtin_amdgcn_logf(l_sink);
                const float lse_keys = __builtin_fmaf(m_run, c, lg) * 0.6931471805599453f, lse_sink = (s2 + lg) * 0.6931471805599453f;
                lse = l_sink > 0.f ? (mc >= s2 ? lse_keys : lse_sink) : -INFINITY;
            } else lse = l_tot > 0.f ? (m_run * c + __builtin_amdgcn_logf(l_tot)) * 0.6931471805599453f : -INFINITY;
            if constexpr (VARLEN) p.lse[lse_row0 + my_q] = lse;
            else p.lse[((int64_t)b * p.H + hh) * p.Sq + my_q] = lse;
        }
    }

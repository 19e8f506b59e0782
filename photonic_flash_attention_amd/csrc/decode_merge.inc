// decode_merge.inc -- the merge of the four waves' partials (m, l, O^T) through LDS, for the kernels of the 16-key tile (included once,
// behind the tile loop; a file and not a function for decode_tile16.inc's reason).  The O^T columns go through a [NW][ROWS][PCOLS] fp32
// buffer in PASSES passes of PCOLS columns each, the (m, l) pairs lie behind it; the buffer lies under the waves' images, which are dead
// after the first barrier.  No thread returns in front of a barrier: a dead row's thread only skips the rest of its pass.
// The file LEAVES ITS PASS LOOP OPEN, at a live row's thread: the includer writes the pass's stores and closes the loop.  They are, with
// acc = sum over w of sc[w] * mo[(w * ROWS + orow) * PCOLS + d0 + d] for d = 0, 4, .. < DPT: nsplit == 1, acc / L (0 where L == 0) to
// O[b][oi][oh][col + d] and, at col == 0, the LSE (M + log2 L) ln 2 (-inf where L == 0); else acc to part_o[prow][col + d] of the partial
// layout [nsplit][B][H][Sq][PASSES * PCOLS] and, at col == 0, (M, L) to part_ml[prow], for fa3_decode_combine_kernel.  (Each kernel keeps
// the form of these stores it was built with: either form, written here, changes the other kernel's code.)
// In scope where it is included: `constexpr int PASSES, PCOLS, NDB`; smem; p; tid, wave, the lane's (c, h); the item's rb; grp and kvh
// (the item's rows are packed r = i * grp + g and belong to heads kvh * grp + g); oacc, m, l.
// Leaves in scope: mo, orow, d0, DPT, sc[NW], M, L (complete from pass 0 on), oi, oh, and inside the loop `pass` and `col`.
    // row sum over the row's four lane groups
    l += __shfl_xor(l, 16);
    l += __shfl_xor(l, 32);

    __syncthreads();
    float* mo = (float*)smem;                                   // [NW][ROWS][PCOLS]
    float* mml = (float*)(smem + NW * ROWS * PCOLS * 4);        // [NW][ROWS][2]
    constexpr int TPR = THREADS / ROWS, DPT = PCOLS / TPR;      // threads per row, columns per thread and pass
    const int orow = tid / TPR, d0 = (tid % TPR) * DPT;
    const int rr = rb * ROWS + orow;
    const bool live = rr < p.Sq * grp;
    const int oi = live ? rr / grp : 0, oh = kvh * grp + (live ? rr % grp : 0);
    float M = -__builtin_inff(), L = 0.f, sc[NW];
#pragma unroll
    for (int pass = 0; pass < PASSES; ++pass) {
        if (pass) __syncthreads();                              // the pass before's reads are done before the buffer is written again
#pragma unroll
        for (int d = 0; d < NDB / PASSES; ++d) *(f32x4*)(mo + (wave * ROWS + c) * PCOLS + 16 * d + 4 * h) = oacc[pass * (NDB / PASSES) + d];
        if (pass == 0 && h == 0) {
            mml[(wave * ROWS + c) * 2] = m;
            mml[(wave * ROWS + c) * 2 + 1] = l;
        }
        __syncthreads();
        if (pass == 0) {
            float mw[NW];
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                mw[w] = mml[(w * ROWS + orow) * 2];
                M = fmaxf(M, mw[w]);
            }
            const float Mu = M == -__builtin_inff() ? 0.f : M;  // a row no wave saw a key of: not -inf - (-inf)
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                sc[w] = __builtin_amdgcn_exp2f(mw[w] - Mu);
                L += sc[w] * mml[(w * ROWS + orow) * 2 + 1];
            }
        }
        if (!live) continue;
        const int col = pass * PCOLS + d0;

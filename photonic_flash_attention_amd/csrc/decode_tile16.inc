// decode_tile16.inc -- the math of one 16-key tile behind its S^T MFMAs, for the kernels of decode_parts.h's 16-key tile (included once in
// each kernel's tile body).  A file and not a function: called through a function, even one that is always inlined, the kernels get other
// register assignments and instruction orders than the ones they had (tools/isa_same.py).
// In scope where it is included: T, `constexpr bool WINDOW, SPLIT_P`, `constexpr int NDB`; v4, E, E16; p.scale_log2;
// the tile's first key t0 and `edge` (the tile reaches past the split's hi, the causal cut, below a row's window, or a key mask exists);
// the lane group h; hi, row_lim; row_lo and window (read under WINDOW only); km (const uint8_t*: the batch's key mask or nullptr); vimg, vtr (image_tr_offset).
// Reads and writes: sacc (S^T in, P out), m, l, oacc.
            // scores in log2 units; a key is tested on edge tiles only
            float mx = -__builtin_inff();
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float sc = sacc[e] * p.scale_log2;
                if (edge) {
                    const int key = t0 + 4 * h + e;
                    bool vis;
                    if constexpr (WINDOW) vis = key < hi && (uint32_t)(key - row_lo) < (uint32_t)window;   // row_lo <= key < row_lim
                    else vis = key < hi && key < row_lim;
                    if (vis && km) vis = km[key] != 0;
                    sc = vis ? sc : -__builtin_inff();
                }
                sacc[e] = sc;
                mx = fmaxf(mx, sc);
            }
            mx = fmaxf(mx, __shfl_xor(mx, 16));
            mx = fmaxf(mx, __shfl_xor(mx, 32));
            const float m_new = fmaxf(m, mx);
            const float m_use = m_new == -__builtin_inff() ? 0.f : m_new;     // no key visible yet: not -inf - (-inf)
            const float alpha = __builtin_amdgcn_exp2f(m - m_use);
            m = m_new;
            float ps = 0.f;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float pe = __builtin_amdgcn_exp2f(sacc[e] - m_use);
                sacc[e] = pe;
                ps += pe;
            }
            l = l * alpha + ps;
#pragma unroll
            for (int d = 0; d < NDB; ++d) oacc[d] *= alpha;

            // P^T operand: keys 4h .. 4h + 3 of row c, as the accumulator holds them (fp32 output: a 16-bit hi + lo pair, two MFMAs)
            v4 pf, plo;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                pf[e] = (T)sacc[e];
                if constexpr (SPLIT_P) plo[e] = (T)(sacc[e] - (float)pf[e]);
            }
            asm volatile("" ::: "memory");     // the image writes above stay ahead of the transposed reads below (in-order LDS)
            // O^T += V^T P^T: the tile's 16 keys are the x16 MFMA's k dimension
#pragma unroll
            for (int d = 0; d < NDB; ++d) {
                const v4 va = E::tr_read(vimg + vtr + d * 32);
                oacc[d] = E16::mfma(va, pf, oacc[d]);
                if constexpr (SPLIT_P) oacc[d] = E16::mfma(va, plo, oacc[d]);
            }
            asm volatile("" ::: "memory");     // ... and the next tile's image writes behind them

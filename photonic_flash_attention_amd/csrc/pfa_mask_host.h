// pfa_mask_host.h -- host side of the condensed masks (internal): the forward, the weights pass and the backward turn a u8 mask into one
// 64-bit word per mask row and 64-key tile (fa3_maskbits*_kernel) and a first / last visible tile per 256 rows (fa3_maskrange_kernel)
// in front of their kernels.  One geometry of that scratch and one function that fills it.
#pragma once
#include "fa3_fwd_kernel.h"
#include "pfa_host.h"

namespace pfa {

// [row words][row ranges] of a mask: its own (un-broadcast) extents, the source's byte strides, the words' strides (0 = broadcast).
struct MaskWords {
    const uint8_t* src = nullptr;                // null: no mask, or one past the launch limits (the byte path serves those)
    int Bm = 0, Hm = 0, Qm = 0, Sk = 0, nt = 0;  // nt: 64-key tiles
    int ngran = 0;                               // 256-row granules (fa3_maskrange_kernel: first / last visible tile of each)
    int64_t sb = 0, sh = 0, sq = 0, sk = 0;      // byte strides of the source mask
    int64_t ob = 0, oh = 0, oq = 0;              // word strides of the row words
    size_t word_bytes() const { return src ? (size_t)Bm * Hm * Qm * nt * sizeof(unsigned long long) : 0; }
    size_t range_bytes() const { return src ? (size_t)Bm * Hm * ngran * RANGE_PARTS * 2 * sizeof(int) : 0; }
    size_t bytes() const { return word_bytes() + range_bytes(); }
    // strides of the ranges, in granule pairs
    int64_t range_sb() const { return Bm > 1 ? (int64_t)Hm * ngran : 0; }
    int64_t range_sh() const { return Hm > 1 ? ngran : 0; }
    int64_t range_q() const { return Qm > 1 ? 1 : 0; }
};
inline MaskWords mask_words(const uint8_t* src, int Bm, int Hm, int Qm, int Sk, int64_t sb, int64_t sh, int64_t sq, int64_t sk) {
    MaskWords m;
    if (!src || Qm > 65535 || (int64_t)Bm * Hm > 65535) return m;       // launch limits: rows are blockIdx.y, (batch, head) blockIdx.z
    m.src = src; m.Bm = Bm; m.Hm = Hm; m.Qm = Qm; m.Sk = Sk;
    m.sb = sb; m.sh = sh; m.sq = sq; m.sk = sk;
    m.nt = (Sk + 63) / 64;
    m.ngran = (Qm + 255) / 256;
    m.oq = Qm > 1 ? m.nt : 0;
    m.oh = Hm > 1 ? (int64_t)Qm * m.nt : 0;
    m.ob = Bm > 1 ? (int64_t)Hm * Qm * m.nt : 0;
    return m;
}
// ... of the element mask of an argument block (pfa_fa3_args, pfa_fa3_bwd_args): a dim of stride 0 is broadcast
template <typename Args>
inline MaskWords element_mask_words(const Args* a) {
    return mask_words(a->mask, a->mask_stride_b ? a->B : 1, a->mask_stride_h ? a->H : 1, a->mask_stride_q ? a->Sq : 1, a->Sk, a->mask_stride_b,
                      a->mask_stride_h, a->mask_stride_q, a->mask_stride_k);
}

// ... of a forward call (pfa_fa3_args): the [B, Sk] key mask as one row per batch, else the element mask
inline MaskWords fwd_mask_words(const pfa_fa3_args* a) {
    return a->key_mask ? mask_words(a->key_mask, a->B, 1, 1, a->Sk, a->key_mask_stride_b, 0, 0, 1) : element_mask_words(a);
}
// mask + enough workspace: one word per row and tile instead of a mask byte per score (without workspace the byte path runs)
template <typename Params>
inline bool take_mask_words(Params& p, const MaskWords& mb, const pfa_fa3_args* a) {
    const bool use = mb.src && a->workspace && a->workspace_bytes >= mb.bytes();
    p.mbits = use ? (const unsigned long long*)a->workspace : nullptr;
    p.mb_sb = mb.ob; p.mb_sh = mb.oh; p.mb_sq = mb.oq;
    return use;
}
// what the parameter blocks of the dense forward calls share besides the strides: key counts, mask, shape and the K/V head grouping
template <typename Params>
inline void fill_common(Params& p, const pfa_fa3_args* a) {
    p.seqlens_k = a->seqlens_k;
    fill_mask(p, a);
    p.B = a->B; p.H = a->H; p.Sq = a->Sq; p.Sk = a->Sk;
    p.kv_group = kv_group_of(a);
}

// Enqueue the two kernels that fill the scratch at `ws` (m.bytes() of it).  false: a launch failed (its HIP error is not kept).
template <int UNUSED = 0>      // (a template so that the kernels are instantiated where a translation unit first calls it, not where it includes this)
bool launch_row_words(const MaskWords& m, void* ws, void* stream) {
    launch_mask_words(m.src, m.sb, m.sh, m.sq, m.sk, m.Bm, m.Hm, m.Qm, m.Sk, m.nt, (unsigned long long*)ws, m.ob, m.oh, m.oq, (hipStream_t)stream);
    if (hipGetLastError() != hipSuccess) return false;
    hipLaunchKernelGGL(fa3_maskrange_kernel<256>, dim3((unsigned)(m.ngran * RANGE_PARTS), (unsigned)(m.Bm * m.Hm)), dim3(256), 0, (hipStream_t)stream,
                       (const unsigned long long*)ws, m.ob, m.oh, m.oq, m.Hm, m.Qm, m.nt, (int*)((char*)ws + m.word_bytes()), m.ngran);
    return hipGetLastError() == hipSuccess;
}

}  // namespace pfa

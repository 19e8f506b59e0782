// pfa_bwd_capi.hip -- C ABI of the backward pass (include/pfa_hip.h: pfa_fa3_bwd).  Separate translation unit:
// the key-stationary dK/dV kernel runs one wave per SIMD on the whole register file and is compiled with
// -mllvm -amdgpu-mfma-vgpr-form (see Makefile) so that hipcc keeps its MFMA accumulators in place.
#include "pfa_hip.h"

#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include "fa3_bwd_kernels.h"
#include "fa3_bwd_f32_kernel.h"
#include "pfa_host.h"
#include "pfa_mask_host.h"

namespace {

// The rules of pfa_fa3_bwd_args, in the order their errors are reported (tests/test_bwd_host.py pins it).
int check_bwd(const pfa_fa3_bwd_args* a) {
    using pfa::aligned16; using pfa::aligned4; using pfa::multiples_of; using pfa::slab_bytes;
    if (!a) return PFA_ERR_NULL;
    if (a->size != sizeof(pfa_fa3_bwd_args)) return PFA_ERR_STRUCT_SIZE;
    if (a->flags) return PFA_ERR_FLAGS;
    const bool f32 = a->dtype == PFA_DTYPE_FP32;      // fp32 backward kernels (fa3_bwd_f32_kernel.h): fp32 everything, the only path with dropout
    if (a->kv_group < 0 || (a->kv_group > 1 && (a->H % a->kv_group || f32))) return PFA_ERR_FLAGS;   // (fp32 kernels: one K/V head per query head)
    if (!f32 && a->drop_mask) return PFA_ERR_FLAGS;
    if (!a->q || !a->k || !a->v || !a->o || !a->dout || !a->lse || !a->dq || !a->dk || !a->dv || (!f32 && !a->delta)) return PFA_ERR_NULL;
    if (a->B <= 0 || a->H <= 0 || a->Sq <= 0 || a->Sk <= 0) return PFA_ERR_SHAPE;
    if (a->D != 64 && a->D != 128) return PFA_ERR_HEAD_DIM;
    const bool g32 = a->dtype_grad == PFA_DTYPE_FP32;
    if (f32 ? !g32 : ((a->dtype != PFA_DTYPE_BF16 && a->dtype != PFA_DTYPE_FP16) || (a->dtype_grad != a->dtype && !g32))) return PFA_ERR_DTYPE;
    if (!pfa::scale_ok(a->softmax_scale)) return PFA_ERR_SHAPE;
    const int32_t Sq = a->Sq, Sk = a->Sk, D = a->D;
    if (f32) {
        if (a->drop_mask && (!(a->drop_scale >= 1.f) || !isfinite(a->drop_scale))) return PFA_ERR_FLAGS;
        // dout is read in 16-byte pieces like q / k / v (fa3_bwd_f32_kernel MODE 0); o and the gradients are 4-byte accesses
        if (!pfa::qkv_strides_multiples_of(4, a) || !multiples_of(4, {a->do_stride_b, a->do_stride_h, a->do_stride_s})) return PFA_ERR_STRIDE;
        if (!aligned16(a->q) || !aligned16(a->k) || !aligned16(a->v) || !aligned16(a->dout)) return PFA_ERR_ALIGN;
        if (!aligned4(a->o) || !aligned4(a->dq) || !aligned4(a->dk) || !aligned4(a->dv) || !aligned4(a->lse)) return PFA_ERR_ALIGN;
        // row strides: non-negative, rows at least D apart, every tensor addressable with 32-bit element offsets inside one (b, h) slab
        const struct { int32_t S; int64_t stride; } rows[] = {{Sq, a->q_stride_s}, {Sk, a->k_stride_s}, {Sk, a->v_stride_s}, {Sq, a->o_stride_s},
                                                             {Sq, a->do_stride_s}, {Sq, a->dq_stride_s}, {Sk, a->dk_stride_s}, {Sk, a->dv_stride_s}};
        for (const auto& r : rows)
            if (r.stride < D) return PFA_ERR_STRIDE;
        for (const auto& r : rows)
            if (!pfa::slab_fits32(r.S, r.stride, D, 4)) return PFA_ERR_SHAPE;
        return PFA_OK;
    }
    if (!pfa::qkv_strides_multiples_of(8, a) ||
        !multiples_of(8, {a->o_stride_b, a->o_stride_h, a->o_stride_s, a->do_stride_b, a->do_stride_h, a->do_stride_s}))
        return PFA_ERR_STRIDE;
    if (!multiples_of(g32 ? 4 : 8, {a->dq_stride_b, a->dq_stride_h, a->dq_stride_s, a->dk_stride_b, a->dk_stride_h, a->dk_stride_s, a->dv_stride_b,
                                    a->dv_stride_h, a->dv_stride_s}))      // gradient rows leave in 16-byte pieces
        return PFA_ERR_STRIDE;
    for (const void* p : {a->q, a->k, a->v, a->o, a->dout, (const void*)a->dq, (const void*)a->dk, (const void*)a->dv})
        if (!aligned16(p)) return PFA_ERR_ALIGN;
    for (int64_t s : {slab_bytes(Sk, a->k_stride_s, D, 2), slab_bytes(Sk, a->v_stride_s, D, 2), slab_bytes(Sq, a->q_stride_s, D, 2),
                      slab_bytes(Sq, a->do_stride_s, D, 2)})
        if (s > 0x7fffffffLL || s <= 0) return PFA_ERR_SHAPE;
    return PFA_OK;
}

// The condensed element mask in pfa_fa3_bwd_args.mask_workspace (see BwdParams): [row words][row ranges] as the forward has them
// (pfa_mask_host.h), then [column words][column ranges] for the key-stationary dK/dV kernel
struct BwdMaskWs {
    pfa::MaskWords row;
    int ntq = 0, nkb = 0;                        // 64-row tiles of the problem, 128-key blocks
    size_t colw = 0, colr = 0;
    size_t bytes() const { return row.bytes() + colw + colr; }
};
BwdMaskWs bwd_mask_ws(const pfa_fa3_bwd_args* a) {
    BwdMaskWs w;
    if (!a || !a->mask || a->dtype == PFA_DTYPE_FP32) return w;
    if (a->mask_stride_h == 0 && a->mask_stride_q == 0) return w;              // key-only masks never reach the element-mask kernels
    const int ntq = (a->Sq + 63) / 64;
    if (ntq > 65535) return w;                                                 // launch limits: the byte paths serve these
    w.row = pfa::element_mask_words(a);
    if (!w.row.src) return w;
    w.ntq = ntq; w.nkb = (a->Sk + 127) / 128;
    const size_t bh = (size_t)w.row.Bm * w.row.Hm;
    w.colw = bh * (size_t)a->Sk * w.ntq * 8; w.colr = bh * w.nkb * pfa::RANGE_PARTS * 8;
    return w;
}

}  // namespace

extern "C" {

size_t pfa_fa3_bwd_mask_workspace_bytes(const pfa_fa3_bwd_args* a) { return bwd_mask_ws(a).bytes(); }

size_t pfa_fa3_bwd_workspace_bytes(const pfa_fa3_bwd_args* a) {
    if (!a || a->B <= 0 || a->H <= 0 || a->Sq <= 0) return 0;
    return (size_t)a->B * a->H * a->Sq * sizeof(float);
}

int pfa_fa3_bwd(const pfa_fa3_bwd_args* a, void* stream) {
    const int st = check_bwd(a);
    if (st != PFA_OK) return st;
    const int BH = a->B * a->H;
    if (a->dtype == PFA_DTYPE_FP32) {
        pfa::F32BwdParams p;
        p.q = (const float*)a->q; p.k = (const float*)a->k; p.v = (const float*)a->v; p.o = (const float*)a->o;
        p.dout = (const float*)a->dout; p.lse = a->lse;
        p.dq = (float*)a->dq; p.dk = (float*)a->dk; p.dv = (float*)a->dv;
        p.seqlens_k = a->seqlens_k; p.mask = a->mask; p.drop_mask = a->drop_mask;
        pfa::fill_bwd_strides(p, a);
        p.B = a->B; p.H = a->H; p.Sq = a->Sq; p.Sk = a->Sk; p.causal = a->causal != 0;
        p.scale = a->softmax_scale; p.drop_scale = a->drop_scale;
        const auto f0 = pfa::dispatch_dim(a->D, [](auto d) -> pfa::KernelFn<pfa::F32BwdParams> { return &pfa::fa3_bwd_f32_kernel<d.value, 0>; });
        const auto f1 = pfa::dispatch_dim(a->D, [](auto d) -> pfa::KernelFn<pfa::F32BwdParams> { return &pfa::fa3_bwd_f32_kernel<d.value, 1>; });
        const size_t lds = pfa::dispatch_dim(a->D, [](auto d) { return pfa::f32_bwd_lds_bytes<d.value>(); });
        const pfa::DeviceScope dev(a->device_id);
        if (pfa::hip_failed(dev.error())) return PFA_ERR_DEVICE;
        const int st0 = pfa::launch(f0, dim3((unsigned)(((a->Sq + pfa::F32B_BM - 1) / pfa::F32B_BM) * BH)), 256, p, lds, stream);
        return st0 != PFA_OK ? st0 : pfa::launch(f1, dim3((unsigned)(((a->Sk + pfa::F32B_BM - 1) / pfa::F32B_BM) * BH)), 256, p, lds, stream);
    }
    pfa::BwdParams p;
    p.q = a->q; p.k = a->k; p.v = a->v; p.o = a->o; p.dout = a->dout; p.lse = a->lse; p.delta = a->delta;
    p.dq = a->dq; p.dk = a->dk; p.dv = a->dv; p.seqlens_k = a->seqlens_k;
    p.mask = a->mask;
    pfa::fill_bwd_strides(p, a);
    p.B = a->B; p.H = a->H; p.Sq = a->Sq; p.Sk = a->Sk;
    p.kv_group = pfa::kv_group_of(a);
    // a mask of the keys only (the reference's 2-D [B,Sk] mask arrives as [B,1,1,Sk]) runs on the unmasked kernels: see BwdParams::keymask
    const bool key_only = a->mask && a->mask_stride_h == 0 && a->mask_stride_q == 0 && a->mask_stride_k == 1 && a->Sk % 4 == 0 &&
                          a->mask_stride_b % 4 == 0 && pfa::aligned4(a->mask);
    p.keymask = key_only ? a->mask : nullptr;
    p.km_sb = a->mask_stride_b;
    if (key_only) p.mask = nullptr;
    p.mask_dw = (p.mask && a->mask_stride_k == 1 && a->Sk % 4 == 0 && a->mask_stride_b % 4 == 0 && a->mask_stride_h % 4 == 0 &&
                 a->mask_stride_q % 4 == 0 && pfa::aligned4(a->mask)) ? 1 : 0;
    p.scale = a->softmax_scale;
    p.scale_log2 = a->softmax_scale * pfa::LOG2E;
    // element mask + scratch: words, transposed words and tile ranges (filled below, in front of the two kernels)
    const BwdMaskWs mw = p.mask ? bwd_mask_ws(a) : BwdMaskWs();
    const pfa::MaskWords& row = mw.row;
    const bool use_words = mw.bytes() > 0 && a->mask_workspace && a->mask_workspace_bytes >= mw.bytes();

    const bool causal = a->causal != 0, g32 = a->dtype_grad == PFA_DTYPE_FP32, kmask = p.mask != nullptr;     // (not for key-only masks)
    pfa::KernelFn<pfa::BwdParams> kdq = nullptr, kdkdv = nullptr;
    pfa::dispatch_elem_dim(a->dtype, a->D, [&](auto t) {
        using T = typename decltype(t)::type;
        constexpr int D = decltype(t)::D;
        return pfa::dispatch_bools([&](auto c, auto k, auto o32) {
            using OT = pfa::out_t<decltype(o32)::value, T>;
            kdq = &pfa::fa3_bwd_dq_kernel<T, D, decltype(c)::value, decltype(k)::value, OT>;
            kdkdv = &pfa::fa3_bwd_dkdv_kernel<T, D, decltype(c)::value, decltype(k)::value, OT>;
            return 0;
        }, causal, kmask, g32);
    });
    const pfa::DeviceScope dev(a->device_id);
    if (pfa::hip_failed(dev.error())) return PFA_ERR_DEVICE;
    if (use_words) {
        char* const ws = (char*)a->mask_workspace;
        char* const col_words = ws + row.bytes();
        p.mw_row = (const unsigned long long*)ws;
        p.mw_sq = row.oq; p.mw_sh = row.oh; p.mw_sb = row.ob;
        p.rg_row = (const int*)(ws + row.word_bytes());
        p.rg_q = row.range_q(); p.rg_sh = row.range_sh(); p.rg_sb = row.range_sb();
        p.mw_col = (const unsigned long long*)col_words;
        p.ntq = mw.ntq; p.cw_sh = row.Hm > 1 ? (int64_t)a->Sk * mw.ntq : 0; p.cw_sb = row.Bm > 1 ? (int64_t)row.Hm * a->Sk * mw.ntq : 0;
        p.rg_col = (const int*)(col_words + mw.colw);
        p.crg_sh = row.Hm > 1 ? mw.nkb : 0; p.crg_sb = row.Bm > 1 ? (int64_t)row.Hm * mw.nkb : 0;
        const unsigned bh = (unsigned)(row.Bm * row.Hm);
        if (!pfa::launch_row_words(row, ws, stream)) return PFA_ERR_LAUNCH;
        // (the transposed words always have the problem's own row count: a mask without a row dimension is the same word in every row)
        hipLaunchKernelGGL(pfa::fa3_maskbitsT_kernel<0>, dim3((unsigned)((row.nt + 3) / 4), (unsigned)mw.ntq, bh), dim3(256), 0, (hipStream_t)stream,
                           (const unsigned long long*)ws, row.ob, row.oh, row.oq, row.Hm, row.Qm, a->Sq, a->Sk, row.nt, mw.ntq,
                           (unsigned long long*)col_words);
        hipLaunchKernelGGL(pfa::fa3_maskrange_kernel<128>, dim3((unsigned)(mw.nkb * pfa::RANGE_PARTS), bh), dim3(256), 0, (hipStream_t)stream,
                           (const unsigned long long*)col_words, (int64_t)row.Hm * a->Sk * mw.ntq, (int64_t)a->Sk * mw.ntq, (int64_t)mw.ntq, row.Hm,
                           a->Sk, mw.ntq, (int*)(col_words + mw.colw), mw.nkb);
        if (hipGetLastError() != hipSuccess) return PFA_ERR_LAUNCH;
    }
    // (the dQ kernel computes delta = rowsum(dO o O) for its own rows and publishes it for the dK/dV kernel behind it)
    const size_t lds = 2 * 2 * pfa::BLOCK_N * a->D * 2;
    p.nblk = (a->Sq + 255) / 256;
    const int stq = pfa::launch(kdq, dim3((unsigned)(p.nblk * BH)), 512, p, lds, stream);
    if (stq != PFA_OK) return stq;
    p.nblk = (a->Sk + 127) / 128;
    // a workgroup per key block and K/V head; its tile stages + the per-row constants exceed the default 64 KiB dynamic-LDS limit
    return pfa::launch(kdkdv, dim3((unsigned)(p.nblk * (BH / p.kv_group))), 256, p, lds + 1024, stream);
}

}  // extern "C"

// pfa_varlen_bwd_capi.hip -- C ABI of the packed variable-length backward (include/pfa_hip.h, pfa_fa3_varlen_bwd*): validation and the
// two launches of fa3_bwd_dq_kernel / fa3_bwd_dkdv_kernel<..., Packed<store type>>, the dense backward kernels' packed mode.  A translation unit of
// its own, built with the per-object flags of pfa_bwd_capi.hip (Makefile): the packed kernels must return the dense kernels' bits.
#include "pfa_hip.h"

#include <hip/hip_runtime.h>
#include <stdio.h>

#include "fa3_bwd_kernels.h"
#include "pfa_varlen_host.h"

namespace {

// The rules of pfa_fa3_varlen_bwd_args, in the order their errors are reported.
int check(const pfa_fa3_varlen_bwd_args* a) {
    using pfa::aligned16; using pfa::multiples_of;
    if (!a) return PFA_ERR_NULL;
    if (a->size != sizeof(pfa_fa3_varlen_bwd_args)) return PFA_ERR_STRUCT_SIZE;
    const int st = pfa::varlen::check_head(a, !a->dout || !a->lse || !a->dq || !a->dk || !a->dv || !a->delta);
    if (st != PFA_OK) return st;
    const bool g32 = a->dtype_grad == PFA_DTYPE_FP32;
    if ((a->dtype != PFA_DTYPE_BF16 && a->dtype != PFA_DTYPE_FP16) || (a->dtype_grad != a->dtype && !g32)) return PFA_ERR_DTYPE;
    if (!pfa::scale_ok(a->softmax_scale)) return PFA_ERR_SHAPE;
    if (!multiples_of(8, {a->q_stride_s, a->q_stride_h, a->k_stride_s, a->k_stride_h, a->v_stride_s, a->v_stride_h, a->o_stride_s, a->o_stride_h,
                          a->do_stride_s, a->do_stride_h}))
        return PFA_ERR_STRIDE;
    if (!multiples_of(g32 ? 4 : 8, {a->dq_stride_s, a->dq_stride_h, a->dk_stride_s, a->dk_stride_h, a->dv_stride_s, a->dv_stride_h}))
        return PFA_ERR_STRIDE;                                                                 // gradient rows leave in 16-byte pieces
    for (const void* p : {a->q, a->k, a->v, a->o, a->dout, (const void*)a->dq, (const void*)a->dk, (const void*)a->dv})
        if (!aligned16(p)) return PFA_ERR_ALIGN;
    if (!pfa::aligned4(a->delta)) return PFA_ERR_ALIGN;
    if (!pfa::slab_fits32(a->max_seqlen_q, a->do_stride_s, a->D, 2) || a->do_stride_s < 0) return PFA_ERR_SHAPE;   // the dK/dV kernel's dO tiles
    return pfa::varlen::check_tail(a);
}

void tag(const pfa_fa3_varlen_bwd_args* a, char* buf, size_t n) {
    snprintf(buf, n, "%s_d%d_%s_%s", pfa::varlen::elem_name(a->dtype), a->D, a->causal ? "causal" : "full",
             a->dtype_grad == PFA_DTYPE_FP32 ? "g32" : "g16");
}

}  // namespace

extern "C" {

size_t pfa_fa3_varlen_bwd_workspace_bytes(const pfa_fa3_varlen_bwd_args* a) {
    if (!a || a->H <= 0 || a->total_q <= 0) return 0;
    return (size_t)a->H * a->total_q * sizeof(float);
}

int pfa_fa3_varlen_bwd_check(const pfa_fa3_varlen_bwd_args* a) { return check(a); }

int pfa_fa3_varlen_bwd_describe(const pfa_fa3_varlen_bwd_args* a, char* buf, size_t n, int32_t* dkdv_workgroups) {
    const int st = check(a);
    if (st != PFA_OK) return st;
    if (buf && n) {
        char t[48];
        tag(a, t, sizeof(t));
        snprintf(buf, n, "fa3_bwd_dq_varlen_%s+fa3_bwd_dkdv_varlen_%s", t, t);
    }
    if (dkdv_workgroups) *dkdv_workgroups = (int32_t)pfa::varlen::k_workgroups(a);
    return (int)pfa::varlen::q_workgroups(a);
}

int pfa_fa3_varlen_bwd(const pfa_fa3_varlen_bwd_args* a, void* stream) {
    const int st = check(a);
    if (st != PFA_OK) return st;
    pfa::BwdParams p;
    p.q = a->q; p.k = a->k; p.v = a->v; p.o = a->o; p.dout = a->dout; p.lse = a->lse; p.delta = a->delta;
    p.dq = a->dq; p.dk = a->dk; p.dv = a->dv;
    p.seqlens_k = nullptr; p.mask = nullptr; p.keymask = nullptr; p.km_sb = 0; p.mask_dw = 0;
    p.m_sb = p.m_sh = p.m_sq = p.m_sk = 0;
    p.q_sb = p.k_sb = p.v_sb = p.o_sb = p.do_sb = p.dq_sb = p.dk_sb = p.dv_sb = 0;
    p.q_sh = a->q_stride_h; p.q_ss = a->q_stride_s; p.k_sh = a->k_stride_h; p.k_ss = a->k_stride_s;
    p.v_sh = a->v_stride_h; p.v_ss = a->v_stride_s; p.o_sh = a->o_stride_h; p.o_ss = a->o_stride_s;
    p.do_sh = a->do_stride_h; p.do_ss = a->do_stride_s; p.dq_sh = a->dq_stride_h; p.dq_ss = a->dq_stride_s;
    p.dk_sh = a->dk_stride_h; p.dk_ss = a->dk_stride_s; p.dv_sh = a->dv_stride_h; p.dv_ss = a->dv_stride_s;
    p.B = a->B; p.H = a->H; p.Sq = a->max_seqlen_q; p.Sk = a->max_seqlen_k;
    p.kv_group = a->H / a->Hkv;
    p.scale = a->softmax_scale;
    p.scale_log2 = a->softmax_scale * pfa::LOG2E;
    p.cu_q = a->cu_seqlens_q; p.cu_k = a->cu_seqlens_k; p.total_q = a->total_q; p.total_k = a->total_k;

    const bool causal = a->causal != 0, g32 = a->dtype_grad == PFA_DTYPE_FP32;
    pfa::KernelFn<pfa::BwdParams> kdq = nullptr, kdkdv = nullptr;
    pfa::dispatch_elem_dim(a->dtype, a->D, [&](auto t) {
        using T = typename decltype(t)::type;
        constexpr int D = decltype(t)::D;
        return pfa::dispatch_bools([&](auto c, auto o32) {
            using OTM = pfa::Packed<pfa::out_t<decltype(o32)::value, T>>;
            kdq = &pfa::fa3_bwd_dq_kernel<T, D, decltype(c)::value, false, OTM>;
            kdkdv = &pfa::fa3_bwd_dkdv_kernel<T, D, decltype(c)::value, false, OTM>;
            return 0;
        }, causal, g32);
    });
    const pfa::DeviceScope dev(a->device_id);
    if (pfa::hip_failed(dev.error())) return PFA_ERR_DEVICE;
    // (the dQ kernel computes delta = rowsum(dO o O) for its own rows and publishes it for the dK/dV kernel behind it)
    const size_t lds = 2 * 2 * pfa::BLOCK_N * a->D * 2;
    p.nblk = (a->max_seqlen_q + 255) / 256;
    const int stq = pfa::launch(kdq, dim3((unsigned)pfa::varlen::q_workgroups(a)), 512, p, lds, stream);
    if (stq != PFA_OK) return stq;
    p.nblk = (a->max_seqlen_k + 127) / 128;
    // a workgroup per key block and K/V head; its tile stages + the per-row constants exceed the default 64 KiB dynamic-LDS limit
    return pfa::launch(kdkdv, dim3((unsigned)pfa::varlen::k_workgroups(a)), 256, p, lds + 1024, stream);
}

}  // extern "C"

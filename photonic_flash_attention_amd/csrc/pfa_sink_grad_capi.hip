// pfa_sink_grad_capi.hip -- C ABI of the gradient of the attention sinks (include/pfa_hip_train_sinks.h, pfa_fa3_sink_grad*): validation and the two
// launches of sink_grad_kernel.h.  No allocation, no synchronisation, no process-wide state; the workspace is the caller's.
#include "pfa_hip_train_sinks.h"

#include <hip/hip_runtime.h>
#include <stdio.h>

#include "pfa_host.h"
#include "sink_grad_kernel.h"

namespace {

int64_t nchunk(const pfa_fa3_sink_grad_args* a) { return ((int64_t)a->Sq + pfa::SINK_GRAD_CHUNK - 1) / pfa::SINK_GRAD_CHUNK; }
// stage-1 workgroups = partial sums (after the shape rules: all factors >= 1), saturated so that the product cannot wrap
int64_t partials(const pfa_fa3_sink_grad_args* a) {
    const int64_t lim = 0x7fffffffLL, bh = (int64_t)a->B * a->H;
    return bh > lim || bh * nchunk(a) > lim ? lim + 1 : bh * nchunk(a);
}

// the rules a workspace size can be made from: no pointers, no strides
int check_shape(const pfa_fa3_sink_grad_args* a, bool packed) {
    if (a->B < 1 || a->H < 1 || a->Sq < 1) return PFA_ERR_SHAPE;
    if (packed && (a->total_q < 1 || a->Sq > a->total_q)) return PFA_ERR_SHAPE;
    return PFA_OK;
}
int check_limits(const pfa_fa3_sink_grad_args* a) {      // the row index and the grid inside 32 bits, as pfa_attn_merge refuses its items
    return ((int64_t)a->Sq + pfa::SINK_GRAD_CHUNK > 0x7fffffffLL || partials(a) > 0x7fffffffLL) ? PFA_ERR_SHAPE : PFA_OK;
}

size_t workspace_bytes(const pfa_fa3_sink_grad_args* a) { return (size_t)partials(a) * sizeof(float); }

int check(const pfa_fa3_sink_grad_args* a) {
    using pfa::aligned4;
    if (!a) return PFA_ERR_NULL;
    if (a->size != sizeof(pfa_fa3_sink_grad_args)) return PFA_ERR_STRUCT_SIZE;
    if (a->flags != 0 || a->reserved0 != 0) return PFA_ERR_FLAGS;
    const bool packed = a->cu_seqlens_q != nullptr;
    if (!a->lse || !a->delta || !a->sinks || !a->d_sinks || !a->workspace) return PFA_ERR_NULL;
    int st = check_shape(a, packed);
    if (st != PFA_OK) return st;
    if (!packed) {      // rows contiguous, heads and batches at least a sequence apart where there is more than one
        for (const int64_t s : {a->lse_stride_b, a->lse_stride_h, a->delta_stride_b, a->delta_stride_h})
            if (s < 0) return PFA_ERR_STRIDE;
        if (a->H > 1 && (a->lse_stride_h < a->Sq || a->delta_stride_h < a->Sq)) return PFA_ERR_STRIDE;
        if (a->B > 1 && (a->lse_stride_b < a->Sq || a->delta_stride_b < a->Sq)) return PFA_ERR_STRIDE;
    }
    if (!aligned4(a->lse) || !aligned4(a->delta) || !aligned4(a->sinks) || !aligned4(a->d_sinks) || !aligned4(a->cu_seqlens_q) ||
        !aligned4(a->workspace))
        return PFA_ERR_ALIGN;
    st = check_limits(a);
    if (st != PFA_OK) return st;
    if (a->workspace_bytes < workspace_bytes(a)) return PFA_ERR_NULL;
    return PFA_OK;
}

}  // namespace

extern "C" {

size_t pfa_fa3_sink_grad_workspace_bytes(const pfa_fa3_sink_grad_args* a) {
    if (!a || a->size != sizeof(pfa_fa3_sink_grad_args)) return 0;
    if (check_shape(a, a->cu_seqlens_q != nullptr) != PFA_OK || check_limits(a) != PFA_OK) return 0;
    return workspace_bytes(a);
}

int pfa_fa3_sink_grad_check(const pfa_fa3_sink_grad_args* a) { return check(a); }

int pfa_fa3_sink_grad_describe(const pfa_fa3_sink_grad_args* a, char* buf, size_t n) {
    const int st = check(a);
    if (st != PFA_OK) return st;
    if (buf && n) snprintf(buf, n, "sink_grad_%s_c%d+final", a->cu_seqlens_q ? "packed" : "dense", pfa::SINK_GRAD_CHUNK);
    return (int)partials(a);
}

int pfa_fa3_sink_grad(const pfa_fa3_sink_grad_args* a, void* stream) {
    const int st = check(a);
    if (st != PFA_OK) return st;
    pfa::SinkGradParams p;
    p.lse = a->lse; p.delta = a->delta; p.sinks = a->sinks; p.d_sinks = a->d_sinks;
    p.partial = (float*)a->workspace;
    p.cu_q = a->cu_seqlens_q;
    p.l_sb = a->lse_stride_b; p.l_sh = a->lse_stride_h; p.d_sb = a->delta_stride_b; p.d_sh = a->delta_stride_h;
    p.B = a->B; p.H = a->H; p.Sq = a->Sq; p.total_q = a->total_q;
    p.nchunk = (int32_t)nchunk(a);
    const pfa::KernelFn<pfa::SinkGradParams> stage1 = p.cu_q ? &pfa::sink_grad_partial_kernel<true> : &pfa::sink_grad_partial_kernel<false>;
    const pfa::DeviceScope dev(a->device_id);
    if (pfa::hip_failed(dev.error())) return PFA_ERR_DEVICE;
    const int st1 = pfa::launch(stage1, dim3((unsigned)partials(a)), pfa::SINK_GRAD_THREADS, p, 0, stream);
    if (st1 != PFA_OK) return st1;
    return pfa::launch(pfa::KernelFn<pfa::SinkGradParams>(&pfa::sink_grad_final_kernel<0>), dim3((unsigned)a->H), pfa::SINK_GRAD_THREADS, p, 0, stream);
}

}  // extern "C"

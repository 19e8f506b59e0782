// pfa_varlen_capi.hip -- C ABI of the packed variable-length forward (include/pfa_hip.h, pfa_fa3_varlen_check / _fwd / _describe):
// validation and the launch of fa3_fwd_kernel<..., Packed<store type>>, the 8-wave forward's packed mode.  A translation unit of its own, built with the
// flags of pfa_capi.hip (whose dense instantiations of the same body it must match bit for bit); the backward's is
// pfa_varlen_bwd_capi.hip, built with pfa_bwd_capi.hip's.  No allocation, no synchronisation, no process-wide state, no workspace.
#include "pfa_hip.h"

#include <hip/hip_runtime.h>
#include <stdio.h>

#include "fa3_fwd_kernel.h"
#include "pfa_varlen_host.h"

namespace {

// The rules of pfa_fa3_varlen_args, in the order their errors are reported.
int check(const pfa_fa3_varlen_args* a) {
    using pfa::aligned16; using pfa::multiples_of;
    if (!a) return PFA_ERR_NULL;
    if (a->size != sizeof(pfa_fa3_varlen_args)) return PFA_ERR_STRUCT_SIZE;
    const int st = pfa::varlen::check_head(a, false);
    if (st != PFA_OK) return st;
    if (a->dtype_in != PFA_DTYPE_BF16 && a->dtype_in != PFA_DTYPE_FP16) return PFA_ERR_DTYPE;
    if (a->dtype_out != a->dtype_in && a->dtype_out != PFA_DTYPE_FP32) return PFA_ERR_DTYPE;
    if (!pfa::scale_ok(a->softmax_scale)) return PFA_ERR_SHAPE;
    if (!multiples_of(8, {a->q_stride_s, a->q_stride_h, a->k_stride_s, a->k_stride_h, a->v_stride_s, a->v_stride_h}) ||
        !multiples_of(a->dtype_out == PFA_DTYPE_FP32 ? 4 : 8, {a->o_stride_s, a->o_stride_h}))      // 16-bit rows leave in 16-byte pieces
        return PFA_ERR_STRIDE;
    if (!aligned16(a->q) || !aligned16(a->k) || !aligned16(a->v) || !aligned16(a->o)) return PFA_ERR_ALIGN;
    return pfa::varlen::check_tail(a);
}

bool split_p(const pfa_fa3_varlen_args* a) { return a->dtype_out == PFA_DTYPE_FP32; }      // fp32 output is the parity mode

}  // namespace

extern "C" {

int pfa_fa3_varlen_check(const pfa_fa3_varlen_args* a) { return check(a); }

int pfa_fa3_varlen_describe(const pfa_fa3_varlen_args* a, char* buf, size_t n) {
    const int st = check(a);
    if (st != PFA_OK) return st;
    if (buf && n)
        snprintf(buf, n, "fa3_fwd_varlen_%s_d%d_%s%s_%s", pfa::varlen::elem_name(a->dtype_in), a->D, a->causal ? "causal" : "full",
                 split_p(a) ? "_splitp" : "", a->dtype_out == PFA_DTYPE_FP32 ? "o32" : "o16");
    return (int)pfa::varlen::q_workgroups(a);
}

int pfa_fa3_varlen_fwd(const pfa_fa3_varlen_args* a, void* stream) {
    const int st = check(a);
    if (st != PFA_OK) return st;
    pfa::FwdParams p;
    pfa::varlen::fill_fwd_params(p, a);
    const bool causal = a->causal != 0, out32 = a->dtype_out == PFA_DTYPE_FP32;
    // (split P goes with the fp32 store: two of the four combinations exist)
    const auto fn = pfa::dispatch_elem_dim(a->dtype_in, a->D, [&](auto t) {
        using T = typename decltype(t)::type;
        return pfa::dispatch_bools([](auto c, auto o32) -> pfa::KernelFn<pfa::FwdParams> {
            return &pfa::fa3_fwd_kernel<T, decltype(t)::D, c.value, o32.value, false, pfa::Packed<pfa::out_t<o32.value, T>>>;
        }, causal, out32);
    });
    const pfa::DeviceScope dev(a->device_id);
    if (pfa::hip_failed(dev.error())) return PFA_ERR_DEVICE;
    const size_t lds = 2 * 2 * pfa::BLOCK_N * a->D * 2;      // two buffers of a K and a V tile image
    return pfa::launch(fn, dim3((unsigned)pfa::varlen::q_workgroups(a)), pfa::FWD_THREADS, p, lds, stream);
}

}  // extern "C"

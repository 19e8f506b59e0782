// pfa_varlen_sink_capi.hip -- C ABI of the packed variable-length forward with attention sinks (include/pfa_hip_train_sinks.h,
// pfa_fa3_varlen_fwd_sink*): the entry points and the SINK instantiations of fa3_fwd_kernel<..., Packed<store type>>.  The rules of
// pfa_fa3_sinks come first, then everything pfa_fa3_varlen_check says; a NULL block is pfa_fa3_varlen_fwd itself.  A translation unit of
// its own, built with the flags of pfa_varlen_capi.hip.  No allocation, no synchronisation, no process-wide state, no workspace.
#include "pfa_hip_train_sinks.h"

#include <hip/hip_runtime.h>
#include <stdio.h>

#include "fa3_fwd_kernel.h"
#include "pfa_cache_modes.h"
#include "pfa_varlen_host.h"

namespace {

using SinkParams = pfa::FwdBlock<true>;

int check(const pfa_fa3_varlen_args* a, const pfa_fa3_sinks* sinks) {
    const int st = pfa::check_sinks(sinks);
    return st != PFA_OK ? st : pfa_fa3_varlen_check(a);
}

}  // namespace

extern "C" {

int pfa_fa3_varlen_fwd_sink_check(const pfa_fa3_varlen_args* a, const pfa_fa3_sinks* sinks) {
    return sinks ? check(a, sinks) : pfa_fa3_varlen_check(a);
}

int pfa_fa3_varlen_fwd_sink_describe(const pfa_fa3_varlen_args* a, const pfa_fa3_sinks* sinks, char* buf, size_t n) {
    if (!sinks) return pfa_fa3_varlen_describe(a, buf, n);
    const int st = check(a, sinks);
    if (st != PFA_OK) return st;
    const bool out32 = a->dtype_out == PFA_DTYPE_FP32;
    if (buf && n)
        snprintf(buf, n, "fa3_fwd_varlen_%s_d%d_%s%s_%s_sink", pfa::varlen::elem_name(a->dtype_in), a->D, a->causal ? "causal" : "full",
                 out32 ? "_splitp" : "", out32 ? "o32" : "o16");
    return (int)pfa::varlen::q_workgroups(a);
}

int pfa_fa3_varlen_fwd_sink(const pfa_fa3_varlen_args* a, const pfa_fa3_sinks* sinks, void* stream) {
    if (!sinks) return pfa_fa3_varlen_fwd(a, stream);
    const int st = check(a, sinks);
    if (st != PFA_OK) return st;
    SinkParams p;
    pfa::varlen::fill_fwd_params(p, a);
    p.sinks = sinks->sinks;
    const bool causal = a->causal != 0, out32 = a->dtype_out == PFA_DTYPE_FP32;
    // (split P goes with the fp32 store: two of the four combinations exist)
    const auto fn = pfa::dispatch_elem_dim(a->dtype_in, a->D, [&](auto t) {
        using T = typename decltype(t)::type;
        return pfa::dispatch_bools([](auto c, auto o32) -> pfa::KernelFn<SinkParams> {
            return &pfa::fa3_fwd_kernel<T, decltype(t)::D, c.value, o32.value, false, pfa::Packed<pfa::out_t<o32.value, T>>>;
        }, causal, out32);
    });
    const pfa::DeviceScope dev(a->device_id);
    if (pfa::hip_failed(dev.error())) return PFA_ERR_DEVICE;
    const size_t lds = 2 * 2 * pfa::BLOCK_N * a->D * 2;      // two buffers of a K and a V tile image
    return pfa::launch(fn, dim3((unsigned)pfa::varlen::q_workgroups(a)), pfa::FWD_THREADS, p, lds, stream);
}

}  // extern "C"

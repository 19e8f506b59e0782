// pfa_w4.hip -- instantiations of the 4-wave x 64-row forward (fa3_fwd_w4_kernel.h) in a translation unit of their own:
// the kernel wants the 512-register budget and is iterated on separately from the 8-wave kernels in pfa_capi.hip.
#include <hip/hip_runtime.h>

#include "fa3_fwd_w4_kernel.h"
#include "pfa_host.h"

namespace pfa {

template <typename T>
static KernelFn<FwdParams> w4_kernel_of(bool causal, bool out32) {
    return dispatch_bools([](auto c, auto o32) -> KernelFn<FwdParams> { return &fa3_fwd_w4_kernel<T, c.value, out_t<o32.value, T>>; }, causal, out32);
}
// dtype: PFA_DTYPE_BF16 or PFA_DTYPE_FP16; out32: fp32 store.
KernelFn<FwdParams> w4_kernel(int dtype, bool causal, bool out32) {
    return dtype == PFA_DTYPE_BF16 ? w4_kernel_of<__bf16>(causal, out32) : w4_kernel_of<_Float16>(causal, out32);
}

}  // namespace pfa

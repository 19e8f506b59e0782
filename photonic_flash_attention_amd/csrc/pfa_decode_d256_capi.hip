// pfa_decode_d256_capi.hip -- C ABI of the split-KV decode at head dim 256 (include/pfa_hip_decode_d256.h, ABI v9 additive): the entry
// points and the 16 instantiations of fa3_decode_d256_kernel (bf16 / fp16 x output x paged x window) with the 4 of the combine kernel at
// D = 256.  Validation (pfa_fa3_decode_ex's rules with the head dims named HeadDims::D256), the split rule, the describe, the parameter fill
// and the workspace layout are pfa_decode_host.h's, which every decode unit shares; the kernel table and the launch are here because the
// kernel is another one.  A file of its own: the other decode objects are built from what they were built from.
// No allocation, no synchronisation, no process-wide state, a grid from host shapes only.
#include "fa3_decode_d256_kernel.h"
#include "pfa_decode_host.h"
#include "pfa_hip_decode_d256.h"

using namespace pfa::decode;
using pfa::HeadDims;

namespace {

// fa3_decode_d256_kernel for (dtype, out, paged) at the window mode the caller fixes
template <bool WINDOW>
pfa::KernelFn<Params<WINDOW>> kernel_d256(int dtype, bool out32, bool paged) {
    return pfa::dispatch_bools([](auto bf, auto o32, auto pg) -> pfa::KernelFn<Params<WINDOW>> {
        using T = std::conditional_t<bf.value, __bf16, _Float16>;
        return &pfa::dec::fa3_decode_d256_kernel<T, pfa::out_t<o32.value, T>, pg.value, WINDOW>;
    }, dtype == PFA_DTYPE_BF16, out32, paged);
}

}  // namespace

extern "C" {

size_t pfa_fa3_decode_d256_workspace_bytes(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext) {
    return workspace_bytes<false, HeadDims::D256>(a, {ext});
}

int pfa_fa3_decode_d256_check(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext) { return check_only<false, HeadDims::D256>(a, {ext}); }

int pfa_fa3_decode_d256_describe(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, char* buf, size_t n, int32_t* nsplit) {
    return describe<false, HeadDims::D256>(a, {ext}, buf, n, nsplit);
}

int pfa_fa3_decode_d256(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, void* stream) {
    pfa::CacheModes m;
    Plan pl;
    const int st = check<false, HeadDims::D256>(a, {ext}, &m, &pl);
    if (st != PFA_OK) return st;
    return pfa::dispatch_bools([&](auto w) -> int {
        constexpr bool W = w.value;
        Params<W> p;
        fill_params(p, a, pl);
        pfa::fill_modes<W, false, false, false, false>(p, m);
        const bool out32 = a->dtype_out == PFA_DTYPE_FP32;
        const auto fn = kernel_d256<W>(a->dtype_in, out32, a->block_table != nullptr);
        const auto cfn = combine_at<256>(a->dtype_in, out32);
        return launch_with_combine(fn, cfn, p, a, pl, pl.items, 0, stream);
    }, m.window != 0);
}

}  // extern "C"

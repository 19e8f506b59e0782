// pfa_prefill_d256_capi.hip -- C ABI of the forward over a KV cache at head dim 256, uniform and ragged (include/pfa_hip_prefill_d256.h,
// ABI v9 additive): the entry points and the 48 instantiations of fa3_prefill_d256_kernel (bf16 / fp16 x output x paged x ragged x {not
// causal, causal, causal + window}).  Validation (pfa_fa3_prefill_ex's and pfa_fa3_prefill_varlen_ex's rules with the head dims named
// HeadDims::D256 and 128 rows per workgroup), the describe and the parameter fill are pfa_prefill_host.h's, which every prefill unit
// shares; the kernel table and the launch are here because the kernel is another one.  A file of its own: the other prefill objects are
// built from what they were built from.
// No allocation, no synchronisation, no process-wide state, no workspace, a grid from host shapes only.
#include "fa3_prefill_d256_kernel.h"
#include "pfa_prefill_host.h"
#include "pfa_hip_prefill_d256.h"

using namespace pfa::prefill;
using pfa::HeadDims;

static_assert(rows_per_workgroup(HeadDims::D256) == pfa::P256_BLOCK_M, "the grid rule and the kernel agree on the q block");

namespace {

// fa3_prefill_d256_kernel for (dtype, causal, paged, out) in the mode set the caller fixes; a window without the causal flag does not
// exist (validation refuses it) and has nullptr, which no launch accepts.  fp32 output: P carried as a 16-bit hi + lo pair (SPLITP)
template <bool VARLEN, bool WINDOW>
pfa::KernelFn<Params<VARLEN, WINDOW>> kernel_d256(int dtype, bool causal, bool paged, bool out32) {
    return pfa::dispatch_bools([](auto bf, auto c, auto pg, auto o32) -> pfa::KernelFn<Params<VARLEN, WINDOW>> {
        using T = std::conditional_t<bf.value, __bf16, _Float16>;
        if constexpr (WINDOW && !c.value) return nullptr;
        else return &pfa::fa3_prefill_d256_kernel<T, c.value, o32.value, pg.value, pfa::out_t<o32.value, T>, VARLEN, WINDOW>;
    }, dtype == PFA_DTYPE_BF16, causal, paged, out32);
}

// of arguments that pass the check: the block of the call's mode set and one launch on `stream`
template <typename Args>
int run_d256(const Args* a, const pfa_fa3_cache_ext* ext, void* stream) {
    constexpr bool VARLEN = kVarlen<Args>;
    pfa::CacheModes m;
    const int st = check<false, HeadDims::D256>(a, ext, nullptr, nullptr, &m);
    if (st != PFA_OK) return st;
    return pfa::dispatch_bools([&](auto w) -> int {
        constexpr bool W = w.value;
        Params<VARLEN, W> p;
        fill_prefill_params<VARLEN, HeadDims::D256>(p, a);
        pfa::fill_modes<W, false, false, false, false>(p, m);
        const auto fn = kernel_d256<VARLEN, W>(a->dtype_in, a->causal != 0, a->block_table != nullptr, a->dtype_out == PFA_DTYPE_FP32);
        if (!fn) return PFA_ERR_FLAGS;
        const pfa::DeviceScope dev(a->device_id);
        if (pfa::hip_failed(dev.error())) return PFA_ERR_DEVICE;
        return pfa::launch(fn, dim3((unsigned)workgroups<HeadDims::D256>(a)), pfa::P256_THREADS, p, pfa::P256_LDS_BYTES, stream);
    }, m.window != 0);
}

}  // namespace

extern "C" {

int pfa_fa3_prefill_d256_check(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext) {
    return entry_check<false, HeadDims::D256>(a, ext, nullptr, nullptr);
}
int pfa_fa3_prefill_d256_describe(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, char* buf, size_t n) {
    return entry_describe<false, HeadDims::D256>(a, ext, nullptr, nullptr, buf, n);
}
int pfa_fa3_prefill_d256(const pfa_fa3_decode_args* a, const pfa_fa3_cache_ext* ext, void* stream) { return run_d256(a, ext, stream); }

int pfa_fa3_prefill_varlen_d256_check(const pfa_fa3_prefill_varlen_args* a, const pfa_fa3_cache_ext* ext) {
    return entry_check<false, HeadDims::D256>(a, ext, nullptr, nullptr);
}
int pfa_fa3_prefill_varlen_d256_describe(const pfa_fa3_prefill_varlen_args* a, const pfa_fa3_cache_ext* ext, char* buf, size_t n) {
    return entry_describe<false, HeadDims::D256>(a, ext, nullptr, nullptr, buf, n);
}
int pfa_fa3_prefill_varlen_d256(const pfa_fa3_prefill_varlen_args* a, const pfa_fa3_cache_ext* ext, void* stream) {
    return run_d256(a, ext, stream);
}

}  // extern "C"
